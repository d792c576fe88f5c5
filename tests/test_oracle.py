"""The CPU oracle against the reference's own artefacts (no GPU).

Pins, strongest first:
  1. raw-RGBA SHA-256 + ray counts of the unmodified reference binary at
     640x360x4, row mode, recorded in SURVEY.md §8c (the survey compiled
     /root/reference/source and ran it in this container);
  2. the reference's committed renders result{1..4}*.png (macOS build: its
     libm differs, so they pin statistically -- exact-pixel fractions and max
     deltas as measured in SURVEY.md §4);
  3. internal consistency: octree (reference) == exact BVH == linear scan.
"""
import hashlib
import json
import os

import numpy as np
import pytest
from PIL import Image

import oracle
from conftest import GOLDEN, data

# SURVEY.md §8c "[probe] Oracle values here (clang, row mode, 640x360x4)"
REFERENCE_BINARY = {
    "triangle": ("7aa3820992abf7eb", 1932.5),
    "cube": ("da6b5abfaccbc394", 2419.3),
    "suzanne": ("c9a035a993b4ee32", 2559.7),
    "teapot": ("aa59780a14a04ba5", 2388.5),
}
# reference result PNG, min exact-pixel fraction, max |delta| (SURVEY.md §4:
# 99.9987 %/1, 99.9948 %/1, 99.858 %/13, 99.372 %/36)
GOLDEN_PNG = {
    "triangle": ("result1Triangle.png", 0.99995, 2),
    "cube": ("result2Cube.png", 0.9999, 2),
    "suzanne": ("result3Suzanne.png", 0.998, 20),
    "teapot": ("result4Teapot.png", 0.993, 48),
}


def _render(name, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, seed=oracle.SEED_ROW,
            w=640, h=360, spp=4):
    tris, bmin, bmax = oracle.load_scene(data(name + ".obj"))
    cam = oracle.camera_for_scene(bmin, bmax, w, h)
    sc = oracle.Scene(tris, accel=accel, tie=tie, bmin=bmin, bmax=bmax)
    return sc.render(cam, w, h, spp, seed_mode=seed)


@pytest.fixture(scope="module")
def row_images():
    return {n: _render(n) for n in REFERENCE_BINARY}


@pytest.mark.parametrize("name", list(REFERENCE_BINARY))
def test_oracle_reproduces_reference_binary(row_images, name):
    img, rays = row_images[name]
    sha = hashlib.sha256(np.ascontiguousarray(img[::-1]).tobytes()).hexdigest()[:16]
    assert (sha, round(rays / 1000.0, 1)) == REFERENCE_BINARY[name]


@pytest.mark.parametrize("name", list(GOLDEN_PNG))
def test_oracle_vs_committed_reference_pngs(row_images, name):
    fname, min_frac, max_delta = GOLDEN_PNG[name]
    ref = np.asarray(Image.open(os.path.join(GOLDEN, fname)).convert("RGBA"))
    img = row_images[name][0][::-1]  # PNGs are written flipped (main.cpp:341)
    same = (img == ref).all(-1).mean()
    delta = np.abs(img.astype(int) - ref.astype(int)).max()
    mse = ((img[..., :3].astype(float) - ref[..., :3]) ** 2).mean()
    psnr = 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))
    assert same >= min_frac and delta <= max_delta and psnr > 50, (same, delta, psnr)


@pytest.mark.parametrize("name", ["cube", "suzanne", "teapot"])
def test_scene_query_variants_agree(row_images, name):
    """Tie rule (visit order vs lowest index) and accelerator (octree vs the
    exact-semantics BVH) do not change the pinned images."""
    ref = row_images[name][0]
    for accel, tie in ((oracle.ACCEL_OCTREE, oracle.TIE_INDEX), (oracle.ACCEL_BVH, oracle.TIE_INDEX)):
        img, rays = _render(name, accel, tie)
        assert np.array_equal(img, ref) and rays == row_images[name][1]


def _rays(tris, n, seed):
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    o = lo - 0.2 * (hi - lo) + rng.random((n, 3)) * 1.4 * (hi - lo)
    t = rng.integers(0, tris.shape[0], n)
    b = rng.random((n, 3))
    b[rng.random(n) < 0.3, rng.integers(0, 3, n)[:1]] = 0
    b /= b.sum(1, keepdims=True)
    d = (np.einsum("kj,kjc->kc", b, tris[t]) - o).astype(np.float32)
    d /= np.sqrt((d ** 2).sum(1, keepdims=True))
    return np.concatenate([o, d], 1).astype(np.float32)


@pytest.mark.parametrize("name", ["cube", "suzanne"])
def test_bvh_equals_linear_scan(name):
    tris, bmin, bmax = oracle.load_scene(data(name + ".obj"))
    rays = _rays(tris, 20000, 3)
    a = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX).hit_batch(rays, 0.001, 1e7)
    b = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR).hit_batch(rays, 0.001, 1e7)
    assert np.array_equal(a[0], b[0])
    h = a[0] >= 0
    assert h.sum() > 100 and np.array_equal(a[1][h].view(np.uint32), b[1][h].view(np.uint32))
    if name == "suzanne":
        # origins 100 scene diagonals away (ray_cases.py): still inside the domain on
        # which the padded leaf boxes cover Moller-Trumbore's acceptance region
        import ray_cases
        far = ray_cases.families(tris, 20000, 5)["far_sphere_100"]
        a = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX).hit_batch(far, 0.001, 1e7)
        b = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR).hit_batch(far, 0.001, 1e7)
        assert np.array_equal(a[0], b[0])
        h = a[0] >= 0
        assert h.sum() > 2000 and np.array_equal(a[1][h].view(np.uint32), b[1][h].view(np.uint32))


# ---------------------------------------------------------------- golden fixtures
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


def _bits(a):
    return [f"{x:08x}" for x in np.asarray(a, np.float32).ravel().view(np.uint32)]


def test_rng_kats(golden):
    for seed, kat in golden["kat"].items():
        s = int(seed)
        assert [int(x) for x in oracle.xorshift_seq(s, 32)] == kat["xorshift"]
        assert _bits(oracle.float01_seq(s, 32)) == kat["float01"]
        assert _bits(oracle.disk_seq(s, 16)[0]) == kat["disk"]
        assert _bits(oracle.unit_vector_seq(s, 16)[0]) == kat["unit_vector"]
    for key, v in golden["pixel_seed"].items():
        x, y, w = map(int, key.split(","))
        assert oracle.pixel_seed(x, y, w) == v


def test_xorshift_independent_restatement():
    """maths.cpp:5-18 restated in numpy, independent of the C oracle."""
    s = np.uint32(9781 * 3 + 1)
    out = []
    for _ in range(1000):
        s ^= np.uint32(s << np.uint32(13))
        s ^= np.uint32(s >> np.uint32(17))
        s ^= np.uint32(s << np.uint32(15))
        out.append(int(s))
    assert out == [int(x) for x in oracle.xorshift_seq(9781 * 3 + 1, 1000)]
    f = np.float32(np.uint32(out[-1]) & np.uint32(0xFFFFFF)) / np.float32(16777216.0)
    assert f == oracle.float01_seq(9781 * 3 + 1, 1000)[-1]


@pytest.mark.parametrize("seed", [1, 9781 * 7 + 1, 0xDEADBEEF])
def test_xorshift_jump_equals_sequential_steps(seed):
    """GF(2) jump (checker for the planned per-sample substream mode) == n single steps."""
    seq = oracle.xorshift_seq(seed, 70000)
    for n in (1, 2, 3, 17, 1000, 65536, 70000):
        assert oracle.xorshift_jump(seed, n) == int(seq[n - 1])
    assert oracle.xorshift_jump(seed, 0) == seed
    # composition: M^(a+b) = M^a M^b, at offsets far past any sequential check
    a, b = 2**16 * 63, 2**40 + 5
    assert oracle.xorshift_jump(oracle.xorshift_jump(seed, a), b) == oracle.xorshift_jump(seed, a + b)
    # period of xorshift32 over nonzero states is 2^32 - 1
    assert oracle.xorshift_jump(seed, 2**32 - 1) == seed


def test_disk_and_unit_vector_properties():
    d, _ = oracle.disk_seq(5, 2000)
    assert (d[:, 2] == 0).all() and ((d[:, :2].astype(np.float64) ** 2).sum(1) < 1).all()
    u, _ = oracle.unit_vector_seq(5, 2000)
    assert np.allclose(np.linalg.norm(u.astype(np.float64), axis=1), 1.0, atol=1e-5)


def test_camera_golden(golden):
    for key, want in golden["camera"].items():
        name, size = key.rsplit("_", 1)
        w, h = map(int, size.split("x"))
        if name == "sponza_standin":
            import gen_standin_sponza
            path, sponza = gen_standin_sponza.ensure(), True
        else:
            path, sponza = data(name + ".obj"), False
        _, bmin, bmax = oracle.load_scene(path)
        assert _bits(oracle.camera_for_scene(bmin, bmax, w, h, sponza)) == want


@pytest.mark.parametrize("name", ["triangle", "cube", "suzanne", "teapot", "sponza_standin"])
def test_image_golden(golden, name):
    g = golden["images"][name]
    if name == "sponza_standin":
        import gen_standin_sponza
        path, sponza = gen_standin_sponza.ensure(), True
    else:
        path, sponza = data(name + ".obj"), False
    tris, bmin, bmax = oracle.load_scene(path)
    assert tris.shape[0] == g["tris"]
    cam = oracle.camera_for_scene(bmin, bmax, g["w"], g["h"], sponza)
    modes = [("pixel", oracle.ACCEL_BVH, oracle.TIE_INDEX, oracle.SEED_PIXEL)]
    if "row" in g:
        modes.append(("row", oracle.ACCEL_OCTREE, oracle.TIE_VISIT, oracle.SEED_ROW))
    for mode, accel, tie, seed in modes:
        sc = oracle.Scene(tris, accel=accel, tie=tie, bmin=bmin, bmax=bmax)
        img, rays = sc.render(cam, g["w"], g["h"], g["spp"], seed_mode=seed)
        sha = hashlib.sha256(np.ascontiguousarray(img[::-1]).tobytes()).hexdigest()
        assert (sha, rays) == (g[mode]["sha256"], g[mode]["rays"]), mode


def test_sponza_standin_is_deterministic(golden):
    import gen_standin_sponza

    path = gen_standin_sponza.ensure()
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == golden["sponza_standin_sha256"]
    m = gen_standin_sponza.build()
    assert m.ntris == 66450


def test_pixel_rows_are_independent():
    """Pixel seeding makes every row a pure function of its index: rendering a
    row subset equals the same rows of the full frame (what sharding relies on)."""
    tris, bmin, bmax = oracle.load_scene(data("suzanne.obj"))
    cam = oracle.camera_for_scene(bmin, bmax, 160, 90)
    sc = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    full, _ = sc.render(cam, 160, 90, 2, seed_mode=oracle.SEED_PIXEL)
    part, _ = sc.render(cam, 160, 90, 2, seed_mode=oracle.SEED_PIXEL, y0=3, row_step=7)
    rows = np.arange(3, 90, 7)
    assert np.array_equal(part[rows], full[rows])


# ---------------------------------------------------------------- sample seeding
def _xorshift_np(x, n):
    """n xorshift steps (maths.cpp:5-13) of every state in x, numpy, independent of the C oracle."""
    x = x.astype(np.uint32).copy()
    for _ in range(n):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(15)
    return x


def test_sample_seed_is_the_stream_at_sample_offsets():
    """Sample seeding: sample s of a pixel starts 2^16 * s xorshift steps into
    the pixel's own stream -- checked against sequential numpy steps."""
    seeds = np.array([oracle.pixel_seed(x, y, 640) for x, y in ((0, 0), (5, 3), (639, 359), (100, 200))],
                     np.uint32)
    cur = seeds.copy()
    for s in range(4):
        assert [oracle.sample_seed(int(p), s) for p in seeds] == [int(v) for v in cur]
        cur = _xorshift_np(cur, oracle.SAMPLE_STRIDE)
    assert oracle.sample_seed(int(seeds[1]), 1000) == oracle.xorshift_jump(int(seeds[1]), 1000 * 2**16)


def test_sample_mode_render_restated_from_primitives():
    """The oracle's sample-seeded image loop (render_row with ORC_SEED_SAMPLE)
    equals the loop of main.cpp:202-233 written out in Python over the oracle's
    own pinned primitives, with each sample's stream started at its offset."""
    tris, bmin, bmax = oracle.load_scene(data("suzanne.obj"))
    w, h, spp = 12, 7, 3
    cam = oracle.camera_for_scene(bmin, bmax, w, h)
    sc = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    img, rays = sc.render(cam, w, h, spp, seed_mode=oracle.SEED_SAMPLE)
    inv_w, inv_h, recip = np.float32(1) / np.float32(w), np.float32(1) / np.float32(h), np.float32(1) / np.float32(spp)
    ref = np.zeros((h, w, 4), np.uint8)
    total = 0
    for y in range(h):
        for x in range(w):
            col = np.zeros(3, np.float32)
            for s in range(spp):
                st = oracle.sample_seed(oracle.pixel_seed(x, y, w), s)
                jx, jy = oracle.float01_seq(st, 2)
                st = int(oracle.xorshift_seq(st, 2)[-1])
                u = (np.float32(x) + jx) * inv_w
                v = (np.float32(y) + jy) * inv_h
                o, d, st = oracle.get_ray(cam, float(u), float(v), st)
                c, st, r = sc.trace(o, d, st)
                col = col + c
                total += r
            col = np.sqrt(col * recip)
            ref[y, x, :3] = (np.minimum(np.maximum(col, 0), 1) * np.float32(255)).astype(np.uint8)
            ref[y, x, 3] = 255
    assert rays == total
    assert np.array_equal(img, ref)


def test_sample_mode_first_sample_is_pixel_mode():
    """Sample 0 starts at the pixel seed: a 1-spp frame is the pixel-mode frame,
    and with more samples the two modes differ (different streams)."""
    tris, bmin, bmax = oracle.load_scene(data("cube.obj"))
    cam = oracle.camera_for_scene(bmin, bmax, 80, 45)
    sc = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    a, ra = sc.render(cam, 80, 45, 1, seed_mode=oracle.SEED_SAMPLE)
    b, rb = sc.render(cam, 80, 45, 1, seed_mode=oracle.SEED_PIXEL)
    assert ra == rb and np.array_equal(a, b)
    a, _ = sc.render(cam, 80, 45, 4, seed_mode=oracle.SEED_SAMPLE)
    b, _ = sc.render(cam, 80, 45, 4, seed_mode=oracle.SEED_PIXEL)
    assert not np.array_equal(a, b)


def _sample_from_state(sc, cam, x, y, w, h, st):
    """One camera sample of main.cpp:212-218 from RNG state st, over the
    oracle's pinned primitives: (colour, end state, rays)."""
    inv_w, inv_h = np.float32(1) / np.float32(w), np.float32(1) / np.float32(h)
    jx, jy = oracle.float01_seq(st, 2)
    st = int(oracle.xorshift_seq(st, 2)[-1])
    o, d, st = oracle.get_ray(cam, float((np.float32(x) + jx) * inv_w), float((np.float32(y) + jy) * inv_h), st)
    return sc.trace(o, d, st)


def test_speculative_row_chains_restated():
    """The speculative row engine's method (tmpt_rows.hip render_rowspec),
    restated in Python over the oracle's primitives: per row and iteration,
    trace one sample at EVERY even RNG offset of a window (and of a lookahead
    window for the next pixel), then walk the chain through them.  The image
    and ray count equal the oracle's row-seeded loop (main.cpp:202-233, the
    reference's own RNG), and every sample takes an even number of draws --
    the fact the method rests on.  Small windows force chains that leave a
    window mid-pixel and next pixels that start outside the lookahead."""
    tris, bmin, bmax = oracle.load_scene(data("suzanne.obj"))
    w, h, spp = 9, 4, 3
    cam = oracle.camera_for_scene(bmin, bmax, w, h)
    sc = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    ref, ref_rays = sc.render(cam, w, h, spp, seed_mode=oracle.SEED_ROW)
    img = np.zeros_like(ref)
    total = 0
    recip = np.float32(1) / np.float32(spp)
    cache = {}

    def unit(x, y, st):  # (colour, draws, end state, rays) of the sample starting at st
        key = (x, y, st)
        if key not in cache:
            c, end, r = _sample_from_state(sc, cam, x, y, w, h, st)
            draws = 1
            s = int(oracle.xorshift_seq(st, 1)[-1])
            while s != end:
                s = int(oracle.xorshift_seq(s, 1)[-1])
                draws += 1
                assert draws < 10000
            assert draws % 2 == 0
            cache[key] = (c, draws, end, r)
        return cache[key]

    for y in range(h):
        st = y * 9781 + 1  # main.cpp:204
        x, k, col = 0, 0, np.zeros(3, np.float32)
        while x < w:
            # windows (offset start, count) for pixels x and x + 1, in units of 2 draws
            wins = [(0, 5), (3, 12)] if x + 1 < w else [(0, 5)]
            units = [[unit(x + i, y, oracle.xorshift_jump(st, 2 * (s0 + j))) for j in range(n)]
                     for i, (s0, n) in enumerate(wins)]
            j, i, last = 0, 0, None
            while wins[i][0] <= j < wins[i][0] + wins[i][1]:
                c, draws, end, r = units[i][j - wins[i][0]]
                col = col + c
                total += r
                last = end
                j += draws // 2
                k += 1
                if k == spp:
                    v = np.sqrt(col * recip)
                    img[y, x, :3] = (np.minimum(np.maximum(v, 0), 1) * np.float32(255)).astype(np.uint8)
                    img[y, x, 3] = 255
                    x, k, col = x + 1, 0, np.zeros(3, np.float32)
                    i += 1
                    if i >= len(wins):
                        break
            st = last  # the next sample's start state
    assert total == ref_rays
    assert np.array_equal(img, ref)
