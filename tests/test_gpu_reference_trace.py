"""The library's float outputs against the reference itself, sample by sample.

tests/golden/ref/trace_<case>.npz hold what the compiled, unmodified reference
answered for every sample of four 32x18x8 frames (oracle/ref/ref_trace.cpp runs
its Camera::GetRay, Scene::HitScene and main.cpp's own Trace(); cases and format
in tests/ref_cases.py, the CPU side in test_reference_trace_pin.py).  Every
expectation here is formed in numpy float32 from those recorded values alone --
no oracle call -- by the summation code the oracle-based tests use
(render_restate.radiance_sum / aov_sums, adaptive_restate.adaptive_expect), and
the scenes, cameras and seeds are read from the fixtures.

Held to the reference: trace_radiance's float tile, bytes and ray count in both
seedings, trace_image's bytes and ray count through every engine, camera_rays'
ray and RNG words, trace_aov's normal, depth and hits, trace_adaptive's map,
tile, bytes, rays and passes.  NOT held to it here: trace_aov's direct, lit and
tri_id -- the reference never forms a first-bounce light scalar or a triangle
id, so they stay pinned to the oracle only (test_gpu_aov.py) -- and word [7] of
a camera_rays entry, which has no counterpart there.  The seeds of pixel and
sample seeding are this project's by design; the fixture stores the states.

Tolerance: none.  Floats are compared as bits.
"""
import functools

import numpy as np
import pytest

import ref_cases as C
import toymeshpathtracer_amd as tm
from adaptive_restate import adaptive_expect
from render_restate import aov_sums, pack, radiance_sum, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
ONE = f32(1).view(np.uint32)
WAVES = (4, 5)
CASES = [(name, waves) for name in C.TRACE_CASES for waves in WAVES]
CASE_IDS = [f"{name}-waves{waves}" for name, waves in CASES]
#: adaptive thresholds, chosen on the CPU over the reference's colours so that the
#: schedule 2, 4, 6, 8 stops pixels at every one of its counts (asserted from the expectation)
TAU = {"cube": 0.05, "room": 0.1, "room_open": 0.05, "grid": 0.05}
SPP_MIN, SPP_STEP = 2, 2


@functools.lru_cache(maxsize=None)
def _case(name):
    """The fixture and its per-sample values in frame shape [h, w, spp, ...] (read-only)."""
    fx = C.load_trace(name)
    w, h, spp = (int(v) for v in fx["size"])
    n = (h, w, spp)
    out = dict(fx=fx, w=w, h=h, spp=spp,
               col={tm.SEED_SAMPLE: fx["s_col"].reshape(n + (3,)), tm.SEED_PIXEL: fx["p_col"].reshape(n + (3,))},
               rays={tm.SEED_SAMPLE: fx["s_rays"].reshape(n).astype(np.int64),
                     tm.SEED_PIXEL: fx["p_rays"].reshape(n).astype(np.int64)},
               hit=fx["s_hit"].reshape(n).astype(bool), t=fx["s_tn"][:, 0].reshape(n),
               nrm=fx["s_tn"][:, 1:4].reshape(n + (3,)))
    for v in list(out["rays"].values()) + [out["hit"]]:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _radiance(name, seed, spp):
    """(float32[h, w, 3], bytes, rays) the reference's samples give at spp (a prefix of each pixel's 8)."""
    c = _case(name)
    rad, rays = radiance_sum(c["col"][seed], c["rays"][seed], spp)
    return rad, pack(rad), rays


def _scene(name, waves):
    fx = _case(name)["fx"]
    sc = tm.Scene(fx["tris"], bounds=(fx["bmin"], fx["bmax"]))
    sc.set_option("path_waves", waves)
    return sc


def _camera(name):
    a = [float(v) for v in _case(name)["fx"]["cam"]]
    return tm.Camera.create(a[0:3], a[3:6], a[6:9], a[9], a[10], a[11], a[12])


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_radiance_equals_reference(gpu, name, waves):
    """Sample and pixel seeding at 1, 3 and 8 spp: the float tile bit for bit (the
    sum in sample order times 1.0f / spp, alpha 1.0), its bytes, its ray count."""
    c = _case(name)
    w, h = c["w"], c["h"]
    cam = _camera(name)
    with _scene(name, waves) as sc:
        for seed, sname in ((tm.SEED_SAMPLE, "sample"), (tm.SEED_PIXEL, "pixel")):
            for spp in (1, 3, 8):
                want, want_img, want_rays = _radiance(name, seed, spp)
                rad, img, rays = sc.trace_radiance(cam, w, h, spp, seed_mode=seed)
                what = f"{name} {sname} seeding x{spp}, path_waves {waves}"
                assert rad.shape == (h, w, 4) and rad.dtype == f32
                same_bits(rad[..., :3], want, what)
                assert (rad[..., 3].view(np.uint32) == ONE).all(), what
                assert np.array_equal(img, want_img), f"{what}: {int((img != want_img).any(-1).sum())} pixels differ"
                assert rays == want_rays, f"{what}: rays {rays} vs {want_rays}"


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_image_equals_reference(gpu, name, waves):
    """trace_image at 8 spp: pixel seeding through the three engines, sample
    seeding through the persistent engine with shadow_split 1 / 0 and tie_defer
    0 / 1 -- the packed bytes and the ray count of the reference's samples."""
    c = _case(name)
    w, h, spp = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    with _scene(name, waves) as sc:
        _, want_img, want_rays = _radiance(name, tm.SEED_PIXEL, spp)
        for engine in (tm.ENGINE_WAVEFRONT, tm.ENGINE_MEGAKERNEL, tm.ENGINE_PERSISTENT):
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_PIXEL, engine=engine)
            what = f"{name} pixel seeding, engine {engine}, path_waves {waves}"
            assert np.array_equal(img, want_img), f"{what}: {int((img != want_img).any(-1).sum())} pixels differ"
            assert rays == want_rays, f"{what}: rays {rays} vs {want_rays}"
        _, want_img, want_rays = _radiance(name, tm.SEED_SAMPLE, spp)
        for split in (1, 0):
            for defer in (0, 1):
                sc.set_option("shadow_split", split)
                sc.set_option("tie_defer", defer)
                img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, engine=tm.ENGINE_PERSISTENT)
                st = sc.stats()
                used = int(sc.get_option("shadow_split_used"))
                what = f"{name} sample seeding, shadow_split {split}, tie_defer {defer}, path_waves {waves}"
                print(what, "-> split used", used, "tie_path", st.tie_path, "tie_queries", st.tie_queries,
                      "redo_samples", st.redo_samples, "octree_flat", st.octree_flat)
                # the routes are the ones meant (include/tmpt.h, shadow_split): grid has triangles flat on
                # octree planes, so it keeps the fused kernel and the octree answers its ties; elsewhere the
                # 5-wave kernels really run the split
                if name == "grid":
                    assert st.octree_flat > 0 and used == 0 and st.tie_queries > 0, what
                else:
                    assert st.octree_flat == 0, what
                    if not split:
                        assert used == 0, what
                    elif waves == 5:
                        assert used == 1, what
                assert np.array_equal(img, want_img), f"{what}: {int((img != want_img).any(-1).sum())} pixels differ"
                assert rays == want_rays, f"{what}: rays {rays} vs {want_rays}"


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_camera_rays_equal_reference(gpu, name, waves):
    """At 8 spp words [0:6] of every entry are the reference ray's bits and word
    [6] the RNG state after GetRay ([7], the flag word, has no counterpart)."""
    c = _case(name)
    fx, w, h, spp = c["fx"], c["w"], c["h"], c["spp"]
    with _scene(name, waves) as sc:
        got = sc.camera_rays(_camera(name), w, h, spp)
    assert got.shape == (h * w, spp, 8)
    want = np.concatenate([np.ascontiguousarray(fx["s_ray"]).view(np.uint32), fx["s_state_ray"][:, None]], 1)
    bad = np.argwhere(got[..., :7] != want.reshape(h * w, spp, 7))
    assert len(bad) == 0, f"{name}: {len(bad)} words differ, first (slot, sample, word) {bad[0]}"


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_aov_equals_reference(gpu, name, waves):
    """trace_aov at 1 and 8 spp with aov_group 1 and auto: normal, depth and hits
    are the sums over the reference's first hits in include/tmpt.h's order."""
    c = _case(name)
    w, h = c["w"], c["h"]
    cam = _camera(name)
    with _scene(name, waves) as sc:
        for spp in (1, 8):
            nrm, depth, hits = aov_sums(c["hit"], c["nrm"], c["t"], spp)
            for group in (1, 0):
                sc.set_option("aov_group", group)
                rec, rays = sc.trace_aov(cam, w, h, spp)
                what = f"{name} x{spp}, aov_group {group}, path_waves {waves}"
                assert rec.shape == (h, w)
                assert np.array_equal(rec["hits"], hits), f"{what}: hits differ at {np.argwhere(rec['hits'] != hits)[:4]}"
                same_bits(rec["normal"], nrm, what + " normal")
                same_bits(rec["depth"], depth, what + " depth")
                assert rays == w * h * spp + int(hits.sum()), what


@functools.lru_cache(maxsize=None)
def _adaptive(name):
    c = _case(name)
    return adaptive_expect(c["col"][tm.SEED_SAMPLE], c["rays"][tm.SEED_SAMPLE], SPP_MIN, SPP_STEP, TAU[name])


@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_adaptive_equals_reference(gpu, name, waves):
    """Cap 8, spp_min 2, spp_step 2: the spp map, the float tile, the bytes, the
    rays and pass_pixels of include/tmpt.h's contract over the reference's colours."""
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    want_n, want_rad, want_rays, want_pp = _adaptive(name)
    assert len(np.unique(want_n)) >= 3, np.unique(want_n, return_counts=True)
    with _scene(name, waves) as sc:
        rad, img, n_p, rays, info = sc.trace_adaptive(_camera(name), w, h, cap, SPP_MIN, SPP_STEP, TAU[name])
    what = f"{name} tau {TAU[name]}, path_waves {waves}"
    assert np.array_equal(n_p, want_n), f"{what}: spp map differs at {np.argwhere(n_p != want_n)[:4]}"
    same_bits(rad[..., :3], want_rad, what)
    assert (rad[..., 3].view(np.uint32) == ONE).all()
    assert np.array_equal(img, pack(want_rad)), what
    assert rays == want_rays, f"{what}: rays {rays} vs {want_rays}"
    assert info == {"passes": len(want_pp), "samples": int(want_n.sum()), "pass_pixels": want_pp}, what
