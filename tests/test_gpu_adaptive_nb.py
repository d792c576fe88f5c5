"""Adaptive sampling's neighbourhood rule on the GPU (tmpt_adaptive_desc.radius /
Scene.trace_adaptive(radius=...)): bit for bit the rule of include/tmpt.h
restated over the CPU oracle (adaptive_nb_restate.py) -- the spp map, the float
frame, the bytes, the ray count and the passes -- over frames whose rows take one
word, two words with a tail and a radius beyond the band; shards against the
whole frame; per-count identity; every route of the persistent engine.
No tolerances: floats compared as bits.  test_adaptive_nb.py shows that each
case here moves pixels off their radius-0 counts."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from adaptive_nb_restate import NB_CASES, NB_IDS, counts_of, nb_case_expect
from adaptive_restate import camera, load
from conftest import ROOT, data
from render_restate import pack, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")
ONE = f32(1).view(np.uint32)


def _scene(name, options=None, octree=True):
    tris, bmin, bmax = load(name)
    return tm.Scene(tris, bounds=(bmin, bmax) if octree else None, options=options)


def _same(a, b, what=""):
    """Two results of trace_adaptive: every output and the ray count; the passes too."""
    assert np.array_equal(a[2], b[2]), f"{what}: spp maps differ at {np.argwhere(a[2] != b[2])[:4]}"
    assert a[0].tobytes() == b[0].tobytes(), f"{what}: radiance differs"
    assert np.array_equal(a[1], b[1]), f"{what}: bytes differ"
    assert a[3] == b[3], f"{what}: rays {a[3]} vs {b[3]}"
    assert a[4] == b[4], f"{what}: info {a[4]} vs {b[4]}"


def _against(res, want, what):
    """A result of trace_adaptive over the whole frame against the restatement's."""
    rad, img, n_p, rays, info = res
    want_n, want_rad, want_rays, want_pp = want
    assert rad.dtype == f32 and n_p.dtype == np.int32 and rad.shape == want_n.shape + (4,)
    assert np.array_equal(n_p, want_n), (what, np.argwhere(n_p != want_n)[:6])
    same_bits(rad[..., :3], want_rad, what)
    assert (rad[..., 3].view(np.uint32) == ONE).all()
    assert np.array_equal(img, pack(rad))
    assert rays == want_rays
    assert info == {"passes": len(want_pp), "samples": int(want_n.sum()), "pass_pixels": want_pp}


# ---- 1. against the oracle
@pytest.mark.parametrize("case", NB_CASES, ids=NB_IDS)
def test_adaptive_nb_matches_oracle(gpu, case):
    name, w, h, cap, spp_min, spp_step, tau, index, radius, band_rows = case
    with _scene(name, "tie_rule=index" if index else None) as sc:
        res = sc.trace_adaptive(camera(name, w, h), w, h, cap, spp_min, spp_step, tau, band_rows=band_rows,
                                radius=radius)
        st = sc.stats()
    _against(res, nb_case_expect(case), NB_IDS[NB_CASES.index(case)])
    assert st.extend_rays + st.shadow_rays == res[3] and st.iterations == res[4]["passes"]


# ---- 2. shards and bands
def test_adaptive_nb_shards_assemble(gpu):
    name, w, h, cap, band, shards, r = "suzanne.obj", 37, 11, 16, 3, 3, 2
    cam = camera(name, w, h)
    banded = next(c for c in NB_CASES if c[1:4] == (w, h, cap) and c[8:] == (r, band))
    whole = next(c for c in NB_CASES if c[1:4] == (w, h, cap) and c[8:] == (r, 0))
    with _scene(name) as sc:
        one = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band, radius=r)
        rad, img, n_p, rays, info = one
        f_rad, f_img, f_n = np.zeros_like(rad), np.zeros_like(img), np.zeros_like(n_p)
        total, samples, pass_pixels = 0, 0, [0] * info["passes"]
        for k in range(shards):
            t_rad, t_img, t_n, t_rays, t_info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band, shard=k,
                                                                  num_shards=shards, radius=r)
            rows = tm.tile_row_to_y(w, h, band, k, shards)
            f_rad[rows], f_img[rows], f_n[rows] = t_rad, t_img, t_n
            total += t_rays
            samples += t_info["samples"]
            for i, v in enumerate(t_info["pass_pixels"]):
                pass_pixels[i] += v
        unbanded = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, radius=r)
    _against(one, nb_case_expect(banded), "band_rows 3, one shard")
    assert info["pass_pixels"] == [407, 236, 149, 127] and rays == 9784
    assert f_rad.tobytes() == rad.tobytes() and np.array_equal(f_img, img) and np.array_equal(f_n, n_p)
    assert total == rays and samples == info["samples"] == int(n_p.sum()) and pass_pixels == info["pass_pixels"]
    _against(unbanded, nb_case_expect(whole), "band_rows 0")
    assert unbanded[4]["pass_pixels"] == [407, 273, 166, 147] and unbanded[3] == 10234
    assert int((unbanded[2] != n_p).sum()) == 50  # the result depends on band_rows


def test_adaptive_nb_one_row_bands_reach_sideways_only(gpu):
    """band_rows = 1 (the multi-GPU dealing): the tiles of two shards assemble
    into the restatement's frame, whose neighbourhoods are horizontal."""
    name, w, h, cap, r = "suzanne.obj", 37, 11, 16, 2
    cam = camera(name, w, h)
    case = next(c for c in NB_CASES if c[1:4] == (w, h, cap) and c[8:] == (r, 1))
    want_n = nb_case_expect(case)[0]
    assert counts_of(want_n) == {4: 226, 8: 71, 12: 11, 16: 99}
    f_n = np.zeros_like(want_n)
    with _scene(name) as sc:
        for k in range(2):
            t_n = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=1, shard=k, num_shards=2, radius=r)[2]
            f_n[tm.tile_row_to_y(w, h, 1, k, 2)] = t_n
    assert np.array_equal(f_n, want_n)


# ---- 3. per-count identity
def test_adaptive_nb_per_count_identity(gpu):
    name, w, h, cap, r = "suzanne.obj", 100, 28, 12, 2
    cam = camera(name, w, h)
    with _scene(name) as sc:
        rad, img, n_p, rays, info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, radius=r)
        counts = [int(n) for n in np.unique(n_p)]
        assert counts == [4, 8, 12]
        for n in counts:
            u_rad, u_img, _ = sc.trace_radiance(cam, w, h, n)
            m = n_p == n
            assert rad[m].tobytes() == u_rad[m].tobytes(), n
            assert np.array_equal(img[m], u_img[m]), n


# ---- 4. routes
ROUTES = [
    ("path_waves-4", None, {"path_waves": 4}, True),
    ("path_waves-5", None, {"path_waves": 5}, True),
    ("cam_pre-0", None, {"cam_pre": 0}, True),
    ("tie_defer-0", None, {"tie_defer": 0}, True),
    ("tie_defer-1", None, {"tie_defer": 1}, True),
    ("sample_block-1", None, {"sample_block": 1}, True),
    ("layout-soa", "layout=soa", {}, True),
    ("no-octree", None, {}, False),
]
ROUTE_ARGS = ("suzanne.obj", 64, 36, 20, 4, 8, 0.02)


@pytest.fixture(scope="module")
def default_route(gpu):
    name, w, h, cap, spp_min, spp_step, tau = ROUTE_ARGS
    with _scene(name) as sc:
        res = sc.trace_adaptive(camera(name, w, h), w, h, cap, spp_min, spp_step, tau, radius=1)
        own = sc.trace_adaptive(camera(name, w, h), w, h, cap, spp_min, spp_step, tau)
    counts = counts_of(res[2])
    assert set(counts) == {4, 12, 20} and min(counts.values()) >= 3, counts
    moved = int((res[2] != own[2]).sum())
    assert (res[2] >= own[2]).all() and 10 * moved >= res[2].size, moved  # the rule decides pixels here
    return res


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_adaptive_nb_routes(gpu, default_route, route):
    rid, options, sets, octree = route
    name, w, h, cap, spp_min, spp_step, tau = ROUTE_ARGS
    with _scene(name, options, octree) as sc:
        for k, v in sets.items():
            sc.set_option(k, v)
        res = sc.trace_adaptive(camera(name, w, h), w, h, cap, spp_min, spp_step, tau, radius=1)
    _same(res, default_route, rid)


# ---- 5. radius 0 and the range
def test_adaptive_nb_radius_zero_is_the_call_without_it(gpu):
    name, w, h, cap = "suzanne.obj", 37, 11, 16
    cam = camera(name, w, h)
    with _scene(name) as sc:
        for band in (0, 3):
            plain = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band)
            nb = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band, radius=1)  # the planes allocated
            zero = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band, radius=0)
            _same(zero, plain, f"radius 0, band_rows {band}")
            assert not np.array_equal(nb[2], plain[2])


def test_adaptive_nb_radius_out_of_range(gpu):
    name, w, h, cap = "cube.obj", 16, 9, 8
    cam = camera(name, w, h)
    with _scene(name) as sc:
        for radius in (-1, 9):
            with pytest.raises(tm.TmptError) as e:
                sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, radius=radius)
            assert "radius" in str(e.value), str(e.value)
        # and through the C ABI: -22
        fn = tm._lib.tmpt_render_adaptive
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 9
        cnt = np.zeros((h, w), np.int32)
        desc, c_cam = tm._desc(w, h, cap, tm.SEED_SAMPLE), cam._to_c()
        for radius, want in ((-1, -22), (9, -22), (8, 0), (0, 0)):
            ad = tm._AdaptiveDesc()
            ad.spp_min, ad.spp_step, ad.threshold, ad.radius = 4, 4, 0.02, radius
            rc = fn(sc._h, ctypes.byref(c_cam), ctypes.byref(desc), ctypes.byref(ad), None, None, cnt.ctypes.data, None,
                    None)
            assert rc == want, (radius, rc, tm._last_error().decode())
            assert rc == 0 or "radius" in tm._last_error().decode()


# ---- 6. device outputs
def test_adaptive_nb_device_outputs(gpu):
    """All three outputs as torch buffers filled on torch's current stream just
    before the call (wait_stream orders the passes after the fills)."""
    import torch

    name, w, h, cap = "suzanne.obj", 32, 18, 16
    cam = camera(name, w, h)
    with _scene(name) as sc:
        want = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, radius=1)
        t32 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        tn = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        assert t32.data_ptr() % 16 == 0
        t32.fill_(7.0)
        t8.fill_(7)
        tn.fill_(7)
        a, b, c, rays, info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02,
                                                out=(t32.data_ptr(), t8.data_ptr(), tn.data_ptr()), radius=1)
        got = (t32.cpu().numpy(), t8.cpu().numpy(), tn.cpu().numpy())
    _against(want, nb_case_expect(NB_CASES[0]), "host outputs")
    assert a is None and b is None and c is None and rays == want[3] and info == want[4]
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- 7. the checked build
CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        cam = tm.Camera.for_scene(bmin, bmax, 37, 11)
        for name, band in (("whole", 0), ("banded", 3)):
            rad, img, n_p, rays, info = sc.trace_adaptive(cam, 37, 11, 16, 4, 4, 0.02, band_rows=band, radius=2)
            out[name] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(),
                         hashlib.sha256(n_p.tobytes()).hexdigest(), rays, info]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_adaptive_nb_checked_build(gpu):
    """The checked library (device index tests compiled in) computes the same
    frames under the neighbourhood rule and no check fails (no -30)."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    assert "device index check failed" not in r.stderr
    want = {}
    with _scene("suzanne.obj") as sc:
        for name, band in (("whole", 0), ("banded", 3)):
            rad, img, n_p, rays, info = sc.trace_adaptive(camera("suzanne.obj", 37, 11), 37, 11, 16, 4, 4, 0.02,
                                                          band_rows=band, radius=2)
            want[name] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(),
                          hashlib.sha256(n_p.tobytes()).hexdigest(), rays, info]
    assert got == want and want["whole"] != want["banded"]


# ---- 8. nothing sticks
def test_adaptive_nb_between_two_progressive_passes(gpu):
    name, w, h, spp = "suzanne.obj", 32, 18, 8
    cam = camera(name, w, h)
    with _scene(name) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        alone = sc.trace_adaptive(cam, w, h, 16, 4, 4, 0.02, radius=1)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        assert done == 3
        between = sc.trace_adaptive(cam, w, h, 16, 4, 4, 0.02, radius=1)  # between the two passes
        done, last, r_b = next(passes)
        assert done == spp
    assert np.array_equal(last, once) and r_a + r_b == rays
    _same(between, alone, "between the passes")
    _against(alone, nb_case_expect(NB_CASES[0]), "alone")
