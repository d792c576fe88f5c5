"""Adaptive sampling on the GPU (tmpt_render_adaptive / Scene.trace_adaptive):
bit for bit the contract of include/tmpt.h restated over the CPU oracle
(adaptive_restate.py) -- the spp map, the float frame, the bytes, the ray count
and the passes -- and, per stopping count, the very pixels of
Scene.trace_radiance at that spp, in every route of the persistent engine.
No tolerances: floats compared as bits."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from adaptive_restate import CASES, CASE_IDS, adaptive_expect, camera, case_expect, load, scene_samples
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


# ---- 1. against the oracle
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_adaptive_matches_oracle(gpu, case):
    name, w, h, cap, spp_min, spp_step, tau, index = case
    want_n, want_rad, want_rays, want_pp = case_expect(case)
    with _scene(name, "tie_rule=index" if index else None) as sc:
        rad, img, n_p, rays, info = sc.trace_adaptive(camera(name, w, h), w, h, cap, spp_min, spp_step, tau)
        st = sc.stats()
    assert rad.shape == (h, w, 4) and rad.dtype == f32 and img.shape == (h, w, 4) and n_p.dtype == np.int32
    assert np.array_equal(n_p, want_n), np.argwhere(n_p != want_n)[:4]
    same_bits(rad[..., :3], want_rad, CASE_IDS[CASES.index(case)])
    assert (rad[..., 3].view(np.uint32) == ONE).all()
    assert np.array_equal(img, pack(rad))
    assert rays == want_rays
    assert info == {"passes": len(want_pp), "samples": int(want_n.sum()), "pass_pixels": want_pp}
    assert st.extend_rays + st.shadow_rays == rays and st.iterations == info["passes"]


# ---- 2. the ends of the range
def test_adaptive_ends_of_the_range(gpu):
    name, w, h, cap = "suzanne.obj", 32, 18, 16
    cam = camera(name, w, h)
    col, srays = scene_samples(name, w, h, cap)
    assert (adaptive_expect(col, srays, 4, 4, 0.0)[0] == cap).all()  # tau 0 on this frame: no pixel stops early
    with _scene(name) as sc:
        low = sc.trace_radiance(cam, w, h, 4)
        full = sc.trace_radiance(cam, w, h, cap)
        for kw, want, n, passes in ((dict(spp_min=4, spp_step=4, threshold=1.0), low, 4, 1),
                                    (dict(spp_min=4, spp_step=4, threshold=0.0), full, cap, 4),
                                    (dict(spp_min=cap, spp_step=4, threshold=0.02), full, cap, 1)):
            rad, img, n_p, rays, info = sc.trace_adaptive(cam, w, h, cap, **kw)
            assert (n_p == n).all(), kw
            assert rad.tobytes() == want[0].tobytes() and np.array_equal(img, want[1]) and rays == want[2], kw
            assert info == {"passes": passes, "samples": n * w * h, "pass_pixels": [w * h] * passes}, kw


# ---- 3. per-count identity on a frame with deferred ties
def test_adaptive_per_count_identity_with_deferred_ties(gpu, sponza_path):
    tris, bmin, bmax = tm.load_scene(sponza_path)
    w, h, cap = 160, 90, 16
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    res = {}
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        sc.set_option("redo_inline", 0)
        for defer in (0, 1):
            sc.set_option("tie_defer", defer)
            res[defer] = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02)
            st = sc.stats()
            print("tie_defer", defer, res[defer][4], "tie_queries", st.tie_queries, "redo_samples", st.redo_samples,
                  "tie_path", st.tie_path)
            assert st.tie_queries > 0
            if defer:
                assert st.tie_path == 2 and st.redo_samples > 0
        # the deferring list kernels at 4 waves and without the camera pre-pass
        for key, value, back in (("path_waves", 4, 0), ("cam_pre", 0, -1)):
            sc.set_option(key, value)
            other = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02)
            assert sc.stats().tie_path == 2
            _same(other, res[1], f"{key} {value}, deferred")
            sc.set_option(key, back)
        sc.set_option("tie_defer", -1)
        rad, img, n_p, rays, info = res[1]
        counts = [int(n) for n in np.unique(n_p)]
        assert len(counts) >= 3, counts
        for n in counts:
            u_rad, u_img, _ = sc.trace_radiance(cam, w, h, n)
            m = n_p == n
            assert rad[m].tobytes() == u_rad[m].tobytes(), n
            assert np.array_equal(img[m], u_img[m]), n
    _same(res[0], res[1], "tie_defer 0 / 1")


# ---- 4. routes
ROUTES = [
    ("path_waves-4", None, {"path_waves": 4}, True),
    ("path_waves-5", None, {"path_waves": 5}, True),
    ("cam_pre-0", None, {"cam_pre": 0}, True),
    ("cam_pre-1", None, {"cam_pre": 1}, True),
    ("tie_defer-0", None, {"tie_defer": 0}, True),
    ("tie_defer-1", None, {"tie_defer": 1}, True),
    ("sample_block-1", None, {"sample_block": 1}, True),
    ("sample_block-2", None, {"sample_block": 2}, True),
    ("sample_block-8", None, {"sample_block": 8}, True),
    ("sample_tail-0", None, {"sample_tail": 0}, True),
    ("layout-soa", "layout=soa", {}, True),
    ("no-octree", None, {}, False),
    # beyond the single options: so that every LIST line of kPathVariants runs (the deferring
    # ones in test_adaptive_per_count_identity_with_deferred_ties)
    ("path_waves-4-tie_defer-0", None, {"path_waves": 4, "tie_defer": 0}, True),
    ("no-octree-path_waves-4", None, {"path_waves": 4}, False),
    ("no-octree-cam_pre-0", None, {"cam_pre": 0}, False),
]


@pytest.fixture(scope="module")
def default_route(gpu):
    name, w, h = "suzanne.obj", 64, 36
    with _scene(name) as sc:
        res = sc.trace_adaptive(camera(name, w, h), w, h, 20, 4, 8, 0.02)
    counts = {int(n): int((res[2] == n).sum()) for n in np.unique(res[2])}
    assert set(counts) == {4, 12, 20} and min(counts.values()) >= 3, counts
    return res


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_adaptive_routes(gpu, default_route, route):
    rid, options, sets, octree = route
    name, w, h = "suzanne.obj", 64, 36
    with _scene(name, options, octree) as sc:
        for k, v in sets.items():
            sc.set_option(k, v)
        res = sc.trace_adaptive(camera(name, w, h), w, h, 20, 4, 8, 0.02)
    _same(res, default_route, rid)


# ---- 5. shards assemble
def test_adaptive_shards_assemble(gpu):
    name, w, h, cap, band, shards = "suzanne.obj", 37, 11, 16, 2, 3
    cam = camera(name, w, h)
    with _scene(name) as sc:
        rad, img, n_p, rays, info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02)
        f_rad, f_img, f_n = np.zeros_like(rad), np.zeros_like(img), np.zeros_like(n_p)
        total, samples = 0, 0
        for k in range(shards):
            t_rad, t_img, t_n, r, t_info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, band_rows=band, shard=k,
                                                             num_shards=shards)
            rows = tm.tile_row_to_y(w, h, band, k, shards)
            f_rad[rows], f_img[rows], f_n[rows] = t_rad, t_img, t_n
            total += r
            samples += t_info["samples"]
    assert len(np.unique(n_p)) >= 3
    assert f_rad.tobytes() == rad.tobytes() and np.array_equal(f_img, img) and np.array_equal(f_n, n_p)
    assert total == rays and samples == info["samples"] == int(n_p.sum())


# ---- 6. nothing sticks
def test_adaptive_leaves_the_scene_as_it_was(gpu):
    name, w, h, spp = "suzanne.obj", 32, 18, 8
    cam = camera(name, w, h)
    _, bmin, bmax = load(name)
    other = tm.Camera.for_scene(bmin - f32(0.5), bmax + f32(0.25), w, h)
    with _scene(name) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        alone = sc.trace_adaptive(other, w, h, 16, 4, 4, 0.02)
        again, rays_a = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        assert np.array_equal(again, once) and rays_a == rays
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        assert done == 3
        between = sc.trace_adaptive(other, w, h, 16, 4, 4, 0.02)  # between the two passes
        done, last, r_b = next(passes)
        assert done == spp
    assert np.array_equal(last, once) and r_a + r_b == rays
    _same(between, alone, "between the passes")


# ---- 7. argument errors
def test_adaptive_argument_errors(gpu):
    w, h, cap = 16, 9, 8
    cam = camera("cube.obj", w, h)._to_c()
    rad, img, cnt = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), np.uint8), np.zeros((h, w), np.int32)
    rays = ctypes.c_uint64()
    fn = tm._lib.tmpt_render_adaptive
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def call(handle, desc, ad, outs=(True, True, True)):
        a = tm._AdaptiveDesc()
        a.spp_min, a.spp_step, a.threshold = ad
        ptr = [arr.ctypes.data if on else None for arr, on in zip((rad, img, cnt), outs)]
        rc = fn(handle, ctypes.byref(cam), ctypes.byref(desc), ctypes.byref(a), ptr[0], ptr[1], ptr[2], None,
                ctypes.byref(rays))
        return rc, tm._last_error().decode()

    ok = tm._desc(w, h, cap, tm.SEED_SAMPLE)
    with _scene("cube.obj") as sc:
        for desc, ad, msg in ((tm._desc(w, h, cap, tm.SEED_ROW), (4, 4, 0.02), "seed_mode"),
                              (tm._desc(w, h, cap, tm.SEED_PIXEL), (4, 4, 0.02), "seed_mode"),
                              (tm._desc(w, h, cap, tm.SEED_SAMPLE, engine=tm.ENGINE_WAVEFRONT), (4, 4, 0.02), "engine"),
                              (tm._desc(w, h, cap, tm.SEED_SAMPLE, engine=tm.ENGINE_MEGAKERNEL), (4, 4, 0.02), "engine"),
                              (tm._desc(w, h, cap, tm.SEED_SAMPLE, spp_begin=1), (4, 4, 0.02), "spp_begin"),
                              (tm._desc(w, h, cap, tm.SEED_SAMPLE, spp_count=1), (4, 4, 0.02), "spp_begin"),
                              (tm._desc(w, h, cap, tm.SEED_SAMPLE, flags=tm.FLAG_COUNT_VISITS), (4, 4, 0.02),
                               "COUNT_VISITS"),
                              (ok, (1, 4, 0.02), "spp_min"), (ok, (cap + 1, 4, 0.02), "spp_min"),
                              (ok, (-2, 4, 0.02), "spp_min"), (ok, (4, -1, 0.02), "spp_step"),
                              (ok, (4, 4, float("nan")), "threshold"), (ok, (4, 4, float("inf")), "threshold"),
                              (tm._desc(w, h, 1, tm.SEED_SAMPLE), (0, 0, -1.0), "spp_min"),
                              (tm._desc(w, h, 200, tm.SEED_SAMPLE), (2, 1, 0.02), "64 passes")):
            rc, err = call(sc._h, desc, ad)
            assert rc == -22 and msg in err, (msg, rc, err)
        rc, err = call(sc._h, ok, (4, 4, 0.02), (False, False, False))
        assert rc == -22 and "no output" in err, (rc, err)
        want = sc.trace_adaptive(camera("cube.obj", w, h), w, h, cap, 4, 4, 0.02)
        for outs in ((True, False, False), (False, True, False), (False, False, True)):  # any single output alone
            rad[:], img[:], cnt[:] = 0, 0, 0
            rc, err = call(sc._h, ok, (4, 4, 0.02), outs)
            assert rc == 0, err
            assert rays.value == want[3]
            got = (rad, img, cnt)
            for i, on in enumerate(outs):
                assert got[i].tobytes() == want[i].tobytes() if on else not got[i].any(), (outs, i)
        rc, err = call(sc._h, ok, (0, 0, -1.0))  # all defaults
        assert rc == 0, err
        sc.set_option("sbuf_max", 1)
        rc, err = call(sc._h, ok, (4, 4, 0.02))
        assert rc == -12 and "colour buffer" in err, (rc, err)


# ---- 8. device outputs
def test_adaptive_device_outputs(gpu):
    """All three outputs as torch buffers filled on torch's current stream just
    before the call (wait_stream orders the passes after the fills)."""
    import torch

    name, w, h, cap = "suzanne.obj", 32, 18, 16
    cam = camera(name, w, h)
    with _scene(name) as sc:
        want = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02)
        t32 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        tn = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        assert t32.data_ptr() % 16 == 0
        t32.fill_(7.0)
        t8.fill_(7)
        tn.fill_(7)
        a, b, c, rays, info = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02,
                                                out=(t32.data_ptr(), t8.data_ptr(), tn.data_ptr()))
        got = (t32.cpu().numpy(), t8.cpu().numpy(), tn.cpu().numpy())
        tn.fill_(3)
        _, _, _, rays_n, _ = sc.trace_adaptive(cam, w, h, cap, 4, 4, 0.02, out=(None, None, tn.data_ptr()))
        only_n = tn.cpu().numpy()
    assert a is None and b is None and c is None and rays == rays_n == want[3] and info == want[4]
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(only_n, want[2])


# ---- 9. the checked build
CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        cam = tm.Camera.for_scene(bmin, bmax, 32, 18)
        for name, defer in (("auto", -1), ("deferred", 1)):
            sc.set_option("tie_defer", defer)
            rad, img, n_p, rays, info = sc.trace_adaptive(cam, 32, 18, 16, 4, 4, 0.02)
            out[name] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(),
                         hashlib.sha256(n_p.tobytes()).hexdigest(), rays, info]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_adaptive_checked_build(gpu):
    """The checked library (device index tests compiled in) computes the same
    adaptive frames and no check fails (no -30)."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    assert "device index check failed" not in r.stderr
    with _scene("suzanne.obj") as sc:
        rad, img, n_p, rays, info = sc.trace_adaptive(camera("suzanne.obj", 32, 18), 32, 18, 16, 4, 4, 0.02)
    want = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(),
            hashlib.sha256(n_p.tobytes()).hexdigest(), rays, info]
    assert got == {"auto": want, "deferred": want}
