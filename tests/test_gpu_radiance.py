"""The float frame of a render (tmpt_render_radiance / Scene.trace_radiance):
bit for bit the CPU oracle's colour sums, and in every route of the persistent
engine the very frame of Scene.trace_image -- same bytes, same ray count, and
bytes that are the packed float tile.  No tolerances: floats compared as bits."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import toymeshpathtracer_amd as tm
from conftest import ROOT, data
from render_restate import pack, radiance_expect, same_bits as _same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")


@functools.lru_cache(maxsize=None)
def _load(name):
    return tm.load_scene(data(name))


def _scene(name, options=None, octree=True):
    tris, bmin, bmax = _load(name)
    return tm.Scene(tris, bounds=(bmin, bmax) if octree else None, options=options)


def _cam(name, w, h):
    _, bmin, bmax = _load(name)
    return tm.Camera.for_scene(bmin, bmax, w, h)


@functools.lru_cache(maxsize=None)
def _expect(name, w, h, spp, seed_mode, index=False):
    """(float32[h, w, 3] colour sum in sample order times 1/spp, rays) from the
    oracle's pieces: the seeds, the two jitter draws, get_ray, Scene.trace."""
    tris, bmin, bmax = _load(name)
    cam = tm.Camera.for_scene(bmin, bmax, w, h).as_array()
    osc = (oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX, bmin=bmin, bmax=bmax) if index else
           oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax))
    return radiance_expect(osc, cam, w, h, spp, seed_mode)


@pytest.mark.parametrize("seed", [tm.SEED_SAMPLE, tm.SEED_PIXEL], ids=["sample", "pixel"])
@pytest.mark.parametrize("name,w,h,spp,index", [("suzanne.obj", 32, 18, 4, False), ("cube.obj", 16, 9, 3, False),
                                                ("cube.obj", 16, 9, 3, True), ("teapot.obj", 24, 14, 2, False)])
def test_radiance_matches_oracle(gpu, name, w, h, spp, index, seed):
    want, want_rays = _expect(name, w, h, spp, seed, index)
    assert want.max() > 0.25 and want.min() >= 0  # the sky alone reaches 0.5 x its gradient
    with _scene(name, "tie_rule=index" if index else None) as sc:
        rad, img, rays = sc.trace_radiance(_cam(name, w, h), w, h, spp, seed_mode=seed)
    assert rad.shape == (h, w, 4) and rad.dtype == f32 and img.shape == (h, w, 4)
    _same_bits(rad[..., :3], want, f"{name} {w}x{h}x{spp}")
    assert (rad[..., 3].view(np.uint32) == f32(1).view(np.uint32)).all()
    assert rays == want_rays
    assert np.array_equal(img, pack(rad))


ROUTES = [
    # (id, seeding, scene options, set_option calls, octree, layout of the call)
    ("sample-default", tm.SEED_SAMPLE, None, {}, True, {}),
    ("sample-no-colour-buffer", tm.SEED_SAMPLE, None, {"sbuf_max": 1}, True, {}),
    ("sample-no-colour-buffer-4waves", tm.SEED_SAMPLE, None, {"sbuf_max": 1, "path_waves": 4}, True, {}),
    ("sample-no-colour-buffer-no-octree", tm.SEED_SAMPLE, None, {"sbuf_max": 1}, False, {}),
    ("sample-no-colour-buffer-no-octree-4waves", tm.SEED_SAMPLE, None, {"sbuf_max": 1, "path_waves": 4}, False, {}),
    ("sample-no-colour-buffer-soa", tm.SEED_SAMPLE, "layout=soa", {"sbuf_max": 1}, True, {}),
    ("sample-tie_defer-0", tm.SEED_SAMPLE, None, {"tie_defer": 0}, True, {}),
    ("sample-tie_defer-1", tm.SEED_SAMPLE, None, {"tie_defer": 1}, True, {}),
    ("sample-tie_defer-1-late", tm.SEED_SAMPLE, None, {"tie_defer": 1, "redo_inline": 0}, True, {}),
    ("sample-path_waves-4", tm.SEED_SAMPLE, None, {"path_waves": 4}, True, {}),
    ("sample-path_waves-5", tm.SEED_SAMPLE, None, {"path_waves": 5}, True, {}),
    ("sample-sharded", tm.SEED_SAMPLE, None, {}, True, dict(band_rows=1, num_shards=3, shard=1)),
    ("pixel-default", tm.SEED_PIXEL, None, {}, True, {}),
    ("pixel-no-pilot", tm.SEED_PIXEL, None, {"pilot": 0}, True, {}),
    ("pixel-chains-0", tm.SEED_PIXEL, None, {"pixel_chains": 0}, True, {}),
    ("pixel-chains-64", tm.SEED_PIXEL, None, {"pixel_chains": 64}, True, {}),
    ("pixel-path_waves-4", tm.SEED_PIXEL, None, {"path_waves": 4}, True, {}),
    ("pixel-path_waves-5", tm.SEED_PIXEL, None, {"path_waves": 5}, True, {}),
    ("pixel-no-octree", tm.SEED_PIXEL, None, {}, False, {}),
    ("pixel-sharded", tm.SEED_PIXEL, None, {}, True, dict(band_rows=1, num_shards=3, shard=1)),
]
STAT_FIELDS = ("extend_rays", "shadow_rays", "extend_launches", "iterations", "tie_queries", "root_misses",
               "crack_queries", "chain_pixels", "redo_samples", "redo_launches", "tie_path")


def _same_frame(sc, cam, w, h, spp, seed, kw):
    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=seed, **kw)
    st_img = sc.stats()
    rad, img_r, rays_r = sc.trace_radiance(cam, w, h, spp, seed_mode=seed, **kw)
    st_rad = sc.stats()
    again, rays_a = sc.trace_image(cam, w, h, spp, seed_mode=seed, **kw)  # and nothing stuck to the scene
    assert rays_r == rays == rays_a
    assert np.array_equal(img_r, img) and np.array_equal(again, img)
    assert np.array_equal(pack(rad), img)
    assert (rad[..., 3] == 1).all() and np.isfinite(rad).all() and rad[..., :3].max() > 0.25
    for f in STAT_FIELDS:
        assert getattr(st_rad, f) == getattr(st_img, f), f
    return st_rad


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_radiance_is_the_frame_of_trace_image(gpu, route):
    _, seed, options, sets, octree, kw = route
    w, h, spp = 64, 36, 8
    cam = _cam("suzanne.obj", w, h)
    with _scene("suzanne.obj", options, octree) as sc:
        for k, v in sets.items():
            sc.set_option(k, v)
        st = _same_frame(sc, cam, w, h, spp, seed, kw)
    print(route[0], {f: getattr(st, f) for f in STAT_FIELDS})
    if sets.get("pixel_chains"):
        assert st.chain_pixels > 0


@pytest.mark.parametrize("redo_inline", [1, 0])
def test_radiance_with_deferred_ties(gpu, sponza_path, redo_inline):
    """The stand-in sponza's camera stands inside the octree's root box, so
    tie_defer = 1 does defer (tie_path 2): dropped samples are traced again in
    the launch's tail (redo_inline 1) or by k_redo (0), and their colours reach
    the float sums through the colour buffer."""
    tris, bmin, bmax = tm.load_scene(sponza_path)
    w, h, spp = 160, 90, 8
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        sc.set_option("tie_defer", 1)
        sc.set_option("redo_inline", redo_inline)
        st = _same_frame(sc, cam, w, h, spp, tm.SEED_SAMPLE, {})
    print({f: getattr(st, f) for f in STAT_FIELDS})
    assert st.tie_path == 2 and st.redo_samples > 0
    if not redo_inline:
        assert st.redo_launches == 1


@pytest.mark.parametrize("seed", [tm.SEED_SAMPLE, tm.SEED_PIXEL], ids=["sample", "pixel"])
def test_radiance_48_spp(gpu, seed):
    w, h, spp = 64, 36, 48
    with _scene("suzanne.obj") as sc:
        _same_frame(sc, _cam("suzanne.obj", w, h), w, h, spp, seed, {})


def test_radiance_shards_assemble(gpu):
    w, h, spp, band, shards = 37, 11, 3, 2, 3
    cam = _cam("suzanne.obj", w, h)
    with _scene("suzanne.obj") as sc:
        full, img, rays = sc.trace_radiance(cam, w, h, spp)
        frame, total = np.zeros((h, w, 4), f32), 0
        for k in range(shards):
            tile, _, r = sc.trace_radiance(cam, w, h, spp, band_rows=band, shard=k, num_shards=shards)
            frame[tm.tile_row_to_y(w, h, band, k, shards)] = tile
            total += r
    assert frame.tobytes() == full.tobytes() and total == rays


@pytest.mark.parametrize("seed", [tm.SEED_SAMPLE, tm.SEED_PIXEL], ids=["sample", "pixel"])
def test_radiance_leaves_the_progressive_state_alone(gpu, seed):
    w, h, spp = 32, 18, 8
    cam = _cam("suzanne.obj", w, h)
    _, bmin, bmax = _load("suzanne.obj")
    other = tm.Camera.for_scene(bmin - f32(0.5), bmax + f32(0.25), w, h)
    with _scene("suzanne.obj") as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=seed)
        alone, _, _ = sc.trace_radiance(other, w, h, spp, seed_mode=seed)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=seed)
        done, _, r_a = next(passes)
        assert done == 3
        between, _, _ = sc.trace_radiance(other, w, h, spp, seed_mode=seed)  # between the two passes
        done, last, r_b = next(passes)
        assert done == spp
    assert np.array_equal(last, once) and r_a + r_b == rays
    assert between.tobytes() == alone.tobytes()


def test_radiance_argument_errors(gpu):
    w, h, spp = 16, 9, 2
    cam = _cam("cube.obj", w, h)._to_c()
    rad = np.zeros((h, w, 4), f32)
    rays = ctypes.c_uint64()

    def call(handle, desc, ptr):
        rc = tm._render_radiance(handle, ctypes.byref(cam), ctypes.byref(desc), ptr, None, ctypes.byref(rays))
        return rc, tm._last_error().decode()

    with _scene("cube.obj") as sc:
        p = rad.ctypes.data_as(ctypes.c_void_p)
        for desc, msg in ((tm._desc(w, h, spp, tm.SEED_ROW), "seed_mode"),
                          (tm._desc(w, h, spp, tm.SEED_SAMPLE, engine=tm.ENGINE_WAVEFRONT), "engine"),
                          (tm._desc(w, h, spp, tm.SEED_PIXEL, engine=tm.ENGINE_MEGAKERNEL), "engine"),
                          (tm._desc(w, h, spp, tm.SEED_SAMPLE, spp_begin=1), "spp_begin"),
                          (tm._desc(w, h, spp, tm.SEED_PIXEL, spp_count=1), "spp_begin"),
                          (tm._desc(w, h, spp, tm.SEED_SAMPLE, flags=tm.FLAG_COUNT_VISITS), "COUNT_VISITS"),
                          (tm._desc(0, h, spp, tm.SEED_SAMPLE), "width")):
            rc, err = call(sc._h, desc, p)
            assert rc == -22 and msg in err, (rc, err)
        rc, err = call(sc._h, tm._desc(w, h, spp, tm.SEED_SAMPLE), None)
        assert rc == -22 and "null" in err, (rc, err)
        rc, err = call(sc._h, tm._desc(w, h, spp, tm.SEED_SAMPLE), p)  # rgba8_out = NULL is fine
        assert rc == 0, err
        want, _, want_rays = sc.trace_radiance(_cam("cube.obj", w, h), w, h, spp)
    assert rays.value == want_rays and rad.tobytes() == want.tobytes()


@pytest.mark.parametrize("seed", [tm.SEED_SAMPLE, tm.SEED_PIXEL], ids=["sample", "pixel"])
def test_radiance_device_outputs(gpu, seed):
    """Both outputs as torch buffers filled on torch's current stream just
    before the call (wait_stream orders the render after the fills)."""
    import torch

    w, h, spp = 32, 18, 4
    cam = _cam("suzanne.obj", w, h)
    with _scene("suzanne.obj") as sc:
        rad, img, rays = sc.trace_radiance(cam, w, h, spp, seed_mode=seed)
        t32 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        assert t32.data_ptr() % 16 == 0
        t32.fill_(7.0)
        t8.fill_(7)
        a, b, rays_dev = sc.trace_radiance(cam, w, h, spp, seed_mode=seed, out=(t32.data_ptr(), t8.data_ptr()))
        got32, got8 = t32.cpu().numpy(), t8.cpu().numpy()
        t32.fill_(3.0)
        _, _, rays_f = sc.trace_radiance(cam, w, h, spp, seed_mode=seed, out=t32.data_ptr())  # float tile alone
        only32 = t32.cpu().numpy()
    assert a is None and b is None and rays_dev == rays == rays_f
    assert got32.tobytes() == rad.tobytes() and np.array_equal(got8, img)
    assert only32.tobytes() == rad.tobytes()


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        cam = tm.Camera.for_scene(bmin, bmax, 32, 18)
        for name, seed in (("sample", tm.SEED_SAMPLE), ("pixel", tm.SEED_PIXEL)):
            rad, img, rays = sc.trace_radiance(cam, 32, 18, 4, seed_mode=seed)
            out[name] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(), rays]
        sc.set_option("sbuf_max", 1)
        rad, img, rays = sc.trace_radiance(cam, 32, 18, 4)
        out["sums"] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(), rays]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_radiance_checked_build(gpu):
    """The checked library (device index tests compiled in) computes the same
    float frames and no check fails (no -30)."""
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
        cam = _cam("suzanne.obj", 32, 18)
        for name, seed in (("sample", tm.SEED_SAMPLE), ("pixel", tm.SEED_PIXEL)):
            rad, img, rays = sc.trace_radiance(cam, 32, 18, 4, seed_mode=seed)
            want[name] = [hashlib.sha256(rad.tobytes()).hexdigest(), hashlib.sha256(img.tobytes()).hexdigest(), rays]
        want["sums"] = want["sample"]
    assert got == want
