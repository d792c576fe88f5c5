"""tmpt_denoise_moments (Scene.denoise_moments) on the device against the numpy
float32 restatement of include/tmpt.h (noise_aware_restate.np_denoise_moments),
bit for bit: synthetic frames with every case the moments plane knows, real
frames, the temporal pipeline, the identity with tmpt_denoise at a huge shrink,
and the quality the filter is there for.  Floats are compared as bits."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_refit_restate as F
import temporal_restate as T
import toymeshpathtracer_amd as tm
from conftest import ROOT, data
from noise_aware_restate import (SHRINK_DEFAULT, build_digests, check_synthetic_moments, np_denoise_moments,
                                 synthetic_moments, v0_expect)
from test_gpu_denoise import CHECK_LIB, _any_scene, _bits_equal, _rmse, pack, synthetic

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(1, 1), (5, 3), (37, 23), (130, 9)]


@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_frames_bit_for_bit(gpu, w, h):
    rad, aov, spp = synthetic(w, h)
    mom = synthetic_moments(w, h)
    if w * h > 8:
        check_synthetic_moments(mom)
        cov = aov["hits"] > 0
        assert cov.any() and not cov.all()
    with _any_scene() as sc:
        for levels in range(1, 7):
            for shrink in (0.5, 4.0, 64.0):
                want = np_denoise_moments(rad, aov, mom, spp, shrink, levels)
                for lds in (0, 1):
                    sc.set_option("denoise_lds", lds)
                    got, img = sc.denoise_moments(rad, aov, mom, spp, shrink, levels=levels)
                    _bits_equal(got, want, f"{w}x{h} levels={levels} shrink={shrink} denoise_lds={lds}")
                    assert np.array_equal(img, pack(want))
        sc.set_option("denoise_lds", -1)
        # the defaults by their 0 / -1 values, and spelled out
        got, img = sc.denoise_moments(rad, aov, mom, spp)
        assert SHRINK_DEFAULT == f32(2.0)
        _bits_equal(got, np_denoise_moments(rad, aov, mom, spp, 2.0, 5, 5, f32(1) / f32(h), f32(0.05)),
                    "defaults spelled out")
        # other sigmas, and the filter in place
        for levels in (1, 2, 5):
            want = np_denoise_moments(rad, aov, mom, spp, 2.0, levels, 3, 0.05, 0.3)
            buf = rad.copy()
            got, img = sc.denoise_moments(buf, aov, mom, spp, 2.0, levels=levels, normal_exp=3, sigma_depth=0.05,
                                          sigma_direct=0.3, out=buf)
            assert got is buf
            _bits_equal(buf, want, f"in place, levels={levels}")
            assert np.array_equal(img, pack(want))
    assert (want[..., 3].view(np.uint32) == rad[..., 3].view(np.uint32)).all()  # .w passes through


@pytest.mark.parametrize("w,h", SIZES)
def test_huge_shrink_is_the_plain_filter(gpu, w, h):
    """shrink = 3e38 on a plane with v_0 > 0 everywhere: every gain is 0, the output is denoise's."""
    rad, aov, spp = synthetic(w, h)
    mom = synthetic_moments(w, h, positive=True)
    assert (v0_expect(mom) > 0).all() and (rad > 0).all() and np.isfinite(rad).all()
    with _any_scene() as sc:
        for levels in range(1, 7):
            for lds in (0, 1):
                sc.set_option("denoise_lds", lds)
                want, want8 = sc.denoise(rad, aov, spp, levels=levels)
                got, got8 = sc.denoise_moments(rad, aov, mom, spp, 3e38, levels=levels)
                _bits_equal(got, want, f"{w}x{h} levels={levels} denoise_lds={lds}")
                assert np.array_equal(got8, want8)


@functools.lru_cache(maxsize=None)
def _frame(name, w, h, spp):
    """(radiance, moments, aov) of a uniform frame at the reference's camera placement."""
    tris, bmin, bmax = tm.load_scene(data(name))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, mom, _, _, _, _ = sc.trace_moments(cam, w, h, spp)
        aov, _ = sc.trace_aov(cam, w, h, spp)
    return rad, mom, aov


@functools.lru_cache(maxsize=None)
def _truth(name, w, h):
    tris, bmin, bmax = tm.load_scene(data(name))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        return sc.trace_radiance(cam, w, h, 512)[0]


@pytest.mark.parametrize("name,w,h", [("suzanne.obj", 64, 36), ("cube.obj", 32, 18)])
def test_real_frame_bit_for_bit(gpu, name, w, h):
    spp = 4
    rad, mom, aov = _frame(name, w, h, spp)
    cov = aov["hits"] > 0
    assert cov.any() and not cov.all()
    want = np_denoise_moments(rad, aov, mom, spp)
    with _any_scene() as sc:
        for lds in (0, 1, -1):
            sc.set_option("denoise_lds", lds)
            got, img = sc.denoise_moments(rad, aov, mom, spp)
            _bits_equal(got, want, f"{name} denoise_lds={lds}")
            assert np.array_equal(img, pack(want))
        plain, _ = sc.denoise(rad, aov, spp)
    assert not np.array_equal(want[..., :3], plain[..., :3])
    assert not np.array_equal(want[..., :3], rad[..., :3])


def test_temporal_pipeline_bit_for_bit(gpu):
    """Two frames of a refit twist at 32 x 18: colour and moments go through temporal, then the filter."""
    w, h, spp = 32, 18, 2
    rest, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    now = F.twist(rest, 10.0)
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(rest) as sc:
        rad0, mom0 = sc.trace_moments(cam, w, h, spp)[:2]
        mot0, _ = sc.trace_motion(cam, cam, w, h)
        sc.update(now, "refit")
        sc.set_option("sample_base", spp)
        rad1, mom1 = sc.trace_moments(cam, w, h, spp)[:2]
        mot1, _ = sc.trace_motion(cam, cam, w, h, rest)
        aov1, _ = sc.trace_aov(cam, w, h, spp)
        acc, _ = sc.temporal(rad1, mot1, mot0, rad0)
        macc, _ = sc.temporal(mom1, mot1, mot0, mom0)
        got, img = sc.denoise_moments(acc, aov1, macc, spp)
    want_acc, want_macc = T.blend(rad1, mot1, mot0, rad0), T.blend(mom1, mot1, mot0, mom0)
    assert (want_macc[..., 3] == 2).any() and (want_macc[..., 3] == 1).any()
    _bits_equal(acc, want_acc, "accumulated colour")
    _bits_equal(macc, want_macc, "accumulated moments")
    want = np_denoise_moments(want_acc, aov1, want_macc, spp)
    _bits_equal(got, want, "pipeline")
    assert np.array_equal(img, pack(want))


@pytest.mark.parametrize("name", ["suzanne.obj", "teapot.obj"])
def test_quality(gpu, name):
    """RMSE over r, g, b against the 512-spp frame, shrink 4.0, 5 levels, 64 x 36.
    At 4 spp the new filter beats the unfiltered frame (on the CPU restatement
    0.77 - 0.83 of it); at 32 spp it beats the plain filter (0.98 - 1.01 of the
    unfiltered frame against the plain filter's 1.17 - 1.21)."""
    w, h = 64, 36
    truth = _truth(name, w, h)
    with _any_scene() as sc:
        for spp in (4, 32):
            rad, mom, aov = _frame(name, w, h, spp)
            new, _ = sc.denoise_moments(rad, aov, mom, spp, shrink=4.0, levels=5)
            plain, _ = sc.denoise(rad, aov, spp, levels=5)
            e_raw, e_plain, e_new = _rmse(rad, truth), _rmse(plain, truth), _rmse(new, truth)
            print(f"{name} {w}x{h} {spp} spp: E_unfiltered = {e_raw:.5f}  E_plain-filtered = {e_plain:.5f}  "
                  f"E_new = {e_new:.5f}  (new / unfiltered {e_new / e_raw:.3f}, plain / unfiltered {e_plain / e_raw:.3f})")
            if spp == 4:
                assert e_new < e_raw
            else:
                assert e_new < e_plain


def test_device_pointers(gpu):
    import torch

    w, h, spp = 64, 36, 4
    rad, mom, aov = _frame("suzanne.obj", w, h, spp)
    with _any_scene() as sc:
        want, want8 = sc.denoise_moments(rad, aov, mom, spp)
        t_in = torch.from_numpy(rad).to("cuda:0")
        t_mom = torch.from_numpy(mom).to("cuda:0")
        t_aov = torch.from_numpy(aov.view(np.uint8).reshape(h, w, 32).copy()).to("cuda:0")
        t_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t_8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        size = dict(width=w, height=h)
        ptrs = (t_in.data_ptr(), t_aov.data_ptr(), t_mom.data_ptr())
        assert sc.denoise_moments(*ptrs, spp, out=(t_out.data_ptr(), t_8.data_ptr()), **size) == (None, None)
        got, got8 = t_out.cpu().numpy(), t_8.cpu().numpy()
        assert t_in.cpu().numpy().tobytes() == rad.tobytes() and t_mom.cpu().numpy().tobytes() == mom.tobytes()
        with pytest.raises(tm.TmptError, match="aligned"):
            sc.denoise_moments(ptrs[0], ptrs[1], ptrs[2] + 8, spp, out=(t_out.data_ptr(), None), **size)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(tm.TmptError, match="shrink"):
                sc.denoise_moments(*ptrs, spp, shrink=bad, out=(t_out.data_ptr(), None), **size)
        sc.denoise_moments(*ptrs, spp, out=(t_in.data_ptr(), None), **size)  # in place
        inplace = t_in.cpu().numpy()
    assert got.tobytes() == want.tobytes() and np.array_equal(got8, want8) and inplace.tobytes() == want.tobytes()


def test_cli_shrink_png(gpu, tmp_path):
    """--denoise OUT.png --shrink K on the plain frame and on an --adaptive frame; without --shrink nothing changes."""
    from PIL import Image

    w, h, spp = 32, 18, 4
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    load = lambda p: np.asarray(Image.open(p).convert("RGBA"))[::-1]  # flipped on write
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        aov, _ = sc.trace_aov(cam, w, h, spp)
        rad, mom = sc.trace_moments(cam, w, h, spp)[:2]
        _, want_uniform = sc.denoise_moments(rad, aov, mom, spp, shrink=2.0)
        _, want_default = sc.denoise_moments(rad, aov, mom, spp)
        _, want_plain = sc.denoise(rad, aov, spp)
        rad, mom = sc.trace_moments(cam, w, h, spp, 2, 1, 0.02)[:2]
        _, want_adaptive = sc.denoise_moments(rad, aov, mom, spp, shrink=2.0)
    base = [cli, str(w), str(h), str(spp), data("suzanne.obj"), "--seed", "sample", "--out", str(tmp_path / "frame.png")]
    for extra, want in ((["--shrink", "2"], want_uniform), (["--shrink", "0"], want_default), ([], want_plain),
                        (["--shrink", "2", "--adaptive", "0.02,2,1"], want_adaptive)):
        out = str(tmp_path / "den.png")
        r = subprocess.run(base + ["--denoise", out] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("noise-aware" in r.stdout) == bool(extra), r.stdout
        assert np.array_equal(load(out), want), extra
    assert not np.array_equal(want_uniform, want_plain)


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import toymeshpathtracer_amd as tm
from noise_aware_restate import build_digests
try:
    out = build_digests(tm, sys.argv[2])
except tm.TmptError as e:
    out = {"error": str(e)}
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_checked_build(gpu):
    """The checked library gives both new calls' outputs the same bits, and no index check fails."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    assert got == json.loads(json.dumps(build_digests(tm, data("suzanne.obj"))))
