"""The noise-aware filter's surface without a GPU: tmpt_render_moments and
tmpt_denoise_moments are declared and exported, every argument check of both
calls answers -22 before any device work (the scene is the last thing either
looks at, or the first thing tmpt_render_moments shares with
tmpt_render_adaptive), the CLI's usage text, and the restatement's own checks:
with shrink = 3e38 it is np_denoise, and a constant frame passes through."""
import ctypes
import os
import re
import subprocess

import numpy as np

import toymeshpathtracer_amd as tm
from conftest import ROOT
from noise_aware_restate import (SHRINK_DEFAULT, check_synthetic_moments, moments_expect, np_denoise_moments,
                                 synthetic_moments, v0_expect)
from test_gpu_denoise import np_denoise, synthetic

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "tmpt.h")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_entry_points_are_declared_and_exported():
    text = open(HEADER).read()
    lib = ctypes.CDLL(tm.lib_path)
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    for name in ("tmpt_render_moments", "tmpt_denoise_moments"):
        assert name in tm.EXPORTS
        assert f"int {name}(" in text
        assert hasattr(lib, name)
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert callable(tm.Scene.trace_moments) and callable(tm.Scene.denoise_moments)
    assert "does NOT mean" in text  # ad NULL is the uniform schedule, said where the call is declared


# ---- tmpt_render_moments
def _moments_fn():
    return tm._sig("tmpt_render_moments", ctypes.c_int, [ctypes.c_void_p] * 10)


def _render(scene=0x1000, cam=True, desc=True, ad=None, ptrs=(True, True, True, True), **kw):
    """The call with a scene handle that is never read: every case here fails a check first."""
    c = tm.Camera.create([0, 0, 3], [0, 0, 0], [0, 1, 0], 40.0, 2.0, 0.0, 3.0)._to_c()
    d = tm._desc(8, 4, 4, tm.SEED_SAMPLE)
    for k, v in kw.items():
        setattr(d, k, v)
    bufs = [np.zeros((4, 8, 4), f32), np.zeros((4, 8, 4), f32), np.zeros((4, 8, 4), np.uint8), np.zeros((4, 8), np.int32)]
    a = [(p if isinstance(p, int) and not isinstance(p, bool) else (b.ctypes.data if p else None))
         for p, b in zip(ptrs, bufs)]
    adp = None
    if ad is not None:
        r = tm._AdaptiveDesc()
        for k, v in ad.items():
            setattr(r, k, v)
        adp = ctypes.cast(ctypes.pointer(r), ctypes.c_void_p)
    rc = _moments_fn()(scene, ctypes.byref(c) if cam else None, ctypes.byref(d) if desc else None, adp, a[0], a[1],
                       a[2], a[3], None, None)
    return rc, tm._last_error().decode()


def test_render_moments_checks_before_any_device_work():
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(scene=None), "null argument"), (dict(cam=False), "null argument"), (dict(desc=False), "null argument"),
        (dict(width=0), "width"), (dict(width=10001), "width"), (dict(height=0), "height"), (dict(height=10001), "height"),
        (dict(spp=0), "samplesPerPixel"), (dict(spp=1025), "samplesPerPixel"),
        (dict(seed_mode=tm.SEED_PIXEL), "seed_mode"), (dict(seed_mode=tm.SEED_ROW), "seed_mode"),
        (dict(engine=tm.ENGINE_WAVEFRONT), "engine"), (dict(engine=tm.ENGINE_MEGAKERNEL), "engine"),
        (dict(spp_begin=1), "spp_begin"), (dict(spp_count=2), "spp_begin"),
        (dict(flags=tm.FLAG_COUNT_VISITS), "COUNT_VISITS"),
        (dict(num_shards=3, shard=3), "shard"), (dict(num_shards=2, shard=-1), "shard"),
        (dict(ad=dict(threshold=nan)), "threshold"), (dict(ad=dict(threshold=inf)), "threshold"),
        (dict(ad=dict(threshold=-inf)), "threshold"),
        (dict(ad=dict(spp_min=1)), "spp_min"), (dict(ad=dict(spp_min=5)), "spp_min"), (dict(ad=dict(spp_min=-2)), "spp_min"),
        (dict(spp=1), "spp_min"),  # uniform: spp_min = spp, and spp >= 2
        (dict(spp=1, ad=dict(threshold=-1.0)), "spp_min"),
        (dict(ad=dict(spp_min=2, spp_step=-1)), "spp_step"),
        (dict(ad=dict(radius=-1)), "radius"), (dict(ad=dict(radius=9)), "radius"),
        (dict(spp=1024, ad=dict(spp_min=2, spp_step=1)), "64 passes"),
        (dict(ptrs=(True, False, True, True)), "moments_out"), (dict(ptrs=(False, False, False, False)), "moments_out"),
        (dict(flags=tm.FLAG_OUT_DEVICE, ptrs=(0x1008, 0x2000, 0x3000, 0x4000)), "aligned"),
        (dict(flags=tm.FLAG_OUT_DEVICE, ptrs=(0x1000, 0x2008, 0x3000, 0x4000)), "aligned"),
        (dict(flags=tm.FLAG_OUT_DEVICE, ptrs=(0x1000, 0x2000, 0x3002, 0x4000)), "aligned"),
        (dict(flags=tm.FLAG_OUT_DEVICE, ptrs=(0x1000, 0x2000, 0x3000, 0x4002)), "aligned"),
    ]
    for kw, msg in cases:
        rc, err = _render(**kw)
        assert rc == -22 and "tmpt_render_moments: " in err and msg in err, (kw, rc, err)
    # an earlier failure wins: the size before the schedule, the schedule before the missing plane
    rc, err = _render(width=0, ad=dict(spp_min=1), ptrs=(True, False, True, True))
    assert rc == -22 and "width" in err
    rc, err = _render(ad=dict(spp_min=1), ptrs=(True, False, True, True))
    assert rc == -22 and "spp_min" in err
    # tmpt_render_adaptive's own messages keep its name
    fn = tm._sig("tmpt_render_adaptive", ctypes.c_int, [ctypes.c_void_p] * 9)
    assert fn(None, None, None, None, None, None, None, None, None) == -22
    assert "tmpt_render_adaptive: null argument" in tm._last_error().decode()


# ---- tmpt_denoise_moments
def _ddesc(**kw):
    d = tm._DenoiseDesc()
    d.width, d.height, d.spp = 8, 4, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _denoise_fn():
    return tm._sig("tmpt_denoise_moments", ctypes.c_int,
                   [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 5)


def _denoise(d, shrink=0.0, rad=True, aov=True, mom=True, f32o=True, u8=True, ptrs=None):
    bufs = [np.zeros((4, 8, 4), f32), np.zeros((4, 8), tm.AOV_DTYPE), np.zeros((4, 8, 4), f32), np.zeros((4, 8, 4), f32),
            np.zeros((4, 8, 4), np.uint8)]
    a = [b.ctypes.data if on else None for on, b in zip((rad, aov, mom, f32o, u8), bufs)]
    if ptrs:
        a = list(ptrs)
    rc = _denoise_fn()(None, ctypes.byref(d) if d is not None else None, shrink, *a)
    return rc, tm._last_error().decode()


def test_denoise_moments_checks_in_order():
    inf, nan = float("inf"), float("nan")
    rc, err = _denoise(None)
    assert rc == -22 and "tmpt_denoise_moments: null descriptor" in err
    steps = [
        (dict(d=_ddesc(width=0)), "width"), (dict(d=_ddesc(width=10001)), "width"), (dict(d=_ddesc(height=0)), "height"),
        (dict(d=_ddesc(spp=0)), "samplesPerPixel"), (dict(d=_ddesc(spp=1025)), "samplesPerPixel"),
        (dict(d=_ddesc(levels=-1)), "levels"), (dict(d=_ddesc(levels=7)), "levels"),
        (dict(d=_ddesc(normal_exp=-2)), "normal_exp"), (dict(d=_ddesc(normal_exp=9)), "normal_exp"),
        (dict(d=_ddesc(sigma_depth=-1.0)), "sigma_depth"), (dict(d=_ddesc(sigma_depth=nan)), "sigma_depth"),
        (dict(d=_ddesc(sigma_direct=-1.0)), "sigma_direct"), (dict(d=_ddesc(sigma_direct=inf)), "sigma_direct"),
        (dict(shrink=-1.0), "shrink"), (dict(shrink=-1e-30), "shrink"), (dict(shrink=nan), "shrink"),
        (dict(shrink=inf), "shrink"), (dict(shrink=-inf), "shrink"),
        (dict(d=_ddesc(flags=2)), "flag"), (dict(d=_ddesc(flags=8)), "flag"),
        (dict(f32o=False, u8=False), "no output"),
        (dict(rad=False), "null argument"), (dict(aov=False), "null argument"), (dict(mom=False), "null argument"),
    ]
    for kw, msg in steps:
        kw = dict(kw)
        rc, err = _denoise(kw.pop("d", _ddesc()), **kw)
        assert rc == -22 and "tmpt_denoise_moments: " in err and msg in err, (msg, rc, err)
    # (the alignment of device pointers comes after the scene, as in tmpt_denoise: test_gpu_denoise_moments.py)
    # order between the groups: size < levels < sigma < shrink < flag < output < pointer
    chain = [(dict(width=0), {}, "width"), (dict(levels=9), {}, "levels"), (dict(sigma_depth=-1.0), {}, "sigma_depth"),
             ({}, dict(shrink=-2.0), "shrink"), (dict(flags=2), {}, "flag"), ({}, dict(f32o=False, u8=False), "no output"),
             ({}, dict(mom=False), "null argument")]
    for i, (_, _, msg) in enumerate(chain):
        fields, kw = {}, {}
        for f, k, _ in chain[i:]:
            fields.update(f)
            kw.update(k)
        rc, err = _denoise(_ddesc(**fields), **kw)
        assert rc == -22 and msg in err, (i, msg, rc, err)
    # everything in range, shrink at both ends of its domain: as far as the missing scene
    for shrink in (0.0, 1e-30, 4.0, 3e38):
        rc, err = _denoise(_ddesc(), shrink=shrink)
        assert rc == -22 and "null argument" in err, (shrink, rc, err)
    # tmpt_denoise keeps its name
    fn = tm._sig("tmpt_denoise", ctypes.c_int, [ctypes.c_void_p] * 6)
    assert fn(None, None, None, None, None, None) == -22 and "tmpt_denoise: null descriptor" in tm._last_error().decode()


def test_cli_usage_mentions_shrink():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout and "--shrink" in r.stdout
    obj = os.path.join(ROOT, "data", "cube.obj")
    for extra in (["--shrink", "4"], ["--shrink", "4", "--seed", "sample"],
                  ["--seed", "pixel", "--denoise", "x.png", "--shrink", "4"],
                  ["--seed", "sample", "--denoise", "x.png", "--shrink", "-1"],
                  ["--seed", "sample", "--denoise", "x.png", "--shrink", "nan"]):
        r = subprocess.run([cli, "8", "4", "2", obj] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--shrink" in r.stdout, (extra, r.stdout)


# ---- the restatement's own checks
def test_moments_restated():
    rng = np.random.default_rng(3)
    col = rng.random((3, 5, 8, 3)).astype(f32)
    n_p = np.array([[2, 4, 6, 8, 2]] * 3, np.int32)
    mom = moments_expect(col, n_p)
    assert mom.shape == (3, 5, 4) and mom.dtype == f32
    for (y, x), n in np.ndenumerate(n_p):  # one pixel at a time, a scalar loop
        m1 = m2 = f32(0)
        for s in range(n):
            c = col[y, x, s]
            lum = (f32(0.2126) * c[0] + f32(0.7152) * c[1]) + f32(0.0722) * c[2]
            m1, m2 = m1 + lum, m2 + lum * lum
        want = np.array([m1 / f32(n), m2 / f32(n), f32(1) / f32(n), 1], f32)
        assert (_bits(mom[y, x]) == _bits(want)).all()
    assert (_bits(moments_expect(col, 8)) == _bits(moments_expect(col, np.full((3, 5), 8)))).all()
    # a moments tile of n samples: v_0 is the unbiased variance of the mean, to rounding
    v0 = v0_expect(moments_expect(col, 8)).astype(np.float64)
    lum = 0.2126 * col[..., 0].astype(np.float64) + 0.7152 * col[..., 1] + 0.0722 * col[..., 2]
    assert np.allclose(v0, lum.var(-1, ddof=1) / 8, rtol=1e-4, atol=1e-7)


def test_synthetic_moments_hold_their_cases():
    for w, h in ((5, 3), (37, 23), (130, 9)):
        check_synthetic_moments(synthetic_moments(w, h))
        pos = synthetic_moments(w, h, positive=True)
        assert (v0_expect(pos) > 0).all() and np.isfinite(v0_expect(pos)).all()


def test_huge_shrink_is_the_plain_filter():
    """shrink = 3e38 on a plane with v_0 > 0 everywhere: every gain is 0."""
    for w, h in ((1, 1), (5, 3), (37, 23)):
        rad, aov, spp = synthetic(w, h)
        mom = synthetic_moments(w, h, positive=True)
        for levels in (1, 2, 3, 6):
            got = np_denoise_moments(rad, aov, mom, spp, 3e38, levels, 3, 0.05, 0.3)
            assert (_bits(got) == _bits(np_denoise(rad, aov, spp, levels, 3, 0.05, 0.3))).all(), (w, h, levels)
        assert (_bits(np_denoise_moments(rad, aov, mom, spp, 3e38)) == _bits(np_denoise(rad, aov, spp))).all()


def test_a_constant_frame_passes_through():
    """Every level's output is the constant to the last bit or not, but d is what was removed and
    the variance explains none of it when it is 0: out = c_N + (c_0 - c_N) level by level."""
    w, h = 37, 23
    rad, aov, spp = synthetic(w, h)
    rad[..., :3] = f32(0.75)
    mom = synthetic_moments(w, h, positive=True)
    mom[..., 1] = mom[..., 0] * mom[..., 0]  # zero variance: n = 0, every gain is 1 where anything was removed
    got = np_denoise_moments(rad, aov, mom, spp, 4.0)
    assert np.abs(got[..., :3] - f32(0.75)).max() < 1e-6
    assert (_bits(got[..., 3]) == _bits(rad[..., 3])).all()


def test_the_default_shrink_spelled_out():
    rad, aov, spp = synthetic(37, 23)
    mom = synthetic_moments(37, 23)
    assert SHRINK_DEFAULT == f32(2.0)
    assert "0 selects the default, 2.0f" in open(HEADER).read()
    default, two, four = (np_denoise_moments(rad, aov, mom, spp, s) for s in (0.0, 2.0, 4.0))
    assert (_bits(default) == _bits(two)).all() and not (_bits(default) == _bits(four)).all()


def test_the_filter_takes_detail_back_where_the_variance_is_small():
    """Between the two ends: shrink -> 0 returns the input (every gain -> 1); a shrink in between
    is neither the input nor the plain filter."""
    w, h = 37, 23
    rad, aov, spp = synthetic(w, h)
    mom = synthetic_moments(w, h, positive=True)
    tiny = np_denoise_moments(rad, aov, mom, spp, 1e-30)
    assert np.abs(tiny[..., :3] - rad[..., :3]).max() < 1e-4
    plain = np_denoise(rad, aov, spp)
    mid = np_denoise_moments(rad, aov, mom, spp, 4.0)
    assert not np.array_equal(mid, plain) and not np.array_equal(mid, tiny)
