"""History-guided sampling without a GPU: the two entry points (declared,
exported, the ABI version kept), tmpt_sample_plan's argument checks in
tmpt_temporal's order and tmpt_render_guided's refusal before any device call,
the restatement (guided_restate.py) against a scalar second statement of the
plan on every case its statement knows, its degenerate end (the null prior is
adaptive_expect exactly) and a condition on the inputs of the GPU tests, so
that none of them can pass vacuously."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import guided_restate as G
import ref_cases as C
import toymeshpathtracer_amd as tm
from adaptive_restate import adaptive_expect
from conftest import ROOT
from render_restate import same_bits
from test_gpu_reference_trace import SPP_MIN, SPP_STEP, TAU, _case

f32 = np.float32
HEADER = os.path.join(ROOT, "include", "tmpt.h")
PTRS = ("mot", "pmot", "hist", "out")


def _bits_or_nan(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(np.where(np.isnan(want), ~np.isnan(got), a != b))
    assert len(bad) == 0, f"{what}: {len(bad)} floats differ, first at {bad[0]}"


# ---------------------------------------------------------------- the ABI
def test_header_declares_and_the_library_exports():
    text = open(HEADER).read()
    out = subprocess.run(["nm", "-D", "--defined-only", tm.lib_path], capture_output=True, text=True).stdout
    for name in ("tmpt_sample_plan", "tmpt_render_guided"):
        assert name in tm.EXPORTS and hasattr(tm._lib, name)
        assert f"int {name}(" in text
        assert re.search(rf" T {name}$", out, flags=re.M)
    assert tm.abi_version() == 9  # additive: detected by symbol, the version stays
    assert callable(tm.Scene.sample_plan) and callable(tm.Scene.trace_guided)
    # the sentence the null prior rests on
    flat = " ".join(text.replace("*", " ").split())
    assert "se2b = se2 and meanb = mean exactly for every finite mean and every non-negative, infinite or NaN se2" in flat
    assert "tmpt_render_moments bit for bit" in flat


def _plan_fn():
    return tm._sig("tmpt_sample_plan", ctypes.c_int, [ctypes.c_void_p] * 6)


def _desc(**kw):
    d = tm._TemporalDesc()
    d.width, d.height = 8, 4
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(d, ptrs=None, **given):
    """tmpt_sample_plan without a scene: host frames of 8 x 4; given[name] = False
    removes a pointer, ptrs = {name: address} sets raw addresses."""
    bufs = dict(mot=np.zeros((4, 8), tm.MOTION_DTYPE), pmot=np.zeros((4, 8), tm.MOTION_DTYPE),
                hist=np.zeros((4, 8, 4), f32), out=np.zeros((4, 8, 4), f32))
    on = dict(mot=True, pmot=True, hist=True, out=True)
    on.update(given)
    a = [bufs[k].ctypes.data if on[k] else None for k in PTRS]
    for k, v in (ptrs or {}).items():
        a[PTRS.index(k)] = v
    rc = _plan_fn()(None, ctypes.byref(d) if d is not None else None, *a)
    return rc, tm._last_error().decode()


def test_sample_plan_checks_in_order():
    rc, err = _call(None)
    assert rc == -22 and "tmpt_sample_plan: null descriptor" in err, (rc, err)
    inf, nan = float("inf"), float("nan")
    dev = tm.FLAG_OUT_DEVICE
    steps = [
        (dict(d=_desc(width=0)), "width"), (dict(d=_desc(width=10001)), "width"),
        (dict(d=_desc(height=0)), "height"), (dict(d=_desc(height=10001)), "height"),
        (dict(mot=False), "null argument"), (dict(pmot=False), "null argument"), (dict(hist=False), "null argument"),
        (dict(out=False), "null argument"),
        (dict(d=_desc(n_max=0.5)), "n_max"), (dict(d=_desc(n_max=-1.0)), "n_max"), (dict(d=_desc(n_max=inf)), "n_max"),
        (dict(d=_desc(n_max=nan)), "n_max"),
        (dict(d=_desc(sigma_depth=-0.1)), "sigma_depth"), (dict(d=_desc(sigma_depth=inf)), "sigma_depth"),
        (dict(d=_desc(sigma_depth=nan)), "sigma_depth"),
        (dict(d=_desc(flags=2)), "flag"), (dict(d=_desc(flags=8)), "flag"),
    ]
    for kw, msg in steps:
        kw = dict(kw)
        rc, err = _call(kw.pop("d", _desc()), **kw)
        assert rc == -22 and "tmpt_sample_plan: " in err and msg in err, (msg, rc, err)
    al = {k: 0x10000 * (i + 1) for i, k in enumerate(PTRS)}
    for k in PTRS:  # each device pointer's alignment
        p = dict(al)
        p[k] += 8
        rc, err = _call(_desc(flags=dev), ptrs=p)
        assert rc == -22 and "aligned" in err, (k, rc, err)
    n = 8 * 4 * 16
    for a, b in ((0x4000, 0x4000), (0x4000, 0x4000 + n - 16), (0x4000 + n - 16, 0x4000)):  # by one pixel, either side
        for flags in (dev, 0):
            rc, err = _call(_desc(flags=flags), ptrs=dict(al, hist=a, out=b))
            assert rc == -22 and "prior_out overlaps moments_history" in err, (a, b, rc, err)
    # the order between the groups: size < pointer < n_max < sigma_depth < flag < alignment < overlap < scene
    chain = [(dict(width=0), "width"), (None, "null argument"), (dict(n_max=0.25), "n_max"),
             (dict(sigma_depth=-1.0), "sigma_depth"), (dict(flags=dev | 2), "flag")]
    for i, (_, msg) in enumerate(chain):
        fields = {}
        for kw, _ in chain[i:]:
            fields.update(kw or {})
        rc, err = _call(_desc(**fields), hist=i > 1)
        assert rc == -22 and msg in err, (i, msg, rc, err)
    rc, err = _call(_desc(flags=dev), ptrs=dict(al, mot=0x10008, out=al["hist"]))  # misaligned and overlapping
    assert rc == -22 and "aligned" in err, (rc, err)
    for d, kw in ((_desc(), {}), (_desc(n_max=1.0, sigma_depth=3.0), {}), (_desc(n_max=500.0), {}),
                  (_desc(flags=dev | tm.FLAG_WAIT_STREAM), dict(ptrs=al)),
                  (_desc(flags=dev), dict(ptrs=dict(al, out=al["hist"] + n)))):  # everything in range: as far as the scene
        rc, err = _call(d, **kw)
        assert rc == -22 and "null scene" in err, (kw, rc, err)


def test_render_guided_refuses_before_any_device_call():
    fn = tm._sig("tmpt_render_guided", ctypes.c_int, [ctypes.c_void_p] * 11)
    rad = np.zeros((4, 8, 4), f32)
    cam, d = tm._Camera(), tm._desc(8, 4, 4, tm.SEED_SAMPLE, 0, 0, 1, tm.ENGINE_PERSISTENT, 0, 0, 0)
    rc = fn(None, ctypes.byref(cam), ctypes.byref(d), None, None, rad.ctypes.data, None, None, None, None, None)
    assert rc == -22 and "tmpt_render_guided: null argument" in tm._last_error().decode()


def test_python_argument_errors():
    sc = tm.Scene.__new__(tm.Scene)  # no device: the checks below come before any call into the library
    sc._h, sc.device = None, 0
    mom, mot = np.zeros((4, 8, 4), f32), np.zeros((4, 8), tm.MOTION_DTYPE)
    with pytest.raises(ValueError, match="width, height and out"):
        sc.sample_plan(0x1000, 0x2000, 0x3000)
    for bad in (dict(moments_history=mom[..., :3]), dict(motion=mot[:, :3]), dict(prev_motion=mot[:2])):
        a = dict(motion=mot, prev_motion=mot, moments_history=mom)
        a.update(bad)
        with pytest.raises(ValueError, match="one whole frame"):
            sc.sample_plan(**a)
    for out in (np.zeros((4, 8, 4), np.float64), np.zeros((4, 8, 3), f32), [1]):
        with pytest.raises(ValueError, match="out must be"):
            sc.sample_plan(mot, mot, mom, out=out)
    with pytest.raises(tm.TmptError, match="overlaps"):
        sc.sample_plan(mot, mot, mom, out=mom)
    with pytest.raises(tm.TmptError, match="null scene"):
        sc.sample_plan(mot, mot, mom)
    with pytest.raises(ValueError, match="whole frame"):
        sc.trace_guided(tm.Camera.create([0, 0, 3], [0, 0, 0], [0, 1, 0], 60.0, 2.0, 0.0, 1.0), 8, 4, 4, prior=mom[:2])


def test_cli_usage_mentions_guided():
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    r = subprocess.run([cli], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout and "--guided" in r.stdout
    obj = os.path.join(ROOT, "data", "cube.obj")
    for extra in (["--guided"], ["--guided", "2,2"], ["--twist", "10,2", "--guided", "2,2,0.02,8"]):
        r = subprocess.run([cli, "8", "4", "4", obj, "--seed", "sample"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--guided needs --temporal" in r.stdout, (extra, r.stdout)
    r = subprocess.run([cli, "8", "4", "4", obj, "--seed", "sample", "--twist", "10,2", "--temporal", "--guided", "x"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "invalid --guided argument" in r.stdout, r.stdout


# ---------------------------------------------------------------- the plan's restatement
def test_plan_frames_hold_every_case():
    mot, pmot, hist, cases = G.plan_frames()
    assert hist.shape == (G.PLAN_SIZE[1], G.PLAN_SIZE[0], 4) and G.PLAN_SIZE == (67, 35)
    pr = G.plan(mot, pmot, hist)
    null = (pr == G.NULL_PRIOR).all(-1)
    for name in ("px_nan", "px_out_of_range", "taps_outside", "all_taps_rejected"):
        assert null[cases[name]], name
    for name in ("taps_outside_edge", "tap_depth_rejected", "hz_zero", "length_at_n_max", "length_beyond_n_max"):
        assert not null[cases[name]], name
    assert np.isnan(mot["px"][cases["px_nan"]])
    # the edge pixel and the depth-rejected pixel lost taps: their weights no longer sum to one
    from temporal_clip_restate import fetch
    go, _, nsum, wsum, _ = fetch(mot, pmot, hist, f32(0.05), hist)
    for name in ("taps_outside_edge", "tap_depth_rejected"):
        assert go[cases[name]] and 0 < wsum[cases[name]] < 0.95, (name, wsum[cases[name]])
    assert not go[cases["all_taps_rejected"]] and wsum[cases["all_taps_rejected"]] == 0
    # hz = 0: an infinite effective count, no history variance; the blend factor is still the length's
    p = pr[cases["hz_zero"]]
    assert p[1] == 0 and p[3] >= 1 and p[2] == f32(1) / min(p[3] + f32(1), f32(3))
    # lengths at and beyond n_max: the blend factor is the cap's
    assert pr[cases["length_at_n_max"]][3] == 2 and pr[cases["length_at_n_max"]][2] == f32(1) / f32(3)
    assert pr[cases["length_beyond_n_max"]][3] == 5 and pr[cases["length_beyond_n_max"]][2] == f32(1) / f32(3)
    assert G.plan(mot, pmot, hist, n_max=8.0)[cases["length_beyond_n_max"]][2] == f32(1) / f32(6)
    assert 0.1 < null.mean() < 0.9 and (pr[..., 1][~null] > 0).any() and (pr[..., 1][~null] == 0).any()


@pytest.mark.parametrize("n_max,sigma", [(0.0, 0.0), (8.0, 0.02), (1.0, 0.5)])
def test_plan_equals_its_scalar_statement(n_max, sigma):
    mot, pmot, hist, _ = G.plan_frames()
    _bits_or_nan(G.plan(mot, pmot, hist, n_max, sigma), G.plan_scalar(mot, pmot, hist, n_max, sigma),
                 f"plan n_max {n_max} sigma {sigma}")
    if n_max == 1.0:  # a = 1, b = 0: the history brings no variance and the frame is taken whole
        pr = G.plan(mot, pmot, hist, n_max, sigma)
        live = ~(pr == G.NULL_PRIOR).all(-1)
        assert (pr[live][:, 2] == 1).all() and (pr[live][:, 1] == 0).all()


def test_defaults_are_tmpt_temporals():
    mot, pmot, hist, _ = G.plan_frames()
    same_bits(G.plan(mot, pmot, hist), G.plan(mot, pmot, hist, 3.0, 0.05), "defaults spelled out")


# ---------------------------------------------------------------- the guided test's restatement
@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_null_prior_is_adaptive_expect(name):
    c = _case(name)
    col, rays = c["col"][tm.SEED_SAMPLE], c["rays"][tm.SEED_SAMPLE]
    want = adaptive_expect(col, rays, SPP_MIN, SPP_STEP, TAU[name])
    for prior in (None, np.broadcast_to(G.NULL_PRIOR, (c["h"], c["w"], 4)).copy()):
        got = G.guided_expect(col, rays, SPP_MIN, SPP_STEP, TAU[name], prior)
        assert np.array_equal(got[0], want[0]) and got[2] == want[2] and got[3] == want[3]
        same_bits(got[1], want[1], f"{name} null prior")


@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_gpu_cases_move_pixels(name):
    """The synthetic prior moves at least 10 % of the pixels to another count,
    every schedule end occurs, and the nh = 0 columns are unchanged."""
    c = _case(name)
    col, rays = c["col"][tm.SEED_SAMPLE], c["rays"][tm.SEED_SAMPLE]
    assert (c["w"], c["h"], c["spp"]) == (32, 18, 8)
    plain = adaptive_expect(col, rays, SPP_MIN, SPP_STEP, TAU[name])[0]
    null_cols = (np.arange(c["w"]) // 4) % 4 == 0
    for n_max in G.N_MAX_CASES:
        prior = G.synthetic_prior(col, n_max)
        assert (prior[:, null_cols] == G.NULL_PRIOR).all() and not (prior[:, ~null_cols] == G.NULL_PRIOR).all(-1).any()
        n_p = G.guided_expect(col, rays, SPP_MIN, SPP_STEP, TAU[name], prior)[0]
        differ = n_p != plain
        counts = [int((n_p == n).sum()) for n in (2, 4, 6, 8)]
        print(f"{name} n_max {n_max}: {100 * differ.mean():.1f} % differ, stops at 2/4/6/8 {counts}, "
              f"earlier {int((n_p < plain).sum())} later {int((n_p > plain).sum())}")
        assert differ.mean() >= 0.10, differ.mean()
        assert min(counts) > 0, counts
        assert not differ[:, null_cols].any()
