"""History-guided sampling on the device (tmpt_sample_plan / Scene.sample_plan,
tmpt_render_guided / Scene.trace_guided).

1  the plan is bit for bit tests/guided_restate.py (proved on the CPU by
   test_guided_abi.py): on a rendered two-frame sequence and on the synthetic
   records with every case of its statement, host and device pointers;
2  the guided render over the reference's own per-sample colours
   (tests/golden/ref/trace_<case>.npz, 32x18x8) with the synthetic prior of
   guided_restate.synthetic_prior: counts, radiance, moments, bytes, rays and
   info against the restatement; the null prior against trace_moments; per-count
   identity; sample_base; shards; the progressive state; the CLI's --guided; the
   checked build.

Tolerance: none.  Floats are compared as bits (a NaN for a NaN in the plan, whose
synthetic inputs hold some).
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_refit_restate as F
import guided_restate as G
import toymeshpathtracer_amd as tm
from conftest import ROOT, data
from noise_aware_restate import moments_expect
from render_restate import pack, same_bits
from test_gpu_reference_trace import CASES, CASE_IDS, SPP_MIN, SPP_STEP, TAU, _camera, _case, _radiance, _scene
from test_gpu_temporal import CHECK_LIB, _mesh
from test_gpu_temporal_clip import _cli_poses, same

pytestmark = pytest.mark.gpu

f32 = np.float32
ONE = f32(1).view(np.uint32)


def _col(name):
    c = _case(name)
    return c["col"][tm.SEED_SAMPLE], c["rays"][tm.SEED_SAMPLE]


@functools.lru_cache(maxsize=None)
def _prior(name, n_max):
    return G.synthetic_prior(_col(name)[0], n_max)


@functools.lru_cache(maxsize=None)
def _expect(name, n_max):
    col, rays = _col(name)
    return G.guided_expect(col, rays, SPP_MIN, SPP_STEP, TAU[name], _prior(name, n_max))


def _same_results(got, want, what):
    """Two results of trace_moments / trace_guided, everything bit for bit."""
    for k, part in enumerate(("radiance", "moments")):
        same_bits(got[k], want[k], f"{what} {part}")
    assert np.array_equal(got[2], want[2]), what + " bytes"
    assert np.array_equal(got[3], want[3]), what + " spp map"
    assert got[4] == want[4], f"{what}: rays {got[4]} vs {want[4]}"
    assert got[5] == want[5], f"{what}: info {got[5]} vs {want[5]}"


# ---------------------------------------------------------------- 1  the plan
@functools.lru_cache(maxsize=None)
def _sequence():
    """suzanne at rest and twisted by 5 degrees (a refit), 96 x 54: frame 0's moments at 4 spp, both frames' records."""
    w, h, spp = 96, 54, 4
    rest, bmin, bmax = _mesh("suzanne.obj")
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(rest) as sc:
        mom0 = sc.trace_moments(cam, w, h, spp)[1]
        mot0, _ = sc.trace_motion(cam, cam, w, h)
        sc.update(F.twist(rest, 5.0), mode="refit")
        mot1, _ = sc.trace_motion(cam, cam, w, h, rest)
    for a in (mom0, mot0, mot1):
        a.setflags(write=False)
    return w, h, mom0, mot0, mot1


def _dev(a):
    import torch

    h, w = a.shape[:2]
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")


def test_plan_on_real_frames(gpu):
    import torch

    w, h, mom0, mot0, mot1 = _sequence()
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as sc:  # any scene: it lends its device and stream
        for n_max, sigma in ((0.0, 0.0), (8.0, 0.02)):
            want = G.plan(mot1, mot0, mom0, n_max, sigma)
            null = (want == G.NULL_PRIOR).all(-1)
            assert null.any() and null.mean() < 0.9 and (want[..., 3][~null] == 1).all() and (want[..., 1][~null] > 0).any()
            what = f"suzanne twist n_max {n_max} sigma {sigma}"
            got = sc.sample_plan(mot1, mot0, mom0, n_max, sigma)
            same(got, want, what)
            assert sc.stats().render_ms > 0
            out = np.full((h, w, 4), 7, f32)
            assert sc.sample_plan(mot1, mot0, mom0, n_max, sigma, out=out) is out and out.tobytes() == got.tobytes()
            # torch tensors: the prior is a tensor; raw device pointers: into out
            t_m1, t_m0, t_h = _dev(mot1), _dev(mot0), torch.from_numpy(mom0.copy()).to("cuda:0")
            t = sc.sample_plan(t_m1, t_m0, t_h, n_max, sigma)
            assert isinstance(t, torch.Tensor) and t.cpu().numpy().tobytes() == got.tobytes()
            t_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
            assert sc.sample_plan(t_m1.data_ptr(), t_m0.data_ptr(), t_h.data_ptr(), n_max, sigma, out=t_out.data_ptr(),
                                  width=w, height=h) is None
            assert t_out.cpu().numpy().tobytes() == got.tobytes()
            assert t_h.cpu().numpy().tobytes() == mom0.tobytes() and t_m1.cpu().numpy().tobytes() == mot1.tobytes()
        with pytest.raises(tm.TmptError, match="overlaps"):
            sc.sample_plan(t_m1.data_ptr(), t_m0.data_ptr(), t_h.data_ptr(), out=t_h.data_ptr() + 16 * w, width=w, height=h)
        with pytest.raises(tm.TmptError, match="aligned"):
            sc.sample_plan(t_m1.data_ptr(), t_m0.data_ptr(), t_h.data_ptr(), out=t_out.data_ptr() + 8, width=w, height=h)
        # a second step: the accumulated moments (mixed lengths) are the next history
        acc = sc.temporal(mom0, mot1, mot0, mom0)[0]
        assert len(np.unique(acc[..., 3])) >= 2
        same(sc.sample_plan(mot0, mot1, acc), G.plan(mot0, mot1, acc), "second step")


def test_plan_on_synthetic_records(gpu):
    import torch

    mot, pmot, hist, cases = G.plan_frames()
    h, w = hist.shape[:2]
    assert (w, h) == (67, 35)
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as sc:
        for n_max, sigma in ((0.0, 0.0), (8.0, 0.02), (1.0, 0.5), (64.0, 0.0)):
            want = G.plan(mot, pmot, hist, n_max, sigma)
            what = f"synthetic 67x35 n_max {n_max} sigma {sigma}"
            got = sc.sample_plan(mot, pmot, hist, n_max, sigma)
            same(got, want, what)
            t = sc.sample_plan(_dev(mot), _dev(pmot), torch.from_numpy(hist.copy()).to("cuda:0"), n_max, sigma)
            same(t.cpu().numpy(), want, what + " (device)")
        for name in ("px_nan", "px_out_of_range", "taps_outside", "all_taps_rejected"):
            assert (got[cases[name]] == G.NULL_PRIOR).all(), name


# ---------------------------------------------------------------- 2  the guided render
@pytest.mark.parametrize("name,waves", CASES, ids=CASE_IDS)
def test_guided_equals_restatement(gpu, name, waves):
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    col = _col(name)[0]
    with _scene(name, waves) as sc:
        for n_max in G.N_MAX_CASES:
            prior = _prior(name, n_max)
            want_n, want_rad, want_rays, want_pp = _expect(name, n_max)
            what = f"{name} n_max {n_max}, path_waves {waves}"
            rad, mom, img, n_p, rays, info = sc.trace_guided(cam, w, h, cap, prior, SPP_MIN, SPP_STEP, TAU[name])
            assert np.array_equal(n_p, want_n), f"{what}: spp map differs at {np.argwhere(n_p != want_n)[:4]}"
            same_bits(rad[..., :3], want_rad, what)
            assert (rad[..., 3].view(np.uint32) == ONE).all()
            same_bits(mom, moments_expect(col, want_n), what + " moments")
            assert np.array_equal(img, pack(want_rad)), what
            assert rays == want_rays, f"{what}: rays {rays} vs {want_rays}"
            assert info == {"passes": len(want_pp), "samples": int(want_n.sum()), "pass_pixels": want_pp}, what
            # per-count identity: each pixel is the uniform frame's at its own count
            for n in np.unique(n_p):
                at = n_p == n
                same_bits(rad[..., :3][at], _radiance(name, tm.SEED_SAMPLE, int(n))[0][at], f"{what} count {n}")
            # radius 1: monotone, and the moments at the call's own counts
            r1 = sc.trace_guided(cam, w, h, cap, prior, SPP_MIN, SPP_STEP, TAU[name], radius=1)
            assert (r1[3] >= n_p).all(), what
            same_bits(r1[1], moments_expect(col, r1[3]), what + " radius 1 moments")


@pytest.mark.parametrize("name", ["cube", "room"])
def test_null_prior_is_trace_moments(gpu, name):
    import torch

    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    null = np.broadcast_to(G.NULL_PRIOR, (h, w, 4)).copy()
    with _scene(name, 5) as sc:
        for radius in (0, 1):
            kw = dict(spp_min=SPP_MIN, spp_step=SPP_STEP, threshold=TAU[name], radius=radius)
            want = sc.trace_moments(cam, w, h, cap, **kw)
            assert radius or len(np.unique(want[3])) >= 3
            _same_results(sc.trace_guided(cam, w, h, cap, **kw), want, f"{name} prior None radius {radius}")
            _same_results(sc.trace_guided(cam, w, h, cap, null, **kw), want, f"{name} null prior radius {radius}")
            _same_results(sc.trace_guided(cam, w, h, cap, torch.from_numpy(null).to("cuda:0"), **kw), want,
                          f"{name} null prior tensor radius {radius}")
        # uniform (ad NULL), whatever the prior says
        want = sc.trace_moments(cam, w, h, 4)
        _same_results(sc.trace_guided(cam, w, h, 4, _prior(name, 3.0)), want, f"{name} uniform")
        # the device form: moments_out may be left out, one output is enough
        prior = _prior(name, 3.0)
        kw = dict(spp_min=SPP_MIN, spp_step=SPP_STEP, threshold=TAU[name])
        host = sc.trace_guided(cam, w, h, cap, prior, **kw)
        tn = torch.full((h, w), 7, dtype=torch.int32, device="cuda:0")
        t32 = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        res = sc.trace_guided(cam, w, h, cap, torch.from_numpy(prior.copy()).to("cuda:0"), out=(None, None, None, tn.data_ptr()), **kw)
        assert res[:4] == (None,) * 4 and res[4] == host[4] and res[5] == host[5]
        assert np.array_equal(tn.cpu().numpy(), host[3])
        sc.trace_guided(cam, w, h, cap, prior, out=(t32.data_ptr(), None, None, None), **kw)  # a host prior is staged
        same_bits(t32.cpu().numpy(), host[0], "device radiance")
        with pytest.raises(tm.TmptError, match="no output"):
            sc.trace_guided(cam, w, h, cap, out=(None, None, None, None), **kw)


@pytest.mark.parametrize("name", ["cube", "room"])
def test_sample_base_moves_the_window(gpu, name):
    """sample_base = 4 at cap 4: the schedule 2, 4 over samples 4 .. 7 of the fixture."""
    c = _case(name)
    w, h = c["w"], c["h"]
    col, rays = _col(name)
    prior = _prior(name, 3.0)
    want_n, want_rad, want_rays, want_pp = G.guided_expect(col[:, :, 4:8], rays[:, :, 4:8], 2, 2, TAU[name], prior)
    plain = G.guided_expect(col[:, :, 4:8], rays[:, :, 4:8], 2, 2, TAU[name])[0]
    assert (want_n != plain).any() and len(np.unique(want_n)) == 2
    with _scene(name, 5) as sc:
        sc.set_option("sample_base", 4)
        rad, mom, img, n_p, got_rays, info = sc.trace_guided(_camera(name), w, h, 4, prior, 2, 2, TAU[name])
    assert np.array_equal(n_p, want_n) and got_rays == want_rays and info["pass_pixels"] == want_pp
    same_bits(rad[..., :3], want_rad, f"{name} sample_base 4")
    same_bits(mom, moments_expect(col[:, :, 4:8], want_n), f"{name} sample_base 4 moments")


def test_shard_tiles_assemble(gpu):
    name = "room"
    c = _case(name)
    w, h, cap = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    band, shards = 4, 3
    prior = _prior(name, 3.0)
    with _scene(name, 5) as sc:
        for radius in (0, 1):
            kw = dict(spp_min=SPP_MIN, spp_step=SPP_STEP, threshold=TAU[name], radius=radius, band_rows=band)
            whole = sc.trace_guided(cam, w, h, cap, prior, **kw)
            if radius == 0:
                assert np.array_equal(whole[3], _expect(name, 3.0)[0])
            frame = [np.full((h, w, 4), np.nan, f32), np.full((h, w, 4), np.nan, f32), np.zeros((h, w, 4), np.uint8),
                     np.zeros((h, w), np.int32)]
            rays = 0
            for k in range(shards):
                part = sc.trace_guided(cam, w, h, cap, prior, shard=k, num_shards=shards, **kw)  # the whole-frame prior
                rows = tm.tile_row_to_y(w, h, band, k, shards)
                assert part[1].shape == (len(rows), w, 4)
                for f, p in zip(frame, part[:4]):
                    f[rows] = p
                rays += part[4]
            same_bits(frame[0], whole[0], f"shards radius {radius} radiance")
            same_bits(frame[1], whole[1], f"shards radius {radius} moments")
            assert np.array_equal(frame[2], whole[2]) and np.array_equal(frame[3], whole[3]) and rays == whole[4]


def test_the_calls_leave_the_progressive_state_alone(gpu):
    name = "room"
    c = _case(name)
    w, h, spp = c["w"], c["h"], c["spp"]
    cam = _camera(name)
    mot, pmot, hist, _ = G.plan_frames()
    with _scene(name, 5) as fresh:
        once, rays = fresh.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
    with _scene(name, 5) as sc:
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        assert done == 3
        sc.sample_plan(mot, pmot, hist)  # between the two passes
        between = sc.trace_guided(cam, w, h, spp, _prior(name, 3.0), SPP_MIN, SPP_STEP, TAU[name])
        done, last, r_b = next(passes)
        assert done == spp and np.array_equal(last, once) and r_a + r_b == rays
        after, rays2 = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
    assert np.array_equal(after, once) and rays2 == rays
    assert np.array_equal(between[3], _expect(name, 3.0)[0])


def test_cli_guided_pngs(gpu, tmp_path):
    w, h, spp, frames = 32, 18, 8, 3
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    stem = str(tmp_path / "tw")
    args = [cli, str(w), str(h), str(spp), data("suzanne.obj"), "--seed", "sample", "--twist", f"20,{frames}", "--out",
            stem + ".png", "--temporal"]
    digest = lambda n: hashlib.sha256(open(str(tmp_path / n), "rb").read()).hexdigest()
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    for clip in (True, False):
        extra = (["--clip"] if clip else []) + ["--guided", "2,2,0.05", "--spp-map", str(tmp_path / "map.png")]
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        names = [f"tw_{f:03d}.png" for f in range(frames)] + [f"tw_temporal_{f:03d}.png" for f in range(frames)] + \
                [f"map_{f:03d}.png" for f in range(frames)]
        assert sorted(os.listdir(tmp_path)) == sorted(names)
        got = [[digest(f"tw_{f:03d}.png"), digest(f"tw_temporal_{f:03d}.png"), digest(f"map_{f:03d}.png")]
               for f in range(frames)]
        want, fewer = [], 0
        with tm.Scene(tris) as sc:
            acc = macc = pmot = prev = None
            for f, (pose, lo, hi) in enumerate(_cli_poses(tris, 20.0, frames)):
                sc.set_option("sample_base", f * spp)
                sc.update(pose, "refit")
                sc.build_octree(*tm.octree_bounds(lo, hi))
                mot, _ = sc.trace_motion(cam, cam, w, h, prev)
                prior = sc.sample_plan(mot, pmot, macc) if f else None
                rad, mom, img, n_p, _, info = sc.trace_guided(cam, w, h, spp, prior, 2, 2, 0.05)
                fewer += int(info["samples"] < w * h * spp)
                timg = img
                if f and clip:
                    acc, timg, macc = sc.temporal_clip(rad, mot, pmot, acc, aux=mom, aux_history=macc)
                elif f:
                    acc, timg = sc.temporal(rad, mot, pmot, acc)
                    macc, _ = sc.temporal(mom, mot, pmot, macc)
                else:
                    acc, macc = rad, mom
                pmot, prev = mot, pose
                grey = np.full((h, w, 4), 255, np.uint8)
                grey[..., :3] = (n_p.astype(f32) / f32(spp) * f32(255)).astype(np.uint8)[..., None]
                one = []
                for a in (img, timg, grey):
                    tm.write_png(str(tmp_path / "py.png"), a)
                    one.append(digest("py.png"))
                want.append(one)
        os.remove(str(tmp_path / "py.png"))
        assert got == want, clip
        assert fewer == frames  # the test stopped pixels in every frame
        for n in names:
            os.remove(str(tmp_path / n))


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import guided_restate as G
import toymeshpathtracer_amd as tm
print(json.dumps(G.build_digests(tm, sys.argv[2])))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_guided_checked_build(gpu):
    """The checked library computes the same plan and the same guided frames, and no index check fails."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    assert got == json.loads(json.dumps(G.build_digests(tm, data("suzanne.obj"))))
