"""History clipping on the device (tmpt_temporal_clip / Scene.temporal_clip).

1  the kernel is bit for bit tests/temporal_clip_restate.py (proved on the CPU by
   test_temporal_clip_restate.py): on test_gpu_temporal's synthetic frames
   extended with constant windows, isolated covered pixels, a coverage
   checkerboard and a NaN / inf in the frame and in the statistics frame, at
   sizes that give a lone pixel, windows cut by every edge and tile edges with
   the halo crossing them; with gamma = 3e38 also against Scene.temporal itself;
2  on the rendered suzanne twist pair, a second step, the device-pointer form;
3  refusals, the kept staging buffer, the progressive state, the CLI's --clip,
   the checked build.

Tolerance: none.  A NaN's sign and payload are not part of the contract (the
host's and the device's default NaN differ in the sign bit): where the
restatement holds a NaN the device must hold one, every other float agrees in
its bits; a packed byte is compared where its float is not a NaN.
"""
import functools
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_clip_restate as K
import temporal_restate as T
import toymeshpathtracer_amd as tm
from conftest import ROOT, data
from test_gpu_temporal import CHECK_LIB, _mesh, _twist_pair, synthetic

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(1, 1), (5, 3), (37, 23), (130, 9), (33, 9)]


def same(got, want, what):
    """Bit for bit, a NaN for a NaN."""
    assert got.dtype == f32 and got.shape == want.shape, what
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    nan = np.isnan(want)
    bad = np.argwhere(np.where(nan, ~np.isnan(got), a != b))
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} floats differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def same_bytes(img, want, what):
    ok = ~np.isnan(want[..., :3])
    assert np.array_equal(img[..., :3][ok], T.pack(want)[..., :3][ok]) and (img[..., 3] == 255).all(), what


@functools.lru_cache(maxsize=None)
def extended(w, h, seed=1):
    """synthetic() plus a statistics frame and an aux pair, and: a block of equal
    values (windows with sd = 0) in both frames, a block that is uncovered but
    for lone covered pixels, a coverage checkerboard, a NaN and an inf in the
    frame and in the statistics frame.  On the small sizes the blocks wrap and
    overlap; 1 x 1 keeps its one pixel finite."""
    cur, mot, pmot, hist = (a.copy() for a in synthetic(w, h, seed))
    rng = np.random.default_rng(77 + w * 131 + h + seed)
    stat = (rng.random((h, w, 4)) * 4).astype(f32)
    aux = (rng.random((h, w, 4)) * 4).astype(f32)
    aux_hist = (rng.random((h, w, 4)) * 4).astype(f32)
    aux_hist[..., 3] = hist[..., 3]
    ys, xs = np.mgrid[0:h, 0:w]
    if w * h > 1:
        const = (xs % 37 < 9) & (ys % 23 < 8) if w >= 20 else (xs < 3) & (ys < 3)
        cur[const, :3] = f32(0.7)
        stat[const, :3] = f32(1.3)
        lone = (xs % 37 >= 12) & (xs % 37 < 24) & (ys % 23 >= 3)
        mot["flags"][lone] = np.where((xs % 4 == 1) & (ys % 4 == 2), 3, 0).astype(np.uint32)[lone]
        board = (xs % 37 >= 26) & (ys % 23 < 12)
        mot["flags"][board] = np.where((xs + ys) % 2 == 0, 3, 2).astype(np.uint32)[board]
        flat = rng.permutation(w * h)
        at = lambda k: np.unravel_index(flat[k % (w * h)], (h, w))
        cur[at(0)][0], cur[at(1)][2], stat[at(2)][1], stat[at(3)][0] = np.nan, np.inf, np.nan, np.inf
    frames = dict(cur=cur, mot=mot, pmot=pmot, hist=hist, stat=stat, aux=aux, aux_hist=aux_hist)
    for a in frames.values():
        a.setflags(write=False)
    return frames


# ---------------------------------------------------------------- 1  synthetic frames
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_clip_bit_for_bit(gpu, w, h):
    fr = extended(w, h)
    cur, mot, pmot, hist = fr["cur"], fr["mot"], fr["pmot"], fr["hist"]
    tris, _, _ = _mesh("cube.obj")
    seen = dict(clipped=0, kept=0, reset=0, lone=0)
    with tm.Scene(tris) as sc:
        for radius in (1, 2, 3):
            for gamma in (0.0, 0.5, 3e38):
                for n_max in (0.0, 1.0, 64.0):
                    for stat in (None, fr["stat"]):
                        p = K.parts(cur, mot, pmot, hist, gamma, radius, n_max, 0.0, stat, fr["aux"], fr["aux_hist"])
                        want, want_aux = p["out"], p["aux_out"]
                        what = f"{w}x{h} radius {radius} gamma {gamma} n_max {n_max} stat {stat is not None}"
                        got, img, got_aux = sc.temporal_clip(cur, mot, pmot, hist, gamma, radius, n_max, stat=stat,
                                                             aux=fr["aux"], aux_history=fr["aux_hist"])
                        same(got, want, what)
                        same(got_aux, want_aux, what + " (aux)")
                        same_bytes(img, want, what)
                        got2, img2, none = sc.temporal_clip(cur, mot, pmot, hist, gamma, radius, n_max, stat=stat)
                        assert none is None and got2.tobytes() == got.tobytes() and np.array_equal(img2, img), what
                        go = p["go"]
                        seen["clipped"] += int((go & (p["e"] > 0)).sum())
                        seen["kept"] += int((go & (p["e"] == 0)).sum())
                        seen["reset"] += int((~go).sum())
                        seen["lone"] += int((go & (p["cnt"] == 1)).sum())
                        if gamma == 3e38 and stat is None and n_max:
                            # where no history value left its box the plain blend's bits, from the kernel itself
                            plain, _ = sc.temporal(cur, mot, pmot, hist, n_max=n_max)
                            keep = ~(go & ~(p["e"] == 0))
                            assert w * h < 100 or keep.sum() > 0.5 * keep.size
                            same(got[keep], np.where(np.isnan(want[keep]), want[keep], plain[keep]), what + " vs Scene.temporal")
        same(sc.temporal_clip(cur, mot, pmot, hist)[0],
             K.clip(cur, mot, pmot, hist, float(K.GAMMA_DEFAULT), K.RADIUS_DEFAULT, float(K.N_MAX_DEFAULT), 0.05)[0],
             "defaults spelled out")
    if w * h > 100:  # the branches are all there (the block of lone pixels needs the tall frame's rows)
        assert min(v for k, v in seen.items() if k != "lone" or h > 20) > 0, seen
    elif w * h == 1:
        assert seen["clipped"] + seen["kept"] + seen["reset"] == 54


# ---------------------------------------------------------------- 2  rendered frames
@functools.lru_cache(maxsize=None)
def _moments_pair():
    """The twist pair's poses again with their moments frames (2 spp, sample_base 0 and 2)."""
    import bvh_refit_restate as F

    w, h, spp = 64, 36, 2
    rest, bmin, bmax = _mesh("suzanne.obj")
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(rest) as sc:
        mom0 = sc.trace_moments(cam, w, h, spp)[1]
        sc.update(F.twist(rest, 10.0), "refit")
        sc.set_option("sample_base", spp)
        mom1 = sc.trace_moments(cam, w, h, spp)[1]
    return mom0, mom1


def test_real_frames_clip_bit_for_bit(gpu):
    import torch

    w, h, rad0, mot0, rad1, mot1 = _twist_pair()
    mom0, mom1 = _moments_pair()
    p = K.parts(rad1, mot1, mot0, rad0, aux=mom1, aux_hist=mom0)
    want, want_aux = p["out"], p["aux_out"]
    assert (p["go"] & (p["e"] > 0)).sum() > 20 and (p["go"] & (p["e"] == 0)).sum() > 20 and (~p["go"]).any()
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as sc:  # any scene: it lends its device and stream
        got, img, got_aux = sc.temporal_clip(rad1, mot1, mot0, rad0, aux=mom1, aux_history=mom0)
        same(got, want, "suzanne twist pair")
        same(got_aux, want_aux, "suzanne twist pair, moments")
        same_bytes(img, want, "suzanne twist pair")
        again, again_aux = K.clip(rad0, mot0, mot0, got, aux=mom0, aux_hist=got_aux)  # a history of mixed lengths
        assert len(np.unique(got[..., 3])) > 3
        step2 = sc.temporal_clip(rad0, mot0, mot0, got, aux=mom0, aux_history=got_aux)
        same(step2[0], again, "second step")
        same(step2[2], again_aux, "second step, moments")
        for radius, gamma, n_max in ((2, 0.5, 16.0), (3, 2.0, 32.0)):
            same(sc.temporal_clip(rad1, mot1, mot0, rad0, gamma, radius, n_max, stat=rad0)[0],
                 K.clip(rad1, mot1, mot0, rad0, gamma, radius, n_max, stat=rad0)[0], f"radius {radius}")
        # device pointers: the same bytes, the inputs untouched
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
        host = dict(cur=rad1, hist=rad0, m=mot1, pm=mot0, aux=mom1, aux_hist=mom0)
        t = {k: dev(v) for k, v in host.items()}
        t_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t_aux = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t_8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        size = dict(width=w, height=h)
        ptr = lambda k: t[k].data_ptr()
        assert sc.temporal_clip(ptr("cur"), ptr("m"), ptr("pm"), ptr("hist"), aux=ptr("aux"), aux_history=ptr("aux_hist"),
                                out=(t_out.data_ptr(), t_8.data_ptr(), t_aux.data_ptr()), **size) == (None, None, None)
        assert t_out.cpu().numpy().tobytes() == got.tobytes() and np.array_equal(t_8.cpu().numpy(), img)
        assert t_aux.cpu().numpy().tobytes() == got_aux.tobytes()
        assert sc.stats().render_ms > 0
        t_8.fill_(9)
        t_out.fill_(9.0)
        sc.temporal_clip(ptr("cur"), ptr("m"), ptr("pm"), ptr("hist"), out=(None, t_8.data_ptr(), None), **size)
        assert np.array_equal(t_8.cpu().numpy(), img) and (t_out.cpu().numpy() == 9).all()
        sc.temporal_clip(ptr("cur"), ptr("m"), ptr("pm"), ptr("hist"), stat=ptr("cur"), aux=ptr("aux"),
                         aux_history=ptr("aux_hist"), out=(t_out.data_ptr(), None, ptr("aux")), **size)  # aux_out = aux_cur
        assert t_out.cpu().numpy().tobytes() == got.tobytes() and t["aux"].cpu().numpy().tobytes() == got_aux.tobytes()
        for k in ("cur", "hist", "m", "pm", "aux_hist"):
            assert t[k].cpu().numpy().tobytes() == np.ascontiguousarray(host[k]).tobytes(), k
        # each overlap is refused, device and host form
        o, o8, oa = t_out.data_ptr(), t_8.data_ptr(), t_aux.data_ptr()
        four = (ptr("cur"), ptr("m"), ptr("pm"), ptr("hist"))
        for kw, msg in ((dict(out=(ptr("cur"), o8, None)), "rgba32f_out overlaps rgba32f_cur"),
                        (dict(out=(ptr("aux"), o8, None), stat=ptr("aux")), "rgba32f_out overlaps rgba32f_stat"),
                        (dict(out=(ptr("hist") + 16 * w, o8, None)), "rgba32f_out overlaps rgba32f_history"),
                        (dict(out=(o, o8, ptr("aux_hist")), aux=ptr("aux"), aux_history=ptr("aux_hist")),
                         "aux_out overlaps aux_history"),
                        (dict(out=(o, o8, ptr("cur")), aux=ptr("aux"), aux_history=ptr("aux_hist")),
                         "aux_out overlaps rgba32f_cur")):
            with pytest.raises(tm.TmptError, match=msg):
                sc.temporal_clip(*four, **kw, **size)
        for kw, msg in ((dict(out=rad1), "overlaps rgba32f_cur"), (dict(out=rad0), "overlaps rgba32f_history"),
                        (dict(out=mom1, stat=mom1), "overlaps rgba32f_stat")):
            with pytest.raises(tm.TmptError, match=msg):
                sc.temporal_clip(rad1, mot1, mot0, rad0, **kw)
        assert rad1.tobytes() == _twist_pair()[4].tobytes()


# ---------------------------------------------------------------- 3  buffers, state, CLI, checked build
def test_the_staging_buffer_is_kept(gpu):
    w, h, rad0, mot0, rad1, mot1 = _twist_pair()
    mom0, mom1 = _moments_pair()
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as probe:
        live0 = probe.get_option("live_device_objects")
        with tm.Scene(tris) as sc:
            sc.temporal(rad1, mot1, mot0, rad0)  # the scene's events are there
            live1 = sc.get_option("live_device_objects")
            first = sc.temporal_clip(rad1, mot1, mot0, rad0, stat=rad0, aux=mom1, aux_history=mom0)  # the largest form first
            live2 = sc.get_option("live_device_objects")
            assert live2 == live1 + 1  # the kept staging buffer
            for kw in (dict(), dict(stat=rad0), dict(aux=mom1, aux_history=mom0), dict(stat=rad0, aux=mom1, aux_history=mom0)):
                res = sc.temporal_clip(rad1, mot1, mot0, rad0, **kw)
                assert sc.get_option("live_device_objects") == live2, kw
            assert res[0].tobytes() == first[0].tobytes() and res[2].tobytes() == first[2].tobytes()
            small = extended(5, 3)
            sc.temporal_clip(small["cur"], small["mot"], small["pmot"], small["hist"])
            assert sc.get_option("live_device_objects") == live2
        assert probe.get_option("live_device_objects") == live0


def test_clip_leaves_the_progressive_state_alone(gpu):
    w, h, spp = 32, 18, 8
    tris, bmin, bmax = _mesh("suzanne.obj")
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        rad, _, _ = sc.trace_radiance(cam, w, h, 2)
        mot, _ = sc.trace_motion(cam, cam, w, h)
        alone, _, _ = sc.temporal_clip(rad, mot, mot, rad)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        acc, _, _ = sc.temporal_clip(rad, mot, mot, rad)
        before = sc.stats()
        done, last, r_b = next(passes)
    assert done == spp and np.array_equal(last, once) and r_a + r_b == rays
    assert acc.tobytes() == alone.tobytes() and before.render_ms > 0


def _cli_poses(tris, degrees, frames):
    """tmpt_cli.cpp's --twist poses and mesh bounds (the floor's two triangles
    come last), in its arithmetic: doubles, libm's cos and sin."""
    t = np.asarray(tris, f32).reshape(-1, 3)
    lo, hi = t.astype(np.float64).min(0), t.astype(np.float64).max(0)
    cx, cz, height = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[2] + hi[2]), hi[1] - lo[1]
    for f in range(frames):
        full = degrees * (f / (frames - 1) if frames > 1 else 1.0) * 3.14159265358979323846 / 180.0
        cur = t.copy()
        for i in range(len(t)):
            x, y, z = float(t[i, 0]) - cx, float(t[i, 1]), float(t[i, 2]) - cz
            a = full * (y - lo[1]) / height if height > 0 else 0.0
            cur[i, 0] = f32(cx + math.cos(a) * x + math.sin(a) * z)
            cur[i, 2] = f32(cz - math.sin(a) * x + math.cos(a) * z)
        mesh = cur[:-6] if len(t) > 6 else cur
        yield cur.reshape(-1, 3, 3), mesh.min(0), mesh.max(0)


def test_cli_clip_pngs(gpu, tmp_path):
    w, h, spp, frames = 32, 18, 2, 3
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    stem = str(tmp_path / "tw")
    args = [cli, str(w), str(h), str(spp), data("suzanne.obj"), "--seed", "sample", "--twist", f"20,{frames}", "--out",
            stem + ".png", "--temporal"]
    digest = lambda n: hashlib.sha256(open(str(tmp_path / n), "rb").read()).hexdigest()
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = [digest(f"tw_temporal_{f:03d}.png") for f in range(frames)]
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    for clip, kw in ((["--clip"], {}), (["--clip", "1.5,2,16"], dict(gamma=1.5, radius=2, n_max=16.0))):
        r = subprocess.run(args + clip, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(tmp_path)) == sorted([f"tw_{f:03d}.png" for f in range(frames)] +
                                                      [f"tw_temporal_{f:03d}.png" for f in range(frames)])
        got = [digest(f"tw_temporal_{f:03d}.png") for f in range(frames)]
        want = []
        with tm.Scene(tris) as sc:
            acc = pmot = prev = None
            for f, (pose, lo, hi) in enumerate(_cli_poses(tris, 20.0, frames)):
                sc.set_option("sample_base", f * spp)
                sc.update(pose, "refit")
                sc.build_octree(*tm.octree_bounds(lo, hi))
                rad, img, _ = sc.trace_radiance(cam, w, h, spp)
                mot, _ = sc.trace_motion(cam, cam, w, h, prev)
                if f:
                    acc, img, _ = sc.temporal_clip(rad, mot, pmot, acc, **kw)
                else:
                    acc = rad
                pmot, prev = mot, pose
                tm.write_png(str(tmp_path / "py.png"), img)
                want.append(digest("py.png"))
        os.remove(str(tmp_path / "py.png"))
        assert got == want, clip
        assert got[0] == plain[0] and got[1:] != plain[1:]  # frame 0 is its own history; then the clip shows


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import bvh_refit_restate as F
import toymeshpathtracer_amd as tm
rest, bmin, bmax = tm.load_scene(sys.argv[2])
out = {}
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
try:
    cam = tm.Camera.for_scene(bmin, bmax, 64, 36)
    with tm.Scene(rest) as sc:
        rad0, _, _ = sc.trace_radiance(cam, 64, 36, 2)
        mot0, _ = sc.trace_motion(cam, cam, 64, 36)
        sc.update(F.twist(rest, 10.0), "refit")
        sc.set_option("sample_base", 2)
        rad1, _, _ = sc.trace_radiance(cam, 64, 36, 2)
        mot1, _ = sc.trace_motion(cam, cam, 64, 36, rest)
        for radius in (1, 2, 3):
            acc, img, aux = sc.temporal_clip(rad1, mot1, mot0, rad0, radius=radius, stat=rad0, aux=rad0, aux_history=rad1)
            out["clip%d" % radius] = [sha(acc), sha(img), sha(aux)]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_temporal_clip_checked_build(gpu):
    """The checked library computes the same clipped frames, and no index check fails."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    w, h, rad0, mot0, rad1, mot1 = _twist_pair()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    tris, _, _ = _mesh("cube.obj")
    want = {}
    with tm.Scene(tris) as sc:
        for radius in (1, 2, 3):
            acc, img, aux = sc.temporal_clip(rad1, mot1, mot0, rad0, radius=radius, stat=rad0, aux=rad0, aux_history=rad1)
            want[f"clip{radius}"] = [sha(acc), sha(img), sha(aux)]
    assert got == want
