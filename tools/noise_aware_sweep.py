"""The noise-aware filter (Scene.denoise_moments) judged by RMSE against 512-spp
frames, over shrink in {1, 2, 4, 8, 16} at 5 levels, beside the plain filter
(Scene.denoise) and the unfiltered frame.  Every E is an RMSE over r, g, b.

Three groups of rows:
  uniform   the seven frames of tools/denoise_sweep.py at 4 and at 64 spp:
            radiance and moments from Scene.trace_moments (uniform), AOVs at the
            same spp
  adaptive  the four frames of tools/adaptive_sweep.py, cap 64, the adaptive
            defaults (spp_min 24, spp_step 8, tau 0.015): each pixel's moments at
            its own count n_p, AOVs at 64 spp
  temporal  the static and the 20 degree sequences of tools/temporal_sweep.py
            (16 frames, 4 spp a frame, a refit per frame) at n_max 3 and 16: colour
            and moments are accumulated alike (Scene.temporal), then a copy of the
            accumulated frame is filtered both ways; E is the mean over frames
            1 .. 15, each frame against the 512-spp frame of its own pose

The rule for the default shrink, fixed before the run: per row the figure of
merit is E_new / min(E_plain-filtered, E_unfiltered), what the new filter costs
against the better of the two choices there were; the default is the grid
point whose worst row is smallest.  The rows where the new filter still loses
at that point (a figure above 1) are listed at the end.

A pixel whose radiance is not finite in a frame compared (counted; the stand-in
sponza has a few) is zeroed, moments too, before any filter and left out of
every RMSE.

  python tools/noise_aware_sweep.py

profiles/noise_aware_sweep.log is this tool's output; DESIGN.md "Noise-aware
filter" reads the default off it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402
from bvh_refit_restate import twist  # noqa: E402

SHRINK = (1.0, 2.0, 4.0, 8.0, 16.0)
LEVELS, TRUTH = 5, 512
SPP_T, FRAMES = 4, 16  # the temporal sequences
ROWS = []  # (label, E_unfiltered, E_plain, [E_new per shrink])


def rmse(a, b, m):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[m]
    return float(np.sqrt((d * d).mean())) if d.size else float("nan")


def zeroed(a, bad):
    return np.where(bad[..., None], np.float32(0), a).astype(np.float32)


def row(label, e_raw, e_plain, e_new):
    ROWS.append((label, e_raw, e_plain, list(e_new)))
    ref = min(e_raw, e_plain)
    print(f"  {label:<34s} {e_raw:8.5f} {e_plain / e_raw:7.3f}  " + " ".join(f"{e / e_raw:7.3f}" for e in e_new)
          + "   | " + " ".join(f"{e / ref:6.3f}" for e in e_new), flush=True)


def head(what):
    print(f"{what}\n  {'frame':<34s} {'E_unf':>8s} {'plain':>7s}  " + " ".join(f"s={s:<5g}" for s in SHRINK)
          + "   | E_new / min(E_plain, E_unf): " + " ".join(f"s={s:<4g}" for s in SHRINK), flush=True)


def filtered(sc, rad, aov, mom, spp):
    plain = sc.denoise(rad, aov, spp, levels=LEVELS)[0]
    return plain, [sc.denoise_moments(rad, aov, mom, spp, shrink=s, levels=LEVELS)[0] for s in SHRINK]


def uniform_and_adaptive(obj, sponza):
    frames = [("suzanne", obj("suzanne.obj"), False, 96, 54), ("teapot", obj("teapot.obj"), False, 96, 54),
              ("suzanne", obj("suzanne.obj"), False, 384, 216), ("teapot", obj("teapot.obj"), False, 384, 216),
              ("sponza", sponza, True, 96, 54), ("sponza", sponza, True, 384, 216), ("sponza", sponza, True, 960, 540)]
    adaptive = {("suzanne", 384, 216), ("teapot", 384, 216), ("sponza", 384, 216), ("sponza", 960, 540)}
    head("uniform frames at 4 and 64 spp, adaptive frames (cap 64, the defaults); columns: E / E_unfiltered")
    for name, path, is_sponza, w, h in frames:
        tris, bmin, bmax = tm.load_scene(path)
        cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
        with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
            truth, _, _ = sc.trace_radiance(cam, w, h, TRUTH)
            cases = [(f"{name} {w}x{h} {spp} spp", spp, None) for spp in (4, 64)]
            if (name, w, h) in adaptive:
                cases.append((f"{name} {w}x{h} adaptive", 64, 0))
            for label, spp, spp_min in cases:
                rad, mom, _, n_p, _, _ = sc.trace_moments(cam, w, h, spp, spp_min=spp_min)
                aov, _ = sc.trace_aov(cam, w, h, spp)
                bad = ~np.isfinite(rad).all(-1) | ~np.isfinite(mom).all(-1)
                m = ~(bad | ~np.isfinite(truth).all(-1))
                rad, mom = zeroed(rad, bad), zeroed(mom, bad)
                mom[..., 2:][bad] = 1  # a zeroed pixel: one sample, no variance
                plain, new = filtered(sc, rad, aov, mom, spp)
                if spp_min is not None:
                    label += f" (mean n_p {float(n_p.mean()):.1f})"
                row(label + (f" [{int((~m).sum())} px out]" if (~m).any() else ""), rmse(rad, truth, m),
                    rmse(plain, truth, m), [rmse(x, truth, m) for x in new])


def temporal(sc, name, path, is_sponza, w, h, degrees):
    rest, bmin, bmax = tm.load_scene(path)
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
    seq, prev = [], None
    with tm.Scene(rest, bounds=(bmin, bmax)) as rs:
        for f in range(FRAMES):
            pose = twist(rest, degrees * f / (FRAMES - 1))
            rs.update(pose, "refit")
            rs.set_option("sample_base", SPP_T * f)
            rad, mom = rs.trace_moments(cam, w, h, SPP_T)[:2]
            aov, _ = rs.trace_aov(cam, w, h, SPP_T)
            rs.set_option("sample_base", 0)
            truth, _, _ = rs.trace_radiance(cam, w, h, TRUTH)
            mot, _ = rs.trace_motion(cam, cam, w, h, prev)
            seq.append(dict(rad=rad, mom=mom, aov=aov, mot=mot, truth=truth))
            prev = pose
    good = np.ones((h, w), bool)
    for fr in seq:
        good &= np.isfinite(fr["rad"]).all(-1) & np.isfinite(fr["mom"]).all(-1) & np.isfinite(fr["truth"]).all(-1)
    for fr in seq:
        fr["rad"], fr["mom"] = zeroed(fr["rad"], ~good), zeroed(fr["mom"], ~good)
        fr["mom"][..., 2:][~good] = 1
    for n_max in (3.0, 16.0):
        e_raw, e_plain, e_new = [], [], [[] for _ in SHRINK]
        acc = macc = None
        for f, fr in enumerate(seq):
            if f == 0:
                acc, macc = fr["rad"], fr["mom"]
                continue
            acc = sc.temporal(fr["rad"], fr["mot"], seq[f - 1]["mot"], acc, n_max=n_max)[0]
            macc = sc.temporal(fr["mom"], fr["mot"], seq[f - 1]["mot"], macc, n_max=n_max)[0]
            plain, new = filtered(sc, acc, fr["aov"], macc, SPP_T)
            e_raw.append(rmse(acc, fr["truth"], good))
            e_plain.append(rmse(plain, fr["truth"], good))
            for k, x in enumerate(new):
                e_new[k].append(rmse(x, fr["truth"], good))
        row(f"{name} {w}x{h} {degrees:g} deg n_max {n_max:g}", float(np.mean(e_raw)), float(np.mean(e_plain)),
            [float(np.mean(e)) for e in e_new])


def main():
    obj = lambda n: os.path.join(ROOT, "data", n)
    sponza = gen_standin_sponza.ensure()
    print(f"shrink grid {SHRINK}, {LEVELS} levels, truth {TRUTH} spp", flush=True)
    uniform_and_adaptive(obj, sponza)
    head(f"temporal: {FRAMES} frames at {SPP_T} spp, accumulated colour and moments, then filtered; E = mean over "
         f"frames 1 .. {FRAMES - 1}; E_unf = the accumulated frame's")
    tris, _, _ = tm.load_scene(obj("cube.obj"))
    with tm.Scene(tris) as sc:  # lends its device to the blends and the filters
        for deg in (0.0, 20.0):
            temporal(sc, "suzanne", obj("suzanne.obj"), False, 192, 108, deg)
            temporal(sc, "teapot", obj("teapot.obj"), False, 192, 108, deg)
            temporal(sc, "sponza", sponza, True, 384, 216, deg)
    merit = lambda r, k: r[3][k] / min(r[1], r[2])
    print("the rule: per shrink, the worst row of E_new / min(E_plain-filtered, E_unfiltered), and its mean")
    worst = {}
    for k, s in enumerate(SHRINK):
        col = [merit(r, k) for r in ROWS]
        worst[s] = max(col)
        print(f"  shrink {s:4g}: worst {max(col):.3f} ({ROWS[int(np.argmax(col))][0]}), mean {float(np.mean(col)):.3f}, "
              f"rows above 1: {sum(c > 1 for c in col)} of {len(col)}")
    best = min(worst, key=worst.get)
    k = SHRINK.index(best)
    print(f"the grid point whose worst row is smallest: shrink {best:g}")
    print(f"rows where the new filter still loses at shrink {best:g} (E_new / the better of the two, and which that is):")
    for r in ROWS:
        if merit(r, k) > 1:
            print(f"  {r[0]:<40s} {merit(r, k):.3f}  (against the {'plain filter' if r[2] < r[1] else 'unfiltered frame'})")


if __name__ == "__main__":
    main()
