"""History clipping (Scene.temporal_clip) judged by RMSE against 512-spp frames
on tools/temporal_sweep.py's sequences: suzanne, teapot and the stand-in sponza,
each over a 20 degree twist and static, 16 frames at 4 spp, every frame against
the 512-spp frame of its own pose, RMSE over r, g, b; the figure of a sequence
is the mean over frames 1 .. 15 of accumulated / plain.  The 90 degree
sequences (suzanne, teapot, sponza) are reported apart and choose nothing.

The rules, fixed before the first run:
  grid      n_max {3, 4, 8, 16, 32} x gamma {0.5, 1, 1.5, 2, 3} x radius {1, 2, 3},
            the window statistics from the frame itself (stat = cur)
  yardstick Scene.temporal at n_max 3 (its default) and at every n_max of the
            grid, measured in this run on the same frames
  defaults  the grid point whose worst of the six sequences is best -- the rule
            that chose Scene.temporal's n_max = 3
  stat      for the three best grid points, the statistics taken from
            Scene.denoise(cur) at 2 levels instead
  pipeline  at the chosen point: clip with the moments frame as aux, then
            Scene.denoise_moments, against accumulate-then-denoise
            (Scene.temporal on colour and moments alike at its default and at
            the chosen n_max, then Scene.denoise_moments)

A pixel whose radiance is not finite in any frame of a sequence (counted; the
stand-in sponza has a few) is zeroed before any filter and left out of every RMSE.

  python tools/temporal_clip_sweep.py

profiles/temporal_clip_sweep.log is this tool's output; DESIGN.md "History
clipping" reads the defaults off it."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402
from bvh_refit_restate import twist  # noqa: E402

N_MAX = (3.0, 4.0, 8.0, 16.0, 32.0)
GAMMA = (0.5, 1.0, 1.5, 2.0, 3.0)
RADIUS = (1, 2, 3)
SPP, FRAMES, TRUTH = 4, 16, 512


def rmse(a, b, m):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[m]
    return float(np.sqrt((d * d).mean())) if d.size else float("nan")


def render_sequence(path, is_sponza, w, h, degrees):
    rest, bmin, bmax = tm.load_scene(path)
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
    seq, prev = [], None
    with tm.Scene(rest, bounds=(bmin, bmax)) as sc:
        for f in range(FRAMES):
            pose = twist(rest, degrees * f / (FRAMES - 1))
            sc.update(pose, "refit")
            sc.set_option("sample_base", SPP * f)
            rad, mom = sc.trace_moments(cam, w, h, SPP)[:2]
            aov, _ = sc.trace_aov(cam, w, h, SPP)
            sc.set_option("sample_base", 0)
            truth, _, _ = sc.trace_radiance(cam, w, h, TRUTH)
            mot, _ = sc.trace_motion(cam, cam, w, h, prev)
            seq.append(dict(rad=rad, mom=mom, aov=aov, mot=mot, truth=truth))
            prev = pose
    good = np.ones((h, w), bool)
    for fr in seq:
        good &= np.isfinite(fr["rad"]).all(-1) & np.isfinite(fr["mom"]).all(-1) & np.isfinite(fr["truth"]).all(-1)
    for fr in seq:
        fr["rad"] = np.where(good[..., None], fr["rad"], np.float32(0)).astype(np.float32)
        fr["mom"] = np.where(good[..., None], fr["mom"], np.float32(0)).astype(np.float32)
        fr["mom"][..., 2:][~good] = 1
    return seq, good


class Sequence:
    def __init__(self, sc, name, path, is_sponza, w, h, degrees):
        t0 = time.perf_counter()
        self.sc, self.name = sc, f"{name} {degrees:g}"
        self.seq, self.good = render_sequence(path, is_sponza, w, h, degrees)
        self.e_plain = [rmse(fr["rad"], fr["truth"], self.good) for fr in self.seq]
        print(f"{name} {w}x{h}, {FRAMES} frames over {degrees:g} degrees, {SPP} spp per frame, truth {TRUTH} spp; "
              f"{int((~self.good).sum())} pixels left out (not finite); rendered in {time.perf_counter() - t0:.1f} s",
              flush=True)

    def errors(self, frames):
        return [rmse(x, fr["truth"], self.good) for x, fr in zip(frames, self.seq)]

    def ratio(self, frames):
        return float(np.mean([e / p for e, p in zip(self.errors(frames)[1:], self.e_plain[1:])]))

    def plain(self, n_max, key="rad"):
        out, acc = [], None
        for f, fr in enumerate(self.seq):
            acc = fr[key] if f == 0 else self.sc.temporal(fr[key], fr["mot"], self.seq[f - 1]["mot"], acc, n_max=n_max)[0]
            out.append(acc)
        return out

    def stat2(self):
        """Scene.denoise(cur) at 2 levels, per frame, made once."""
        for fr in self.seq:
            if "stat2" not in fr:
                fr["stat2"] = self.sc.denoise(fr["rad"], fr["aov"], SPP, levels=2)[0]

    def clip(self, n_max, gamma, radius, stat=False, aux=False):
        """-> (accumulated frames, accumulated moments or None)"""
        out, mout, acc, macc = [], [], None, None
        for f, fr in enumerate(self.seq):
            if f == 0:
                acc, macc = fr["rad"], fr["mom"] if aux else None
            else:
                acc, _, macc = self.sc.temporal_clip(fr["rad"], fr["mot"], self.seq[f - 1]["mot"], acc, gamma, radius, n_max,
                                                     stat=fr["stat2"] if stat else None, aux=fr["mom"] if aux else None,
                                                     aux_history=macc)
            out.append(acc)
            mout.append(macc)
        return out, (mout if aux else None)

    def denoised(self, frames, moments):
        return [self.sc.denoise_moments(a, fr["aov"], m, SPP)[0] for a, m, fr in zip(frames, moments, self.seq)]


def grid_table(s):
    """Prints the sequence's tables, returns {(n_max, gamma, radius): ratio} and {n_max: Scene.temporal's ratio}."""
    base = {n: s.ratio(s.plain(n)) for n in N_MAX}
    print("  Scene.temporal / plain;                n_max: " + " ".join(f"{n:7.0f}" for n in N_MAX), flush=True)
    print("                                                " + " ".join(f"{base[n]:7.4f}" for n in N_MAX), flush=True)
    table = {}
    for radius in RADIUS:
        print(f"  Scene.temporal_clip / plain, radius {radius};  gamma \\ n_max", flush=True)
        for gamma in GAMMA:
            for n in N_MAX:
                table[(n, gamma, radius)] = s.ratio(s.clip(n, gamma, radius)[0])
            print(f"    {gamma:5.1f}                                       "
                  + " ".join(f"{table[(n, gamma, radius)]:7.4f}" for n in N_MAX), flush=True)
    return table, base


def point(p):
    return f"n_max {p[0]:g} gamma {p[1]:g} radius {p[2]}"


def main():
    obj = lambda n: os.path.join(ROOT, "data", n)
    sponza = gen_standin_sponza.ensure()
    scenes = (("suzanne", obj("suzanne.obj"), False, 192, 108), ("teapot", obj("teapot.obj"), False, 192, 108),
              ("sponza", sponza, True, 384, 216))
    tris, _, _ = tm.load_scene(obj("cube.obj"))
    with tm.Scene(tris) as sc:  # lends its device to the blends and the filters
        seqs, tables, bases = [], {}, {}
        for deg in (20.0, 0.0):
            for sn in scenes:
                s = Sequence(sc, *sn, deg)
                tables[s.name], bases[s.name] = grid_table(s)
                seqs.append(s)
        names = [s.name for s in seqs]
        worst = {p: max(tables[n][p] for n in names) for p in tables[names[0]]}
        ranked = sorted(worst, key=worst.get)
        best = ranked[0]
        bworst = {n: max(bases[name][n] for name in names) for n in N_MAX}
        print("summary: accumulated / plain (mean over frames 1 .. %d) per sequence (scene, degrees)" % (FRAMES - 1))
        print("  " + " " * 44 + " ".join(f"{n:>11s}" for n in names) + "       worst")
        for n in N_MAX:
            print(f"  Scene.temporal n_max {n:<22g} " + " ".join(f"{bases[name][n]:11.4f}" for name in names)
                  + f" {bworst[n]:11.4f}")
        print("  the ten grid points whose worst sequence is best:")
        for p in ranked[:10]:
            print(f"  clip {point(p):<38s} " + " ".join(f"{tables[name][p]:11.4f}" for name in names) + f" {worst[p]:11.4f}")
        print(f"  chosen (the grid point whose worst sequence is best): {point(best)}, worst {worst[best]:.4f}; "
              f"Scene.temporal at its default n_max 3: worst {bworst[3.0]:.4f}, at its own best n_max "
              f"{min(bworst, key=bworst.get):g}: {min(bworst.values()):.4f}")
        print(f"  the best point per radius: " + "; ".join(
            f"{point(min((p for p in worst if p[2] == r), key=worst.get))} {min(worst[p] for p in worst if p[2] == r):.4f}"
            for r in RADIUS))
        print("  static sequences, clip against Scene.temporal at equal n_max (gamma and radius of the chosen point):")
        for n in N_MAX:
            p = (n, best[1], best[2])
            print(f"    n_max {n:<4g} " + "  ".join(f"{name}: {tables[name][p]:.4f} vs {bases[name][n]:.4f}"
                                                    for name in names if name.endswith(" 0")))

        print("statistics from Scene.denoise(cur) at 2 levels (stat) instead of the frame, the three best points:")
        print("  " + " " * 44 + " ".join(f"{n:>11s}" for n in names) + "       worst")
        for s in seqs:
            s.stat2()
        for p in ranked[:3]:
            row = [s.ratio(s.clip(*p, stat=True)[0]) for s in seqs]
            print(f"  clip {point(p):<30s} stat=cur " + " ".join(f"{tables[name][p]:11.4f}" for name in names)
                  + f" {worst[p]:11.4f}")
            print(f"  clip {point(p):<30s} denoised " + " ".join(f"{e:11.4f}" for e in row) + f" {max(row):11.4f}", flush=True)

        print(f"pipeline at {point(best)}: then Scene.denoise_moments (defaults) with the moments accumulated alongside; "
              "/ plain:")
        print("  " + " " * 44 + " ".join(f"{n:>11s}" for n in names) + "       worst")
        rows = {}
        for n in sorted({3.0, best[0]}):
            rows[f"temporal n_max {n:g} -> denoise_moments"] = [s.ratio(s.denoised(s.plain(n), s.plain(n, "mom"))) for s in seqs]
        rows["clip + aux moments -> denoise_moments"] = [s.ratio(s.denoised(*s.clip(*best, aux=True))) for s in seqs]
        for label, row in rows.items():
            print(f"  {label:<43s} " + " ".join(f"{e:11.4f}" for e in row) + f" {max(row):11.4f}", flush=True)

        print("fast twist (90 degrees over the same frames), reported apart; accumulated / plain, and per frame "
              "for Scene.temporal at n_max 3 | the chosen clip:")
        for sn in scenes:
            s = Sequence(sc, *sn, 90.0)
            print("  Scene.temporal, n_max " + " ".join(f"{n:g}: {s.ratio(s.plain(n)):.4f} " for n in N_MAX))
            for p in ranked[:3]:
                print(f"  clip {point(p)}: {s.ratio(s.clip(*p)[0]):.4f}")
            a, b = s.errors(s.plain(3.0)), s.errors(s.clip(*best)[0])
            print("  frame: " + " ".join(f"{f:11d}" for f in range(1, FRAMES)))
            print("         " + " ".join(f"{x / p:5.3f}|{y / p:5.3f}" for x, y, p in zip(a[1:], b[1:], s.e_plain[1:])),
                  flush=True)


if __name__ == "__main__":
    main()
