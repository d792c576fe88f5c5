"""History-guided sampling judged by RMSE against 512-spp frames on
tools/temporal_clip_sweep.py's six sequences: suzanne, teapot and the stand-in
sponza, each over a 20 degree twist and static, 16 frames, every frame against
the 512-spp frame of its own pose, RMSE over r, g, b.

The guided pipeline, per frame f (sample_base = f * cap): the motion pass, the
sample plan over the accumulated moments of frame f - 1 (frame 0: no prior), the
guided render with its moments, Scene.temporal_clip with the moments frame as
aux; the accumulated colour and moments are the next history.  n_max, gamma and
the clip's radius are temporal_clip's defaults; the adaptive radius is 0.

The rules, fixed before the first run:
  grid        spp_min 2; tau {0.01, 0.015, 0.02, 0.03} x spp_step {2, 4} x cap {8, 16}
  comparator  the same pipeline (motion, uniform Scene.trace_moments, temporal_clip
              with aux) at the uniform spp equal to the guided run's mean samples
              per pixel over the whole sequence, rounded UP: the comparator never
              has fewer samples
  merit       guided / uniform.  Whole frame: the mean over frames 1 .. 15 of the
              two accumulated frames' RMSE ratio.  Restarted pixels: the RMSE pooled
              over frames 1 .. 15 and over the covered pixels whose history
              restarted in that frame (the plan's null prior on a hit pixel; the
              same pixels in both runs, the fetch reads the records alone), guided /
              uniform; n/a where a sequence has none
  default     the grid point whose worst sequence has the best whole-frame merit;
              the feature is opt-in whatever the outcome

A pixel whose radiance or moments are not finite is zeroed before the blend
(moments: 1/n and length 1) and left out of every RMSE of its sequence.

  python tools/guided_sweep.py

profiles/guided_sweep.log is this tool's output; DESIGN.md "History-guided
sampling" reads it."""
import math
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

TAU = (0.01, 0.015, 0.02, 0.03)
STEP = (2, 4)
CAP = (8, 16)
SPP_MIN, FRAMES, TRUTH = 2, 16, 512
GRID = [(tau, step, cap) for cap in CAP for step in STEP for tau in TAU]
NULL = np.array([0, 0, 1, 0], np.float32)


def clean(rad, mom):
    ok = np.isfinite(rad).all(-1) & np.isfinite(mom).all(-1)
    rad = np.where(ok[..., None], rad, np.float32(0)).astype(np.float32)
    mom = np.where(ok[..., None], mom, np.float32(0)).astype(np.float32)
    mom[..., 2:][~ok] = 1
    return rad, mom, ok


def na(v, width):
    return f"{'n/a':>{width}s}" if math.isnan(v) else f"{v:{width}.4f}"


class Run:
    """One pipeline's state over a sequence: the histories, and per frame the squared error map."""

    def __init__(self, h, w):
        self.acc = self.macc = None
        self.se, self.samples = [], 0
        self.bad = np.zeros((h, w), bool)

    def step(self, sc, f, rad, mom, mot, pmot, truth):
        rad, mom, ok = clean(rad, mom)
        self.bad |= ~ok
        if f == 0:
            self.acc, self.macc = rad, mom
        else:
            self.acc, _, self.macc = sc.temporal_clip(rad, mot, pmot, self.acc, aux=mom, aux_history=self.macc)
        d = self.acc[..., :3].astype(np.float64) - truth[..., :3].astype(np.float64)
        self.se.append((d * d).sum(-1))


def poses(sc, rest, cam, w, h, degrees, per_frame):
    """Refits the scene through the sequence; per_frame(f, mot, pmot) runs at each pose."""
    prev = pmot = None
    for f in range(FRAMES):
        pose = twist(rest, degrees * f / (FRAMES - 1))
        sc.update(pose, "refit")
        mot, _ = sc.trace_motion(cam, cam, w, h, prev)
        per_frame(f, mot, pmot)
        prev, pmot = pose, mot


def sequence(name, path, is_sponza, w, h, degrees):
    t0 = time.perf_counter()
    rest, bmin, bmax = tm.load_scene(path)
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
    truths, restarted = [], []
    guided = {p: Run(h, w) for p in GRID}
    with tm.Scene(rest, bounds=(bmin, bmax)) as sc:
        def first(f, mot, pmot):
            sc.set_option("sample_base", 0)
            truth = sc.trace_radiance(cam, w, h, TRUTH)[0]
            truths.append(truth)
            hit = (mot["flags"] & 1) != 0
            for k, p in enumerate(GRID):
                tau, step, cap = p
                r = guided[p]
                prior = sc.sample_plan(mot, pmot, r.macc) if f else None
                if k == 0:  # the fetch reads the records alone: the same pixels restart in every run
                    restarted.append(hit & (prior == NULL).all(-1) if f else np.zeros((h, w), bool))
                sc.set_option("sample_base", f * cap)
                rad, mom, _, _, _, info = sc.trace_guided(cam, w, h, cap, prior, SPP_MIN, step, tau)
                r.samples += info["samples"]
                r.step(sc, f, rad, mom, mot, pmot, truth)
        poses(sc, rest, cam, w, h, degrees, first)
        mean = {p: guided[p].samples / (FRAMES * w * h) for p in GRID}
        need = sorted({max(2, math.ceil(mean[p])) for p in GRID})
        uniform = {u: Run(h, w) for u in need}

        def second(f, mot, pmot):
            for u, r in uniform.items():
                sc.set_option("sample_base", f * u)
                rad, mom = sc.trace_moments(cam, w, h, u)[:2]
                r.step(sc, f, rad, mom, mot, pmot, truths[f])
        poses(sc, rest, cam, w, h, degrees, second)
    good = np.ones((h, w), bool)
    for t in truths:
        good &= np.isfinite(t).all(-1)
    for r in list(guided.values()) + list(uniform.values()):
        good &= ~r.bad
    covered = float(np.mean([((restarted[f] & good).sum() / max(1, (good).sum())) for f in range(1, FRAMES)]))
    label = f"{name} {degrees:g}"
    print(f"{label}: {w}x{h}, {FRAMES} frames, truth {TRUTH} spp; {int((~good).sum())} pixels left out (not finite); "
          f"restarted covered pixels per frame {100 * covered:.2f} % of the frame; {time.perf_counter() - t0:.1f} s", flush=True)
    print("    tau  step cap   mean spp  uniform   whole-frame  restarted", flush=True)
    whole, rest_merit = {}, {}
    for p in GRID:
        g, u = guided[p], uniform[max(2, math.ceil(mean[p]))]
        ratios, sg, su, cnt = [], 0.0, 0.0, 0
        for f in range(1, FRAMES):
            ratios.append(math.sqrt(g.se[f][good].mean() / u.se[f][good].mean()))
            m = restarted[f] & good
            sg, su, cnt = sg + g.se[f][m].sum(), su + u.se[f][m].sum(), cnt + int(m.sum())
        whole[p] = float(np.mean(ratios))
        rest_merit[p] = math.sqrt(sg / su) if cnt and su > 0 else float("nan")
        print(f"  {p[0]:6.3f} {p[1]:4d} {p[2]:3d}   {mean[p]:8.3f}  {max(2, math.ceil(mean[p])):7d}   {whole[p]:11.4f}  "
              f"{na(rest_merit[p], 9)}", flush=True)
    return label, whole, rest_merit, mean


def main():
    obj = lambda n: os.path.join(ROOT, "data", n)
    sponza = gen_standin_sponza.ensure()
    scenes = (("suzanne", obj("suzanne.obj"), False, 192, 108), ("teapot", obj("teapot.obj"), False, 192, 108),
              ("sponza", sponza, True, 384, 216))
    print(f"guided / uniform RMSE against {TRUTH}-spp frames; spp_min {SPP_MIN}; the comparator's spp is the guided run's "
          "mean samples per pixel rounded up", flush=True)
    results = [sequence(*sn, deg) for deg in (20.0, 0.0) for sn in scenes]
    names = [r[0] for r in results]
    worst = {p: max(r[1][p] for r in results) for p in GRID}
    ranked = sorted(GRID, key=worst.get)
    print("summary: whole-frame merit (guided / uniform, below 1 = guided wins) per sequence")
    print("    tau  step cap " + " ".join(f"{n:>11s}" for n in names) + "       worst")
    for p in ranked:
        print(f"  {p[0]:6.3f} {p[1]:4d} {p[2]:3d} " + " ".join(f"{r[1][p]:11.4f}" for r in results) + f" {worst[p]:11.4f}")
    print("summary: restarted-pixel merit per sequence (n/a: no covered pixel restarted)")
    for p in ranked:
        print(f"  {p[0]:6.3f} {p[1]:4d} {p[2]:3d} " + " ".join(na(r[2][p], 11) for r in results))
    best = ranked[0]
    wins = worst[best] < 1.0
    print(f"chosen (the grid point whose worst sequence is best): tau {best[0]:g} step {best[1]} cap {best[2]}, worst "
          f"{worst[best]:.4f}: " + ("it wins on its worst sequence" if wins else
                                    "NO grid point wins on its worst sequence; it loses on "
                                    + ", ".join(r[0] for r in results if r[1][best] >= 1.0)))


if __name__ == "__main__":
    main()
