"""Adaptive sampling's defaults (tmpt_adaptive_desc: spp_min, spp_step, threshold, radius),
judged by RMSE against a 512-spp frame at equal samples: for suzanne, teapot and
the stand-in sponza at 384x216 and the stand-in sponza at 960x540, cap S = 64,
a grid of tau, a few (spp_min, spp_step) pairs and the radii of the neighbourhood
rule.  Every point reports

  E_ad   the adaptive frame's RMSE in display space (saturate(sqrtf(k)) of the
         float frame, over r, g, b) against the 512-spp uniform frame
  E_un   the same for the uniform frame (Scene.trace_radiance) whose spp is the
         adaptive run's samples per pixel rounded up
  both ray counts, and the ratio E_ad / E_un (below 1: adaptive wins at equal samples)

A pixel whose radiance is not finite in the 512-spp frame or in either frame
compared (counted) is left out of both RMSEs.  Last, per point, the scenes on
which it has the lowest ratio: the defaults are the point that wins on the
most scenes (ties: the lowest mean ratio).

  python tools/adaptive_sweep.py [radius ...]     (default: 0 1 2 4)

profiles/adaptive_sweep.log is this tool's output at radius 0 alone, from before
it had the axis (DESIGN.md "Adaptive sampling" reads the defaults off it);
profiles/adaptive_nb_sweep.log its output over the four radii ("Neighbourhood
rule").  Last of all, per (spp_min, spp_step, tau), the ratio at each radius
side by side."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402

CAP = 64
TAUS = (0.0025, 0.005, 0.01, 0.015, 0.02, 0.03, 0.05)
PAIRS = ((4, 4), (8, 8), (8, 16), (16, 8), (16, 16), (24, 8), (32, 16))
RADII = (0, 1, 2, 4)


def display(rad):
    return np.clip(np.sqrt(np.maximum(rad[..., :3].astype(np.float64), 0.0)), 0.0, 1.0)


def rmse(a, b, m):
    d = (display(a) - display(b))[m]
    return float(np.sqrt((d * d).mean()))


def main():
    radii = tuple(int(a) for a in sys.argv[1:]) or RADII
    obj = lambda n: os.path.join(ROOT, "data", n)
    sponza = gen_standin_sponza.ensure()
    scenes = [("suzanne", obj("suzanne.obj"), False, 384, 216), ("teapot", obj("teapot.obj"), False, 384, 216),
              ("sponza", sponza, True, 384, 216), ("sponza", sponza, True, 960, 540)]
    ratios = {}  # point -> {scene label: ratio}
    for name, path, is_sponza, w, h in scenes:
        label = f"{name} {w}x{h}"
        tris, bmin, bmax = tm.load_scene(path)
        cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
        with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
            truth, _, _ = sc.trace_radiance(cam, w, h, 512)
            bad = ~np.isfinite(truth).all(-1)
            uniform = {}
            print(f"{label}, cap {CAP}: non-finite pixels at 512 spp {int(bad.sum())}", flush=True)
            print("  spp_min spp_step    tau  r | passes samples/pixel |    E_ad    rays_ad | spp_un    E_un    rays_un | E_ad/E_un")
            for spp_min, spp_step in PAIRS:
                for tau, radius in ((t, r) for t in TAUS for r in radii):
                    rad, _, n_p, rays, info = sc.trace_adaptive(cam, w, h, CAP, spp_min, spp_step, tau, radius=radius)
                    mean = info["samples"] / (w * h)
                    k = min(CAP, int(np.ceil(mean)))
                    if k not in uniform:
                        uniform[k] = sc.trace_radiance(cam, w, h, k)
                    u_rad, _, u_rays = uniform[k]
                    m = ~(bad | ~np.isfinite(rad).all(-1) | ~np.isfinite(u_rad).all(-1))
                    e_ad, e_un = rmse(rad, truth, m), rmse(u_rad, truth, m)
                    ratios.setdefault((spp_min, spp_step, tau, radius), {})[label] = e_ad / e_un
                    print(f"  {spp_min:7d} {spp_step:8d} {tau:6.4f} {radius:2d} | {info['passes']:6d} {mean:13.2f} | {e_ad:7.5f} "
                          f"{rays:10d} | {k:6d} {e_un:7.5f} {u_rays:10d} | {e_ad / e_un:9.4f}"
                          f"{'' if m.sum() == m.size else f'  ({int(m.size - m.sum())} pixels left out)'}", flush=True)
    labels = [f"{n} {w}x{h}" for n, _, _, w, h in scenes]
    best = {lb: min(ratios, key=lambda p: ratios[p][lb]) for lb in labels}
    print("lowest ratio per scene: " + "; ".join(f"{lb}: {best[lb]} {ratios[best[lb]][lb]:.4f}" for lb in labels))
    print("  spp_min spp_step    tau  r | wins | mean ratio | " + " | ".join(labels))
    order = sorted(ratios, key=lambda p: (-sum(best[lb] == p for lb in labels), np.mean(list(ratios[p].values()))))
    for p in order:
        print(f"  {p[0]:7d} {p[1]:8d} {p[2]:6.4f} {p[3]:2d} | {sum(best[lb] == p for lb in labels):4d} | "
              f"{np.mean(list(ratios[p].values())):10.4f} | " + " | ".join(f"{ratios[p][lb]:.4f}" for lb in labels))
    print(f"the defaults by this rule: spp_min {order[0][0]}, spp_step {order[0][1]}, tau {order[0][2]}, "
          f"radius {order[0][3]}")
    # the radius axis: per (spp_min, spp_step, tau) and scene, the ratio at each radius
    print("ratio by radius " + " / ".join(str(r) for r in radii) + ":")
    print("  spp_min spp_step    tau | " + " | ".join(f"{lb:>{7 * len(radii) - 1}s}" for lb in labels))
    for spp_min, spp_step in PAIRS:
        for tau in TAUS:
            print(f"  {spp_min:7d} {spp_step:8d} {tau:6.4f} | " + " | ".join(
                " ".join(f"{ratios[(spp_min, spp_step, tau, r)][lb]:6.3f}" for r in radii) for lb in labels))
    for r in radii:  # how often a radius beats radius 0 at the same (spp_min, spp_step, tau), per scene
        if r == radii[0]:
            continue
        wins = [sum(ratios[(a, b, t, r)][lb] < ratios[(a, b, t, radii[0])][lb] for a, b in PAIRS for t in TAUS)
                for lb in labels]
        print(f"radius {r} below radius {radii[0]} at " + "; ".join(f"{lb}: {v} of {len(PAIRS) * len(TAUS)} points"
                                                                     for lb, v in zip(labels, wins)))


if __name__ == "__main__":
    main()
