"""Temporal accumulation judged by RMSE against 512-spp frames: the CLI's
--twist sequence (tests/bvh_refit_restate.py twist: DEG at the top, nothing at
the bottom, frame f at DEG * f / (FRAMES - 1), a refit per frame, the camera
staying frame 0's) on suzanne, teapot and the stand-in sponza at 4 spp per
frame, every frame against the 512-spp frame of its own pose, RMSE over r, g, b.

Five variants per frame:
  plain      the 4-spp frame (sample_base = 4 f)
  plain+dn   that frame through Scene.denoise (defaults, AOVs at 4 spp)
  acc        the accumulated frame: blended with the kept accumulation of the
             frames before it (Scene.temporal), frame 0 being its own
  acc+dn     a copy of the accumulated frame through Scene.denoise (the
             accumulation itself stays the history: DESIGN.md's order)
  acc@0      accumulated likewise, but every frame rendered at sample_base = 0:
             what the option buys
The per-frame table is at the defaults; then, over a grid of n_max and
sigma_depth, the mean over frames 1 .. FRAMES-1 of each accumulated variant's
RMSE / the plain frame's.  Every scene is taken twice, over the 20 degree twist
and static (0 degrees: what a long history buys where nothing moves); a last
block repeats suzanne and the stand-in sponza with a fast twist (90 degrees
over the same frames).  Every block ends with the share of the last frame's
covered pixels whose history restarted in that frame (length < 2) and the RMSE
ratio on them.  The summary sets the grid's n_max (at sigma_depth 0.05) and
sigma_depth (at the n_max chosen) side by side over the six gridded blocks,
with the worst block of each: the defaults are the grid point whose worst block
is best.

A pixel whose radiance is not finite in any frame of a sequence (counted; the
stand-in sponza has a few) is zeroed before any filter and left out of every RMSE.

  python tools/temporal_sweep.py

profiles/temporal_sweep.log is this tool's output; DESIGN.md "Temporal
accumulation" reads the defaults off it."""
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

N_MAX = (2.0, 3.0, 4.0, 6.0, 8.0, 16.0, 32.0)
SIGMA_DEPTH = (0.01, 0.02, 0.05, 0.1, 0.2)
SPP, FRAMES, TRUTH = 4, 16, 512


def rmse(a, b, m):
    d = (a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))[m]
    return float(np.sqrt((d * d).mean())) if d.size else float("nan")


def clean(a):
    return np.where(np.isfinite(a).all(-1, keepdims=True), a, np.float32(0)).astype(np.float32)


def render_sequence(path, is_sponza, w, h, degrees):
    """Per frame: the plain frame at its own base and at base 0, the AOVs, the motion records, the truth."""
    rest, bmin, bmax = tm.load_scene(path)
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=is_sponza)
    seq = []
    with tm.Scene(rest, bounds=(bmin, bmax)) as sc:
        prev = None
        for f in range(FRAMES):
            pose = twist(rest, degrees * f / (FRAMES - 1))
            sc.update(pose, "refit")
            sc.set_option("sample_base", SPP * f)
            rad, _, _ = sc.trace_radiance(cam, w, h, SPP)
            aov, _ = sc.trace_aov(cam, w, h, SPP)
            sc.set_option("sample_base", 0)
            rad0, _, _ = sc.trace_radiance(cam, w, h, SPP)
            truth, _, _ = sc.trace_radiance(cam, w, h, TRUTH)
            mot, _ = sc.trace_motion(cam, cam, w, h, prev)
            seq.append(dict(rad=rad, rad0=rad0, aov=aov, mot=mot, truth=truth))
            prev = pose
        good = np.ones((h, w), bool)
        for fr in seq:
            for k in ("rad", "rad0", "truth"):
                good &= np.isfinite(fr[k]).all(-1)
        for fr in seq:
            fr["rad"], fr["rad0"] = clean(fr["rad"]), clean(fr["rad0"])
    return seq, good


def accumulate(sc, seq, key, n_max, sigma):
    out, acc = [], None
    for f, fr in enumerate(seq):
        acc = fr[key] if f == 0 else sc.temporal(fr[key], fr["mot"], seq[f - 1]["mot"], acc, n_max=n_max, sigma_depth=sigma)[0]
        out.append(acc)
    return out


def block(sc, name, path, is_sponza, w, h, degrees, grid):
    seq, good = render_sequence(path, is_sponza, w, h, degrees)
    print(f"{name} {w}x{h}, {FRAMES} frames over {degrees:g} degrees, {SPP} spp per frame, truth {TRUTH} spp; "
          f"{int((~good).sum())} pixels left out (not finite)", flush=True)
    e_plain = [rmse(fr["rad"], fr["truth"], good) for fr in seq]
    acc = accumulate(sc, seq, "rad", 0.0, 0.0)
    acc0 = accumulate(sc, seq, "rad0", 0.0, 0.0)
    print("  frame   plain  plain+dn     acc    acc+dn   acc@0   mean history", flush=True)
    for f, fr in enumerate(seq):
        dn = sc.denoise(fr["rad"], fr["aov"], SPP)[0]
        adn = sc.denoise(acc[f], fr["aov"], SPP)[0]
        print(f"  {f:5d} {e_plain[f]:7.4f}  {rmse(dn, fr['truth'], good):7.4f} {rmse(acc[f], fr['truth'], good):7.4f}  "
              f"{rmse(adn, fr['truth'], good):7.4f} {rmse(acc0[f], fr['truth'], good):7.4f}   {float(acc[f][..., 3].mean()):6.2f}",
              flush=True)
    last = seq[-1]
    cov = ((last["mot"]["flags"] & 1) != 0) & good
    fresh = cov & (acc[-1][..., 3] < 2)
    print(f"  last frame: {int(fresh.sum())} of {int(cov.sum())} covered pixels restarted their history "
          f"({100.0 * fresh.sum() / max(1, cov.sum()):.1f} %); on them acc / plain = "
          f"{rmse(acc[-1], last['truth'], fresh) / rmse(last['rad'], last['truth'], fresh):.3f}, on the other covered "
          f"pixels {rmse(acc[-1], last['truth'], cov & ~fresh) / rmse(last['rad'], last['truth'], cov & ~fresh):.3f}", flush=True)
    if not grid:
        return None
    table = {}
    mean = lambda es: float(np.mean([e / p for e, p in zip(es[1:], e_plain[1:])]))
    for label, key, dn in (("acc", "rad", False), ("acc+dn", "rad", True), ("acc@0", "rad0", False)):
        print(f"  {label} / plain, mean over frames 1 .. {FRAMES - 1};  n_max \\ sigma_depth: "
              + " ".join(f"{s:7.3f}" for s in SIGMA_DEPTH), flush=True)
        for n_max in N_MAX:
            row = []
            for s in SIGMA_DEPTH:
                a = accumulate(sc, seq, key, n_max, s)
                if dn:
                    a = [sc.denoise(x, fr["aov"], SPP)[0] for x, fr in zip(a, seq)]
                row.append(mean([rmse(x, fr["truth"], good) for x, fr in zip(a, seq)]))
                if label == "acc":
                    table[(n_max, s)] = row[-1]
            print(f"    {n_max:5.0f}                                       " + " ".join(f"{e:7.4f}" for e in row), flush=True)
    return table


def main():
    obj = lambda n: os.path.join(ROOT, "data", n)
    sponza = gen_standin_sponza.ensure()
    tris, _, _ = tm.load_scene(obj("cube.obj"))
    with tm.Scene(tris) as sc:  # lends its device to the blends and the filters
        tables = {}
        for deg in (20.0, 0.0):
            tables[f"suzanne {deg:g}"] = block(sc, "suzanne", obj("suzanne.obj"), False, 192, 108, deg, True)
            tables[f"teapot {deg:g}"] = block(sc, "teapot", obj("teapot.obj"), False, 192, 108, deg, True)
            tables[f"sponza {deg:g}"] = block(sc, "sponza", sponza, True, 384, 216, deg, True)
        block(sc, "suzanne", obj("suzanne.obj"), False, 192, 108, 90.0, False)
        block(sc, "sponza", sponza, True, 384, 216, 90.0, False)
    names = list(tables)
    print("summary: acc / plain (mean over frames 1 .. %d) per block (scene, degrees)" % (FRAMES - 1))
    print("  at sigma_depth 0.05;  n_max: " + " ".join(f"{n:>12s}" for n in names) + "        worst")
    worst = {}
    for n_max in N_MAX:
        row = [tables[n][(n_max, 0.05)] for n in names]
        worst[n_max] = max(row)
        print(f"  {n_max:26.0f}  " + " ".join(f"{e:12.4f}" for e in row) + f" {max(row):12.4f}")
    best = min(worst, key=worst.get)
    print(f"  the n_max whose worst block is best: {best:g}")
    print(f"  at n_max {best:g};  sigma_depth: " + " ".join(f"{n:>12s}" for n in names) + "        worst")
    worst_s = {}
    for s in SIGMA_DEPTH:
        row = [tables[n][(best, s)] for n in names]
        worst_s[s] = max(row)
        print(f"  {s:26.3f}  " + " ".join(f"{e:12.4f}" for e in row) + f" {max(row):12.4f}")
    print(f"  the sigma_depth whose worst block is best: {min(worst_s, key=worst_s.get):g}")


if __name__ == "__main__":
    main()
