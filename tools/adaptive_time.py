"""Adaptive sampling's pass machinery on the bench frame -- stand-in sponza
1920x1080, cap S = 64, sample seeding, the reference octree built -- in one
process on one GPU, every output on the device.  Variants, interleaved, one
warm-up round, then `rounds` timed rounds; medians and the spread (max - min):

  (a) tmpt_render, one call
  (b) the progressive render in 8 passes of 8 (spp_begin / spp_count): the
      baseline for the pass machinery
  (c) tmpt_render_adaptive with tau = 0, (spp_min, spp_step) = (8, 8): the passes
      of (b) plus the update and compaction kernels and the wait after each pass
      -- over every pixel but those whose samples so far all agree (their
      variance is 0, which is not > 0: such a pixel stops whatever tau is), so
      the two are compared by k_path's time per ray as well
  (d) tmpt_render_adaptive with the defaults
  (b0), (c0): (b) and (c) with render option cam_pre = 0
  (dR) for every radius R > 0 given: (d) with the neighbourhood rule at that
      radius (tmpt_adaptive_desc.radius).  Different radii trace different
      samples, so they are compared by the rest per pass and by k_path's time
      per ray, which the table's last lines give

Per variant: tmpt_stats.render_ms (for (b) the sum over its calls), the host's
wall time around the call(s), extend_ms (the k_path launches alone) and the
rest, render_ms - extend_ms - redo_ms: everything of a call that is not path
tracing -- (b): the camera pre-passes and the resolves; (c), (d): the camera
pre-pass of pass 0, the update, scan and scatter kernels, the final kernel and
the host's wait after each pass.  (c) may exceed (b) by the difference of
those rests plus the spread.

For (d) also the time per pass against the pixels it traced: the call with the
cap cut to n_k runs passes 0..k with the same pixels (the test of a pass reads
only the samples so far), so pass k's time is the difference of two such calls.

  python tools/adaptive_time.py [rounds, default 5] [cap, default 64] [radius ...]

profiles/adaptive_time.log is this tool's output (DESIGN.md "Adaptive sampling"),
profiles/adaptive_nb_time.log its output with radii 1 and 2 ("Neighbourhood rule")."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402


SPP_MIN, SPP_STEP = 24, 8  # the library's defaults (include/tmpt.h tmpt_adaptive_desc)


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cap = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    radii = [int(a) for a in sys.argv[3:]]
    w, h = 1920, 1080
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    t32 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    tn = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
    outs = (t32.data_ptr(), t8.data_ptr(), tn.data_ptr())
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        def stat():
            st = sc.stats()
            return np.array([st.render_ms, st.extend_ms, st.render_ms - st.extend_ms - st.redo_ms])

        def run_a():
            _, rays = sc.trace_image(cam, w, h, cap, seed_mode=tm.SEED_SAMPLE, out=t8.data_ptr())
            return stat(), rays, None

        def run_b():
            tot, rays = np.zeros(3), 0
            for b in range(0, cap, 8):
                _, r = sc.trace_image(cam, w, h, cap, seed_mode=tm.SEED_SAMPLE, out=t8.data_ptr(), spp_begin=b,
                                      spp_count=min(8, cap - b))
                tot += stat()
                rays += r
            return tot, rays, None

        def run_b0():
            sc.set_option("cam_pre", 0)
            try:
                return run_b()
            finally:
                sc.set_option("cam_pre", -1)

        def run_c0():
            sc.set_option("cam_pre", 0)
            try:
                return run_c()
            finally:
                sc.set_option("cam_pre", -1)

        def run_c():
            _, _, _, rays, info = sc.trace_adaptive(cam, w, h, cap, 8, 8, 0.0, out=outs)
            return stat(), rays, info

        def run_d():
            _, _, _, rays, info = sc.trace_adaptive(cam, w, h, cap, out=outs)
            return stat(), rays, info

        def run_dr(radius):
            def run():
                _, _, _, rays, info = sc.trace_adaptive(cam, w, h, cap, out=outs, radius=radius)
                return stat(), rays, info
            return run

        variants = (("a", "tmpt_render", run_a), ("b", "progressive, 8 passes of 8", run_b),
                    ("c", "adaptive, tau 0, (8, 8)", run_c), ("d", "adaptive, defaults", run_d),
                    ("b0", "(b) with cam_pre = 0", run_b0), ("c0", "(c) with cam_pre = 0", run_c0))
        variants += tuple((f"d{r}", f"adaptive, defaults, radius {r}", run_dr(r)) for r in radii)
        res = {k: [] for k, _, _ in variants}
        wall = {k: [] for k, _, _ in variants}
        last = {}
        for rnd in range(rounds + 1):  # round 0 warms every variant up
            for k, _, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s, rays, info = fn()
                t1 = time.perf_counter()
                last[k] = (rays, info)
                if rnd:
                    res[k].append(s)
                    wall[k].append((t1 - t0) * 1e3)
        assert last["a"][0] == last["b"][0], "the passes trace the frame's samples"
        # (tau 0 stops a pixel whose samples so far all agree -- var = 0 is not > 0 -- so (c) can trace a few fewer)
        print(f"bench frame {w}x{h}, cap {cap}, sample seeding, {rounds} rounds after a warm-up, variants interleaved; "
              "ms, median (spread)", flush=True)
        for k, name, _ in variants:
            a = np.array(res[k])
            cols = [med(a[:, i]) for i in range(3)]
            wm, ws = med(wall[k])
            rays, info = last[k]
            ns = cols[1][0] * 1e6 / rays
            print(f"  ({k:2s}) {name:30s}: render_ms {cols[0][0]:8.3f} ({cols[0][1]:6.3f})  wall {wm:8.3f} ({ws:6.3f})  "
                  f"extend_ms {cols[1][0]:8.3f} ({cols[1][1]:6.3f})  rest {cols[2][0]:7.3f} ({cols[2][1]:6.3f})  "
                  f"rays {rays} ({ns:.4f} ns of k_path per ray)" + (f"  samples {info['samples']} of {w * h * cap}" if info else ""), flush=True)
        mb, mc = med(np.array(res["b"])[:, 0]), med(np.array(res["c"])[:, 0])
        rb, rc = med(np.array(res["b"])[:, 2]), med(np.array(res["c"])[:, 2])
        print(f"  (c) - (b): render_ms {mc[0] - mb[0]:+.3f} ms; the rests differ by {rc[0] - rb[0]:+.3f} ms; spreads "
              f"{mb[1]:.3f} / {mc[1]:.3f} ms", flush=True)
        for r in radii:  # the rest per pass against (d)'s
            rd, rr = med(np.array(res["d"])[:, 2]), med(np.array(res[f"d{r}"])[:, 2])
            pd, pr = last["d"][1]["passes"], last[f"d{r}"][1]["passes"]
            print(f"  (d{r}) against (d): rest per pass {rr[0] / pr:.3f} ms ({pr} passes) against {rd[0] / pd:.3f} ms "
                  f"({pd} passes): {rr[0] / pr - rd[0] / pd:+.3f} ms per pass; spreads of the rests {rd[1]:.3f} / "
                  f"{rr[1]:.3f} ms; pass_pixels {last[f'd{r}'][1]['pass_pixels']}", flush=True)
        # (d) pass by pass: the cap cut to n_k
        info = last["d"][1]
        ends = [min(SPP_MIN, cap)]
        while ends[-1] < cap:
            ends.append(min(ends[-1] + SPP_STEP, cap))
        ends = ends[:info["passes"]]
        cum = {n: [] for n in ends}
        for rnd in range(rounds + 1):
            for n in ends:
                sc.trace_adaptive(cam, w, h, n, out=outs)
                if rnd:
                    cum[n].append(sc.stats().render_ms)
        print("  (d) pass by pass (the call with the cap cut to n_k, differences of the medians):", flush=True)
        prev = 0.0
        for k, n in enumerate(ends):
            m, sp = med(cum[n])
            px = info["pass_pixels"][k]
            n0 = ends[k - 1] if k else 0
            print(f"    pass {k} (samples {n0}..{n}): {px:8d} pixels  {m - prev:8.3f} ms  "
                  f"{(m - prev) * 1e6 / (px * (n - n0)):8.2f} ns per sample   (cumulative {m:8.3f}, spread {sp:.3f})", flush=True)
            prev = m


if __name__ == "__main__":
    main()
