"""History-guided sampling's cost on the bench frame -- stand-in sponza
1920x1080, the reference octree built -- in one process on one GPU, every buffer
on the device; medians and the spread (max - min) over the rounds, each figure
interleaved with what it is compared against.

Plan: k_sample_plan beside k_temporal on the same records (a static view: every
tap of a covered pixel accepted), tmpt_stats.render_ms of each.  The plan reads
32 B motion and, gathered, once to four times 32 B + 16 B of the previous frame,
and writes 16 B; the blend reads 16 B of colour more and writes 4 B more.

Render: a guided frame (spp_min 2, the schedule and the threshold given below,
the prior planned from a two-frame history of 4-spp moments) beside the uniform
frame of equal samples -- tmpt_render_moments at the guided frame's mean samples
per pixel rounded up, so the uniform frame never has fewer -- and beside the
same schedule with no prior.  render_ms covers the whole call: the guided frame
pays one host wait per pass, the uniform frame one in all.

  python tools/guided_time.py [rounds, default 5]

profiles/guided_time.log is this tool's output; DESIGN.md "History-guided
sampling" quotes it."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402
from temporal_time import med  # noqa: E402

SCHEDULES = ((2, 2, 8), (2, 4, 16))  # (spp_min, spp_step, cap)
TAU = 0.02


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    w, h = 1920, 1080
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
    clean = lambda a, v: np.where(np.isfinite(a).all(-1, keepdims=True), a, np.float32(v)).astype(np.float32)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        mom_a = clean(sc.trace_moments(cam, w, h, 4)[1], 1)
        sc.set_option("sample_base", 4)
        rad_b, mom_b = sc.trace_moments(cam, w, h, 4)[:2]
        rad_b, mom_b = clean(rad_b, 0), clean(mom_b, 1)
        sc.set_option("sample_base", 8)
        mot, _ = sc.trace_motion(cam, cam, w, h)
        hist = sc.temporal(mom_b, mot, mot, mom_a)[0]  # the accumulated moments of two frames: length 2 where covered
        t_mot, t_hist, t_cur = dev(mot), torch.from_numpy(hist).to("cuda:0"), torch.from_numpy(rad_b).to("cuda:0")
        t_prior = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_mom = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        t_n = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
        size = dict(width=w, height=h)
        outs = (t_out.data_ptr(), t_mom.data_ptr(), t_8.data_ptr(), t_n.data_ptr())
        ms = dict(plan=[], blend=[])
        for rnd in range(rounds + 1):  # round 0 warms both up
            sc.sample_plan(t_mot.data_ptr(), t_mot.data_ptr(), t_hist.data_ptr(), out=t_prior.data_ptr(), **size)
            a = sc.stats().render_ms
            sc.temporal(t_cur.data_ptr(), t_mot.data_ptr(), t_mot.data_ptr(), t_hist.data_ptr(),
                        out=(t_out.data_ptr(), t_8.data_ptr()), **size)
            b = sc.stats().render_ms
            if rnd:
                ms["plan"].append(a)
                ms["blend"].append(b)
        prior = t_prior.cpu().numpy()
        null = (prior == np.array([0, 0, 1, 0], np.float32)).all(-1)
        print(f"bench frame {w}x{h}, {len(tris)} triangles, {rounds} rounds after a warm-up, interleaved; static view, "
              f"history of two 4-spp frames; {100 * null.mean():.1f} % of the pixels have the null prior (sky)", flush=True)
        for k, name in (("plan", "k_sample_plan"), ("blend", "k_temporal   ")):
            m, sp = med(ms[k])
            print(f"  {name}: median {m:7.4f} ms  spread {sp:6.4f}", flush=True)
        for spp_min, step, cap in SCHEDULES:
            kw = dict(spp_min=spp_min, spp_step=step, threshold=TAU)
            info = sc.trace_guided(cam, w, h, cap, t_prior, out=outs, **kw)[5]
            mean = info["samples"] / (w * h)
            uni = max(2, math.ceil(mean))
            plain = sc.trace_moments(cam, w, h, cap, out=outs, **kw)[5]
            t = dict(guided=[], uniform=[], unguided=[])
            for rnd in range(rounds + 1):
                sc.trace_guided(cam, w, h, cap, t_prior, out=outs, **kw)
                a = sc.stats().render_ms
                sc.trace_moments(cam, w, h, uni, out=outs)
                b = sc.stats().render_ms
                sc.trace_moments(cam, w, h, cap, out=outs, **kw)
                c = sc.stats().render_ms
                if rnd:
                    t["guided"].append(a)
                    t["uniform"].append(b)
                    t["unguided"].append(c)
            print(f"schedule {spp_min}, +{step}, cap {cap}, tau {TAU}:", flush=True)
            (mg, sg), (mu, su), (mp, sp) = med(t["guided"]), med(t["uniform"]), med(t["unguided"])
            print(f"  guided frame      : median {mg:8.3f} ms  spread {sg:6.3f}; {info['passes']} passes, {mean:.3f} samples "
                  f"per pixel, pass_pixels {info['pass_pixels']}", flush=True)
            print(f"  uniform at {uni:2d} spp  : median {mu:8.3f} ms  spread {su:6.3f}; 1 pass, {uni} samples per pixel; guided "
                  f"/ uniform {mg / mu:.3f} in time, {mean / uni:.3f} in samples", flush=True)
            print(f"  the schedule alone: median {mp:8.3f} ms  spread {sp:6.3f}; {plain['passes']} passes, "
                  f"{plain['samples'] / (w * h):.3f} samples per pixel (no prior)", flush=True)


if __name__ == "__main__":
    main()
