"""The noise-aware filter's cost on the bench frame -- stand-in sponza 1920x1080,
radiance, moments and AOVs at 64 spp, the reference octree built -- in one
process on one GPU, every buffer on the device.

Filter: tmpt_stats.render_ms of Scene.denoise and Scene.denoise_moments
(shrink 4) for levels = 1..6 with option denoise_lds = 1 (strides 1 and 2 read
the staged LDS tile: the default) and 0 (every level reads global memory
directly), one warm-up round, then `rounds` timed rounds with the two calls and
the two variants interleaved; medians and the spread (max - min).  The time of
level L is the median at L + 1 levels minus the median at L levels (level 0
includes the guide preparation and, for the new call, v_0).  Staged and direct
must return the same bits.

Render: tmpt_render_moments (uniform) against tmpt_render_radiance and against
tmpt_render_adaptive at spp_min = spp, interleaved, medians; the three must
agree on the radiance and the ray count.

  python tools/noise_aware_time.py [rounds, default 5] [spp, default 64]

profiles/noise_aware_time.log is this tool's output (DESIGN.md "Noise-aware filter")."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def time_filter(sc, rad, mom, aov, spp, rounds):
    h, w = rad.shape[:2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
    t_in, t_mom, t_aov = dev(rad), dev(mom), dev(aov)
    t_out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    t_8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    out = (t_out.data_ptr(), t_8.data_ptr())
    calls = ("plain", "moments")
    ms = {(c, v, k): [] for c in calls for v in (1, 0) for k in range(1, 7)}
    ref = {}
    for rnd in range(rounds + 1):  # round 0 warms every variant up
        for k in range(1, 7):
            for v in (1, 0):
                sc.set_option("denoise_lds", v)
                for c in calls:
                    if c == "plain":
                        sc.denoise(t_in.data_ptr(), t_aov.data_ptr(), spp, levels=k, width=w, height=h, out=out)
                    else:
                        sc.denoise_moments(t_in.data_ptr(), t_aov.data_ptr(), t_mom.data_ptr(), spp, shrink=4.0, levels=k,
                                           width=w, height=h, out=out)
                    t = sc.stats().render_ms
                    if rnd:
                        ms[(c, v, k)].append(t)
                    else:
                        digest = hashlib.sha256(t_out.cpu().numpy().tobytes() + t_8.cpu().numpy().tobytes()).hexdigest()
                        assert ref.setdefault((c, k), digest) == digest, f"denoise_lds={v} changed {c} at {k} levels"
    sc.set_option("denoise_lds", -1)
    print(f"filter: {w}x{h}, AOVs and moments at {spp} spp, {rounds} rounds after a warm-up, render_ms in ms; "
          "median (spread)", flush=True)
    for v in (1, 0):
        print(f"  denoise_lds={v} ({'LDS tile at strides 1, 2' if v else 'direct loads'}):", flush=True)
        prev = {c: 0.0 for c in calls}
        for k in range(1, 7):
            cells = []
            for c in calls:
                m, sp = med(ms[(c, v, k)])
                cells.append(f"{c} {m:7.4f} ({sp:6.4f}) level {k - 1} {m - prev[c]:7.4f}")
                prev[c] = m
            a, b = med(ms[("plain", v, k)])[0], med(ms[("moments", v, k)])[0]
            print(f"    levels={k} (last stride {1 << (k - 1):2d}): " + " | ".join(cells) + f" | moments / plain {b / a:5.2f}",
                  flush=True)
    for c in calls:
        m, sp = med(ms[(c, 1, 5)])
        print(f"  the default call (5 levels, staged), {c}: {m:.4f} ms (spread {sp:.4f})", flush=True)


def time_render(sc, cam, w, h, spp, rounds):
    t32 = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    tmo = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    tn = torch.empty((h, w), dtype=torch.int32, device="cuda:0")
    ms = {"radiance": [], "adaptive": [], "moments": []}
    for rnd in range(rounds + 1):
        _, _, r0 = sc.trace_radiance(cam, w, h, spp, out=(t32.data_ptr(), t8.data_ptr()))
        a = sc.stats().render_ms
        d0 = hashlib.sha256(t32.cpu().numpy().tobytes()).hexdigest()
        r1 = sc.trace_adaptive(cam, w, h, spp, spp_min=spp, out=(t32.data_ptr(), t8.data_ptr(), tn.data_ptr()))[3]
        b = sc.stats().render_ms
        d1 = hashlib.sha256(t32.cpu().numpy().tobytes()).hexdigest()
        r2 = sc.trace_moments(cam, w, h, spp, out=(t32.data_ptr(), tmo.data_ptr(), t8.data_ptr(), tn.data_ptr()))[4]
        c = sc.stats().render_ms
        d2 = hashlib.sha256(t32.cpu().numpy().tobytes()).hexdigest()
        assert r0 == r1 == r2 and d0 == d1 == d2
        if rnd:
            ms["radiance"].append(a)
            ms["adaptive"].append(b)
            ms["moments"].append(c)
    print(f"render: {w}x{h}x{spp}, sample seeding, whole frame, {rounds} rounds after a warm-up, render_ms in ms", flush=True)
    for k in ("radiance", "adaptive", "moments"):
        m, sp = med(ms[k])
        print(f"  tmpt_render_{k:<9s}{' (spp_min = spp)' if k == 'adaptive' else ' (uniform)' if k == 'moments' else ''}: "
              f"median {m:9.3f} (spread {sp:7.3f})", flush=True)
    print(f"  moments - radiance {med(ms['moments'])[0] - med(ms['radiance'])[0]:+8.3f} ms, moments - adaptive "
          f"{med(ms['moments'])[0] - med(ms['adaptive'])[0]:+8.3f} ms ({w * h * 16 / 1e6:.1f} MB of moments tile)", flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    w, h = 1920, 1080
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, mom = sc.trace_moments(cam, w, h, spp)[:2]
        aov, _ = sc.trace_aov(cam, w, h, spp)
        time_filter(sc, rad, mom, aov, spp, rounds)
        time_render(sc, cam, w, h, spp, rounds)


if __name__ == "__main__":
    main()
