"""k_temporal_clip on the bench frame -- stand-in sponza 1920x1080, the
reference octree built -- in one process on one GPU, every buffer on the device:
radius 1, 2 and 3, with and without the aux frame, interleaved round by round
with k_temporal and one level of tmpt_denoise on the same frame; medians and the
spread (max - min) of tmpt_stats.render_ms over the rounds.

Bytes moved per pixel, without aux: 32 B motion + 16 B colour read, 16 B + 4 B
written, the statistics frame's 16 B and the motion record's flag word (4 B, its
32-byte sector at the worst) once more for the tile -- the halo adds
(32+2r)(8+2r) / 256 - 1 of that -- and, gathered, once to four times 32 B + 16 B
of the previous frame; aux adds 16 B read, 16 B written and once to four times
16 B of its history.  The floor is that over the bandwidth a device-to-device
copy reaches in this run.

  python tools/temporal_clip_time.py [rounds, default 9]

profiles/temporal_clip_time.log is this tool's output; DESIGN.md "History
clipping" quotes it."""
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
from temporal_time import copy_bandwidth, med  # noqa: E402


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    w, h = 1920, 1080
    n = w * h
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, mom = sc.trace_moments(cam, w, h, 4)[:2]
        ok = np.isfinite(rad).all(-1, keepdims=True) & np.isfinite(mom).all(-1, keepdims=True)
        rad, mom = np.where(ok, rad, np.float32(0)).astype(np.float32), np.where(ok, mom, np.float32(1)).astype(np.float32)
        aov, _ = sc.trace_aov(cam, w, h, 4)
        mot, _ = sc.trace_motion(cam, cam, w, h)
        t_cur, t_hist, t_a, t_mot, t_mom, t_mhist = dev(rad), dev(rad), dev(aov), dev(mot), dev(mom), dev(mom)
        t_out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_aux = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        size = dict(width=w, height=h)
        four = (t_cur.data_ptr(), t_mot.data_ptr(), t_mot.data_ptr(), t_hist.data_ptr())
        variants = [(r, aux) for r in (1, 2, 3) for aux in (False, True)]
        ms = {v: [] for v in variants}
        ms["blend"], ms["level"] = [], []
        for rnd in range(rounds + 1):  # round 0 warms every variant up
            for r, aux in variants:
                if aux:
                    sc.temporal_clip(*four, radius=r, aux=t_mom.data_ptr(), aux_history=t_mhist.data_ptr(),
                                     out=(t_out.data_ptr(), t_8.data_ptr(), t_aux.data_ptr()), **size)
                else:
                    sc.temporal_clip(*four, radius=r, out=(t_out.data_ptr(), t_8.data_ptr(), None), **size)
                if rnd:
                    ms[(r, aux)].append(sc.stats().render_ms)
            sc.temporal(*four, out=(t_out.data_ptr(), t_8.data_ptr()), **size)
            a = sc.stats().render_ms
            sc.denoise(t_cur.data_ptr(), t_a.data_ptr(), 4, levels=1, out=(t_out.data_ptr(), t_8.data_ptr()), **size)
            b = sc.stats().render_ms
            if rnd:
                ms["blend"].append(a)
                ms["level"].append(b)
        base_lo, base_hi = (32 + 16 + 16 + 4 + 32 + 16) * n, (32 + 16 + 16 + 4 + 4 * 48) * n
        bw = copy_bandwidth(base_lo, rounds)
        hits = int((mot["flags"] & 1).sum())
        print(f"bench frame {w}x{h}, {len(tris)} triangles, {rounds} rounds after a warm-up, interleaved; static view "
              f"(every tap of the {hits} covered pixels accepted), defaults but for the radius; a device-to-device copy "
              f"reaches {bw:.0f} GB/s", flush=True)
        floor = lambda b: b / (bw * 1e9) * 1e3
        for r, aux in variants:
            tile = (32 + 2 * r) * (8 + 2 * r) / 256.0
            lo = base_lo + (16 + 4) * tile * n + ((16 + 16 + 16) * n if aux else 0)
            hi = base_hi + (16 + 32) * tile * n + ((16 + 16 + 4 * 16) * n if aux else 0)
            m, sp = med(ms[(r, aux)])
            print(f"  k_temporal_clip<{r}>{' + aux' if aux else '      '}: median {m:7.4f} ms  spread {sp:6.4f}; it moves "
                  f"{lo / 1e6:.0f} .. {hi / 1e6:.0f} MB: floor {floor(lo):.4f} .. {floor(hi):.4f} ms", flush=True)
        (mb, sb), (ml, sl) = med(ms["blend"]), med(ms["level"])
        print(f"  k_temporal              : median {mb:7.4f} ms  spread {sb:6.4f}; it moves {base_lo / 1e6:.0f} .. "
              f"{base_hi / 1e6:.0f} MB: floor {floor(base_lo):.4f} .. {floor(base_hi):.4f} ms", flush=True)
        print(f"  tmpt_denoise, levels = 1 : median {ml:7.4f} ms  spread {sl:6.4f}", flush=True)


if __name__ == "__main__":
    main()
