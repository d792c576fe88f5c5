"""Temporal accumulation's two kernels on the bench frame -- stand-in sponza
1920x1080, the reference octree built -- in one process on one GPU, every
buffer on the device, each figure interleaved with what it is compared
against; medians and the spread (max - min) of tmpt_stats.render_ms.

Motion pass: k_motion with option motion_tile = 0 (a wave takes 64 pixels of a
row) and 1 (an 8 x 8 block) beside the AOV pass at spp = 1 (k_aov, one lane per
pixel: the same number of closest-hit rays, jittered, plus a shadow ray per
hit), with the previous pose given (a device pointer) and without.  Both wave
shapes must return the same bytes.

Blend: k_temporal beside one level of tmpt_denoise (levels = 1: the guide
preparation and the stride-1 level) on the same frame, and both against the
streaming floor of the blend: 32 B motion + 16 B colour read, 16 B + 4 B
written, and (gathered, so up to) 4 x (32 B + 16 B) of the previous frame, over
the bandwidth a device-to-device copy reaches in this run.

Upload: the host form of the motion pass with a host prev_triangles against the
same call without one, by the host clock (both allocate and read back the
records; the difference is the copy of n x 36 bytes into the scene's kept
buffer).

  python tools/temporal_time.py [rounds, default 9]

profiles/temporal_time.log is this tool's output; DESIGN.md "Temporal
accumulation" quotes it."""
import hashlib
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


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def copy_bandwidth(nbytes, rounds):
    """GB/s (bytes read + bytes written) of a device-to-device copy that moves nbytes in all."""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    src.fill_(1)
    ms = []
    for rnd in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if rnd:
            ms.append(e0.elapsed_time(e1))
    return 2 * src.numel() / (float(np.median(ms)) * 1e-3) / 1e9


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    w, h = 1920, 1080
    n = w * h
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        t_mot = torch.empty((h, w, 8), dtype=torch.float32, device="cuda:0")
        t_aov = torch.empty((h, w, 8), dtype=torch.float32, device="cuda:0")
        t_prev = torch.from_numpy(np.ascontiguousarray(tris, np.float32).reshape(-1, 9).copy()).to("cuda:0")
        variants = [("motion_tile=0 (row of 64)", 0, None), ("motion_tile=1 (8 x 8 block)", 1, None),
                    ("motion_tile=0, previous pose given", 0, t_prev.data_ptr()),
                    ("motion_tile=1, previous pose given", 1, t_prev.data_ptr())]
        ms = {name: [] for name, _, _ in variants}
        ms["aov"] = []
        digest = set()
        for rnd in range(rounds + 1):  # round 0 warms every variant up
            for name, tile, prev in variants:
                sc.set_option("motion_tile", tile)
                sc.trace_motion(cam, cam, w, h, prev, out=t_mot.data_ptr())
                if rnd:
                    ms[name].append(sc.stats().render_ms)
                else:
                    digest.add(hashlib.sha256(t_mot.cpu().numpy().tobytes()).hexdigest())
            _, aov_rays = sc.trace_aov(cam, w, h, 1, out=t_aov.data_ptr())
            if rnd:
                ms["aov"].append(sc.stats().render_ms)
        assert len(digest) == 1, "the wave shapes (or the given pose) changed the records"
        rec = t_mot.cpu().numpy().view(tm.MOTION_DTYPE).reshape(h, w)
        hits = int((rec["flags"] & 1).sum())
        print(f"bench frame {w}x{h}, {len(tris)} triangles, {rounds} rounds after a warm-up, interleaved; "
              f"{n} centre rays, {hits} hits, {int((rec['flags'] & 2 != 0).sum())} valid reprojections", flush=True)
        for name, _, _ in variants:
            m, sp = med(ms[name])
            print(f"  k_motion {name:38s}: median {m:7.4f} ms  spread {sp:6.4f}  {n / m / 1e3:8.1f} M rays/s", flush=True)
        m, sp = med(ms["aov"])
        print(f"  k_aov at spp = 1 ({aov_rays} rays, a shadow ray per hit)  : median {m:7.4f} ms  spread {sp:6.4f}",
              flush=True)
        sc.set_option("motion_tile", -1)

        # the blend beside one denoise level
        rad, _, _ = sc.trace_radiance(cam, w, h, 4)
        rad = np.where(np.isfinite(rad).all(-1, keepdims=True), rad, np.float32(0)).astype(np.float32)
        aov, _ = sc.trace_aov(cam, w, h, 4)
        t_cur, t_hist, t_a = dev(rad), dev(rad), dev(aov)
        t_out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
        t_8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
        blend, level = [], []
        for rnd in range(rounds + 1):
            sc.temporal(t_cur.data_ptr(), t_mot.data_ptr(), t_mot.data_ptr(), t_hist.data_ptr(), width=w, height=h,
                        out=(t_out.data_ptr(), t_8.data_ptr()))
            a = sc.stats().render_ms
            sc.denoise(t_cur.data_ptr(), t_a.data_ptr(), 4, levels=1, width=w, height=h, out=(t_out.data_ptr(), t_8.data_ptr()))
            b = sc.stats().render_ms
            if rnd:
                blend.append(a)
                level.append(b)
        lo, hi = (32 + 16 + 16 + 4 + 32 + 16) * n, (32 + 16 + 16 + 4 + 4 * 48) * n
        bw = copy_bandwidth(lo, rounds)
        (mb, sb), (ml, sl) = med(blend), med(level)
        print(f"  k_temporal (static view: every tap accepted)            : median {mb:7.4f} ms  spread {sb:6.4f}; "
              f"it moves {lo / 1e6:.0f} .. {hi / 1e6:.0f} MB (each previous pixel fetched once .. four times), a "
              f"device-to-device copy reaches {bw:.0f} GB/s: floor {lo / (bw * 1e9) * 1e3:.4f} .. {hi / (bw * 1e9) * 1e3:.4f} ms",
              flush=True)
        print(f"  tmpt_denoise, levels = 1 (guide preparation + stride 1)  : median {ml:7.4f} ms  spread {sl:6.4f}", flush=True)

        # the upload of a host prev_triangles
        with_prev, without = [], []
        for rnd in range(rounds + 1):
            t0 = time.perf_counter()
            sc.trace_motion(cam, cam, w, h, tris)
            t1 = time.perf_counter()
            sc.trace_motion(cam, cam, w, h)
            t2 = time.perf_counter()
            if rnd:
                with_prev.append((t1 - t0) * 1e3)
                without.append((t2 - t1) * 1e3)
        (mw, sw), (mo, so) = med(with_prev), med(without)
        print(f"  host form of the motion pass (allocation, kernel, {n * 32 / 1e6:.0f} MB read back), host clock: with a host "
              f"prev_triangles ({len(tris) * 36 / 1e6:.2f} MB) median {mw:.3f} ms (spread {sw:.3f}), without {mo:.3f} ms "
              f"(spread {so:.3f}): the upload costs {mw - mo:+.3f} ms", flush=True)


if __name__ == "__main__":
    main()
