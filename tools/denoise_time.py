"""The denoiser (Scene.denoise) and the radiance render (Scene.trace_radiance) on
the bench frame -- stand-in sponza 1920x1080, AOVs and radiance at 64 spp, the
reference octree built -- and on a frame of the 1/8 shard's height (the bench
frame's first 135 rows, filtered as a frame of their own), in one process on
one GPU, every buffer on the device.

Filter: tmpt_stats.render_ms (guide preparation + the levels) for levels = 1..6
with option denoise_lds = 0 (every level reads global memory directly) and 1
(strides 1 and 2 read the staged LDS tile) and -1 (the default), one warm-up
round, then `rounds` timed rounds with the variants interleaved; medians and
the spread (max - min).  The time of level L is the median at L + 1 levels
minus the median at L levels (level 0 includes the guide preparation).  Each
level is set against its streaming floor: the bytes it must move (52 B a pixel:
16 B colour read, 20 B guides read, 16 B colour written; the guide preparation
32 B + 20 B) over the bandwidth a plain device-to-device copy of that many
bytes reaches in this run (torch's contiguous copy_ is one hipMemcpyAsync).
Every variant must return the same bits.

Render: tmpt_render_radiance against tmpt_render of the same desc (sample and
pixel seeding, whole frame and 1/8 shard with 1-row bands), interleaved, medians.

  python tools/denoise_time.py [rounds, default 5] [spp, default 64]

profiles/denoise_time.log is this tool's output; DESIGN.md "Denoiser" reads the
staging choice per stride off it."""
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

VARIANTS = (0, 1, -1)


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


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def time_filter(sc, label, rad, aov, spp, rounds):
    h, w = rad.shape[:2]
    n = w * h
    t_in = torch.from_numpy(rad).to("cuda:0")
    t_aov = torch.from_numpy(aov.view(np.uint8).reshape(h, w, 32).copy()).to("cuda:0")
    t_out = torch.empty_like(t_in)
    t_8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    bw = copy_bandwidth(52 * n, rounds)
    ms = {(v, k): [] for v in VARIANTS for k in range(1, 7)}
    ref = {}
    for rnd in range(rounds + 1):  # round 0 warms every variant up
        for k in range(1, 7):
            for v in VARIANTS:
                sc.set_option("denoise_lds", v)
                sc.denoise(t_in.data_ptr(), t_aov.data_ptr(), spp, levels=k, width=w, height=h,
                           out=(t_out.data_ptr(), t_8.data_ptr()))
                t = sc.stats().render_ms
                if rnd:
                    ms[(v, k)].append(t)
                else:
                    digest = hashlib.sha256(t_out.cpu().numpy().tobytes() + t_8.cpu().numpy().tobytes()).hexdigest()
                    assert ref.setdefault(k, digest) == digest, f"denoise_lds={v} changed the output at {k} levels"
    floor = 52 * n / (bw * 1e9) * 1e3
    print(f"{label}: {w}x{h}, AOVs at {spp} spp, {rounds} rounds after a warm-up; device-to-device copy of "
          f"{52 * n / 1e6:.1f} MB moved: {bw:.0f} GB/s, so a level's streaming floor is {floor:.4f} ms "
          f"(the guide preparation moves as many bytes: level 0, timed with it, is set against two floors)", flush=True)
    for v in VARIANTS:
        name = {0: "direct loads", 1: "LDS tile at strides 1, 2", -1: "default"}[v]
        prev = 0.0
        print(f"  denoise_lds={v:2d} ({name}):", flush=True)
        for k in range(1, 7):
            m, sp = med(ms[(v, k)])
            lvl = m - prev
            fl = floor * (2 if k == 1 else 1)
            print(f"    levels={k}: render_ms median {m:7.4f} spread {sp:6.4f} | level {k - 1} (stride {1 << (k - 1):2d}) "
                  f"{lvl:7.4f} ms = {lvl / fl:5.2f} x floor", flush=True)
            prev = m
    m5, _ = med(ms[(-1, 5)])
    print(f"  the default call (5 levels): {m5:.4f} ms", flush=True)


def time_render(sc, cam, w, h, spp, rounds):
    for label, shards in (("whole frame", 1), ("1/8 shard, 1-row bands", 8)):
        kw = dict(band_rows=1, shard=0, num_shards=shards)
        rows = tm.tile_rows(w, h, 1, 0, shards)
        t32 = torch.empty((rows, w, 4), dtype=torch.float32, device="cuda:0")
        t8 = torch.empty((rows, w, 4), dtype=torch.uint8, device="cuda:0")
        for seed, sname in ((tm.SEED_SAMPLE, "sample"), (tm.SEED_PIXEL, "pixel")):
            plain, rad = [], []
            for rnd in range(rounds + 1):
                _, r0 = sc.trace_image(cam, w, h, spp, seed_mode=seed, out=t8.data_ptr(), **kw)
                a = sc.stats().render_ms
                b8 = t8.cpu().numpy().tobytes()
                _, _, r1 = sc.trace_radiance(cam, w, h, spp, seed_mode=seed, out=(t32.data_ptr(), t8.data_ptr()), **kw)
                b = sc.stats().render_ms
                assert r0 == r1 and t8.cpu().numpy().tobytes() == b8
                if rnd:
                    plain.append(a)
                    rad.append(b)
            (mp, sp), (mr, sr) = med(plain), med(rad)
            print(f"{label}, {sname} seeding, {w}x{h}x{spp}: tmpt_render median {mp:8.3f} ms (spread {sp:6.3f}), "
                  f"tmpt_render_radiance {mr:8.3f} ms (spread {sr:6.3f}), difference {mr - mp:+7.3f} ms "
                  f"({rows * w * 16 / 1e6:.1f} MB of float tile)", flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    w, h = 1920, 1080
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, _, _ = sc.trace_radiance(cam, w, h, spp)
        aov, _ = sc.trace_aov(cam, w, h, spp)
        time_filter(sc, "bench frame", rad, aov, spp, rounds)
        rows = h // 8
        time_filter(sc, "1/8-shard height", np.ascontiguousarray(rad[:rows]), np.ascontiguousarray(aov[:rows]), spp,
                    rounds)
        time_render(sc, cam, w, h, spp, rounds)


if __name__ == "__main__":
    main()
