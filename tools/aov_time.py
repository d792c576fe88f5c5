"""The AOV pass (Scene.trace_aov) on the bench frame -- stand-in sponza
1920x1080x64, the reference octree built -- for the whole frame and for a 1/8
shard with 1-row bands: tmpt_stats.render_ms for aov_group = 1, 2, 4, 8, 16 and
auto, beside the sample-seeded beauty render of the same load, in one process
on one GPU.  Per load one warm-up round, then `rounds` timed rounds with the
variants interleaved; medians and the spread (max - min over the rounds).
Every group size must return the same records and ray count.

  python tools/aov_time.py [rounds, default 5] [spp, default 64]

profiles/aov_pass.log is this tool's output; DESIGN.md "AOV pass" reads the
auto rule off it."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402

GROUPS = (1, 2, 4, 8, 16, 0)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    w, h = 1920, 1080
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        for label, shards in (("whole frame", 1), ("1/8 shard, 1-row bands", 8)):
            kw = dict(band_rows=1, shard=0, num_shards=shards)
            pixels = tm.tile_rows(w, h, 1, 0, shards) * w
            ms = {g: [] for g in GROUPS}
            beauty, ref, rays, brays = [], None, 0, 0
            for rnd in range(rounds + 1):  # round 0 warms every variant up
                for g in GROUPS:
                    sc.set_option("aov_group", g)
                    rec, rays = sc.trace_aov(cam, w, h, spp, **kw)
                    digest = (hashlib.sha256(rec.tobytes()).hexdigest(), rays)
                    ref = ref or digest
                    assert digest == ref, f"aov_group={g} changed the records"
                    if rnd:
                        ms[g].append(sc.stats().render_ms)
                _, brays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, **kw)
                if rnd:
                    beauty.append(sc.stats().render_ms)
            hits = int(rec["hits"].sum())
            print(f"{label}: {w}x{h}x{spp}, {pixels} pixels, {rays} rays ({pixels * spp} camera + {hits} shadow), "
                  f"{rounds} rounds after a warm-up", flush=True)
            for g in GROUPS:
                a = np.array(ms[g])
                m = float(np.median(a))
                print(f"  aov_group={g if g else 'auto':>4}: render_ms median {m:8.3f}  min {a.min():8.3f}  "
                      f"max {a.max():8.3f}  spread {a.max() - a.min():6.3f}  {rays / m / 1e6:7.2f} GRays/s", flush=True)
            b = np.array(beauty)
            m = float(np.median(b))
            print(f"  beauty (sample seeding): render_ms median {m:8.3f}  min {b.min():8.3f}  max {b.max():8.3f}  "
                  f"{brays} rays  {brays / m / 1e6:7.2f} GRays/s", flush=True)


if __name__ == "__main__":
    main()
