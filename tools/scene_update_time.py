"""Scene updates on the bench scene -- the stand-in sponza, twisted about y from 0 to 90
degrees in 16 frames (tests/bvh_refit_restate.twist, floor included) -- in one process on
one GPU.  Per frame, the variants interleaved within a round, one warm-up round, then
`rounds` timed rounds; medians and the spread (max - min):

  refit     Scene.update(frame, "refit") on a scene built in the rest pose: option update_ms
            (events on the scene's stream: the upload through the last kernel) and the
            host's wall time around the call
  rebuild   Scene.update(frame, "rebuild") on a second scene: update_ms and wall time
  create    close() + Scene(frame), no octree: the only route there was before
            tmpt_scene_update, in the same run with the same triangles; wall time
  bvh_cost  of the refitted and of the rebuilt tree
  render    the 1920x1080x8 sample-seeded frame (octree built over the frame's bounds, the
            output on the device) on the refitted tree and on the rebuilt tree of the same
            frame: tmpt_stats.render_ms, and their ratio -- what a refit costs the
            traversal as the mesh leaves its build pose, with bvh_cost's ratio beside it

  python tools/scene_update_time.py [rounds, default 5] [frames, default 16] [degrees, default 90]

profiles/scene_update_time.log is this tool's output (DESIGN.md section 4 "Scene update")."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402
from bvh_refit_restate import twist  # noqa: E402


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    degrees = float(sys.argv[3]) if len(sys.argv) > 3 else 90.0
    w, h, spp = 1920, 1080, 8
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
    t8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0")
    angles = [degrees * f / max(frames - 1, 1) for f in range(frames)]
    poses = [twist(tris, a) for a in angles]
    bounds = [(p[:-2].reshape(-1, 3).min(0), p[:-2].reshape(-1, 3).max(0)) for p in poses]  # the floor comes last
    keys = ("refit_ms", "refit_wall", "rebuild_ms", "rebuild_wall", "create_wall", "render_refit", "render_fresh")
    res = [{k: [] for k in keys} for _ in poses]
    cost = [None] * frames
    rays = [None] * frames

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def render(sc, f):
        sc.build_octree(*tm.octree_bounds(*bounds[f]))
        _, n = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, out=t8.data_ptr())
        return sc.stats().render_ms, n

    a = tm.Scene(tris)      # refitted from the rest pose, frame after frame
    b = tm.Scene(tris)      # rebuilt per frame
    c = tm.Scene(tris)      # destroyed and created per frame
    try:
        for rnd in range(rounds + 1):  # round 0 warms every variant up
            a.update(tris, "rebuild")  # each round's refits start from the rest pose's tree
            for f, pose in enumerate(poses):
                r = res[f]
                tw, _ = wall(lambda: a.update(pose, "refit"))
                ms_a = a.get_option("update_ms")
                tb, _ = wall(lambda: b.update(pose, "rebuild"))
                ms_b = b.get_option("update_ms")

                def recreate():
                    c.close()
                    return tm.Scene(pose)

                tc, c = wall(recreate)
                cost[f] = (a.get_option("bvh_cost"), b.get_option("bvh_cost"))
                ra, na = render(a, f)
                rb, nb = render(b, f)
                assert na == nb, "the refitted and the rebuilt tree answer the same rays"
                rays[f] = na
                if rnd:
                    for k, v in zip(keys, (ms_a, tw, ms_b, tb, tc, ra, rb)):
                        r[k].append(v)
    finally:
        for sc in (a, b, c):
            sc.close()
    print(f"stand-in sponza, {len(tris)} triangles, twist 0..{degrees:g} degrees in {frames} frames; {rounds} rounds "
          f"after a warm-up, variants interleaved; ms, median (spread); render: {w}x{h}x{spp}, sample seeding", flush=True)
    print("  deg | refit update_ms      wall | rebuild update_ms    wall | destroy+create wall | bvh_cost refit  "
          "rebuilt  ratio | render refit        rebuilt        ratio", flush=True)
    for f, r in enumerate(res):
        m = {k: med(v) for k, v in r.items()}
        ca, cb = cost[f]
        print(f"{angles[f]:5.1f} | {m['refit_ms'][0]:7.3f} ({m['refit_ms'][1]:5.3f}) {m['refit_wall'][0]:7.3f} | "
              f"{m['rebuild_ms'][0]:7.3f} ({m['rebuild_ms'][1]:5.3f}) {m['rebuild_wall'][0]:7.3f} | "
              f"{m['create_wall'][0]:8.3f} ({m['create_wall'][1]:6.3f}) | {ca:8.3f} {cb:8.3f} {ca / cb:6.3f} | "
              f"{m['render_refit'][0]:7.3f} ({m['render_refit'][1]:5.3f}) {m['render_fresh'][0]:7.3f} "
              f"({m['render_fresh'][1]:5.3f}) {m['render_refit'][0] / m['render_fresh'][0]:6.3f}", flush=True)
    allv = {k: med(sum((r[k] for r in res[1:]), [])) for k in keys}
    print(f"over the frames after the first: refit wall {allv['refit_wall'][0]:.3f} ms, rebuild wall "
          f"{allv['rebuild_wall'][0]:.3f} ms, destroy + create wall {allv['create_wall'][0]:.3f} ms "
          f"(spread {allv['create_wall'][1]:.3f}): create / refit = {allv['create_wall'][0] / allv['refit_wall'][0]:.1f}, "
          f"rebuild - create = {allv['rebuild_wall'][0] - allv['create_wall'][0]:+.3f} ms", flush=True)
    cr = np.array([cost[f][0] / cost[f][1] for f in range(frames)])
    rr = np.array([med(res[f]["render_refit"])[0] / med(res[f]["render_fresh"])[0] for f in range(frames)])
    if frames > 2:
        print(f"bvh_cost ratio against render-time ratio over the frames: correlation {np.corrcoef(cr, rr)[0, 1]:.3f}; "
              f"at the last frame cost x{cr[-1]:.3f}, render x{rr[-1]:.3f}", flush=True)


if __name__ == "__main__":
    main()
