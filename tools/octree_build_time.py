"""The reference's octree built on the host and on the device (option octree_build),
timed against each other in one process on one GPU.

Scenes: the bench scene (the stand-in sponza) at rest and over the poses of its 0..90 degree
twist (tests/bvh_refit_restate.twist, floor included), and suzanne and teapot as small-scene
rows, where launch overhead may make the device path the slower one.  Per scene and pose the
two paths interleaved within a round (host, then device, on scenes of their own), one warm-up
round, then `rounds` timed rounds; medians and the spread (max - min), in ms:

  build_ms  tmpt_stats.octree_build_ms: the whole tmpt_scene_build_octree call -- the build,
            the crack grid, the flat triangles and their marks, the view's upload
  wall      the host's wall time around Scene.build_octree
  frame     (the twist rows) Scene.update(pose, "refit", bounds=...): the refit and the octree
            of the new pose, wall time -- what a frame of a --twist sequence in reference mode
            pays before its render

Each device-built octree is compared with the host-built one of the same pose (dump_octree,
word for word) once, in the warm-up round.

  python tools/octree_build_time.py [rounds, default 5] [frames, default 16] [degrees, default 90]

profiles/octree_build_time.log is this tool's output (DESIGN.md section 4 "Octree build on
the device")."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402
from bvh_refit_restate import twist  # noqa: E402

PATHS = ("host", "device")


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def same(a, b):
    return (a["info"] == b["info"] and np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["refs"], b["refs"])
            and np.array_equal(a["grid"].view(np.uint32), b["grid"].view(np.uint32)))


def cell(m):
    return f"{m[0]:8.3f} ({m[1]:6.3f})"


def static_row(name, tris, bmin, bmax, rounds):
    """One scene, its octree built again and again over the same bounds."""
    lo, hi = tm.octree_bounds(bmin, bmax)
    res = {p: {"ms": [], "wall": []} for p in PATHS}
    scenes = {p: tm.Scene(tris, options={"octree_build": p}) for p in PATHS}
    try:
        for rnd in range(rounds + 1):
            for p in PATHS:
                w = wall(lambda: scenes[p].build_octree(lo, hi))
                if rnd:
                    res[p]["ms"].append(scenes[p].stats().octree_build_ms)
                    res[p]["wall"].append(w)
            if rnd == 0:
                assert same(scenes["host"].dump_octree(), scenes["device"].dump_octree()), name
        st = scenes["device"].stats()
    finally:
        for sc in scenes.values():
            sc.close()
    m = {p: {k: med(v) for k, v in res[p].items()} for p in PATHS}
    ratio = m["host"]["wall"][0] / m["device"]["wall"][0]
    print(f"{name:>14} | {len(tris):7d} {st.octree_nodes:8d} {st.octree_refs:8d} | {cell(m['host']['ms'])} "
          f"{cell(m['host']['wall'])} | {cell(m['device']['ms'])} {cell(m['device']['wall'])} | {ratio:6.2f}"
          f"{'' if ratio >= 1.0 else '  (the device path is the slower one)'}", flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    degrees = float(sys.argv[3]) if len(sys.argv) > 3 else 90.0
    if rounds < 4:
        raise SystemExit("at least four timed rounds")
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    print(f"octree build, host against device (option octree_build); {rounds} rounds after a warm-up, the two paths "
          "interleaved; ms, median (spread); every device-built octree equal to the host's word for word", flush=True)
    print("         scene |    tris    nodes     refs | host build_ms               wall | device build_ms"
          "             wall | host / device wall", flush=True)
    static_row("sponza stand-in", tris, bmin, bmax, rounds)
    for name in ("suzanne", "teapot"):
        static_row(name, *tm.load_scene(os.path.join(ROOT, "data", name + ".obj")), rounds)

    angles = [degrees * f / max(frames - 1, 1) for f in range(frames)]
    poses = [twist(tris, a) for a in angles]
    bounds = [(p[:-2].reshape(-1, 3).min(0), p[:-2].reshape(-1, 3).max(0)) for p in poses]  # the floor comes last
    keys = ("ms", "wall", "frame")
    res = [{p: {k: [] for k in keys} for p in PATHS} for _ in poses]
    nodes = [0] * frames
    scenes = {p: tm.Scene(tris, options={"octree_build": p}) for p in PATHS}
    try:
        for rnd in range(rounds + 1):
            for f, pose in enumerate(poses):
                box = tm.octree_bounds(*bounds[f])
                for p in PATHS:
                    sc = scenes[p]
                    fw = wall(lambda: sc.update(pose, "refit", bounds=bounds[f]))
                    w = wall(lambda: sc.build_octree(*box))
                    if rnd:
                        r = res[f][p]
                        r["ms"].append(sc.stats().octree_build_ms)
                        r["wall"].append(w)
                        r["frame"].append(fw)
                if rnd == 0:
                    assert same(scenes["host"].dump_octree(), scenes["device"].dump_octree()), f
                    nodes[f] = scenes["device"].stats().octree_nodes
    finally:
        for sc in scenes.values():
            sc.close()
    print(f"stand-in sponza, twist 0..{degrees:g} degrees in {frames} poses; frame = update(refit) + octree, wall", flush=True)
    print("  deg |    nodes | host build_ms               wall             frame | device build_ms             wall"
          "             frame | host / device wall  frame", flush=True)
    for f in range(frames):
        m = {p: {k: med(v) for k, v in res[f][p].items()} for p in PATHS}
        print(f"{angles[f]:5.1f} | {nodes[f]:8d} | " + " | ".join(" ".join(cell(m[p][k]) for k in keys) for p in PATHS)
              + f" | {m['host']['wall'][0] / m['device']['wall'][0]:6.2f} {m['host']['frame'][0] / m['device']['frame'][0]:6.2f}",
              flush=True)
    allv = {p: {k: med(sum((r[p][k] for r in res), [])) for k in keys} for p in PATHS}
    print("over all poses: " + "; ".join(f"{p} build_ms {cell(allv[p]['ms'])} wall {cell(allv[p]['wall'])} frame "
                                         f"{cell(allv[p]['frame'])}" for p in PATHS), flush=True)


if __name__ == "__main__":
    main()
