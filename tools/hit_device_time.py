"""Batched scene queries timed: hit_scene_batch (host arrays, a PCIe round trip and three
allocations per call) against hit_scene_device (torch tensors on the device) under
query_sort 0 / 1 x query_top 0 / 1, and k_intersect on the same device data (option
query_legacy) for the kernel-to-kernel comparison.  One process, one GPU.

Scene: the bench scene (the stand-in sponza), without and with the reference's octree.
Ray sets, n = 2^16, 2^20, 2^22 each:
  (a) primary   the frame's camera rays in pixel order (Scene.camera_rays)
  (b) shuffled  the same rays in a fixed random order
  (c) bounce    cosine-distributed rays from (a)'s hit points (normal + a random unit vector)
Closest hit and any hit.  Per row `rounds` timed rounds after a warm-up round, every
configuration once per round in turn (interleaved); ms, median (spread = max - min):
  batch wall    the host's wall time around hit_scene_batch
  k_intersect   device time of k_intersect on the device data (two events on the scene's stream)
  s0t0 .. s1t1  query_ms of hit_scene_device (the same two events), query_sort s x query_top t;
                in brackets, for s = 1, query_sort_ms: the keys' and the sorts' share of it
  wall          the host's wall time around hit_scene_device under the defaults
Every configuration's ids are compared with k_intersect's once, in the warm-up round.

The rule for the two defaults (DESIGN.md section 4 "Device-resident queries") is evaluated at
the end from the rows: query_top is on if it is not slower than off on any set at n >= 2^20 by
more than the spread; query_sort auto sorts from the smallest n at which sorting, keys and
sort included, takes at most 0.95 of the unsorted time on sets (b) and (c) and at most 1.02
on set (a).

  python tools/hit_device_time.py [rounds, default 5] [log2 of the largest n, default 22]

profiles/hit_device_time.log is this tool's output."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "data"))
import numpy as np  # noqa: E402

import toymeshpathtracer_amd as tm  # noqa: E402
import gen_standin_sponza  # noqa: E402

torch = tm.torch
RNG = (0.001, 1.0e7)
FRAMES = {16: (256, 256, 1), 20: (1024, 1024, 1), 22: (2048, 1024, 2)}
CONFIGS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def med(v):
    a = np.array(v)
    return float(np.median(a)), float(a.max() - a.min())


def cell(m):
    return f"{m[0]:8.3f} ({m[1]:6.3f})"


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def ray_sets(sc, cam, log2n):
    """-> {name: float32 tensor [n, 6] on the device}"""
    w, h, spp = FRAMES[log2n]
    n = 1 << log2n
    cr = sc.camera_rays(cam, w, h, spp)
    prim = np.ascontiguousarray(cr.view(np.float32)[:, :, :6].reshape(-1, 6))
    assert prim.shape == (n, 6)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    a = torch.from_numpy(prim).cuda()
    b = a[torch.randperm(n, device="cuda:0", generator=g)].contiguous()
    ids, hits, _ = sc.hit_scene_device(a, *RNG)
    src = hits[ids >= 0]
    src = src[torch.arange(n, device="cuda:0") % src.shape[0]]  # every bounce ray from a hit point, in pixel order
    v = torch.randn((n, 3), device="cuda:0", generator=g)
    d = src[:, 3:6] + v / v.norm(dim=1, keepdim=True)  # cosine-distributed about the normal
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-20)
    c = torch.cat([src[:, 0:3] + 1e-3 * src[:, 3:6], d], 1).contiguous()
    torch.cuda.synchronize()
    return {"primary": a, "shuffled": b, "bounce": c}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    top = int(sys.argv[2]) if len(sys.argv) > 2 else 22
    if rounds < 4:
        raise SystemExit("at least four timed rounds")
    tris, bmin, bmax = tm.load_scene(gen_standin_sponza.ensure())
    w0, h0, _ = FRAMES[16]
    print(f"batched queries on the stand-in sponza ({len(tris)} triangles); {rounds} rounds after a warm-up, the "
          "configurations interleaved; ms, median (spread)", flush=True)
    print("octree set       log2n kind    | batch wall        | k_intersect       | s0t0              s0t1              "
          "s1t0 [keys+sort]           s1t1 [keys+sort]           | device wall", flush=True)
    rows = {}
    for octree in (False, True):
        sc = tm.Scene(tris, bounds=(bmin, bmax) if octree else None)
        for log2n in [k for k in sorted(FRAMES) if k <= top]:
            w, h, _ = FRAMES[log2n]
            cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=True)
            sets = ray_sets(sc, cam, log2n)
            for name, rays in sets.items():
                host = rays.cpu().numpy()
                for any_hit in (False, True):
                    res = {k: [] for k in ["batch", "legacy", "wall"] + CONFIGS + [("sort",) + c for c in CONFIGS if c[0]]}
                    want = None
                    for rnd in range(rounds + 1):
                        t, _ = wall(lambda: sc.hit_scene_batch(host, *RNG, any_hit=any_hit))
                        sc.set_option("query_legacy", 1)
                        ids = sc.hit_scene_device(rays, *RNG, any_hit=any_hit)[0]
                        leg = sc.get_option("query_ms")
                        sc.set_option("query_legacy", 0)
                        if rnd == 0:
                            want = ids if not any_hit else ids >= 0
                        one = {}
                        for s, tp in CONFIGS:
                            sc.set_option("query_sort", s)
                            sc.set_option("query_top", tp)
                            got = sc.hit_scene_device(rays, *RNG, any_hit=any_hit)[0]
                            one[(s, tp)] = sc.get_option("query_ms")
                            if s:
                                one[("sort", s, tp)] = sc.get_option("query_sort_ms")
                            if rnd == 0:
                                assert torch.equal(got if not any_hit else got >= 0, want), (name, log2n, s, tp)
                        sc.set_option("query_sort", -1)
                        sc.set_option("query_top", -1)
                        tw, _ = wall(lambda: sc.hit_scene_device(rays, *RNG, any_hit=any_hit))
                        if rnd:
                            res["batch"].append(t)
                            res["legacy"].append(leg)
                            res["wall"].append(tw)
                            for k, v in one.items():
                                res[k].append(v)
                    m = {k: med(v) for k, v in res.items()}
                    rows[(octree, name, log2n, any_hit)] = m
                    print(f"{'yes' if octree else 'no ':6} {name:9} {log2n:5d} {'any' if any_hit else 'closest':7} | "
                          f"{cell(m['batch'])} | {cell(m['legacy'])} | {cell(m[(0, 0)])} {cell(m[(0, 1)])} "
                          f"{cell(m[(1, 0)])} [{m[('sort', 1, 0)][0]:7.3f}] {cell(m[(1, 1)])} [{m[('sort', 1, 1)][0]:7.3f}] | "
                          f"{cell(m['wall'])}", flush=True)
            del sets
        sc.close()

    # ---- the rule for the two -1 defaults, from the rows above
    big = [k for k in rows if k[2] >= 20]
    worse = [(k, rows[k][(0, 1)][0] - rows[k][(0, 0)][0], max(rows[k][(0, 1)][1], rows[k][(0, 0)][1])) for k in big]
    lose = [(k, d, s) for k, d, s in worse if d > s]
    print(f"query_top: on is slower than off by more than the spread on {len(lose)} of {len(big)} rows at n >= 2^20"
          + "".join(f"\n    {k}: +{d:.3f} ms (spread {s:.3f})" for k, d, s in lose)
          + f"\n  -> default {'off' if lose else 'on'}", flush=True)
    tp = 0 if lose else 1
    n0 = None
    for log2n in sorted({k[2] for k in rows}):
        ok = True
        for k in [k for k in rows if k[2] == log2n]:
            ratio = rows[k][(1, tp)][0] / rows[k][(0, tp)][0]
            limit = 1.02 if k[1] == "primary" else 0.95
            ok = ok and ratio <= limit
            print(f"  sort / unsorted (top={tp}) {k}: {ratio:.3f} (limit {limit})", flush=True)
        if ok and n0 is None:
            n0 = log2n
    print("query_sort auto: " + (f"sort when n >= 2^{n0}" if n0 is not None else "off -- sorting lost: no measured n qualifies"),
          flush=True)


if __name__ == "__main__":
    main()
