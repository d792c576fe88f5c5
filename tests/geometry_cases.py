"""Adversarial geometry for the BVH build, and rays to query it with.

Pure numpy, seeded: no GPU library and no oracle here, so the same arrays
reach the CPU check of this generator (test_geometry_cases.py) and the GPU
build tests (test_gpu_build_geometry.py).

``cases()``   name -> triangles (n, 3, 3) float32, the smallest shapes at which
              each stage of the build (tmpt_bvh.hip) can go wrong
``rays()``    rays (n, 6) float32 {origin, direction} for one case and the
              (tmin, tmax) range to query them with

The triangle counts of the sweep straddle the build's block (256), the wave
(64), the sort tile (1024), the one-block scan's switch to several entries per
thread (above 4096 keys) and, through the BVH4 node counts they give, the LDS
top caches of the path kernels (80, 116, 120 nodes).
"""
import zlib

import numpy as np

SWEEP_SMALL = tuple(range(3, 273))
SWEEP_LARGE = (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4100)
# 272 triangles of soup give about 80 BVH4 nodes, so two more counts reach the
# other side of the 116- and 120-node caches (the render tests use them)
SWEEP_NODES = (330, 480)
COINCIDENT = (3, 17, 64, 130, 200, 1000)


def _seed(name):
    return zlib.crc32(name.encode())


def soup(n, seed):
    """n triangles, centres uniform in the unit cube, vertices within +-0.075 of them."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3))
    return (c + (rng.random((n, 3, 3)) - 0.5) * 0.15).astype(np.float32)


def sweep_name(n):
    return f"soup{n}"


def zero_area(tris):
    """Triangles with two identical vertices: the points and segments the cases put in."""
    t = np.asarray(tris)
    return ((t[:, 0] == t[:, 1]).all(1) | (t[:, 1] == t[:, 2]).all(1) | (t[:, 0] == t[:, 2]).all(1))


def _floor(lo, hi, z=0.0):
    """Two triangles over [lo, hi]^2 at height z."""
    a, b, c, d = (lo, lo, z), (hi, lo, z), (hi, hi, z), (lo, hi, z)
    return np.array([[a, b, c], [a, c, d]], np.float32)


def _quads(ix, iy, pitch, size):
    """Equal axis-aligned quads (two triangles each) in the plane z = 0, their
    low corners at (ix, iy) * pitch: every coordinate a dyadic fraction."""
    out = np.zeros((len(ix), 2, 3, 3), np.float32)
    x0, y0 = ix * pitch, iy * pitch
    x1, y1 = x0 + size, y0 + size
    for k, (x, y) in enumerate(((x0, y0), (x1, y0), (x1, y1))):
        out[:, 0, k, 0], out[:, 0, k, 1] = x, y
    for k, (x, y) in enumerate(((x0, y0), (x1, y1), (x0, y1))):
        out[:, 1, k, 0], out[:, 1, k, 1] = x, y
    return out.reshape(-1, 3, 3)


def _non_sweep():
    out = {}
    # ---- coincident: one box for every cluster, every closest hit tied on t
    one = soup(1, _seed("coincident"))
    for k in COINCIDENT:
        out[f"coincident{k}"] = np.repeat(one, k, axis=0)
    # zero-area triangles alone answer no ray, so these two sit just above a
    # floor quad (two more triangles) that the rays aimed at them go on to
    p = np.array([0.5, 0.5, 0.015625], np.float32)
    out["points200"] = np.concatenate([np.tile(p, (200, 3, 1)), _floor(0.0, 1.0)])
    a, b = np.array([0.25, 0.25, 0.015625], np.float32), np.array([0.75, 0.5, 0.25], np.float32)
    out["segments200"] = np.concatenate([np.tile(np.stack([a, b, b]), (200, 1, 1)), _floor(0.0, 1.0)])
    # ---- same-box fan: distinct triangles, bit-identical bounding boxes
    rng = np.random.default_rng(_seed("fan"))
    fan = np.zeros((150, 3, 3), np.float32)
    fan[:, 1] = 1.0
    fan[:, 2] = rng.random((150, 3))
    out["samebox_fan150"] = fan
    # ---- nested: scaled copies of one triangle about its centre.  Every union
    # is the larger box, so each cluster's nearest neighbours are all the
    # smaller ones at one and the same area: PLOC merges one pair per pass
    # under either of its tie rules, and the build falls back to the LBVH
    one = soup(1, _seed("nested"))[0].astype(np.float64)
    k = 1.0 + np.arange(200)[:, None, None] / 8.0
    out["nested200"] = (one.mean(0) + k * (one - one.mean(0))).astype(np.float32)
    # ---- degenerate mix: points and segments at random places among a soup
    rng = np.random.default_rng(_seed("degenerate"))
    mix = soup(300, _seed("degenerate_soup"))
    for k in range(30):
        q = soup(1, _seed(f"degenerate{k}"))[0]
        q[1:] = q[0] if k % 2 == 0 else q[1]  # a point, or a segment v0-v1-v1
        mix = np.insert(mix, rng.integers(0, len(mix) + 1), q, axis=0)
    out["degenerate_mix"] = mix
    # ---- flat: one axis of zero extent (-0.0 and 0.0 both occur)
    for ax, nm in enumerate("xyz"):
        t = soup(300, _seed("flat" + nm))
        t[:, :, ax] *= np.float32(0.0)
        out[f"flat_{nm}"] = t
    # ---- collinear centroids: every box centre (and vertex mean) at x = y = 0.5
    rng = np.random.default_rng(_seed("collinear"))
    a = rng.integers(1, 77, 300) / 1024.0
    b = rng.integers(1, 77, 300) / 1024.0
    z = rng.random(300)[:, None] + (rng.random((300, 3)) - 0.5) * 0.15
    col = np.zeros((300, 3, 3))
    col[:, 0, 0], col[:, 0, 1] = 0.5 - a, 0.5 - b
    col[:, 1, 0], col[:, 1, 1] = 0.5 + a, 0.5
    col[:, 2, 0], col[:, 2, 1] = 0.5, 0.5 + b
    col[:, :, 2] = z
    out["collinear_centroids"] = col.astype(np.float32)
    # ---- equal boxes, equally spaced: a strip along x and a 16 x 16 sheet
    i = np.arange(256)
    # (quads of 1/32: Moller-Trumbore's |det| < 1e-5 rejection, maths.cpp:339-346,
    # makes a triangle under about 3e-3 across invisible to every ray)
    out["uniform_strip"] = _quads(i, np.zeros(256, int), 1.0 / 16, 1.0 / 32)
    gy, gx = np.divmod(i, 16)
    out["uniform_sheet"] = _quads(gx, gy, 1.0 / 16, 1.0 / 32)
    # ---- one Morton cell: 500 tiny triangles and a floor 10^7 times their size
    rng = np.random.default_rng(_seed("one_cell"))
    c = np.array([0.0, 0.0, 0.5]) + rng.random((500, 1, 3)) * 1e-2
    tiny = (c + (rng.random((500, 3, 3)) - 0.5) * 1e-3).astype(np.float32)
    out["one_cell"] = np.concatenate([tiny, _floor(-5.0e3, 5.0e3)])
    # ---- far from the origin, small, large, and stretched
    base = soup(300, _seed("moved"))
    out["translated_1e4"] = (base + np.array([1e4, -2e4, 5e3])).astype(np.float32)
    out["translated_3e5"] = (base + np.array([3e5, 3e5, 3e5])).astype(np.float32)
    # at 1e-4 the soup itself is invisible (|det| < 1e-5, above): the rays that
    # cross it are answered by a floor quad just below, large enough to be hit
    out["scaled_1e-4"] = np.concatenate([(base * np.float32(1e-4)).astype(np.float32),
                                         _floor(-1.0e-2, 1.0e-2, -1.0e-5)])
    out["scaled_1e4"] = (base * np.float32(1e4)).astype(np.float32)
    out["anisotropic"] = (base * np.array([1e3, 1.0, 1e-3], np.float32)).astype(np.float32)
    return out


NON_SWEEP = ("coincident3", "coincident17", "coincident64", "coincident130", "coincident200", "coincident1000",
             "points200", "segments200", "samebox_fan150", "nested200", "degenerate_mix", "flat_x", "flat_y", "flat_z",
             "collinear_centroids", "uniform_strip", "uniform_sheet", "one_cell", "translated_1e4",
             "translated_3e5", "scaled_1e-4", "scaled_1e4", "anisotropic")


def case(name):
    """One case by name (a sweep member without building the rest)."""
    if name.startswith("soup"):
        return soup(int(name[4:]), _seed(name))
    return _non_sweep()[name]


def cases():
    """name -> (n, 3, 3) float32: the count sweep, then the named families."""
    out = {sweep_name(n): soup(n, _seed(sweep_name(n))) for n in SWEEP_SMALL + SWEEP_NODES + SWEEP_LARGE}
    out.update(_non_sweep())
    assert tuple(k for k in out if not k.startswith("soup")) == NON_SWEEP
    return out


def ray_range(tris):
    """(tmin, tmax) = (1e-3 D, 1e7 D), D the vertex box diagonal rounded to a
    power of ten: the reference's 0.001 .. 1e7 at unit scale."""
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    e = int(np.round(np.log10(diag)))
    return float(f"1e{e - 3}"), float(f"1e{e + 7}")


def rays(tris, n, seed):
    """-> (rays (n, 6) float32, (tmin, tmax)).  Origins uniform in the vertex
    box padded on every axis by 0.2 x its largest extent (a flat scene gets
    origins out of its plane).  The first half aim at points on triangles -- a
    third of those snapped onto an edge, a tenth onto a vertex: grazing hits
    and t ties -- the other half have random directions."""
    tris = np.asarray(tris, np.float32)
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    pad = 0.2 * (hi - lo).max()
    o = (lo - pad + rng.random((n, 3)) * (hi - lo + 2.0 * pad)).astype(np.float32)
    k = n // 2
    t = rng.integers(0, tris.shape[0], k)
    bary = rng.random((k, 3))
    snap = rng.random(k) < 0.33
    bary[snap, rng.integers(0, 3, snap.sum())] = 0.0
    vert = rng.random(k) < 0.1
    bary[vert] = np.eye(3)[rng.integers(0, 3, vert.sum())]
    bary /= bary.sum(1, keepdims=True)
    target = np.einsum("kj,kjc->kc", bary, tris[t].astype(np.float64))
    d = np.empty((n, 3))
    d[:k] = target - o[:k]
    d[k:] = rng.normal(size=(n - k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d.astype(np.float32)], 1), ray_range(tris)
