"""Adversarial rays for the scene queries: the ray side of geometry_cases.py.

Pure numpy, seeded: no GPU library and no oracle here, so the same arrays
reach the CPU preconditions (test_ray_cases.py) and the GPU tests
(test_gpu_ray_cases.py).

``families()``  name -> rays (n, 6) float32 {origin, direction} for one scene
``ranged()``    the same rays as (n, 8) with a range per ray

Every family aims at target points on random triangles: a third of them on an
edge (one barycentric coordinate zero), a fifth exactly a vertex (its own
float32 values).  L is the vertex box's largest extent, D its diagonal.

axis         direction exactly +-e_k, the two zero components independently
             +0.0 or -0.0, origin the point moved back along the axis by
             (0.5 .. 1.5) L: rays inside the planes of the triangles' own
             bounding boxes (hence of leaf boxes), through shared vertices
             and edges.  What they stress in tmpt_traverse.h: 1/d clamped by
             safe_inv, the octant taken from the sign of 1/d (so of -0.0).
near_axis    the axis rays with the zero components replaced by +-NEAR_EPS --
             values on both sides of safe_inv's clamp (1e-20), one subnormal
             in float32 -- normalised in float64 before the cast.
in_plane     flat scenes only: origin and direction inside the scene's plane;
             every ray misses (Moller-Trumbore's |det| < 1e-5 rejection).
far_sphere_M origin at M D from the box centre in a random direction.
far_axis_M   origin at M D along one signed axis, jittered by the box extent
             on the other two.
             Both: half the rays aim at the point, the other half at the point
             moved by up to 0.3 L (these graze or miss).  The rounding of
             o * (1/d) in the slab test grows with |o|.
"""
import numpy as np

import geometry_cases as G

f32, f64 = np.float32, np.float64

NEAR_EPS = (1e-3, 1e-7, 1e-12, 9e-21, 1.1e-20, 1e-30, 1e-40)
FAR_ASSERTED = (10, 100)
FAR_REPORT = (1000, 10000)
ASSERTED = ("axis", "near_axis") + tuple(f"far_{k}_{m}" for m in FAR_ASSERTED for k in ("sphere", "axis"))
REPORT_ONLY = tuple(f"far_{k}_{m}" for m in FAR_REPORT for k in ("sphere", "axis"))

# the ten ranges of test_hitscene_per_ray_ranges (test_gpu_parity.py), at unit scale
RANGES = np.array([(0.001, 1e7), (0.0, 1e7), (-2.0, 1e7), (0.001, 1.5), (0.5, 4.0), (2.0, 2.0001),
                   (3.0, 1.0), (0.001, 0.001), (-1e7, 0.0), (-0.5, 0.25)], f64)


def _box(tris):
    v = np.asarray(tris, f32).reshape(-1, 3).astype(f64)
    return v.min(0), v.max(0)


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def targets(tris, n, rng):
    """n points on random triangles, float32: a third on an edge, a fifth a vertex."""
    tris = np.asarray(tris, f32)
    t = rng.integers(0, tris.shape[0], n)
    bary = rng.random((n, 3))
    edge = rng.random(n) < 1.0 / 3.0
    bary[edge, rng.integers(0, 3, edge.sum())] = 0.0
    bary /= bary.sum(1, keepdims=True)
    p = np.einsum("kj,kjc->kc", bary, tris[t].astype(f64)).astype(f32)
    vert = rng.random(n) < 0.2
    p[vert] = tris[t[vert], rng.integers(0, 3, vert.sum())]  # the vertex's own bits
    return p


def _signed_zero(rng, n):
    return np.where(rng.random(n) < 0.5, f32(0.0), f32(-0.0)).astype(f32)


def _axis(tris, n, rng):
    """-> (rays, axis k per ray)"""
    lo, hi = _box(tris)
    L = (hi - lo).max()
    p = targets(tris, n, rng)
    k = rng.integers(0, 3, n)
    s = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    d = np.stack([_signed_zero(rng, n) for _ in range(3)], 1)
    d[np.arange(n), k] = s
    o = p.copy()  # the other two coordinates keep the point's bits
    o[np.arange(n), k] = (p[np.arange(n), k].astype(f64) - s * (0.5 + rng.random(n)) * L).astype(f32)
    return np.concatenate([o, d], 1).astype(f32), k


def _near_axis(tris, n, rng):
    rays, k = _axis(tris, n, rng)
    d = rays[:, 3:].astype(f64)
    eps = np.array(NEAR_EPS)[rng.integers(0, len(NEAR_EPS), (n, 3))] * np.where(rng.random((n, 3)) < 0.5, 1.0, -1.0)
    off = np.arange(3)[None, :] != k[:, None]
    d[off] = eps[off]
    rays[:, 3:] = _unit(d).astype(f32)
    return rays


def _in_plane(tris, n, rng):
    """None unless one extent of the scene is zero."""
    lo, hi = _box(tris)
    flat = np.nonzero(hi == lo)[0]
    if flat.size != 1:
        return None
    ax = int(flat[0])
    pad = 0.2 * (hi - lo).max()
    o = (lo - pad + rng.random((n, 3)) * (hi - lo + 2.0 * pad)).astype(f32)
    d = rng.normal(size=(n, 3))
    k = n // 2  # half aim at points of the scene, half go anywhere in the plane
    d[:k] = targets(tris, k, rng).astype(f64) - o[:k]
    d[:, ax] = 0.0
    d = _unit(d).astype(f32)
    o[:, ax] = _signed_zero(rng, n) if lo[ax] == 0.0 else f32(lo[ax])
    d[:, ax] = _signed_zero(rng, n)
    return np.concatenate([o, d], 1).astype(f32)


def _aim(tris, o, rng):
    """Directions from the float32 origins o: half at a target point, half at
    the point moved by up to 0.3 L on every axis."""
    n = o.shape[0]
    lo, hi = _box(tris)
    L = (hi - lo).max()
    p = targets(tris, n, rng).astype(f64)
    p[n // 2:] += (rng.random((n - n // 2, 3)) * 2.0 - 1.0) * 0.3 * L
    return np.concatenate([o, _unit(p - o.astype(f64)).astype(f32)], 1).astype(f32)


def _far_sphere(tris, n, rng, m):
    lo, hi = _box(tris)
    D = np.linalg.norm(hi - lo)
    o = (0.5 * (lo + hi) + m * D * _unit(rng.normal(size=(n, 3)))).astype(f32)
    return _aim(tris, o, rng)


def _far_axis(tris, n, rng, m):
    lo, hi = _box(tris)
    D = np.linalg.norm(hi - lo)
    k = rng.integers(0, 3, n)
    s = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    o = 0.5 * (lo + hi) + (rng.random((n, 3)) * 2.0 - 1.0) * (hi - lo)
    o[np.arange(n), k] = 0.5 * (lo + hi)[k] + s * m * D
    return _aim(tris, o.astype(f32), rng)


def families(tris, n, seed):
    """name -> rays (n, 6) float32; in_plane only for a flat scene."""
    tris = np.asarray(tris, f32)
    out = {}
    rng = lambda i: np.random.default_rng([seed, i])  # noqa: E731  one stream per family
    out["axis"] = _axis(tris, n, rng(0))[0]
    out["near_axis"] = _near_axis(tris, n, rng(1))
    flat = _in_plane(tris, n, rng(2))
    if flat is not None:
        out["in_plane"] = flat
    for i, m in enumerate(FAR_ASSERTED + FAR_REPORT):
        out[f"far_sphere_{m}"] = _far_sphere(tris, n, rng(10 + i), m)
        out[f"far_axis_{m}"] = _far_axis(tris, n, rng(20 + i), m)
    assert all(a.dtype == f32 and a.shape == (n, 6) for a in out.values())
    return out


def range_unit(tris):
    """geometry_cases.ray_range's unit: the scene diagonal rounded to a power of ten."""
    return G.ray_range(tris)[0] / 1e-3


def ranged(rays, seed, unit=1.0):
    """rays (n, 6) -> (n, 8) float32 {origin, direction, tmin, tmax}: each ray
    draws one of RANGES, scaled by unit (range_unit of the scene) -- ranges
    starting behind the origin (the traversal's NEG instantiation) and empty
    ones among them."""
    rays = np.asarray(rays, f32)
    k = np.random.default_rng([seed, 99]).integers(0, len(RANGES), rays.shape[0])
    return np.concatenate([rays, (RANGES[k] * unit).astype(f32)], 1).astype(f32)
