"""Moller-Trumbore as the reference states it (RayIntersectTriangleImproved,
maths.cpp:339-380) in float32 numpy, over rays x triangles: a second
reference for the scene queries, independent of oracle/.

Every operation rounds once to float32, the dot product is (x*x' + y*y') +
z*z' as GLM evaluates it, the cross product is GLM's, 1/det is formed and
multiplied.  A comparison with a NaN is false on both sides, as in C.

``accepted_t()``  t of every (ray, triangle) the test accepts, +inf elsewhere
``closest()``     the linear scan: lowest index among the closest t, its t,
                  and how many triangles are tied on it
``tied_sets()``   the triangles tied on the closest t, per tied ray
``pair_t()``      the accepted t of one given triangle per ray
"""
import numpy as np

f32 = np.float32
EPS = f32(1e-5)
ONE, ZERO = f32(1.0), f32(0.0)
PAIRS = 4_000_000  # (ray, triangle) pairs per chunk


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(x, y):
    return (x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1])


def _mt(o, d, v0, v1, v2, tmin, tmax):
    """o, d, v0, v1, v2: 3-tuples of float32 arrays that broadcast together;
    tmin, tmax float32 scalars or arrays -> t float32, +inf where rejected."""
    with np.errstate(all="ignore"):
        e1, e2 = _sub(v1, v0), _sub(v2, v0)
        pvec = _cross(d, e2)
        det = _dot(e1, pvec)
        ok = ~((det > -EPS) & (det < EPS))
        inv = ONE / det
        tvec = _sub(o, v0)
        u = _dot(tvec, pvec) * inv
        ok &= ~((u < ZERO) | (u > ONE))
        qvec = _cross(tvec, e1)
        v = _dot(d, qvec) * inv
        ok &= ~((v < ZERO) | (u + v > ONE))
        t = _dot(e2, qvec) * inv
        ok &= (t >= tmin) & (t <= tmax)
    assert t.dtype == f32
    return np.where(ok, t, f32(np.inf))


def _cols(a):
    return tuple(a[..., c] for c in range(3))


def _range(x, n):
    return np.broadcast_to(np.asarray(x, f32), (n,)) if np.ndim(x) else np.full(n, f32(x), f32)


def _chunks(rays, tris, tmin, tmax):
    rays = np.asarray(rays, f32)
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    n = rays.shape[0]
    lo, hi = _range(tmin, n), _range(tmax, n)
    v = [_cols(tris[None, :, k]) for k in range(3)]
    step = max(1, PAIRS // max(1, tris.shape[0]))
    for a in range(0, n, step):
        r = rays[a:a + step, None, :]
        yield a, _mt(_cols(r[..., 0:3]), _cols(r[..., 3:6]), v[0], v[1], v[2], lo[a:a + step, None], hi[a:a + step, None])


def accepted_t(rays, tris, tmin, tmax):
    """(rays, triangles) float32: the accepted t, +inf where the test rejects."""
    rays = np.asarray(rays, f32)
    return np.concatenate([t for _, t in _chunks(rays, tris, tmin, tmax)]) if len(rays) else np.zeros((0, 0), f32)


def closest(rays, tris, tmin, tmax):
    """-> (ids int32: lowest index among the closest t or -1, t float32 (+inf
    on a miss), tied int32: triangles at that t)."""
    n = np.asarray(rays).shape[0]
    ids, best, tied = np.full(n, -1, np.int32), np.full(n, np.inf, f32), np.zeros(n, np.int32)
    for a, t in _chunks(rays, tris, tmin, tmax):
        if t.shape[1] == 0:
            continue
        m = t.min(1)
        hit = np.isfinite(m)
        sl = slice(a, a + t.shape[0])
        best[sl] = m
        ids[sl] = np.where(hit, t.argmin(1), -1)  # argmin: the first (lowest) index of the minimum
        tied[sl] = np.where(hit, (t == m[:, None]).sum(1), 0)
    return ids, best, tied


def tied_sets(rays, tris, tmin, tmax):
    """ray index -> triangle indices tied on its closest t (rays with more than one)."""
    out = {}
    for a, t in _chunks(rays, tris, tmin, tmax):
        if t.shape[1] == 0:
            continue
        m = t.min(1)
        eq = (t == m[:, None]) & np.isfinite(m)[:, None]
        for r in np.nonzero(eq.sum(1) > 1)[0]:
            out[a + int(r)] = np.nonzero(eq[r])[0]
    return out


def pair_t(rays, tris, ids, tmin, tmax):
    """The accepted t of triangle ids[i] for ray i (+inf: rejected, or ids[i] < 0)."""
    rays = np.asarray(rays, f32)
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    ids = np.asarray(ids)
    n = rays.shape[0]
    if tris.shape[0] == 0:
        return np.full(n, np.inf, f32)
    tr = tris[np.maximum(ids, 0)]
    t = _mt(_cols(rays[:, 0:3]), _cols(rays[:, 3:6]), _cols(tr[:, 0]), _cols(tr[:, 1]), _cols(tr[:, 2]),
            _range(tmin, n), _range(tmax, n))
    return np.where(ids >= 0, t, f32(np.inf))
