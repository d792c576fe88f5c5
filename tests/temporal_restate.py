"""Temporal accumulation as include/tmpt.h states it (tmpt_render_motion,
tmpt_temporal), restated in float32 numpy: one numpy operation per operation of
the contract, in its order, written from the header and not from the kernels.
tests/test_temporal_restate.py proves this file on the CPU before
tests/test_gpu_temporal.py holds the GPU to it bit for bit.

``centre_rays()``   the motion pass's ray of every pixel (no lens, no draw)
``scan()``          Moller-Trumbore over all triangles in the rounding order
                    tests/mt_numpy.py documents, returning t, u, v and the
                    lowest index among the closest t (the rule of a scene
                    without an octree)
``hit_pos()``       ((1 - u) - v) v0 + u v1 + v v2
``project()``       a world point through a camera: px, py, depth_prev, valid
``motion()``        the records of a whole frame (MOTION_DTYPE's fields)
``blend()``         tmpt_temporal's per-pixel arithmetic over a whole frame
``pack()``          the 8-bit pixels of a float frame

A camera is the 22 floats of ``Camera.as_array()``: origin, lower_left,
horizontal, vertical, u, v, w, lens_radius.
"""
import numpy as np

f32 = np.float32
EPS = f32(1e-5)
ONE, ZERO, HALF = f32(1.0), f32(0.0), f32(0.5)
TMIN, TMAX = f32(0.001), f32(1.0e7)
N_MAX_DEFAULT, SIGMA_DEPTH_DEFAULT = f32(3), f32(0.05)  # tmpt_temporal_desc's 0 values

MOTION_FIELDS = [("px", f32), ("py", f32), ("depth", f32), ("depth_prev", f32), ("u", f32), ("v", f32),
                 ("tri_id", np.int32), ("flags", np.uint32)]
MOTION_DTYPE = np.dtype(MOTION_FIELDS)


def _cam(cam):
    c = np.asarray(cam, f32)
    assert c.shape == (22,)
    return dict(o=c[0:3], ll=c[3:6], hz=c[6:9], vt=c[9:12], w=c[18:21])


def _dot(a, b):  # (ax*bx + ay*by) + az*bz, on the last axis
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - y[..., 1] * x[..., 2], x[..., 2] * y[..., 0] - y[..., 2] * x[..., 0],
                     x[..., 0] * y[..., 1] - y[..., 0] * x[..., 1]], -1)


def centre_rays(cam, w, h, ys=None):
    """-> (o float32[3], d float32[rows, w, 3]) for the global rows ys (default: all)."""
    c = _cam(cam)
    ys = np.arange(h) if ys is None else np.asarray(ys)
    inv_w, inv_h = ONE / f32(w), ONE / f32(h)
    s = (np.arange(w).astype(f32) + HALF) * inv_w
    t = (ys.astype(f32) + HALF) * inv_h
    v = ((c["ll"] + s[None, :, None] * c["hz"]) + t[:, None, None] * c["vt"]) - c["o"]
    d = v * (ONE / np.sqrt(_dot(v, v)))[..., None]
    assert d.dtype == f32
    return c["o"], d


def scan(o, d, tris):
    """The linear scan: o float32[3], d float32[n, 3], tris [m, 3, 3] ->
    (ids int32[n] or -1, t, u, v float32[n]; 0 on a miss)."""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    d = np.asarray(d, f32).reshape(-1, 3)
    n = d.shape[0]
    ids, bt = np.full(n, -1, np.int32), np.zeros(n, f32)
    bu, bv = np.zeros(n, f32), np.zeros(n, f32)
    if tris.shape[0] == 0:
        return ids, bt, bu, bv
    v0, e1, e2 = tris[None, :, 0], tris[None, :, 1] - tris[None, :, 0], tris[None, :, 2] - tris[None, :, 0]
    step = max(1, 2_000_000 // tris.shape[0])
    for a in range(0, n, step):
        dd = d[a:a + step, None, :]
        with np.errstate(all="ignore"):
            pvec = _cross(dd, e2)
            det = _dot(e1, pvec)
            ok = ~((det > -EPS) & (det < EPS))
            inv = ONE / det
            tvec = np.asarray(o, f32) - v0
            u = _dot(tvec, pvec) * inv
            ok &= ~((u < ZERO) | (u > ONE))
            qvec = _cross(tvec, e1)
            v = _dot(dd, qvec) * inv
            ok &= ~((v < ZERO) | (u + v > ONE))
            t = _dot(e2, qvec) * inv
            ok &= (t >= TMIN) & (t <= TMAX)
        assert t.dtype == f32
        tt = np.where(ok, t, f32(np.inf))
        k = tt.argmin(1)  # the first (lowest) index of the minimum
        r = np.arange(tt.shape[0])
        hit = np.isfinite(tt[r, k])
        sl = slice(a, a + tt.shape[0])
        ids[sl] = np.where(hit, k, -1)
        bt[sl] = np.where(hit, t[r, k], ZERO)
        bu[sl] = np.where(hit, np.broadcast_to(u, tt.shape)[r, k], ZERO)
        bv[sl] = np.where(hit, v[r, k], ZERO)
    return ids, bt, bu, bv


def hit_pos(v0, v1, v2, u, v):
    """(((1 - u) - v) * v0 + u * v1) + v * v2, componentwise; u, v float32[n]."""
    w0 = (ONE - u) - v
    return (w0[..., None] * v0 + u[..., None] * v1) + v[..., None] * v2


def project(cam, p, w, h):
    """p float32[..., 3] through the pinhole of cam -> (px, py, depth_prev, valid);
    the three floats are 0 where not valid."""
    c = _cam(cam)
    p = np.asarray(p, f32)
    dd = p - c["o"]
    q = c["ll"] - c["o"]
    den = _dot(dd, c["w"])
    num = _dot(q, c["w"])
    valid = den < ZERO
    with np.errstate(all="ignore"):
        k = num / den
        r = k[..., None] * dd - q
        px = (_dot(r, c["hz"]) / _dot(c["hz"], c["hz"])) * f32(w)
        py = (_dot(r, c["vt"]) / _dot(c["vt"], c["vt"])) * f32(h)
        dp = np.sqrt(_dot(dd, dd))
    assert px.dtype == f32 and dp.dtype == f32
    return (np.where(valid, px, ZERO), np.where(valid, py, ZERO), np.where(valid, dp, ZERO), valid)


def motion(tris, cam, prev_cam, w, h, prev_tris=None, ys=None):
    """The records tmpt_render_motion writes for the global rows ys (default:
    the whole frame), for a scene without an octree."""
    tris = np.asarray(tris, f32).reshape(-1, 3, 3)
    prev = tris if prev_tris is None else np.asarray(prev_tris, f32).reshape(-1, 3, 3)
    assert prev.shape == tris.shape
    o, d = centre_rays(cam, w, h, ys)
    rows = d.shape[0]
    ids, t, u, v = scan(o, d.reshape(-1, 3), tris)
    hit = ids >= 0
    tp = prev[np.maximum(ids, 0)]
    pp = hit_pos(tp[:, 0], tp[:, 1], tp[:, 2], u, v)
    px, py, dp, valid = project(prev_cam, pp, w, h)
    valid &= hit
    rec = np.zeros(rows * w, MOTION_DTYPE)
    rec["px"], rec["py"], rec["depth_prev"] = (np.where(valid, a, ZERO) for a in (px, py, dp))
    rec["depth"], rec["u"], rec["v"], rec["tri_id"] = t, u, v, ids
    rec["flags"] = hit.astype(np.uint32) | (valid.astype(np.uint32) << 1)
    return rec.reshape(rows, w)


def blend(cur, mot, pmot, hist, n_max=0.0, sigma_depth=0.0):
    """tmpt_temporal over a whole frame: cur, hist float32[h, w, 4]; mot, pmot
    records [h, w] -> float32[h, w, 4]."""
    cur, hist = np.asarray(cur, f32), np.asarray(hist, f32)
    h, w = cur.shape[:2]
    n_max = f32(n_max) if n_max else N_MAX_DEFAULT
    sigma = f32(sigma_depth) if sigma_depth else SIGMA_DEPTH_DEFAULT
    out = cur.copy()
    out[..., 3] = ONE
    mpx, mpy, dprev = mot["px"], mot["py"], mot["depth_prev"]
    with np.errstate(all="ignore"):
        ok = ((mot["flags"] & 2) != 0) & (mpx >= f32(-1)) & (mpx < f32(w) + ONE) & (mpy >= f32(-1)) & (mpy < f32(h) + ONE)
        fx, fy = np.where(ok, mpx, ZERO) - HALF, np.where(ok, mpy, ZERO) - HALF
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        csum = np.zeros((h, w, 3), f32)
        nsum, wsum = np.zeros((h, w), f32), np.zeros((h, w), f32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                wgt = (ax if i else ONE - ax) * (ay if j else ONE - ay)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                pm, hq = pmot[cy, cx], hist[cy, cx]
                skip = ~inside | ((pm["flags"] & 1) == 0) | (np.abs(pm["depth"] - dprev) > sigma * dprev)
                take = ok & ~skip
                csum = np.where(take[..., None], csum + hq[..., :3] * wgt[..., None], csum)
                nsum = np.where(take, nsum + hq[..., 3] * wgt, nsum)
                wsum = np.where(take, wsum + wgt, wsum)
        go = ok & (wsum > ZERO)
        hcol = csum / wsum[..., None]
        n = np.fmin(nsum / wsum + ONE, n_max)
        a = ONE / n
        res = hcol + (cur[..., :3] - hcol) * a[..., None]
    assert res.dtype == f32 and n.dtype == f32
    out[..., :3] = np.where(go[..., None], res, out[..., :3])
    out[..., 3] = np.where(go, n, ONE)
    return out


def pack(rad):
    """pack_pixel(col, 1.0f): uint8(saturate(sqrtf(k)) * 255), alpha 255."""
    out = np.full(rad.shape[:-1] + (4,), 255, np.uint8)
    with np.errstate(all="ignore"):
        s = np.sqrt(rad[..., :3])
        # saturate = gmin(gmax(v, 0), 1) with C ternaries: (v < 0) ? 0 : v keeps a NaN, then (1 < x) ? 1 : x keeps it
        s = np.where(s < ZERO, ZERO, s)
        s = np.where(ONE < s, ONE, s)
        out[..., :3] = (s * f32(255)).astype(np.uint8)
    return out
