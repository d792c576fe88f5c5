"""The noise-aware filter's two contracts (include/tmpt.h: tmpt_render_moments,
tmpt_denoise_moments) restated in numpy float32 -- one numpy operation per
operation of the header, in its order.  Written from the header, not from the
kernels.  The moments are formed from per-sample colours (the reference's own,
or the oracle's); the filter restates tmpt_denoise's level with the variance
carried beside it, and test_moments_abi.py holds it to np_denoise (the plain
filter's restatement) where the header says the two agree.

Shared by test_moments_abi.py (CPU), test_gpu_moments.py and
test_gpu_denoise_moments.py.
"""
import numpy as np

f32 = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)
K3 = np.array([0.25, 0.5, 0.25], f32)
#: tmpt_denoise_moments' default, spelled out (include/tmpt.h)
SHRINK_DEFAULT = f32(2.0)


def _dot(a, b):  # (ax*bx + ay*by) + az*bz
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def luminance(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def moments_expect(col, n_p):
    """tmpt_render_moments' moments_out over per-sample colours col[h, w, S, 3]
    (sample order) and each pixel's count n_p[h, w] (an int for a uniform frame):
    {m1 / fn, m2 / fn, 1.0f / fn, 1.0f}, m1 and m2 carried over samples [0, n_p)."""
    col = np.asarray(col, f32)
    h, w, cap = col.shape[:3]
    n_p = np.broadcast_to(np.asarray(n_p, np.int32), (h, w))
    assert n_p.min() >= 1 and n_p.max() <= cap
    m1, m2 = np.zeros((h, w), f32), np.zeros((h, w), f32)
    with np.errstate(all="ignore"):
        for s in range(int(n_p.max())):
            y = luminance(col[:, :, s])
            on = s < n_p
            m1 = np.where(on, m1 + y, m1)
            m2 = np.where(on, m2 + y * y, m2)
        fn = n_p.astype(f32)
        out = np.stack([m1 / fn, m2 / fn, f32(1) / fn, np.ones((h, w), f32)], -1)
    assert out.dtype == f32
    return out


def v0_expect(mom):
    """v_0, the variance of the pixel's mean luminance."""
    mom = np.asarray(mom, f32)
    with np.errstate(all="ignore"):
        ne = mom[..., 3] / mom[..., 2]
        return np.fmax(f32(0), mom[..., 1] - mom[..., 0] * mom[..., 0]) / np.fmax(ne - f32(1), f32(1))


def synthetic_moments(w, h, seed=1, positive=False):
    """A moments plane with every case v_0's statement knows, by pixel index
    (the frames of more than 8 pixels hold all of them; `check_synthetic_moments`
    asserts it): mu2 < mu1 * mu1 (the variance clamps to 0), mu2 == mu1 * mu1
    exactly, history lengths 1 .. 5, mom.z from the counts 2, 3 and 8, and one
    pixel with mom.z = 0.  positive: v_0 > 0 everywhere instead (no such cases)."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    idx = np.arange(w * h).reshape(h, w)
    mu1 = (f32(0.2) + f32(1.8) * rng.random((h, w)).astype(f32)).astype(f32)
    sq = mu1 * mu1
    mu2 = (sq + sq * (f32(0.05) + rng.random((h, w)).astype(f32))).astype(f32)
    count = np.choose(idx % 3, [2, 3, 8]).astype(f32)
    z = (f32(1) / count).astype(f32)
    hist = (1 + idx % 5).astype(f32)
    if not positive:
        mu2 = np.where(idx % 7 == 1, sq * f32(0.9), mu2).astype(f32)
        mu2 = np.where(idx % 7 == 3, sq, mu2).astype(f32)
        if w * h > 8:
            z[idx == 5] = 0
    return np.stack([mu1, mu2, z, hist], -1).astype(f32)


def check_synthetic_moments(mom):
    """The cases synthetic_moments promises, asserted on the plane itself."""
    mu1, mu2, z, hist = (mom[..., k] for k in range(4))
    sq = mu1 * mu1
    assert (mu2 < sq).any() and (mu2 == sq).any() and (mu2 > sq).any()
    assert set(np.unique(hist)) == {1, 2, 3, 4, 5}
    assert {f32(1) / f32(2), f32(1) / f32(3), f32(1) / f32(8)} <= set(np.unique(z))
    assert (z == 0).sum() == 1
    v0 = v0_expect(mom)
    assert np.isfinite(v0).all() and (v0 == 0).any() and (v0 > 0).any()


def build_digests(tm, obj):
    """One synthetic and one real case of each new call through the library `tm` has
    loaded, as digests: run by the checked build in a child process and by the plain
    build in the test itself (test_gpu_denoise_moments.py), which compares the two."""
    import hashlib

    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {}
    w, h, spp = 64, 36, 4
    tris, bmin, bmax = tm.load_scene(obj)
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        rad, mom, img, cnt, rays, info = sc.trace_moments(cam, w, h, spp)
        out["uniform"] = [sha(rad), sha(mom), sha(img), sha(cnt), rays]
        res = sc.trace_moments(cam, w, h, 8, 2, 2, 0.05, radius=1)
        out["adaptive"] = [sha(a) for a in res[:4]] + [res[4], res[5]["pass_pixels"]]
        aov, _ = sc.trace_aov(cam, w, h, spp)
        # a synthetic frame: random guides with a sky block, the moments plane with every case
        rng = np.random.default_rng(11)
        s_rad = (rng.random((23, 37, 4)) * 4).astype(f32)
        s_aov = np.zeros((23, 37), tm.AOV_DTYPE)
        s_aov["hits"] = rng.integers(1, 5, (23, 37))
        s_aov["hits"][15:, 5:30] = 0
        s_aov["normal"] = (rng.random((23, 37, 3)) - 0.5).astype(f32)
        s_aov["depth"] = (3 + rng.random((23, 37))).astype(f32)
        s_aov["direct"] = (rng.random((23, 37)) > 0.5).astype(f32)
        s_mom = synthetic_moments(37, 23)
        for lds in (0, 1):
            sc.set_option("denoise_lds", lds)
            out[f"real{lds}"] = [sha(a) for a in sc.denoise_moments(rad, aov, mom, spp)]
            out[f"synthetic{lds}"] = [sha(a) for a in sc.denoise_moments(s_rad, s_aov, s_mom, 4, 2.0, 6)]
    return out


def _shift(h, w, dx, dy):
    """(p slices, q slices) of the pixels p whose tap q = p + (dx, dy) lies in the frame, or None."""
    py = slice(max(0, -dy), min(h, h - dy))
    px = slice(max(0, -dx), min(w, w - dx))
    if py.start >= py.stop or px.start >= px.stop:
        return None
    return (py, px), (slice(py.start + dy, py.stop + dy), slice(px.start + dx, px.stop + dx))


def np_denoise_moments(rad, aov, mom, spp, shrink=0.0, levels=0, normal_exp=-1, sigma_depth=0.0, sigma_direct=0.0):
    """include/tmpt.h, tmpt_denoise_moments, restated over a whole frame: rad and
    mom float32[h, w, 4], aov the AOV records [h, w] -> float32[h, w, 4]."""
    rad, mom = np.asarray(rad, f32), np.asarray(mom, f32)
    h, w = rad.shape[:2]
    levels = levels or 5
    normal_exp = 5 if normal_exp < 0 else normal_exp
    sigma_depth = f32(sigma_depth) if sigma_depth else f32(1) / f32(h)
    sigma_direct = f32(sigma_direct) if sigma_direct else f32(0.05)
    shrink = f32(shrink) if shrink else SHRINK_DEFAULT
    # the guides, as tmpt_denoise forms them
    hits = aov["hits"]
    cov = hits > 0
    nrm = np.ascontiguousarray(aov["normal"], f32)
    nh = nrm * (f32(1) / np.sqrt(np.fmax(_dot(nrm, nrm), f32(1e-30))))[..., None]
    with np.errstate(all="ignore"):  # zb is read only where cov
        zb = np.where(cov, aov["depth"] * (f32(spp) / hits.astype(f32)), f32(1)).astype(f32)
    dl = np.ascontiguousarray(aov["direct"], f32)
    cur = np.ascontiguousarray(rad, f32).copy()
    v = v0_expect(mom)
    keep = np.zeros((h, w, 3), f32)
    with np.errstate(all="ignore"):
        for level in range(levels):
            s = 1 << level
            csum = np.zeros((h, w, 3), f32)
            wsum, vsum = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    pq = _shift(h, w, s * i, s * j)
                    if pq is None:
                        continue
                    p, q = pq
                    covp = cov[p]
                    if i == 0 and j == 0:
                        wt = np.full(covp.shape, H5[2] * H5[2], f32)
                    else:
                        base = H5[i + 2] * H5[j + 2]
                        c = np.fmax(f32(0), _dot(nh[p], nh[q]))
                        for _ in range(normal_exp):
                            c = c * c
                        g = base * c
                        rz = (zb[p] - zb[q]) / ((sigma_depth * np.fmin(zb[p], zb[q])) * f32(s * max(abs(i), abs(j))))
                        g = g * (f32(1) / (f32(1) + rz * rz))
                        rd = (dl[p] - dl[q]) / sigma_direct
                        g = g * (f32(1) / (f32(1) + rd * rd))
                        wt = np.where(covp, g, base).astype(f32)
                    take = covp == cov[q]
                    csum[p] = np.where(take[..., None], csum[p] + cur[q][..., :3] * wt[..., None], csum[p])
                    wsum[p] = np.where(take, wsum[p] + wt, wsum[p])
                    vsum[p] = np.where(take, vsum[p] + v[q] * (wt * wt), vsum[p])
            nxt = cur.copy()  # .w passes through
            nxt[..., :3] = csum / wsum[..., None]
            vnext = vsum / (wsum * wsum)
            # the 3 x 3 Gaussian of v_L, distance 1 at every level
            gsum, ksum = np.zeros((h, w), f32), np.zeros((h, w), f32)
            for j in range(-1, 2):
                for i in range(-1, 2):
                    pq = _shift(h, w, i, j)
                    if pq is None:
                        continue
                    p, q = pq
                    k = K3[i + 1] * K3[j + 1]
                    take = cov[p] == cov[q]
                    gsum[p] = np.where(take, gsum[p] + v[q] * k, gsum[p])
                    ksum[p] = np.where(take, ksum[p] + k, ksum[p])
            g = gsum / ksum
            d = cur[..., :3] - nxt[..., :3]
            dy = luminance(d)
            e, n = dy * dy, shrink * g
            gain = np.where(e > n, (e - n) / e, f32(0)).astype(f32)  # a NaN compares false
            keep = keep + d * gain[..., None]
            cur, v = nxt, vnext
        out = cur.copy()
        out[..., :3] = cur[..., :3] + keep
    assert out.dtype == f32 and v.dtype == f32 and keep.dtype == f32
    return out
