"""History clipping as include/tmpt.h states it (tmpt_temporal_clip), restated
in float32 numpy: one numpy operation per operation of the contract, in its
order, written from the header and not from the kernel.
tests/test_temporal_clip_restate.py proves this file on the CPU before
tests/test_gpu_temporal_clip.py holds the GPU to it bit for bit.

``fetch()``   tmpt_temporal's reprojected history (the statements
              tests/temporal_restate.py's blend() restates, here with the sums
              kept apart and a second frame through the same taps)
``window()``  the (2r+1)^2 sums over the statistics frame, rows outer
``clip()``    the call over a whole frame -> (out, aux_out or None)
``parts()``   the same, with the intermediate frames a test wants to look at
"""
import numpy as np

from temporal_restate import HALF, ONE, SIGMA_DEPTH_DEFAULT, ZERO, f32

# tmpt_temporal_clip_desc's 0 values
N_MAX_DEFAULT, GAMMA_DEFAULT, RADIUS_DEFAULT = f32(3), f32(0.5), 1


def fetch(mot, pmot, hist, sigma, aux_hist=None):
    """-> (go bool[h, w], csum [h, w, 3], nsum, wsum [h, w], asum [h, w, 3] or None):
    go is False where the pixel resets; the sums are the header's, tap by tap."""
    h, w = hist.shape[:2]
    mpx, mpy, dprev = mot["px"], mot["py"], mot["depth_prev"]
    with np.errstate(all="ignore"):
        ok = ((mot["flags"] & 2) != 0) & (mpx >= f32(-1)) & (mpx < f32(w) + ONE) & (mpy >= f32(-1)) & (mpy < f32(h) + ONE)
        fx, fy = np.where(ok, mpx, ZERO) - HALF, np.where(ok, mpy, ZERO) - HALF
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        csum = np.zeros((h, w, 3), f32)
        asum = None if aux_hist is None else np.zeros((h, w, 3), f32)
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
                if asum is not None:
                    asum = np.where(take[..., None], asum + aux_hist[cy, cx][..., :3] * wgt[..., None], asum)
        go = ok & (wsum > ZERO)
    assert csum.dtype == f32 and nsum.dtype == f32 and wsum.dtype == f32
    return go, csum, nsum, wsum, asum


def window(stat, mot, r):
    """-> (s1 [h, w, 3], s2 [h, w, 3], cnt [h, w]) over q = p + (i, j), j outer."""
    h, w = stat.shape[:2]
    cov = (mot["flags"] & 1).astype(np.int8)
    sp = np.zeros((h + 2 * r, w + 2 * r, 3), f32)
    sp[r:r + h, r:r + w] = stat[..., :3]
    cp = np.full((h + 2 * r, w + 2 * r), 2, np.int8)  # outside the frame: neither coverage
    cp[r:r + h, r:r + w] = cov
    s1, s2, cnt = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
    with np.errstate(all="ignore"):
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                sq = sp[r + j:r + j + h, r + i:r + i + w]
                take = cp[r + j:r + j + h, r + i:r + i + w] == cov
                s1 = np.where(take[..., None], s1 + sq, s1)
                s2 = np.where(take[..., None], s2 + sq * sq, s2)
                cnt = np.where(take, cnt + ONE, cnt)
    assert s1.dtype == f32 and s2.dtype == f32 and cnt.dtype == f32
    return s1, s2, cnt


def parts(cur, mot, pmot, hist, gamma=0.0, radius=0, n_max=0.0, sigma_depth=0.0, stat=None, aux=None, aux_hist=None):
    cur, hist = np.asarray(cur, f32), np.asarray(hist, f32)
    stat = cur if stat is None else np.asarray(stat, f32)
    assert (aux is None) == (aux_hist is None)
    n_max = f32(n_max) if n_max else N_MAX_DEFAULT
    sigma = f32(sigma_depth) if sigma_depth else SIGMA_DEPTH_DEFAULT
    gamma = f32(gamma) if gamma else GAMMA_DEFAULT
    r = int(radius) if radius else RADIUS_DEFAULT
    go, csum, nsum, wsum, asum = fetch(mot, pmot, hist, sigma, None if aux is None else np.asarray(aux_hist, f32))
    s1, s2, cnt = window(stat, mot, r)
    with np.errstate(all="ignore"):
        hcol = csum / wsum[..., None]
        nh = nsum / wsum
        mu = s1 / cnt[..., None]
        var = np.fmax(ZERO, s2 / cnt[..., None] - mu * mu)
        sd = np.sqrt(var)
        g = gamma * sd
        lo, hi = mu - g, mu + g
        hc = np.fmin(np.fmax(hcol, lo), hi)
        d = np.abs(hcol - hc)
        e = np.fmax(np.fmax(d[..., 0], d[..., 1]), d[..., 2])
        span = np.fmax(np.fmax(g[..., 0], g[..., 1]), g[..., 2])
        nhc = np.where(e > ZERO, nh * (span / (span + e)), nh)
        n = np.fmin(nhc + ONE, n_max)
        a = ONE / n
        res = hc + (cur[..., :3] - hc) * a[..., None]
    for x in (hcol, nh, mu, sd, g, hc, e, span, nhc, n, a, res):
        assert x.dtype == f32
    out = cur.copy()
    out[..., :3] = np.where(go[..., None], res, cur[..., :3])
    out[..., 3] = np.where(go, n, ONE)
    aux_out = None
    if aux is not None:
        aux = np.asarray(aux, f32)
        with np.errstate(all="ignore"):
            ha = asum / wsum[..., None]
            ares = ha + (aux[..., :3] - ha) * a[..., None]
        assert ares.dtype == f32
        aux_out = aux.copy()
        aux_out[..., :3] = np.where(go[..., None], ares, aux[..., :3])
        aux_out[..., 3] = np.where(go, n, ONE)
    return dict(out=out, aux_out=aux_out, go=go, h=hcol, nh=nh, mu=mu, sd=sd, hc=hc, e=e, span=span, a=a, n=n, cnt=cnt)


def clip(cur, mot, pmot, hist, gamma=0.0, radius=0, n_max=0.0, sigma_depth=0.0, stat=None, aux=None, aux_hist=None):
    """tmpt_temporal_clip over a whole frame: cur, hist (stat, aux, aux_hist)
    float32[h, w, 4]; mot, pmot records [h, w] -> (out, aux_out or None)."""
    p = parts(cur, mot, pmot, hist, gamma, radius, n_max, sigma_depth, stat, aux, aux_hist)
    return p["out"], p["aux_out"]
