"""History-guided sampling as include/tmpt.h states it (tmpt_sample_plan,
tmpt_render_guided), restated in float32 numpy: one numpy operation per
operation of the contract, in its order, written from the header and not from
the kernels.  tests/test_guided_abi.py proves this file on the CPU before
tests/test_gpu_guided.py holds the GPU to it bit for bit.

``plan()``            tmpt_sample_plan over a whole frame: temporal_clip_restate's
                      fetch (tmpt_temporal's own statements) with the moments
                      frame as the history, then the prior
``plan_scalar()``     the same, pixel by pixel in scalar float32 -- the check of
                      ``plan()`` that shares no array code with it
``guided_expect()``   adaptive_restate.adaptive_expect with a prior argument
``plan_frames()``     synthetic records and a moments history with every case
                      the plan's statement knows
``synthetic_prior()`` the prior the render tests use over a trace fixture
"""
import functools

import numpy as np

from noise_aware_restate import luminance, moments_expect, synthetic_moments
from temporal_clip_restate import fetch
from temporal_restate import HALF, MOTION_DTYPE, N_MAX_DEFAULT, ONE, SIGMA_DEPTH_DEFAULT, ZERO, f32

NULL_PRIOR = np.array([0, 0, 1, 0], f32)
#: the render tests' history lengths, by 4-column blocks: index (x // 4) % 4
NH_BLOCKS = (0, 1, 2, 5)
N_MAX_CASES = (3.0, 8.0)
PLAN_SIZE = (67, 35)  # no multiple of any block shape


def plan(mot, pmot, hist, n_max=0.0, sigma_depth=0.0):
    """tmpt_sample_plan: mot, pmot records [h, w], hist float32[h, w, 4] the
    accumulated moments {mu1, mu2, mean 1/n, length} -> prior float32[h, w, 4]."""
    hist = np.asarray(hist, f32)
    n_max = f32(n_max) if n_max else N_MAX_DEFAULT
    sigma = f32(sigma_depth) if sigma_depth else SIGMA_DEPTH_DEFAULT
    go, _, nsum, wsum, asum = fetch(mot, pmot, hist, sigma, hist)
    with np.errstate(all="ignore"):
        hy, h2, hz = asum[..., 0] / wsum, asum[..., 1] / wsum, asum[..., 2] / wsum
        nh = nsum / wsum
        ne = nh / hz
        vh = np.fmax(ZERO, h2 - hy * hy) / np.fmax(ne - ONE, ONE)
        n = np.fmin(nh + ONE, n_max)
        a = ONE / n
        b = ONE - a
        res = np.stack([hy, (b * b) * vh, a, nh], -1)
    assert res.dtype == f32
    return np.where(go[..., None], res, NULL_PRIOR).astype(f32)


def plan_scalar(mot, pmot, hist, n_max=0.0, sigma_depth=0.0):
    """plan() one pixel and one tap at a time, in numpy float32 scalars."""
    hist = np.asarray(hist, f32)
    h, w = hist.shape[:2]
    n_max = f32(n_max) if n_max else N_MAX_DEFAULT
    sigma = f32(sigma_depth) if sigma_depth else SIGMA_DEPTH_DEFAULT
    out = np.empty((h, w, 4), f32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                m = mot[y, x]
                out[y, x] = NULL_PRIOR
                px, py, dprev = f32(m["px"]), f32(m["py"]), f32(m["depth_prev"])
                if not (int(m["flags"]) & 2) or not (px >= f32(-1) and px < f32(w) + ONE and py >= f32(-1)
                                                      and py < f32(h) + ONE):
                    continue
                fx, fy = px - HALF, py - HALF
                x0, y0 = np.floor(fx), np.floor(fy)
                ax, ay = fx - x0, fy - y0
                asum = [ZERO, ZERO, ZERO]
                nsum = wsum = ZERO
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = int(x0) + i, int(y0) + j
                        wgt = (ax if i else ONE - ax) * (ay if j else ONE - ay)
                        if qx < 0 or qx >= w or qy < 0 or qy >= h:
                            continue
                        pm = pmot[qy, qx]
                        if not (int(pm["flags"]) & 1):
                            continue
                        if np.abs(f32(pm["depth"]) - dprev) > sigma * dprev:
                            continue
                        hq = hist[qy, qx]
                        asum = [asum[k] + hq[k] * wgt for k in range(3)]
                        nsum = nsum + hq[3] * wgt
                        wsum = wsum + wgt
                if not wsum > ZERO:
                    continue
                hy, h2, hz, nh = asum[0] / wsum, asum[1] / wsum, asum[2] / wsum, nsum / wsum
                ne = nh / hz
                vh = np.fmax(ZERO, h2 - hy * hy) / np.fmax(ne - ONE, ONE)
                n = np.fmin(nh + ONE, n_max)
                a = ONE / n
                b = ONE - a
                out[y, x] = (hy, (b * b) * vh, a, nh)
    return out


def guided_expect(col, rays, spp_min, spp_step, tau, prior=None):
    """adaptive_expect (radius 0) with tmpt_render_guided's test: prior
    float32[h, w, 4] over the frame, or None = the null prior everywhere ->
    (spp map int32[h, w], radiance float32[h, w, 3], rays, pass_pixels)."""
    from adaptive_restate import schedule  # (needs the oracle: not at import, the checked build's child has none)

    h, w, cap = rays.shape
    pr = np.broadcast_to(NULL_PRIOR, (h, w, 4)) if prior is None else np.asarray(prior, f32)
    assert pr.shape == (h, w, 4) and pr.dtype == f32
    tau = f32(tau)
    lim4 = f32(4) * (tau * tau)
    ssum = np.zeros((h, w, 3), f32)
    m1, m2 = np.zeros((h, w), f32), np.zeros((h, w), f32)
    active = np.ones((h, w), bool)
    n_p = np.zeros((h, w), np.int32)
    total, pass_pixels, n0 = 0, [], 0
    with np.errstate(all="ignore"):
        for n in schedule(cap, spp_min, spp_step):
            pass_pixels.append(int(active.sum()))
            for s in range(n0, n):  # float32, sample order, the active pixels only
                c = col[:, :, s]
                y = luminance(c)
                ssum = np.where(active[..., None], ssum + c, ssum)
                m1 = np.where(active, m1 + y, m1)
                m2 = np.where(active, m2 + y * y, m2)
                total += int(rays[:, :, s][active].sum())
            fn = f32(n)
            mean = m1 / fn
            var = np.fmax(f32(0), m2 / fn - mean * mean)
            se2 = var / (fn - f32(1))
            se2b = pr[..., 1] + (pr[..., 2] * pr[..., 2]) * se2
            meanb = pr[..., 0] + (mean - pr[..., 0]) * pr[..., 2]
            lim = lim4 * np.fmax(meanb, f32(1) / f32(256))
            n_p = np.where(active, n, n_p).astype(np.int32)
            active = active & (n < cap) & (se2b > lim)  # a NaN compares false
            n0 = n
            if not active.any():
                break
    assert ssum.dtype == f32 and se2b.dtype == f32 and meanb.dtype == f32
    rad = ssum * (f32(1) / n_p.astype(f32))[..., None]
    return n_p, rad.astype(f32), total, pass_pixels


def synthetic_prior(col, n_max):
    """The render tests' prior over per-sample colours col[h, w, 8, 3]: history
    moments = the means of Y and Y * Y over samples 4 .. 7, history length NH_BLOCKS
    by 4-column blocks, ne = 4 * max(nh, 1); the null prior where nh = 0.  The
    statements after the fetch are the header's."""
    h, w = col.shape[:2]
    mom = moments_expect(np.asarray(col, f32)[:, :, 4:8], 4)
    hy, h2 = mom[..., 0], mom[..., 1]
    nh = np.broadcast_to(np.array(NH_BLOCKS, f32)[(np.arange(w) // 4) % 4], (h, w))
    ne = f32(4) * np.fmax(nh, ONE)
    vh = np.fmax(ZERO, h2 - hy * hy) / np.fmax(ne - ONE, ONE)
    n = np.fmin(nh + ONE, f32(n_max))
    a = ONE / n
    b = ONE - a
    res = np.stack([hy, (b * b) * vh, a, nh], -1)
    out = np.where((nh == 0)[..., None], NULL_PRIOR, res).astype(f32)
    out.setflags(write=False)
    return out


def build_digests(tm, obj):
    """One synthetic and one rendered case of each new call through the library
    `tm` has loaded, as digests: run by the checked build in a child process and by
    the plain build in the test itself (test_gpu_guided.py), which compares the two."""
    import hashlib

    import bvh_refit_restate as F

    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {}
    try:
        w, h = 64, 36
        rest, bmin, bmax = tm.load_scene(obj)
        cam = tm.Camera.for_scene(bmin, bmax, w, h)
        mot, pmot, hist, _ = plan_frames()
        with tm.Scene(rest) as sc:
            out["synthetic"] = sha(sc.sample_plan(mot, pmot, hist, 8.0, 0.02))
            mom0 = sc.trace_moments(cam, w, h, 4)[1]
            mot0, _ = sc.trace_motion(cam, cam, w, h)
            sc.update(F.twist(rest, 10.0), "refit")
            sc.set_option("sample_base", 8)
            mot1, _ = sc.trace_motion(cam, cam, w, h, rest)
            prior = sc.sample_plan(mot1, mot0, mom0)
            out["plan"] = sha(prior)
            for radius in (0, 1):
                res = sc.trace_guided(cam, w, h, 8, prior, 2, 2, 0.05, radius=radius)
                out[f"guided{radius}"] = [sha(a) for a in res[:4]] + [res[4], res[5]["pass_pixels"]]
            res = sc.trace_guided(cam, w, h, 8, prior, 2, 2, 0.05, band_rows=4, shard=1, num_shards=3)
            out["shard"] = [sha(a) for a in res[:4]] + [res[4], res[5]["pass_pixels"]]
    except tm.TmptError as e:
        out["error"] = str(e)
    return out


@functools.lru_cache(maxsize=None)
def plan_frames(w=PLAN_SIZE[0], h=PLAN_SIZE[1], seed=1):
    """(mot, pmot, hist, cases): records and an accumulated-moments history, and
    cases = {name: (y, x)} naming one pixel of each case of the plan's statement:
    an m.px that is NaN and one out of range, taps outside the frame, one tap
    rejected by depth, all four taps rejected (wsum = 0), hz = 0, a history at
    n_max = 3 already.  Everything else is random reprojections of about a pixel
    and a half, depths around the 5 % tolerance, flags 0, 1 and 3."""
    rng = np.random.default_rng(4242 + seed * 97 + w * 131 + h)
    hist = synthetic_moments(w, h, seed).copy()  # lengths 1 .. 5, 1/n of 2, 3, 8, mu2 < mu1^2, one 1/n = 0
    y, x = np.mgrid[0:h, 0:w]
    mot, pmot = np.zeros((h, w), MOTION_DTYPE), np.zeros((h, w), MOTION_DTYPE)
    mot["px"] = (x + 0.5 + rng.normal(0, 1.5, (h, w))).astype(f32)
    mot["py"] = (y + 0.5 + rng.normal(0, 1.5, (h, w))).astype(f32)
    depth = (3 + rng.random((h, w))).astype(f32)
    pmot["depth"] = depth
    mot["depth"] = depth
    mot["depth_prev"] = (depth * (1 + rng.normal(0, 0.03, (h, w)))).astype(f32)
    mot["flags"] = rng.choice([0, 1, 3, 3, 3, 3], (h, w)).astype(np.uint32)
    pmot["flags"] = rng.choice([0, 1, 3, 3, 3, 3], (h, w)).astype(np.uint32)
    mot["tri_id"] = rng.integers(-1, 50, (h, w))
    cases = {}

    def aim(name, p, px, py, dprev=None):
        """Pixel p reprojects to (px, py); the taps' records there are covered and at p's depth."""
        mot["px"][p], mot["py"][p], mot["flags"][p] = px, py, 3
        if dprev is not None:
            mot["depth_prev"][p] = dprev
        cases[name] = p

    def taps(px, py):
        x0, y0 = int(np.floor(px - 0.5)), int(np.floor(py - 0.5))
        return [(y0 + j, x0 + i) for j in (0, 1) for i in (0, 1) if 0 <= x0 + i < w and 0 <= y0 + j < h]

    def accept(px, py, d):
        for q in taps(px, py):
            pmot["flags"][q], pmot["depth"][q] = 3, d
    # the targets lie in rows 20 .. 30, away from one another; the sources in rows 2 .. 8
    aim("px_nan", (2, 3), np.nan, 10.5)
    aim("px_out_of_range", (2, 9), w + 1.0, 10.5)
    aim("taps_outside", (2, 15), -0.75, -0.25, 4.0)  # x0 = y0 = -2 .. -1: one tap (0, 0) at most, weight small
    accept(0.6, 0.6, 4.0)
    aim("taps_outside_edge", (2, 21), w + 0.25, 20.3, 4.0)  # the right-hand taps fall off the frame
    accept(w - 0.5, 20.3, 4.0)
    aim("tap_depth_rejected", (4, 3), 30.3, 24.6, 4.0)
    accept(30.3, 24.6, 4.0)
    pmot["depth"][taps(30.3, 24.6)[1]] = 8.0
    aim("all_taps_rejected", (4, 9), 40.3, 24.6, 4.0)
    accept(40.3, 24.6, 9.0)
    aim("hz_zero", (4, 15), 50.5, 26.5, 4.0)  # exactly on pixel (26, 50)'s centre: the other three weights are 0
    accept(50.5, 26.5, 4.0)
    for q in taps(50.5, 26.5):
        hist[q][2] = 0
    aim("length_at_n_max", (4, 21), 20.3, 28.6, 4.0)
    accept(20.3, 28.6, 4.0)
    for q in taps(20.3, 28.6):
        hist[q][3] = 2  # nh + 1 = 3 = the default n_max
    aim("length_beyond_n_max", (6, 3), 10.3, 28.6, 4.0)
    accept(10.3, 28.6, 4.0)
    for q in taps(10.3, 28.6):
        hist[q][3] = 5
    for a in (mot, pmot, hist):
        a.setflags(write=False)
    return mot, pmot, hist, cases
