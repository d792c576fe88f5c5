"""tests/temporal_clip_restate.py proved on the CPU, before the GPU is held to
it: against a plain per-pixel float64 loop written from include/tmpt.h, the two
identities the header states, the aux frame, and what clipping is for -- a step
change in the shading that the depth test cannot see.

Tolerance of the float64 comparison: the frames hold values in [0.5, 4.5] and
history lengths up to 40; the longest float32 chain is the 49-term window sum
(relative error a few eps, eps = 2^-24) followed by var = s2/cnt - mu*mu, which
cancels: on uniform random values var is about a fifth of mu*mu, so the error
grows about fivefold before the square root halves it.  32 ulp at the largest
magnitude in play (4.5 for colours, the history length for .w) covers that with
room and is far below any mistake in the statements (a wrong tap, order or
weight moves a value by its own size).  Decisions (skipped taps, the frame's
edge) are kept away from their thresholds by the generator, so float64 takes
the same branches."""
import numpy as np
import pytest

import temporal_clip_restate as K
import temporal_restate as T

f32 = np.float32
ULP = float(2.0 ** -23)


def frames(w, h, seed, cover=0.8):
    """Random frames whose reprojections stay half a pixel inside or well outside
    the frame, depths that match to 1e-3 or miss by 30 %, mixed coverage."""
    rng = np.random.default_rng(seed)
    cur = (0.5 + 4 * rng.random((h, w, 4))).astype(f32)
    hist = (0.5 + 4 * rng.random((h, w, 4))).astype(f32)
    hist[..., 3] = rng.integers(1, 41, (h, w)).astype(f32)
    stat = (0.5 + 4 * rng.random((h, w, 4))).astype(f32)
    aux = (0.5 + 4 * rng.random((h, w, 4))).astype(f32)
    aux_hist = (0.5 + 4 * rng.random((h, w, 4))).astype(f32)
    y, x = np.mgrid[0:h, 0:w]
    mot, pmot = np.zeros((h, w), T.MOTION_DTYPE), np.zeros((h, w), T.MOTION_DTYPE)
    mot["px"] = (x + 0.5 + rng.uniform(-1.4, 1.4, (h, w))).astype(f32)
    mot["py"] = (y + 0.5 + rng.uniform(-1.4, 1.4, (h, w))).astype(f32)
    far = rng.random((h, w)) < 0.1
    mot["px"][far] = -50.0
    depth = (3 + rng.random((h, w))).astype(f32)
    pmot["depth"] = depth
    mot["depth"] = depth
    miss = rng.random((h, w)) < 0.2
    mot["depth_prev"] = (depth * np.where(miss, 1.3, 1 + rng.uniform(-1e-3, 1e-3, (h, w)))).astype(f32)
    mot["flags"] = np.where(rng.random((h, w)) < cover, 3, 0).astype(np.uint32)
    pmot["flags"] = np.where(rng.random((h, w)) < cover, 3, 0).astype(np.uint32)
    return dict(cur=cur, mot=mot, pmot=pmot, hist=hist, stat=stat, aux=aux, aux_hist=aux_hist)


def loop64(fr, gamma, r, n_max, sigma, use_stat):
    """The header, pixel by pixel, in Python floats."""
    cur, mot, pmot, hist = fr["cur"], fr["mot"], fr["pmot"], fr["hist"]
    S = fr["stat"] if use_stat else cur
    h, w = cur.shape[:2]
    out, aux_out = np.zeros((h, w, 4)), np.zeros((h, w, 4))
    for y in range(h):
        for x in range(w):
            m = mot[y, x]
            c = [float(v) for v in cur[y, x, :3]]
            ac = [float(v) for v in fr["aux"][y, x, :3]]
            out[y, x], aux_out[y, x] = c + [1.0], ac + [1.0]
            px, py = float(m["px"]), float(m["py"])
            if not (m["flags"] & 2) or not (-1 <= px < w + 1 and -1 <= py < h + 1):
                continue
            fx, fy = px - 0.5, py - 0.5
            x0, y0 = int(np.floor(fx)), int(np.floor(fy))
            ax, ay = fx - x0, fy - y0
            csum, asum, nsum, wsum = [0.0] * 3, [0.0] * 3, 0.0, 0.0
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    wgt = (ax if i else 1 - ax) * (ay if j else 1 - ay)
                    if not (0 <= qx < w and 0 <= qy < h) or not (pmot[qy, qx]["flags"] & 1):
                        continue
                    if abs(float(pmot[qy, qx]["depth"]) - float(m["depth_prev"])) > sigma * float(m["depth_prev"]):
                        continue
                    for k in range(3):
                        csum[k] += float(hist[qy, qx, k]) * wgt
                        asum[k] += float(fr["aux_hist"][qy, qx, k]) * wgt
                    nsum += float(hist[qy, qx, 3]) * wgt
                    wsum += wgt
            if not wsum > 0:
                continue
            s1, s2, cnt = [0.0] * 3, [0.0] * 3, 0.0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    qx, qy = x + i, y + j
                    if not (0 <= qx < w and 0 <= qy < h) or (mot[qy, qx]["flags"] & 1) != (m["flags"] & 1):
                        continue
                    for k in range(3):
                        s1[k] += float(S[qy, qx, k])
                        s2[k] += float(S[qy, qx, k]) ** 2
                    cnt += 1
            hh = [csum[k] / wsum for k in range(3)]
            mu = [s1[k] / cnt for k in range(3)]
            g = [gamma * max(0.0, s2[k] / cnt - mu[k] * mu[k]) ** 0.5 for k in range(3)]
            hc = [min(max(hh[k], mu[k] - g[k]), mu[k] + g[k]) for k in range(3)]
            e, span = max(abs(hh[k] - hc[k]) for k in range(3)), max(g)
            nh = nsum / wsum
            if e > 0:
                nh = nh * (span / (span + e))
            n = min(nh + 1, n_max)
            a = 1 / n
            out[y, x] = [hc[k] + (c[k] - hc[k]) * a for k in range(3)] + [n]
            aux_out[y, x] = [asum[k] / wsum + (ac[k] - asum[k] / wsum) * a for k in range(3)] + [n]
    return out, aux_out


@pytest.mark.parametrize("r,gamma,n_max,use_stat", [(1, 1.0, 8.0, False), (2, 0.5, 64.0, True), (3, 2.0, 3.0, False),
                                                    (3, 0.75, 32.0, True)])
def test_restatement_agrees_with_a_float64_loop(r, gamma, n_max, use_stat):
    fr = frames(13, 9, 10 * r + int(use_stat))
    got, got_aux = K.clip(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], gamma, r, n_max, 0.05,
                          fr["stat"] if use_stat else None, fr["aux"], fr["aux_hist"])
    want, want_aux = loop64(fr, gamma, r, n_max, 0.05, use_stat)
    assert got.dtype == f32 and got_aux.dtype == f32
    moved = (got[..., 3] > 1).mean()
    assert 0.3 < moved < 1.0  # both branches are there
    for a, b in ((got, want), (got_aux, want_aux)):
        assert np.abs(a[..., :3] - b[..., :3]).max() <= 32 * ULP * 4.5
        assert (np.abs(a[..., 3] - b[..., 3]) <= 32 * ULP * np.maximum(1.0, b[..., 3])).all()
        assert np.array_equal(a[..., 3] == 1, b[..., 3] == 1)


def test_defaults_are_the_descriptor_zeros():
    fr = frames(11, 7, 3)
    a = K.clip(fr["cur"], fr["mot"], fr["pmot"], fr["hist"])[0]
    b = K.clip(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], float(K.GAMMA_DEFAULT), K.RADIUS_DEFAULT,
               float(K.N_MAX_DEFAULT), float(T.SIGMA_DEPTH_DEFAULT))[0]
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("r", [1, 2, 3])
def test_a_huge_gamma_is_the_plain_blend(r):
    """gamma = 3e38 on frames with sd > 0 in every window: hc = h, e = 0, and the
    output is temporal_restate.blend's bit for bit."""
    for seed, cover in ((1, 1.0), (2, 0.8)):
        fr = frames(17, 11, seed, cover)
        # every window must hold two values at least, an uncovered pixel's too (its equals are
        # the uncovered ones): coverage by whole rows gives every pixel a neighbour of its class
        fr["mot"]["flags"][:] = fr["mot"]["flags"][:, :1]
        for n_max in (3.0, 32.0):
            p = K.parts(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], 3e38, r, n_max, 0.05)
            assert (p["sd"] > 0).all() and (p["cnt"] >= 2).all()
            assert (p["e"][p["go"]] == 0).all() and p["go"].any()
            want = T.blend(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], n_max, 0.05)
            assert p["out"].tobytes() == want.tobytes()


def test_a_centre_only_window_snaps_to_the_frame():
    """1 x 1, and covered pixels with no covered neighbour within the radius:
    mu = S_p, sd = 0, hc = S_p whatever gamma is; a history that differed restarts."""
    for gamma in (0.5, 1.0, 3e38):
        cur = np.array([[[1.5, 2.5, 0.25, 1.0]]], f32)
        hist = np.array([[[0.5, 3.0, 0.25, 9.0]]], f32)
        mot = np.zeros((1, 1), T.MOTION_DTYPE)
        mot["px"], mot["py"], mot["depth"], mot["depth_prev"], mot["flags"] = 0.5, 0.5, 2.0, 2.0, 3
        p = K.parts(cur, mot, mot, hist, gamma, 3, 32.0)
        assert p["go"].all() and np.array_equal(p["hc"][0, 0], cur[0, 0, :3]) and p["sd"].max() == 0
        assert p["out"][0, 0, 3] == 1 and np.array_equal(p["out"][0, 0, :3], cur[0, 0, :3])
        fr = frames(15, 15, 5, 1.0)
        fr["mot"]["flags"][:] = 0  # uncovered but for a lattice of lone pixels, 4 apart: beyond radius 3
        fr["mot"]["flags"][3::4, 3::4] = 3
        fr["pmot"]["flags"][:] = 3
        for r in (1, 2, 3):
            for stat in (None, fr["stat"]):
                p = K.parts(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], gamma, r, 32.0, 0.05, stat)
                lone = (fr["mot"]["flags"] == 3) & p["go"]
                assert lone.sum() >= 4 and (p["cnt"][fr["mot"]["flags"] == 3] == 1).all()
                s = fr["cur"] if stat is None else stat
                assert np.array_equal(p["hc"][lone], s[..., :3][lone])


def test_the_aux_frame_shares_the_blend_factor_and_the_length():
    fr = frames(19, 12, 7)
    p = K.parts(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], 1.0, 2, 16.0, 0.05, None, fr["aux"], fr["aux_hist"])
    out, aux_out, go = p["out"], p["aux_out"], p["go"]
    assert np.array_equal(out[..., 3], aux_out[..., 3])
    assert np.array_equal(aux_out[~go][:, :3], fr["aux"][~go][:, :3]) and (aux_out[~go][:, 3] == 1).all()
    # the aux history is not clipped: it is the plain fetch of aux_hist blended with the colour frame's a
    _, asum, _, wsum, _ = K.fetch(fr["mot"], fr["pmot"], fr["aux_hist"], T.SIGMA_DEPTH_DEFAULT)
    with np.errstate(all="ignore"):
        ha = asum / wsum[..., None]
        want = ha + (fr["aux"][..., :3] - ha) * p["a"][..., None]
    assert np.array_equal(aux_out[go][:, :3], want[go])
    clipped = go & (p["e"] > 0)
    assert clipped.any() and (p["n"][clipped] < np.minimum(p["nh"][clipped] + 1, 16)).any()
    # without aux the colour frame is the same
    assert K.clip(fr["cur"], fr["mot"], fr["pmot"], fr["hist"], 1.0, 2, 16.0)[0].tobytes() == out.tobytes()


def test_a_step_change_is_followed():
    """The history holds A with length 32; the frame shows B plus small noise,
    nothing moved and every depth agrees: the plain blend keeps 31/32 of A, the
    clipped one is strictly closer to B.  With A = B both outputs lie between
    values that are within the noise of B, so they differ by at most the noise's
    peak-to-peak range."""
    w, h, amp = 24, 16, 0.01
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:h, 0:w]
    mot = np.zeros((h, w), T.MOTION_DTYPE)
    mot["px"], mot["py"], mot["depth"], mot["depth_prev"], mot["flags"] = x + 0.5, y + 0.5, 2.0, 2.0, 3
    B = np.array([0.8, 0.5, 0.3], f32)
    cur = np.ones((h, w, 4), f32)
    cur[..., :3] = B + rng.uniform(-amp, amp, (h, w, 3)).astype(f32)
    rmse = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - B) ** 2).mean()))
    for A in (np.array([0.2, 0.9, 0.6], f32), B):
        hist = np.full((h, w, 4), 32.0, f32)
        hist[..., :3] = A
        plain = T.blend(cur, mot, mot, hist, 32.0)
        for r in (1, 2, 3):
            for gamma in (0.5, 1.0, 3.0):
                got = K.clip(cur, mot, mot, hist, gamma, r, 32.0)[0]
                if A is B:
                    assert np.abs(got[..., :3] - plain[..., :3]).max() <= 2 * amp
                else:
                    assert rmse(got) < rmse(plain)
                    assert rmse(got) < 0.1 * rmse(plain)  # not by a hair: the box is a few noise widths from B
                    assert (got[..., 3] < 3).all() and (plain[..., 3] == 32).all()
