"""Adaptive sampling's neighbourhood rule (tmpt_adaptive_desc.radius) restated:
adaptive_restate.adaptive_expect's loop with the stay-active rule of
include/tmpt.h -- a pixel active through a pass stays active iff n < S and the
own test holds for some pixel of its neighbourhood, clipped to the frame and to
its band.  The dilation is written by its definition, pixel by pixel.
Shared by test_adaptive_nb.py (CPU) and test_gpu_adaptive_nb.py.
"""
import functools

import numpy as np

from adaptive_restate import f32, scene_samples, schedule

#: the GPU cases: (scene, width, height, cap, spp_min, spp_step, tau, tie_rule index, radius, band_rows)
NB_CASES = [
    ("suzanne.obj", 32, 18, 16, 4, 4, 0.02, False, 1, 0),
    ("suzanne.obj", 100, 28, 12, 4, 4, 0.02, False, 2, 0),  # rows of two 64-bit words, the second of 36 bits
    ("teapot.obj", 24, 14, 12, 2, 3, 0.02, False, 1, 0),
    ("suzanne.obj", 37, 11, 16, 4, 4, 0.02, False, 8, 0),   # a radius beyond most of the height
    ("suzanne.obj", 37, 11, 16, 4, 4, 0.02, False, 8, 3),   # a radius beyond the band
    ("cube.obj", 16, 9, 19, 6, 5, 0.01, True, 1, 0),
    # the shard and band cases
    ("suzanne.obj", 37, 11, 16, 4, 4, 0.02, False, 2, 3),
    ("suzanne.obj", 37, 11, 16, 4, 4, 0.02, False, 2, 0),
    ("suzanne.obj", 37, 11, 16, 4, 4, 0.02, False, 2, 1),
]
NB_IDS = [f"{c[0].split('.')[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}-tau{c[6]}" + ("-index" if c[7] else "")
          + f"-r{c[8]}-band{c[9]}" for c in NB_CASES]


def neighbourhood_any(own, radius, band_rows):
    """out[p] = any(own[q] for q in N_r(p)): |q.x - p.x| <= r, |q.y - p.y| <= r,
    q inside the frame and q.y // band_rows == p.y // band_rows (band_rows 0:
    the whole height is one band)."""
    h, w = own.shape
    band = band_rows if band_rows > 0 else h
    out = np.zeros((h, w), bool)
    for py in range(h):
        for px in range(w):
            hit = False
            for qy in range(py - radius, py + radius + 1):
                if qy < 0 or qy >= h or qy // band != py // band:
                    continue
                for qx in range(px - radius, px + radius + 1):
                    if 0 <= qx < w and own[qy, qx]:
                        hit = True
            out[py, px] = hit
    return out


def adaptive_nb_expect(col, rays, spp_min, spp_step, tau, radius, band_rows, dilate=neighbourhood_any):
    """The contract with a radius over per-sample colours col[h, w, S, 3] and ray
    counts rays[h, w, S] of a whole frame: (spp map int32[h, w], radiance
    float32[h, w, 3], rays, pass_pixels).  dilate: the neighbourhood's any (a
    test may pass a wrong one, to show that it would be noticed)."""
    h, w, cap = rays.shape
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
                y = (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]
                ssum = np.where(active[..., None], ssum + c, ssum)
                m1 = np.where(active, m1 + y, m1)
                m2 = np.where(active, m2 + y * y, m2)
                total += int(rays[:, :, s][active].sum())
            fn = f32(n)
            mean = m1 / fn
            var = np.fmax(f32(0), m2 / fn - mean * mean)
            se2 = var / (fn - f32(1))
            lim = lim4 * np.fmax(mean, f32(1) / f32(256))
            n_p = np.where(active, n, n_p).astype(np.int32)
            own = active & (n < cap) & (se2 > lim)  # false for every pixel not active through the pass
            near = own if radius == 0 else dilate(own, radius, band_rows)
            active = active & (n < cap) & near
            n0 = n
            if not active.any():
                break
    assert ssum.dtype == f32 and m1.dtype == f32 and m2.dtype == f32
    rad = ssum * (f32(1) / n_p.astype(f32))[..., None]
    return n_p, rad.astype(f32), total, pass_pixels


@functools.lru_cache(maxsize=None)
def nb_case_expect(case):
    name, w, h, cap, spp_min, spp_step, tau, index, radius, band_rows = case
    col, rays = scene_samples(name, w, h, cap, index)
    return adaptive_nb_expect(col, rays, spp_min, spp_step, tau, radius, band_rows)


def counts_of(n_p):
    return {int(n): int((n_p == n).sum()) for n in np.unique(n_p)}
