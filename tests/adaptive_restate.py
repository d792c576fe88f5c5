"""Adaptive sampling (tmpt_render_adaptive) restated from the oracle's pieces:
the loop of render_restate.radiance_expect, keeping each sample's colour and
ray count, then the pass schedule and the variance test of include/tmpt.h in
numpy float32 -- one rounding per operation, in the order the header writes.
Shared by test_adaptive_abi.py (CPU) and test_gpu_adaptive.py.
"""
import functools

import numpy as np

import oracle
import toymeshpathtracer_amd as tm
from conftest import data
from render_restate import oracle_samples

f32 = np.float32

#: the GPU cases: (scene, width, height, cap, spp_min, spp_step, tau, tie_rule index)
CASES = [
    ("suzanne.obj", 32, 18, 16, 4, 4, 0.01, False),
    ("suzanne.obj", 32, 18, 16, 4, 4, 0.02, False),
    ("cube.obj", 16, 9, 19, 6, 5, 0.01, False),
    ("teapot.obj", 24, 14, 12, 2, 3, 0.02, False),
    ("cube.obj", 16, 9, 19, 6, 5, 0.01, True),
]
CASE_IDS = [f"{c[0].split('.')[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}-{c[5]}-tau{c[6]}" + ("-index" if c[7] else "")
            for c in CASES]


@functools.lru_cache(maxsize=None)
def load(name):
    return tm.load_scene(data(name))


def oracle_scene(name, index=False):
    tris, bmin, bmax = load(name)
    if index:
        return oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX, bmin=bmin, bmax=bmax)
    return oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)


def camera(name, w, h):
    _, bmin, bmax = load(name)
    return tm.Camera.for_scene(bmin, bmax, w, h)


def sample_colours(osc, cam, w, h, spp):
    """(colour float32[h, w, spp, 3], rays int64[h, w, spp]) of every sample of a
    sample-seeded frame: radiance_expect's samples, nothing summed."""
    return oracle_samples(osc, cam, w, h, spp, tm.SEED_SAMPLE)


@functools.lru_cache(maxsize=None)
def scene_samples(name, w, h, spp, index=False):
    """sample_colours of the reference's camera placement for a scene file (computed once, never written to)."""
    col, rays = sample_colours(oracle_scene(name, index), camera(name, w, h).as_array(), w, h, spp)
    col.setflags(write=False)
    rays.setflags(write=False)
    return col, rays


def schedule(cap, spp_min, spp_step):
    """The pass ends n_0, n_1, ...: n_0 = spp_min, n_(k+1) = min(n_k + spp_step, cap)."""
    ends = [spp_min]
    while ends[-1] < cap:
        ends.append(min(ends[-1] + spp_step, cap))
    return ends


def adaptive_expect(col, rays, spp_min, spp_step, tau):
    """The contract over per-sample colours col[h, w, S, 3] and ray counts
    rays[h, w, S]: (spp map int32[h, w], radiance float32[h, w, 3], rays,
    pass_pixels)."""
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
            var = np.fmax(f32(0), m2 / fn - mean * mean)  # fmaxf: the other operand for a NaN
            se2 = var / (fn - f32(1))
            lim = lim4 * np.fmax(mean, f32(1) / f32(256))
            n_p = np.where(active, n, n_p).astype(np.int32)
            active = active & (n < cap) & (se2 > lim)  # a NaN compares false
            n0 = n
            if not active.any():
                break
    assert ssum.dtype == f32 and m1.dtype == f32 and m2.dtype == f32
    rad = ssum * (f32(1) / n_p.astype(f32))[..., None]
    return n_p, rad.astype(f32), total, pass_pixels


@functools.lru_cache(maxsize=None)
def case_expect(case):
    name, w, h, cap, spp_min, spp_step, tau, index = case
    col, rays = scene_samples(name, w, h, cap, index)
    return adaptive_expect(col, rays, spp_min, spp_step, tau)
