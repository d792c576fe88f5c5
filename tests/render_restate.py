"""The AOV pass and the float radiance restated from the oracle's pieces, for
any camera and any oracle scene: shared by test_gpu_aov.py, test_gpu_radiance.py
(the reference's camera placement) and test_gpu_cameras.py (Camera.create).
"""
import numpy as np

import oracle
import toymeshpathtracer_amd as tm
from ref_cases import seed_chains

f32 = np.float32


def dot(a, b):  # glm: (x*x' + y*y') + z*z', one rounding per operation
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):  # v * (1 / sqrt(dot(v, v)))
    return v * (f32(1) / np.sqrt(dot(v, v)))


LIGHT = normalize(np.array([-0.7, 1.0, 0.5], f32))


def light_cosine(n, d):
    nl = np.where((dot(n, d) < 0)[:, None], n, -n)
    c = dot(np.broadcast_to(LIGHT, nl.shape), nl)
    return np.where(c > 0, c, f32(0)).astype(f32)


def aov_sums(hit, nrm, t, spp=None):
    """(normal[h, w, 3], depth[h, w], hits[h, w]) of include/tmpt.h's AOV record
    from the samples' first hits -- hit bool[h, w, S], nrm float32[h, w, S, 3],
    t float32[h, w, S], whatever made them (the oracle in aov_expect, the
    reference's recorded answers in test_gpu_reference_trace.py) -- over the
    first spp samples: float32 sums from 0 in sample order, a miss adding
    nothing, each times 1 / spp."""
    spp = hit.shape[2] if spp is None else spp
    h, w = hit.shape[:2]
    nsum, dsum = np.zeros((h, w, 3), f32), np.zeros((h, w), f32)
    for s in range(spp):
        nsum = np.where(hit[..., s, None], nsum + nrm[..., s, :], nsum)
        dsum = np.where(hit[..., s], dsum + t[..., s], dsum)
    recip = f32(1) / f32(spp)
    assert nsum.dtype == f32 and dsum.dtype == f32
    return nsum * recip, dsum * recip, hit[..., :spp].sum(-1)


def aov_expect(osc, cam, w, h, spp):
    """(records[h, w], per-sample counts) of the whole frame from the oracle
    scene osc through the camera array cam."""
    inv_w, inv_h = f32(1) / f32(w), f32(1) / f32(h)
    rays = np.zeros((h, w, spp, 6), f32)
    for y in range(h):
        for x in range(w):
            seed = oracle.pixel_seed(x, y, w)
            for s in range(spp):
                st = oracle.sample_seed(seed, s)
                r = oracle.float01_seq(st, 2)
                state = int(oracle.xorshift_seq(st, 2)[1])
                o, d, _ = oracle.get_ray(cam, float((f32(x) + r[0]) * inv_w), float((f32(y) + r[1]) * inv_h), state)
                rays[y, x, s, :3], rays[y, x, s, 3:] = o, d
    flat = rays.reshape(-1, 6)
    ids, hits = osc.hit_batch(flat, 0.001, 1.0e7)
    hit = ids >= 0
    lc = light_cosine(hits[:, 3:6], flat[:, 3:6])
    want_shadow = hit & (lc > 0)
    sids, _ = osc.hit_batch(np.concatenate([hits[:, 0:3], np.broadcast_to(LIGHT, (len(flat), 3))], 1), 0.001, 1.0e7)
    lit = want_shadow & (sids < 0)
    shape = (h, w, spp)
    hit, lit, lc, ids = hit.reshape(shape), lit.reshape(shape), lc.reshape(shape), ids.reshape(shape)
    rec = np.zeros((h, w), tm.AOV_DTYPE)
    rec["normal"], rec["depth"], rec["hits"] = aov_sums(hit, hits[:, 3:6].reshape(shape + (3,)),
                                                        hits[:, 6].reshape(shape))
    lsum = np.zeros((h, w), f32)
    for s in range(spp):  # as aov_sums sums
        lsum = np.where(lit[..., s], lsum + lc[..., s], lsum)
    rec["direct"] = lsum * (f32(1) / f32(spp))
    rec["tri_id"] = np.where(hit[..., 0], ids[..., 0], -1)
    rec["lit"] = lit.sum(-1)
    per_pixel = hit.sum(-1)
    counts = dict(hits=int(hit.sum()), misses=int((~hit).sum()),
                  shadowed=int((want_shadow.reshape(shape) & ~lit).sum()),
                  partial=int(((per_pixel > 0) & (per_pixel < spp)).sum()))
    return rec, counts


def same_records(got, want):
    """Every field of every record, floats as bits."""
    for f in tm.AOV_DTYPE.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        bad = np.argwhere((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape))
        assert len(bad) == 0, f"{f}: {len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]} vs {b[tuple(bad[0])]}"
    assert got.tobytes() == want.tobytes()


def chain_samples(osc, cam, w, h, chains):
    """The oracle's pieces sample by sample over chains (k, 4) {x, y, state,
    count} (ref_cases.seed_chains): the two jitter draws, get_ray, Scene.trace,
    the state threaded through a chain's samples.  -> dict of ray (n, 6) float32,
    state_ray (n,) uint32 (after get_ray), col (n, 3) float32, state (n,) uint32
    (after trace), rays (n,) int64."""
    inv_w, inv_h = f32(1) / f32(w), f32(1) / f32(h)
    n = int(np.asarray(chains)[:, 3].sum())
    out = dict(ray=np.zeros((n, 6), f32), state_ray=np.zeros(n, np.uint32), col=np.zeros((n, 3), f32),
               state=np.zeros(n, np.uint32), rays=np.zeros(n, np.int64))
    i = 0
    for x, y, state, count in (tuple(int(v) for v in c) for c in chains):
        for _ in range(count):
            r = oracle.float01_seq(state, 2)
            state = int(oracle.xorshift_seq(state, 2)[1])
            o, d, state = oracle.get_ray(cam, float((f32(x) + r[0]) * inv_w), float((f32(y) + r[1]) * inv_h), state)
            out["ray"][i, :3], out["ray"][i, 3:], out["state_ray"][i] = o, d, state
            out["col"][i], state, out["rays"][i] = osc.trace(o, d, state)
            out["state"][i] = state
            i += 1
    return out


def oracle_samples(osc, cam, w, h, spp, seed_mode):
    """(colour float32[h, w, spp, 3], rays int64[h, w, spp]) of every sample of a
    pixel- or sample-seeded frame from the oracle's pieces; nothing summed."""
    s = chain_samples(osc, cam, w, h, seed_chains(w, h, spp, seed_mode == tm.SEED_SAMPLE))
    return s["col"].reshape(h, w, spp, 3), s["rays"].reshape(h, w, spp)


def radiance_sum(col, rays, spp=None):
    """(float32[h, w, 3] colour sum in sample order times 1/spp, rays) over the
    first spp of the samples col[h, w, S, 3], rays[h, w, S], whatever made them
    (oracle_samples, or the reference's recorded answers)."""
    spp = col.shape[2] if spp is None else spp
    acc = np.zeros(col.shape[:2] + (3,), f32)
    for s in range(spp):
        acc = acc + col[:, :, s]  # float32, sample order
    assert acc.dtype == f32
    return acc * (f32(1) / f32(spp)), int(rays[:, :, :spp].sum())


def radiance_expect(osc, cam, w, h, spp, seed_mode):
    """(float32[h, w, 3] colour sum in sample order times 1/spp, rays) from the
    oracle's pieces: the seeds, the two jitter draws, get_ray, Scene.trace."""
    return radiance_sum(*oracle_samples(osc, cam, w, h, spp, seed_mode))


def same_bits(got, want, what=""):
    a, b = np.ascontiguousarray(got, f32).view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{what}: {len(bad)} floats differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def pack(rad):
    """pack_pixel(col, 1.0f) of a float tile (main.cpp:224-233) in numpy float32."""
    out = np.full(rad.shape[:-1] + (4,), 255, np.uint8)
    v = np.minimum(np.maximum(np.sqrt(rad[..., :3]), f32(0)), f32(1)) * f32(255)
    out[..., :3] = v.astype(np.uint8)
    return out
