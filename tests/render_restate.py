"""The AOV pass and the float radiance restated from the oracle's pieces, for
any camera and any oracle scene: shared by test_gpu_aov.py, test_gpu_radiance.py
(the reference's camera placement) and test_gpu_cameras.py (Camera.create).
"""
import numpy as np

import oracle
import toymeshpathtracer_amd as tm

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
    nrm, t = hits[:, 3:6].reshape(shape + (3,)), hits[:, 6].reshape(shape)
    rec = np.zeros((h, w), tm.AOV_DTYPE)
    nsum, dsum, lsum = np.zeros((h, w, 3), f32), np.zeros((h, w), f32), np.zeros((h, w), f32)
    for s in range(spp):  # float32 sums in sample order; a miss adds nothing
        nsum = np.where(hit[..., s, None], nsum + nrm[..., s, :], nsum)
        dsum = np.where(hit[..., s], dsum + t[..., s], dsum)
        lsum = np.where(lit[..., s], lsum + lc[..., s], lsum)
    recip = f32(1) / f32(spp)
    rec["normal"], rec["depth"], rec["direct"] = nsum * recip, dsum * recip, lsum * recip
    rec["tri_id"] = np.where(hit[..., 0], ids[..., 0], -1)
    rec["hits"], rec["lit"] = hit.sum(-1), lit.sum(-1)
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


def radiance_expect(osc, cam, w, h, spp, seed_mode):
    """(float32[h, w, 3] colour sum in sample order times 1/spp, rays) from the
    oracle's pieces: the seeds, the two jitter draws, get_ray, Scene.trace."""
    inv_w, inv_h = f32(1) / f32(w), f32(1) / f32(h)
    out = np.zeros((h, w, 3), f32)
    rays = 0
    for y in range(h):
        for x in range(w):
            seed = oracle.pixel_seed(x, y, w)
            state = seed  # pixel seeding: one stream per pixel, threaded through the samples
            col = np.zeros(3, f32)
            for s in range(spp):
                if seed_mode == tm.SEED_SAMPLE:
                    state = oracle.sample_seed(seed, s)
                r = oracle.float01_seq(state, 2)
                state = int(oracle.xorshift_seq(state, 2)[1])
                o, d, state = oracle.get_ray(cam, float((f32(x) + r[0]) * inv_w), float((f32(y) + r[1]) * inv_h), state)
                c, state, n = osc.trace(o, d, state)
                col = col + c  # float32, sample order
                rays += n
            out[y, x] = col * (f32(1) / f32(spp))
    return out, rays


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
