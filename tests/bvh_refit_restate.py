"""The BVH refit (tmpt_scene_update, mode refit) restated on the host.

Pure numpy over a dump of the form Scene.dump_bvh() gives: neither the GPU
library nor the oracle is imported.  ``refit(dump, new_tris)`` returns the dump
the refit's contract (include/tmpt.h, tmpt_scene_update) gives for the dump's
links and the new triangles:

records   record k keeps its triangle index i = [9] >> 1 and takes v0, e1 = v1 - v0,
          e2 = v2 - v0 of new triangle i (f32, one rounding each); [9] = 2 * i, the
          flat mark cleared; record n stays all zero
unions    for every valid child slot the union U of the padded boxes
          (bvh_check.tri_boxes) beneath it, bottom-up: a leaf's U is the f32 min / max
          over the records of its range, an internal child's the min / max of its
          own slots' U.  min / max are exact, so no order of reduction matters
nodes     bvh_check.encode_nodes over those U and the old links, word for word the
          rule the build encodes by
info      unchanged

The numbering is the dump's own (raw, not canonical): a refit renumbers nothing.
``mut`` names one of MUTATIONS, wrong refits the checker must see
(test_bvh_refit_restate.py).  The five deformations the tests refit to are
functions of the triangles alone, seeded where they draw numbers.
"""
import numpy as np

import bvh_build_restate as R
import bvh_check as B

f32 = np.float32

MUTATIONS = {
    "stale-parent": "one parent of an internal child keeps its old origin, exponents and planes",
    "unpadded": "U is taken from the triangles' unpadded min / max",
}


def _records(dump, tris):
    rec = np.asarray(dump["tris"], np.uint32).copy()
    n = tris.shape[0]
    idx = (rec[:n, 9] >> 1).astype(np.int64)
    t = tris[idx]
    rec[:n, :9] = np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], 1).view(np.uint32)
    rec[:n, 9] = 2 * idx
    return rec, idx


def slot_unions(dump, blo, bhi):
    """-> (slo, shi) float32 [n_nodes4, 4, 3]: U of every valid slot from the record boxes in
    leaf order (blo, bhi), +inf / -inf in an empty slot; bottom-up over the dump's levels."""
    nodes = np.asarray(dump["nodes"], np.uint32)
    n4 = nodes.shape[0]
    d = B.Decoded(nodes, dump["info"]["count_shift"])
    bad = []
    levels = B._levels(d, n4, bad)
    assert not bad, bad
    slo = np.full((n4, 4, 3), np.inf, f32)
    shi = np.full((n4, 4, 3), -np.inf, f32)
    nlo, nhi = np.zeros((n4, 3), f32), np.zeros((n4, 3), f32)
    for lev in reversed(levels):
        for k in range(4):
            leaf_k = lev[d.valid[lev, k] & d.leaf[lev, k]]
            if leaf_k.size:
                f0, c0 = d.first[leaf_k, k], d.count[leaf_k, k]
                lo, hi = blo[f0].copy(), bhi[f0].copy()
                for j in range(1, int(c0.max())):
                    m = c0 > j
                    lo[m] = np.minimum(lo[m], blo[f0[m] + j])
                    hi[m] = np.maximum(hi[m], bhi[f0[m] + j])
                slo[leaf_k, k], shi[leaf_k, k] = lo, hi
            inner_k = lev[d.valid[lev, k] & ~d.leaf[lev, k]]
            if inner_k.size:
                ch = d.link[inner_k, k]
                slo[inner_k, k], shi[inner_k, k] = nlo[ch], nhi[ch]
        nlo[lev], nhi[lev] = slo[lev].min(1), shi[lev].max(1)
    return slo, shi


def refit(dump, new_tris, mut=None):
    """-> {"nodes", "tris", "info", "near_exponent_boundary"}: the dump after a refit to
    new_tris (n, 3, 3), in the dump's own numbering."""
    assert mut is None or mut in MUTATIONS
    tris = np.asarray(new_tris, f32).reshape(-1, 3, 3)
    info = dict(dump["info"])
    n = info["n"]
    assert tris.shape[0] == n, "a refit keeps the triangle count"
    nodes = np.asarray(dump["nodes"], np.uint32)
    if n == 0:
        return {"nodes": nodes.copy(), "tris": np.asarray(dump["tris"], np.uint32).copy(), "info": info,
                "near_exponent_boundary": 0}
    rec, idx = _records(dump, tris)
    if mut == "unpadded":
        blo, bhi = tris.min(1), tris.max(1)
    else:
        blo, bhi = B.tri_boxes(tris)
    slo, shi = slot_unions(dump, blo[idx], bhi[idx])
    out = B.encode_nodes(slo, shi, nodes[:, 12:16])
    assert np.array_equal(out[:, 3] >> 24, nodes[:, 3] >> 24), "the masks are the links' own"
    if mut == "stale-parent":
        d = B.Decoded(nodes, info["count_shift"])
        parents = np.nonzero((d.valid & ~d.leaf).any(1))[0]
        out[parents[-1], :10] = nodes[parents[-1], :10]  # the deepest-numbered node with an internal child
    return {"nodes": out, "tris": rec, "info": info, "near_exponent_boundary": R.near_exponent_boundary(slo, shi)}


# ---------------------------------------------------------------- deformations
def _bounds(tris):
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    return v.min(0), v.max(0)


def twist(tris, degrees=90.0):
    """Every vertex turned about the vertical (y) axis through the centre of the bounds by
    degrees x (y - ymin) / (ymax - ymin): nothing at the bottom, the full angle at the top."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    if t.shape[0] == 0:
        return t.astype(f32)
    lo, hi = _bounds(t)
    c = 0.5 * (lo + hi)
    h = hi[1] - lo[1]
    a = np.radians(degrees) * ((t[..., 1] - lo[1]) / h if h > 0 else np.zeros(t.shape[:2]))
    x, z = t[..., 0] - c[0], t[..., 2] - c[2]
    out = t.copy()
    out[..., 0] = c[0] + np.cos(a) * x + np.sin(a) * z
    out[..., 2] = c[2] - np.sin(a) * x + np.cos(a) * z
    return out.astype(f32)


def jitter(tris, rel=0.05, seed=29):
    """Every coordinate moved by up to +-rel x the largest extent of the bounds."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    if t.shape[0] == 0:
        return t.astype(f32)
    lo, hi = _bounds(t)
    rng = np.random.default_rng(seed)
    return (t + (rng.random(t.shape) * 2.0 - 1.0) * rel * (hi - lo).max()).astype(f32)


def permuted(tris, seed=31):
    """The same triangles in other slots: triangle i becomes triangle perm[i]."""
    t = np.asarray(tris, f32).reshape(-1, 3, 3)
    return t[np.random.default_rng(seed).permutation(t.shape[0])].copy()


def one_point(tris):
    """Every vertex on the centre of the bounds."""
    t = np.asarray(tris, f32).reshape(-1, 3, 3)
    if t.shape[0] == 0:
        return t.copy()
    lo, hi = _bounds(t)
    return np.broadcast_to((0.5 * (lo + hi)).astype(f32), t.shape).copy()


def flat_y(tris, y=0.25):
    """Every y set to 0.25."""
    t = np.asarray(tris, f32).reshape(-1, 3, 3).copy()
    t[..., 1] = f32(y)
    return t


DEFORMATIONS = {"twist90": twist, "jitter5": jitter, "permuted": permuted, "one_point": one_point, "flat_y": flat_y}
