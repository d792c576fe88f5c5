"""Device-resident queries (tmpt_scene_hit_device, Scene.hit_scene_device).

The yardstick is the linear scan -- oracle.Scene(..., ACCEL_LINEAR, TIE_INDEX)
for scenes without an octree, the oracle octree's answers and the committed
tests/golden/ref/hits_<case>.npz with one -- as for hit_scene_batch
(test_gpu_ray_cases.py, test_gpu_reference_mode.py); agreement with
hit_scene_batch on the same scene is checked as well.

Tolerance: none.  ids, the seven record floats, t and (u, v) bit for bit on
every ray, for every value of query_sort x query_top, every chunking and grid.
(u, v) is compared with Moller-Trumbore in float32 numpy (mt_numpy's
operations) for the returned triangle.  Any-hit: the bit equals the scan's,
and a reported record's t and (u, v) are those of the reported triangle.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_cases as G
import mt_numpy as MT
import oracle
import ray_cases as R
import ref_cases as C
import test_gpu_ray_cases as RC
import test_gpu_reference_mode as RM
import test_ray_cases as P
import toymeshpathtracer_amd as tm
from conftest import ROOT, data

pytestmark = pytest.mark.gpu
torch = tm.torch

f32 = np.float32
SCENES = ("soup272", "uniform_sheet", "translated_3e5")
BUILDS = [{}, {"layout": "soa"}, {"leaf_max": 16}]
CONFIGS = [(s, t) for s in (0, 1) for t in (0, 1)]  # query_sort x query_top
OCTREE_CASES = RC.TIED_CASES + ("crack_wall",)
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")
SENTINEL = -12345.5


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, device=0):
    return torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{device}")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _query(sc, rays, *rng, **kw):
    """hit_scene_device on host rays -> numpy (ids, hits, uv)."""
    return tuple(_np(t) for t in sc.hit_scene_device(_dev(rays), *rng, **kw))


def mt_uv(rays, tris, ids):
    """Moller-Trumbore's (u, v) (maths.cpp:339-380) of triangle ids[i] for ray i, float32, by
    mt_numpy's operations; rows of ids < 0 are 0."""
    rays = np.asarray(rays, f32)
    tr = np.asarray(tris, f32).reshape(-1, 3, 3)[np.maximum(ids, 0)]
    o, d = MT._cols(rays[:, 0:3]), MT._cols(rays[:, 3:6])
    v0, v1, v2 = MT._cols(tr[:, 0]), MT._cols(tr[:, 1]), MT._cols(tr[:, 2])
    with np.errstate(all="ignore"):
        e1, e2 = MT._sub(v1, v0), MT._sub(v2, v0)
        pvec = MT._cross(d, e2)
        inv = MT.ONE / MT._dot(e1, pvec)
        tvec = MT._sub(o, v0)
        u = MT._dot(tvec, pvec) * inv
        v = MT._dot(d, MT._cross(tvec, e1)) * inv
    uv = np.stack([u, v], 1).astype(f32)
    uv[ids < 0] = 0
    return uv


def _problems(tag, tris, rays, rng, got, agot, oids, ohits, ranges=None):
    """got / agot: (ids, hits, uv) of the closest and the any-hit query -> what is wrong."""
    ids, hits, uv = got
    aids, ahits, auv = agot
    bad = RC._equal(tag, ids, hits, aids, oids, ohits, ranges)
    miss = ids < 0
    if hits[miss].any() or uv[miss].any():
        bad.append(f"{tag}: rows of missed rays were written")
    w = np.nonzero((_u32(uv) != _u32(mt_uv(rays, tris, ids))).any(1))[0]
    if w.size:
        bad.append(f"{tag}: {w.size} (u, v) differ from Moller-Trumbore's, first rays {w[:5]}")
    # a reported any-hit record is that triangle's: its accepted t, its (u, v); the closest one's record where it is that
    lo, hi = (rays[:, 6], rays[:, 7]) if ranges is not None else rng
    t = MT.pair_t(rays, tris, aids, lo, hi)
    h = aids >= 0
    w = np.nonzero(h & (_u32(t) != _u32(ahits[:, 6])))[0]
    if w.size:
        bad.append(f"{tag}: {w.size} any-hit records whose t is not the reported triangle's, first rays {w[:5]}")
    w = np.nonzero((_u32(auv) != _u32(mt_uv(rays, tris, aids))).any(1))[0]
    if w.size:
        bad.append(f"{tag}: {w.size} any-hit (u, v) are not the reported triangle's, first rays {w[:5]}")
    same = h & (aids == oids)
    w = np.nonzero((_u32(ahits[same]) != _u32(ohits[same])).any(1))[0]
    if w.size:
        bad.append(f"{tag}: {w.size} any-hit records differ from the scan's for the same triangle")
    return bad


@functools.lru_cache(maxsize=None)
def _neg_reference(case, family):
    """One range that starts behind the origin for the whole family, and the scan's answers."""
    tris = P.tris_of(case)
    unit = R.range_unit(tris)
    rng = (float(f32(-2.0 * unit)), float(f32(1e7 * unit)))
    ids, hits = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX).hit_batch(P.rays_of(case)[family], *rng)
    return rng, ids, hits


# ---------------------------------------------------------------- parity with the scan
def _parity(sc, case, tag, families=None):
    tris = P.tris_of(case)
    rng = G.ray_range(tris)
    bad = []
    for family in families or P.asserted(case):
        rays = P.rays_of(case)[family]
        oids, ohits = P.scan_of(case, family)
        r8, roids, rohits = RC._ranged_reference(case, family)
        nrng, noids, nohits = _neg_reference(case, family)
        d6, d8 = _dev(rays), _dev(r8)
        bids, bhits = sc.hit_scene_batch(rays, *rng)
        for sort, top in CONFIGS:
            sc.set_option("query_sort", sort)
            sc.set_option("query_top", top)
            t = f"{tag} {family} sort={sort} top={top}"

            def q(d, *a, **kw):
                return tuple(_np(x) for x in sc.hit_scene_device(d, *a, uv=True, **kw))

            got = q(d6, *rng)
            bad += _problems(t, tris, rays, rng, got, q(d6, *rng, any_hit=True), oids, ohits)
            bad += _problems(t + " ranged", tris, r8, None, q(d8), q(d8, any_hit=True), roids, rohits, ranges=r8[:, 6:])
            bad += _problems(t + " tmin<0", tris, rays, nrng, q(d6, *nrng), q(d6, *nrng, any_hit=True), noids, nohits)
            if not (np.array_equal(got[0], bids) and np.array_equal(_u32(got[1]), _u32(bhits))):
                bad.append(f"{t}: differs from hit_scene_batch on the same scene")
            assert int(sc.get_option("query_sorted")) == sort
        sc.set_option("query_sort", -1)
        sc.set_option("query_top", -1)
    return bad


@pytest.mark.parametrize("case", SCENES)
@pytest.mark.parametrize("opts", BUILDS, ids=RC._opt_id)
def test_parity_with_the_linear_scan(gpu, opts, case):
    with tm.Scene(P.tris_of(case), options=opts or None) as sc:
        bad = _parity(sc, case, f"{case} [{RC._opt_id(opts)}]")
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------- with the octree
@pytest.mark.parametrize("name", OCTREE_CASES)
def test_with_the_octree(gpu, name):
    """Answers and the octree's counters equal hit_scene_batch's on the same scene; answers
    equal the committed reference fixture (hit bit, record) and the oracle octree's ids."""
    c = RM._hit_case(name)
    fx, rid = c["fx"], c["rid"]
    rays, hit, rec = fx["rays"], fx["hit"].astype(bool), fx["rec"]
    bad = []
    counts = lambda st: (st.tie_queries, st.root_misses, st.crack_queries)  # noqa: E731
    with tm.Scene(fx["tris"], bounds=(fx["bmin"], fx["bmax"])) as sc:
        groups = [(None, None, np.arange(len(rays)))] + list(C.range_groups(rays))
        octree_answers = 0
        for lo, hi, sel in groups:
            r = rays[sel] if lo is None else rays[sel, :6]
            rng = () if lo is None else (lo, hi)
            bids, bhits = sc.hit_scene_batch(r, *rng)
            bst = counts(sc.stats())
            baids, _ = sc.hit_scene_batch(r, *rng, any_hit=True)
            bast = counts(sc.stats())
            d = _dev(r)
            for sort in (0, 1):
                sc.set_option("query_sort", sort)
                t = f"{name} range {lo}..{hi} sort={sort}"
                ids, hits, uv = (_np(x) for x in sc.hit_scene_device(d, *rng, uv=True))
                st = counts(sc.stats())
                aids, ahits, auv = (_np(x) for x in sc.hit_scene_device(d, *rng, any_hit=True, uv=True))
                ast = counts(sc.stats())
                if not (np.array_equal(ids, bids) and np.array_equal(_u32(hits), _u32(bhits))):
                    bad.append(f"{t}: answers differ from hit_scene_batch's, first rays {np.nonzero(ids != bids)[0][:5]}")
                if st != bst or ast != bast:
                    bad.append(f"{t}: tie / root / crack counters {st} {ast}, hit_scene_batch's {bst} {bast}")
                if not np.array_equal(aids >= 0, baids >= 0):
                    bad.append(f"{t}: any-hit bits differ from hit_scene_batch's")
                if not np.array_equal(ids >= 0, hit[sel]) or not np.array_equal(aids >= 0, hit[sel]):
                    bad.append(f"{t}: hit bits differ from the reference's")
                h = hit[sel] & (ids >= 0)
                if (_u32(hits[h]) != _u32(rec[sel][h])).any():
                    bad.append(f"{t}: records differ from the reference's")
                if not np.array_equal(ids, rid[sel]):
                    bad.append(f"{t}: ids differ from the oracle octree's")
                if (_u32(uv) != _u32(mt_uv(r, fx["tris"], ids))).any() or (_u32(auv) != _u32(mt_uv(r, fx["tris"], aids))).any():
                    bad.append(f"{t}: (u, v) are not the reported triangle's")
                lohi = (r[:, 6], r[:, 7]) if lo is None else (lo, hi)
                ta = MT.pair_t(r, fx["tris"], aids, *lohi)
                if ((aids >= 0) & (_u32(ta) != _u32(ahits[:, 6]))).any():
                    bad.append(f"{t}: any-hit t is not the reported triangle's")
            sc.set_option("query_sort", -1)
            octree_answers += sum(bst) + sum(bast)
        if name in RC.TIED_CASES:  # the octree took part: ties, root misses or crack queries were counted
            assert octree_answers > 0
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------- shapes
@functools.lru_cache(maxsize=None)
def _soup():
    tris = P.tris_of("soup272")
    rays = np.concatenate([P.rays_of("soup272")["axis"][:600], P.rays_of("soup272")["far_sphere_10"][:400]])
    ids, hits = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX).hit_batch(rays, *G.ray_range(tris))
    assert 100 < (ids >= 0).sum() < 1000
    return tris, rays, ids, hits


def _same(tag, got, ids, hits, tris, rays):
    assert np.array_equal(got[0], ids), f"{tag}: ids"
    assert np.array_equal(_u32(got[1]), _u32(np.where((ids >= 0)[:, None], hits, 0))), f"{tag}: records"
    assert np.array_equal(_u32(got[2]), _u32(mt_uv(rays, tris, ids))), f"{tag}: uv"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_shapes(gpu, n):
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    with tm.Scene(tris) as sc:
        for sort, top in CONFIGS:
            sc.set_option("query_sort", sort)
            sc.set_option("query_top", top)
            got = _query(sc, rays[:n], *rng, uv=True)
            assert got[0].shape == (n,) and got[1].shape == (n, 7) and got[2].shape == (n, 2)
            _same(f"n={n} sort={sort} top={top}", got, ids[:n], hits[:n], tris, rays[:n])
            r8 = np.concatenate([rays[:n], np.tile(np.array(rng, f32), (n, 1))], 1)
            _same(f"n={n} ranged sort={sort} top={top}", _query(sc, r8, uv=True), ids[:n], hits[:n], tris, rays[:n])


def test_grid_and_chunks(gpu):
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    with tm.Scene(tris) as sc:
        sc.set_option("query_sort", 0)
        sc.set_option("query_grid", 1)  # one block loops over four strides
        _same("query_grid=1", _query(sc, rays, *rng, uv=True), ids, hits, tris, rays)
        assert (sc.get_option("query_chunks"), sc.get_option("query_sorted")) == (1, 0)
        sc.set_option("query_sort", 1)
        _same("query_grid=1 sorted", _query(sc, rays, *rng, uv=True), ids, hits, tris, rays)
        sc.set_option("query_grid", 0)
        sc.set_option("query_chunk", 128)  # eight chunks, the last partial
        _same("query_chunk=128", _query(sc, rays, *rng, uv=True), ids, hits, tris, rays)
        assert (sc.get_option("query_chunks"), sc.get_option("query_sorted")) == (8, 1)
        assert sc.get_option("query_ms") > 0 and 0 < sc.get_option("query_sort_ms") <= sc.get_option("query_ms")
        for sort in (1, 0):  # a base 24 bytes into an allocation: not 16-byte aligned, the narrow loads
            sc.set_option("query_sort", sort)
            off = tuple(_np(t) for t in sc.hit_scene_device(_dev(rays)[1:], *rng, uv=True))
            _same(f"offset base sort={sort}", off, ids[1:], hits[1:], tris, rays[1:])
        sc.set_option("query_sort", 1)
        sc.set_option("query_chunk", 1 << 22)
        # one ray a thousand times: all keys equal
        k = int(np.nonzero(ids >= 0)[0][0])
        rep = np.repeat(rays[k:k + 1], 1000, 0)
        _same("one ray repeated", _query(sc, rep, *rng, uv=True), np.repeat(ids[k:k + 1], 1000), np.repeat(hits[k:k + 1], 1000, 0),
              tris, rep)
        # every ray holds a NaN: all misses, as hit_scene_batch gives
        nan = rays.copy()
        nan[np.arange(1000), np.arange(1000) % 6] = np.nan
        for sort in (0, 1):
            sc.set_option("query_sort", sort)
            got = _query(sc, nan, *rng, uv=True)
            assert (got[0] == -1).all() and (sc.hit_scene_batch(nan, *rng)[0] == -1).all()
            assert (_query(sc, nan, *rng, any_hit=True)[0] == -1).all()
            assert not got[1].any() and not got[2].any()


# ---------------------------------------------------------------- optional outputs
def test_optional_outputs_and_sentinels(gpu):
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    d = _dev(rays)
    with tm.Scene(tris) as sc:
        for sort in (0, 1):
            sc.set_option("query_sort", sort)
            full = tuple(_np(t) for t in sc.hit_scene_device(d, *rng, uv=True))
            _same(f"sort={sort}", full, ids, hits, tris, rays)
            i, h, w = sc.hit_scene_device(d, *rng, hits=False)
            assert h is None and w is None and np.array_equal(_np(i), ids)
            i, h, w = sc.hit_scene_device(d, *rng, hits=False, uv=True)
            assert h is None and np.array_equal(_np(i), ids) and np.array_equal(_u32(_np(w)), _u32(full[2]))
            i, h, w = sc.hit_scene_device(d, *rng)
            assert w is None and np.array_equal(_np(i), ids) and np.array_equal(_u32(_np(h)), _u32(full[1]))
            out = (torch.full((1000,), 7, dtype=torch.int32, device="cuda:0"),
                   torch.full((1000, 7), SENTINEL, dtype=torch.float32, device="cuda:0"),
                   torch.full((1000, 2), SENTINEL, dtype=torch.float32, device="cuda:0"))
            res = sc.hit_scene_device(d, *rng, out=out)
            assert all(a is b for a, b in zip(res, out))
            i, h, w = (_np(t) for t in out)
            assert np.array_equal(i, ids)
            assert (h[ids < 0] == f32(SENTINEL)).all() and (w[ids < 0] == f32(SENTINEL)).all()
            assert np.array_equal(_u32(h[ids >= 0]), _u32(hits[ids >= 0])) and np.array_equal(_u32(w[ids >= 0]), _u32(full[2][ids >= 0]))
            res = sc.hit_scene_device(d, *rng, out=(out[0], None, None))
            assert res[1] is None and res[2] is None and np.array_equal(_np(res[0]), ids)


# ---------------------------------------------------------------- stream order
def test_stream_order(gpu):
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    with tm.Scene(tris) as sc:
        eager = _query(sc, rays, *rng, uv=True)
        half = _dev(rays * f32(0.5))
        big = torch.ones((2048, 2048), device="cuda:0")
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            for _ in range(4):  # work the rays' producer waits behind on this stream
                big = (big @ big) * 1e-4
            d = half + half  # rays made on the side stream, behind that work, just before the call
            got = sc.hit_scene_device(d, *rng, uv=True)  # wait_stream="current": the side stream
            got = tuple(t.cpu().numpy() for t in got)  # read on that stream, no explicit synchronise
        torch.cuda.synchronize()
        assert np.array_equal(_u32(_np(d)), _u32(rays))  # 0.5 x + 0.5 x is exact, signed zeros included
        for a, b in zip(got, eager):
            assert np.array_equal(_u32(a), _u32(b))


# ---------------------------------------------------------------- allocations
def test_no_allocation_per_call(gpu):
    import gc
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    d = _dev(rays)
    with tm.Scene(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)) as witness:
        live = lambda: (gc.collect(), int(witness.get_option("live_device_objects")))[1]  # noqa: E731
        before = live()
        sc = tm.Scene(tris)
        for sort in (0, 1):
            sc.set_option("query_sort", sort)
            first = tuple(_np(t) for t in sc.hit_scene_device(d, *rng, uv=True))
            n1 = live()
            again = tuple(_np(t) for t in sc.hit_scene_device(d, *rng, uv=True))
            assert live() == n1, f"sort={sort}: a repeated call moved live_device_objects"
            assert all(np.array_equal(_u32(a), _u32(b)) for a, b in zip(first, again))
        sc.close()
        assert live() == before
        # the scratch does not fit: -12, the scene unchanged, and the next call answers as before
        sc = tm.Scene(tris)
        sc.set_option("query_max", 1)
        n0 = live()
        with pytest.raises(tm.TmptError, match=r"\(-12\).*query_max"):
            sc.hit_scene_device(d, *rng)
        assert live() == n0
        sc.set_option("query_max", 0)
        _same("after -12", tuple(_np(t) for t in sc.hit_scene_device(d, *rng, uv=True)), ids, hits, tris, rays)
        sc.close()
        assert live() == before


# ---------------------------------------------------------------- state neutrality
W, H, SPP = 64, 36, 4
STATS = ("extend_rays", "shadow_rays", "tie_queries", "root_misses", "crack_queries", "tie_rule")


@functools.lru_cache(maxsize=None)
def _suzanne():
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    fam = R.families(tris, 500, 3)
    rays = np.concatenate([fam["axis"], fam["near_axis"], fam["far_sphere_10"]])
    moved = tris.copy()
    moved[::3] += f32(0.01)
    return tris, bmin, bmax, rays, moved


def _stats(sc):
    st = sc.stats()
    return tuple(getattr(st, f) for f in STATS)


def _q(sc):
    tris, bmin, bmax, rays, moved = _suzanne()
    got = sc.hit_scene_device(_dev(rays), 0.001, 1.0e7, uv=True)
    return tuple(_np(t).tobytes() for t in got) + _stats(sc)[2:]


def _b_image(sc, cam):
    img, rays = sc.trace_image(cam, W, H, SPP, seed_mode=tm.SEED_SAMPLE)
    return img.tobytes(), rays, _stats(sc)


def _b_aov(sc, cam):
    rec, rays = sc.trace_aov(cam, W, H, SPP)
    return rec.tobytes(), rays, _stats(sc)


def _b_hit(sc, cam):
    ids, hits = sc.hit_scene_batch(_suzanne()[3], 0.001, 1.0e7)
    return ids.tobytes(), hits.tobytes(), _stats(sc)[2:]


def _b_pass1(sc, cam):
    return sc.trace_image(cam, W, H, SPP, seed_mode=tm.SEED_SAMPLE, spp_begin=0, spp_count=2)[1]


def _b_pass2(sc, cam):
    img, rays = sc.trace_image(cam, W, H, SPP, seed_mode=tm.SEED_SAMPLE, spp_begin=2, spp_count=2)
    return img.tobytes(), rays, _stats(sc)


def _b_refit(sc, cam):
    sc.update(_suzanne()[4], "refit")
    return (sc.get_option("update_kind"),) + _b_hit(sc, cam)


KINDS = {"trace_image": (None, _b_image), "trace_aov": (None, _b_aov), "hit_scene_batch": (None, _b_hit),
         "progressive_pass2": (_b_pass1, _b_pass2), "update_refit": (None, _b_refit)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_state_neutrality(gpu, kind):
    """B after hit_scene_device equals B on a fresh scene (bytes, rays, stats), and
    hit_scene_device after B equals itself on a fresh scene."""
    tris, bmin, bmax, rays, moved = _suzanne()
    cam = tm.Camera.for_scene(bmin, bmax, W, H)
    prefix, b = KINDS[kind]
    fresh = lambda: tm.Scene(tris, bounds=(bmin, bmax))  # noqa: E731
    with fresh() as sc:
        if prefix:
            prefix(sc, cam)
        want_b = b(sc, cam)
        q_after_b = _q(sc)
        if kind == "update_refit":  # the octree is gone: tie_rule index answers, as hit_scene_batch's
            assert sc.stats().tie_rule == 1
            ids, hits = sc.hit_scene_batch(rays, 0.001, 1.0e7)
            assert q_after_b[0] == ids.tobytes() and q_after_b[1] == hits.tobytes()
    with fresh() as sc:
        want_q = _q(sc)
        for sort in (0, 1):  # between the prefix and B, sorted and unsorted
            sc.set_option("query_sort", sort)
            assert _q(sc) == want_q
        sc.set_option("query_sort", -1)
    with fresh() as sc:
        if prefix:
            prefix(sc, cam)
        for sort in (0, 1):
            sc.set_option("query_sort", sort)
            assert _q(sc) == want_q
        sc.set_option("query_sort", -1)
        assert b(sc, cam) == want_b, f"{kind} after hit_scene_device differs from {kind} on a fresh scene"
    if kind == "update_refit":
        with tm.Scene(moved, options={"tie_rule": "index"}) as sc:
            assert _q(sc)[:3] == q_after_b[:3]
    else:
        assert q_after_b == want_q, f"hit_scene_device after {kind} differs from itself on a fresh scene"


# ---------------------------------------------------------------- argument errors from Python
def test_python_argument_errors(gpu):
    tris, rays, ids, hits = _soup()
    rng = G.ray_range(tris)
    d = _dev(rays)
    with tm.Scene(tris) as sc:
        bad = [(torch.from_numpy(rays), rng, {}, "is on cpu"),
               (rays, rng, {}, "torch tensor"),
               (d.double(), rng, {}, "torch.float32"),
               (_dev(np.concatenate([rays, rays], 1))[:, :6], rng, {}, "contiguous"),
               (_dev(rays[:, :5]), rng, {}, r"shape \[n, 6\]"),
               (d, (), {}, r"shape \[n, 8\]"),
               (_dev(np.concatenate([rays, rays[:, :2]], 1)), rng, {}, r"shape \[n, 6\]"),
               (d.reshape(-1), rng, {}, r"shape \[n, 6\]"),
               (d, (rng[0],), {}, "both t_min and t_max"),
               (d, rng, dict(out=(None, None, None)), "ids must be a tensor"),
               (d, rng, dict(out=(torch.zeros(999, dtype=torch.int32, device="cuda:0"), None, None)), "out ids must have shape"),
               (d, rng, dict(out=(torch.zeros(1000, dtype=torch.int64, device="cuda:0"), None, None)), "out ids must be torch.int32"),
               (d, rng, dict(out=(torch.zeros(1000, dtype=torch.int32, device="cuda:0"),
                                  torch.zeros((1000, 6), device="cuda:0"), None)), "out hits must have shape"),
               (d, rng, dict(out=(torch.zeros(1000, dtype=torch.int32, device="cuda:0"), None,
                                  torch.zeros((1000, 2)))), "out uv is on cpu"),
               (d, rng, dict(out=(torch.zeros(1000, dtype=torch.int32, device="cuda:0"),)), "out = "),
               ]
        if torch.cuda.device_count() > 1:
            bad.append((d.to("cuda:1"), rng, {}, "is on cuda:1"))
        for r, a, kw, msg in bad:
            with pytest.raises(ValueError, match=msg):
                sc.hit_scene_device(r, *a, **kw)
        _same("after the errors", tuple(_np(t) for t in sc.hit_scene_device(d, *rng, uv=True)), ids, hits, tris, rays)


def test_c_argument_errors_in_order(gpu):
    """The -22s of the header, in its order, on a live scene; n = 0 launches nothing."""
    import ctypes
    tris, rays, ids, hits = _soup()
    fn = tm._sig("tmpt_scene_hit_device", ctypes.c_int, [ctypes.c_void_p] * 6)
    d = _dev(rays)
    out = torch.zeros(1000, dtype=torch.int32, device="cuda:0")

    def desc(**kw):
        x = tm._HitDesc()
        x.n, x.tmin, x.tmax = 1000, 0.001, 1e7
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    with tm.Scene(tris) as sc:
        err = lambda: tm._last_error().decode()  # noqa: E731
        assert fn(sc._h, None, d.data_ptr(), out.data_ptr(), None, None) == -22 and "null descriptor" in err()
        steps = [(desc(n=-1, flags=2, ranged=2), d.data_ptr(), "n < 0"),
                 (desc(flags=2, ranged=2), None, "null d_rays or d_ids"),
                 (desc(flags=2, ranged=2), d.data_ptr(), "unknown flag"),
                 (desc(flags=1), d.data_ptr(), "unknown flag"),
                 (desc(ranged=2), d.data_ptr(), "ranged and any_hit"),
                 (desc(any_hit=-1), d.data_ptr(), "ranged and any_hit")]
        for x, rp, msg in steps:
            assert fn(sc._h, ctypes.byref(x), rp, out.data_ptr(), None, None) == -22 and msg in err(), (msg, err())
        assert fn(sc._h, ctypes.byref(desc()), d.data_ptr(), None, None, None) == -22 and "null d_rays or d_ids" in err()
        assert fn(sc._h, ctypes.byref(desc(n=0)), None, None, None, None) == 0
        # a non-finite single range is accepted, as tmpt_scene_hit accepts it
        x = desc(tmax=float("inf"))
        assert fn(sc._h, ctypes.byref(x), d.data_ptr(), out.data_ptr(), None, None) == 0
        assert np.array_equal(_np(out), sc.hit_scene_batch(rays, 0.001, float("inf"))[0])
        x = desc(tmin=float("nan"))
        assert fn(sc._h, ctypes.byref(x), d.data_ptr(), out.data_ptr(), None, None) == 0
        assert np.array_equal(_np(out), sc.hit_scene_batch(rays, float("nan"), 1e7)[0]) and (_np(out) == -1).all()


# ---------------------------------------------------------------- the checked build
def parity_digests():
    """soup272's parity queries under every query_sort x query_top -> digests (the child of the checked build runs this)."""
    case = "soup272"
    tris = P.tris_of(case)
    rng = G.ray_range(tris)
    out = {}
    with tm.Scene(tris) as sc:
        for family in ("axis", "far_axis_100"):
            rays = P.rays_of(case)[family]
            r8 = R.ranged(rays, P.SEED, R.range_unit(tris))
            d6, d8 = _dev(rays), _dev(r8)
            for sort, top in CONFIGS:
                sc.set_option("query_sort", sort)
                sc.set_option("query_top", top)
                h = hashlib.sha256()
                for any_hit in (False, True):
                    for res in (sc.hit_scene_device(d6, *rng, any_hit=any_hit, uv=True),
                                sc.hit_scene_device(d8, any_hit=any_hit, uv=True)):
                        for t in res:
                            h.update(_np(t).tobytes())
                out[f"{family} {sort} {top}"] = h.hexdigest()
    return out


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_hit_device as T
print(json.dumps(T.parity_digests()))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_hit_device_checked_build(gpu):
    """The checked library gives the same bits on soup272's parity case and no index check fails (-30)."""
    env = dict(os.environ, TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = parity_digests()
    assert got == want and len(want) == 8
    ids = P.scan_of("soup272", "axis")[0]
    assert (ids >= 0).sum() > 1000  # the digests cover hits
