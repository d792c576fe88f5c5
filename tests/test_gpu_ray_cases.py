"""The scene queries on adversarial rays (ray_cases.py): axis-parallel rays
with zeros of both signs, directions on both sides of safe_inv's clamp and
subnormal ones, rays inside a flat scene's plane, and origins 10 and 100 scene
diagonals away -- what the traversal's arithmetic (tmpt_traverse.h: safe_inv,
the octant from the sign of 1/d, the slab test over o * (1/d), kBoxPadRel and
kTfarSlack) has to survive.

Tolerance: none.  Inside the asserted domain (test_ray_cases.py states and
checks it on the CPU) hit_scene_batch is the linear scan bit for bit: closest
ids, hit records, the any-hit bit, and the per-ray-range form range by range.
Beyond it -- origins 1e3 and 1e4 diagonals away, `anisotropic` from afar, far
origins with the reference's octree -- the answers must still be sound (a hit
is a triangle Moller-Trumbore accepts, with its t bits; never closer than the
scan's, never where the scan misses) and the deviation counts are printed;
DESIGN.md "Scene query contract" holds them.
"""
import functools

import numpy as np
import pytest

import geometry_cases as G
import mt_numpy as MT
import octree_kat as K
import oracle
import ray_cases as R
import test_ray_cases as P
import toymeshpathtracer_amd as tm
from conftest import data

pytestmark = pytest.mark.gpu

N, SEED = P.N, P.SEED
SUBSET = ("soup272", "uniform_sheet", "translated_3e5", "scaled_1e4")
BUILDS = [{}, {"builder": "lbvh"}, {"leaf_max": 16}, {"layout": "soa"}]
TIED_CASES = ("uniform_sheet", "flat_z")


def _opt_id(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ranged_reference(case, family):
    """The family's rays with a range each, and the linear scan's answers range by range."""
    tris = P.tris_of(case)
    r8 = R.ranged(P.rays_of(case)[family], SEED, R.range_unit(tris))
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    oids, ohits = np.full(N, -1, np.int32), np.zeros((N, 7), np.float32)
    pairs = np.unique(r8[:, 6:], axis=0)
    assert len(pairs) == len(R.RANGES)
    for lo, hi in pairs:
        sel = np.nonzero((r8[:, 6] == lo) & (r8[:, 7] == hi))[0]
        oids[sel], ohits[sel] = osc.hit_batch(r8[sel, :6], float(lo), float(hi))
    for a in (r8, oids, ohits):
        a.setflags(write=False)
    return r8, oids, ohits


@functools.lru_cache(maxsize=None)
def _tied(case, family):
    """mt_numpy's linear scan: (lowest index among the closest t, rays tied on it)."""
    tris = P.tris_of(case)
    ids, _, tied = MT.closest(P.rays_of(case)[family], tris, *G.ray_range(tris))
    return ids, np.nonzero(tied > 1)[0]


def _equal(tag, ids, hits, aids, oids, ohits, ranges=None):
    """-> what is wrong (empty: nothing): ids, hit records, the any-hit bit."""
    bad = []
    mism = np.nonzero(ids != oids)[0]
    if mism.size:
        where = "" if ranges is None else f" ranges {[tuple(r) for r in ranges[mism[:5]]]}"
        bad.append(f"{tag}: {mism.size} id mismatches, first rays {mism[:5]} gpu {ids[mism[:5]]} "
                   f"scan {oids[mism[:5]]}{where}")
    h = (ids >= 0) & (ids == oids)
    rec = np.nonzero((_u32(hits[h]) != _u32(ohits[h])).any(1))[0]
    if rec.size:
        bad.append(f"{tag}: {rec.size} hit records differ, first rays {np.nonzero(h)[0][rec[:5]]}")
    anyb = np.nonzero((aids >= 0) != (oids >= 0))[0]
    if anyb.size:
        bad.append(f"{tag}: {anyb.size} any-hit bits differ, first rays {anyb[:5]}")
    return bad


def _check_family(sc, case, family, tag, culls=(-1,), orders=(-1,)):
    """One asserted family on an open scene: the single range and the ranged
    form, closest hit under each pop_cull and any hit under each shadow_order."""
    tris = P.tris_of(case)
    rays = P.rays_of(case)[family]
    tmin, tmax = G.ray_range(tris)
    oids, ohits = P.scan_of(case, family)
    r8, roids, rohits = _ranged_reference(case, family)
    bad = []
    # the any-hit query under each child order (pop culling is the closest hit's alone)
    anys = {}
    for order in orders:
        sc.set_option("shadow_order", order)
        anys[order] = (sc.hit_scene_batch(rays, tmin, tmax, any_hit=True)[0], sc.hit_scene_batch(r8, any_hit=True)[0])
    for k, cull in enumerate(culls):
        sc.set_option("pop_cull", cull)
        ids, hits = sc.hit_scene_batch(rays, tmin, tmax)
        ids8, hits8 = sc.hit_scene_batch(r8)
        for order in orders if k == 0 else orders[:1]:
            t = f"{tag} {family} pop_cull={cull} shadow_order={order}"
            aids, aids8 = anys[order]
            bad += _equal(t, ids, hits, aids, oids, ohits)
            bad += _equal(t + " ranged", ids8, hits8, aids8, roids, rohits, ranges=r8[:, 6:])
        if case in TIED_CASES:
            low, tied = _tied(case, family)
            wrong = tied[ids[tied] != low[tied]]
            if wrong.size:
                bad.append(f"{tag} {family} pop_cull={cull}: {wrong.size} of {tied.size} tied rays not answered "
                           f"with the lowest index, first rays {wrong[:5]} gpu {ids[wrong[:5]]} "
                           f"lowest {low[wrong[:5]]}")
    sc.set_option("pop_cull", -1)
    sc.set_option("shadow_order", -1)
    return bad


def _soundness(tag, tris, rays, rng, ids, hits, aids, oids, ohits):
    """Outside the asserted domain: -> what is unsound; prints the deviation counts."""
    bad = []
    h = ids >= 0
    t = MT.pair_t(rays, tris, ids, *rng)
    wrong = np.nonzero(h & (_u32(t) != _u32(hits[:, 6])))[0]
    if wrong.size:
        bad.append(f"{tag}: {wrong.size} hits Moller-Trumbore does not accept at that t, first rays {wrong[:5]}")
    ghost = np.nonzero(h & (oids < 0))[0]
    if ghost.size:
        bad.append(f"{tag}: {ghost.size} hits where the scan misses, first rays {ghost[:5]}")
    both = h & (oids >= 0)
    near = np.nonzero(both & (hits[:, 6] < ohits[:, 6]))[0]
    if near.size:
        bad.append(f"{tag}: {near.size} hits closer than the scan's, first rays {near[:5]}")
    anyb = np.nonzero((aids >= 0) & (oids < 0))[0]
    if anyb.size:
        bad.append(f"{tag}: {anyb.size} any-hit bits set where the scan misses, first rays {anyb[:5]}")
    print(f"{tag}: of {len(rays)} rays the closest hit differs from the scan on {int((ids != oids).sum())} "
          f"(missed {int(((ids < 0) & (oids >= 0)).sum())}), the any-hit bit on "
          f"{int(((aids >= 0) != (oids >= 0)).sum())}; scan hits {int((oids >= 0).sum())}")
    return bad


# ---------------------------------------------------------------- the asserted domain
@pytest.mark.parametrize("case", P.CASES)
def test_default_build(gpu, case):
    """Every case under the default build: every asserted family equals the
    linear scan (ids, records, any-hit bit, per-ray ranges); tied rays answer
    the lowest index; rays inside a flat scene's plane all miss."""
    tris = P.tris_of(case)
    bad = []
    with tm.Scene(tris) as sc:
        for family in P.asserted(case):
            bad += _check_family(sc, case, family, case)
        if "in_plane" in P.rays_of(case):
            rays = P.rays_of(case)["in_plane"]
            ids, _ = sc.hit_scene_batch(rays, *G.ray_range(tris))
            aids, _ = sc.hit_scene_batch(rays, *G.ray_range(tris), any_hit=True)
            if (ids >= 0).any() or (aids >= 0).any():
                bad.append(f"{case} in_plane: {int((ids >= 0).sum())} closest hits, {int((aids >= 0).sum())} any hits, "
                           f"first rays {np.nonzero((ids >= 0) | (aids >= 0))[0][:5]}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", SUBSET)
@pytest.mark.parametrize("opts", BUILDS, ids=_opt_id)
def test_builds_and_walk_options(gpu, opts, case):
    """The LBVH, 16-wide leaves and the SoA layout (and the default build): the
    closest hit with pop culling off and on, the any-hit query under every
    child order -- the tree and the walk change, the answers do not."""
    bad = []
    with tm.Scene(P.tris_of(case), options=opts or None) as sc:
        for family in P.asserted(case):
            bad += _check_family(sc, case, family, f"{case} [{_opt_id(opts)}]", culls=(0, 1), orders=(0, 1, 2))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- report only: soundness
@pytest.mark.parametrize("case", P.CASES)
def test_beyond_the_domain_is_sound(gpu, case):
    """Origins 1e3 and 1e4 diagonals away (and `anisotropic` at every far
    distance): the padded leaf boxes no longer cover Moller-Trumbore's
    acceptance region, so hits may be missed -- nothing else may happen."""
    tris = P.tris_of(case)
    rng = G.ray_range(tris)
    lin = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    bad = []
    with tm.Scene(tris) as sc:
        for family, rays in P.rays_of(case).items():
            if family in P.asserted(case) or family == "in_plane":
                continue
            oids, ohits = lin.hit_batch(rays, *rng)
            ids, hits = sc.hit_scene_batch(rays, *rng)
            aids, _ = sc.hit_scene_batch(rays, *rng, any_hit=True)
            bad += _soundness(f"{case} {family}", tris, rays, rng, ids, hits, aids, oids, ohits)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["suzanne", "teapot"])
def test_obj_scenes_from_afar(gpu, name):
    """The reference's own meshes without the octree: equal to the linear scan
    from 10 and 100 diagonals away, sound (and counted) from 1e3 and 1e4."""
    tris, fam = P.obj_far_reference(name)
    rng = (0.001, 1.0e7)
    bad = []
    with tm.Scene(tris) as sc:
        for family, (rays, oids, ohits) in fam.items():
            ids, hits = sc.hit_scene_batch(rays, *rng)
            aids, _ = sc.hit_scene_batch(rays, *rng, any_hit=True)
            bad += _soundness(f"{name} {family}", tris, rays, rng, ids, hits, aids, oids, ohits)
            if family in R.ASSERTED:
                bad += _equal(f"{name} {family}", ids, hits, aids, oids, ohits)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- reference mode (the octree decides)
@pytest.mark.parametrize("name", ["suzanne", "teapot"])
def test_reference_mode(gpu, name):
    """With the reference's octree built: axis and near_axis rays equal the
    reference algorithm (oracle octree), ids and records, and every query on
    which it differs from the exact closest hit was counted as a tie or a
    crack query.  The far families are sound (report only)."""
    tris, bmin, bmax = oracle.load_scene(data(name + ".obj"))
    rng = (0.001, 1.0e7)
    fam = R.families(tris, N, SEED)
    rays = np.concatenate([fam["axis"], fam["near_axis"]])
    osc = K.ref_scene(tris, bmin, bmax)
    lin = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    rid, rh = osc.hit_batch(rays, *rng)
    eid, _ = lin.hit_batch(rays, *rng)
    bad = []
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        ids, hits = sc.hit_scene_batch(rays, *rng)
        st = sc.stats()
        aids, _ = sc.hit_scene_batch(rays, *rng, any_hit=True)
        bad += _equal(f"{name} axis+near_axis", ids, hits, aids, rid, rh)
        differs = int((rid != eid).sum())
        print(f"{name}: octree differs from the exact closest hit on {differs} of {len(rays)} rays "
              f"(axis {int((rid != eid)[:N].sum())}, near_axis {int((rid != eid)[N:].sum())}); "
              f"gpu tie_queries {st.tie_queries} crack_queries {st.crack_queries} root_misses {st.root_misses}")
        assert (rid >= 0).sum() > 1000 and differs > 0
        if st.tie_queries + st.crack_queries < differs:
            bad.append(f"{name}: tie_queries {st.tie_queries} + crack_queries {st.crack_queries} < {differs}")
        for m in R.FAR_ASSERTED:
            for kind in ("sphere", "axis"):
                far = fam[f"far_{kind}_{m}"]
                oids, ohits = lin.hit_batch(far, *rng)
                ids, hits = sc.hit_scene_batch(far, *rng)
                aids, _ = sc.hit_scene_batch(far, *rng, any_hit=True)
                bad += _soundness(f"{name} octree far_{kind}_{m}", tris, far, rng, ids, hits, aids, oids, ohits)
    assert not bad, "\n".join(bad)
