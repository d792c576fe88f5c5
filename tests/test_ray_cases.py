"""CPU preconditions of the adversarial-ray tests (ray_cases.py), so that a
failure of test_gpu_ray_cases.py is the GPU's:

- the generator is deterministic, float32, finite, and does what it says;
- the two references agree: mt_numpy (numpy restatement of Moller-Trumbore)
  equals the oracle's linear scan bit for bit, ids and t;
- the families are not vacuous: each hits on at least a tenth of its rays in
  every case, and the axis rays on uniform_sheet tie on the closest t;
- the domain: on the asserted families the oracle BVH -- whose leaf boxes are
  padded by the rule and the constants of the device build -- equals the
  linear scan.  `anisotropic` fails that for far origins (Moller-Trumbore's
  acceptance region widens with |o - v0|, the padded box does not), so it is
  asserted for axis and near_axis only and its far counts are printed.
"""
import functools

import numpy as np
import pytest

import geometry_cases as G
import mt_numpy as MT
import oracle
import ray_cases as R
from conftest import data

CASES = ("soup272", "soup4096", "uniform_sheet", "flat_z", "degenerate_mix", "translated_1e4", "translated_3e5",
         "scaled_1e4", "scaled_1e-4", "one_cell", "anisotropic")
FLAT = ("uniform_sheet", "flat_z")
N = 20000
SEED = 5


def asserted(case):
    """The families on which the case's answers must equal the linear scan's."""
    return ("axis", "near_axis") if case == "anisotropic" else R.ASSERTED


@functools.lru_cache(maxsize=None)
def tris_of(case):
    t = G.case(case)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def rays_of(case):
    fam = R.families(tris_of(case), N, SEED)
    for a in fam.values():
        a.setflags(write=False)
    return fam


@functools.lru_cache(maxsize=None)
def scan_of(case, family):
    """The oracle's linear scan on one family at ray_range's (tmin, tmax)."""
    tris = tris_of(case)
    ids, hits = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX).hit_batch(
        rays_of(case)[family], *G.ray_range(tris))
    ids.setflags(write=False)
    hits.setflags(write=False)
    return ids, hits


@pytest.mark.parametrize("case", CASES)
def test_generator(case):
    tris = tris_of(case)
    fam = rays_of(case)
    again = R.families(tris, N, SEED)
    assert list(fam) == list(again)
    assert set(fam) == set(R.ASSERTED + R.REPORT_ONLY + (("in_plane",) if case in FLAT else ()))
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    L, D, c = (hi - lo).max(), np.linalg.norm(hi - lo), 0.5 * (lo + hi)
    for name, rays in fam.items():
        assert rays.dtype == np.float32 and rays.shape == (N, 6), name
        assert rays.tobytes() == again[name].tobytes(), name
        assert np.isfinite(rays).all(), name
        d = rays[:, 3:].astype(np.float64)
        assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-6, name
    # axis: one component +-1, the others zeros of both signs
    d = fam["axis"][:, 3:]
    assert ((np.abs(d) == 1).sum(1) == 1).all() and ((d == 0).sum(1) == 2).all()
    z = d[d == 0]
    assert 0.4 < np.signbit(z).mean() < 0.6
    back = np.abs(fam["axis"][:, :3].astype(np.float64) - c).max(1)
    assert back.max() < 2.1 * L + np.abs(c).max() * 1e-6
    # near_axis: the off-axis components are tiny but not zero, some below the
    # clamp of safe_inv (1e-20), some subnormal
    d = np.sort(np.abs(fam["near_axis"][:, 3:]), 1)
    assert (d[:, 2] > 0.999).all() and (d[:, 0] > 0).all() and (d[:, 1] < 1.1e-3).all()
    assert (d[:, 0] < 1e-20).any() and (d[:, 0] < np.finfo(np.float32).tiny).any() and (d[:, 1] > 1e-4).any()
    # far: the origins are where the name says
    for m in R.FAR_ASSERTED + R.FAR_REPORT:
        r = np.linalg.norm(fam[f"far_sphere_{m}"][:, :3].astype(np.float64) - c, axis=1) / (m * D)
        assert 0.99 < r.min() and r.max() < 1.01, (m, r.min(), r.max())
        o = np.abs(fam[f"far_axis_{m}"][:, :3].astype(np.float64) - c)
        r = o.max(1) / (m * D)
        assert 0.99 < r.min() and r.max() < 1.01, (m, r.min(), r.max())
        assert (np.sort(o, 1)[:, 1] <= (hi - lo).max() * 1.001 + np.abs(c).max() * 1e-6).all()
    if case in FLAT:
        ax = int(np.nonzero(hi == lo)[0][0])
        r = fam["in_plane"]
        assert (r[:, ax] == lo[ax]).all() and (r[:, 3 + ax] == 0).all()
    # ranged: the same rays, every one of the ten ranges drawn, scaled
    unit = R.range_unit(tris)
    r8 = R.ranged(fam["axis"], SEED, unit)
    assert r8.dtype == np.float32 and r8.shape == (N, 8) and np.array_equal(r8[:, :6], fam["axis"])
    assert r8.tobytes() == R.ranged(fam["axis"], SEED, unit).tobytes()
    assert len(np.unique(r8[:, 6:], axis=0)) == len(R.RANGES)
    assert (r8[:, 6] < 0).any() and (r8[:, 6] > r8[:, 7]).any()
    assert np.float32(1e-3 * unit) == np.float32(G.ray_range(tris)[0])


@pytest.mark.parametrize("case", CASES)
def test_mt_numpy_equals_linear_scan(case):
    """Bit for bit, ids and t, on every asserted family -- and each family hits."""
    tris = tris_of(case)
    tmin, tmax = G.ray_range(tris)
    for family in asserted(case):
        rays = rays_of(case)[family]
        oids, ohits = scan_of(case, family)
        ids, t, tied = MT.closest(rays, tris, tmin, tmax)
        rate = (oids >= 0).mean()
        print(f"{case} {family}: hits {rate:.3f} tied {int((tied > 1).sum())}")
        assert np.array_equal(ids, oids), (family, np.nonzero(ids != oids)[0][:5])
        h = ids >= 0
        assert np.array_equal(t[h].view(np.uint32), ohits[h, 6].view(np.uint32)), family
        assert np.isinf(t[~h]).all()
        assert rate >= 0.10, (family, rate)
        # the elementwise form agrees with the table
        assert np.array_equal(MT.pair_t(rays, tris, ids, tmin, tmax).view(np.uint32), t.view(np.uint32)), family


def test_mt_numpy_ranges_and_ties():
    """Per-ray ranges (negative and empty ones included) against the linear
    scan, range by range; the tied sets hold the answer and only equal t."""
    tris = tris_of("uniform_sheet")
    rays = rays_of("uniform_sheet")["axis"]
    r8 = R.ranged(rays, SEED, R.range_unit(tris))
    ids, t, tied = MT.closest(rays, tris, r8[:, 6], r8[:, 7])
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    for lo, hi in np.unique(r8[:, 6:], axis=0):
        sel = np.nonzero((r8[:, 6] == lo) & (r8[:, 7] == hi))[0]
        oids, ohits = osc.hit_batch(rays[sel], float(lo), float(hi))
        assert np.array_equal(ids[sel], oids), (lo, hi)
        h = oids >= 0
        assert np.array_equal(t[sel][h].view(np.uint32), ohits[h, 6].view(np.uint32)), (lo, hi)
    sets = MT.tied_sets(rays, tris, r8[:, 6], r8[:, 7])
    assert sorted(sets) == list(np.nonzero(tied > 1)[0])
    table = MT.accepted_t(rays[:2000], tris, r8[:2000, 6], r8[:2000, 7])
    for r, s in sets.items():
        assert s[0] == ids[r] and len(s) == tied[r]
        if r < 2000:
            assert (table[r, s] == t[r]).all() and (np.delete(table[r], s) > t[r]).all()


def test_axis_rays_tie_on_uniform_sheet():
    tris = tris_of("uniform_sheet")
    _, _, tied = MT.closest(rays_of("uniform_sheet")["axis"], tris, *G.ray_range(tris))
    print("uniform_sheet axis: rays tied on the closest t", int((tied > 1).sum()))
    assert (tied > 1).sum() >= 500


@pytest.mark.parametrize("case", FLAT)
def test_in_plane_rays_miss(case):
    tris = tris_of(case)
    ids, _, _ = MT.closest(rays_of(case)["in_plane"], tris, *G.ray_range(tris))
    assert (ids < 0).all()
    oids, _ = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR).hit_batch(rays_of(case)["in_plane"], *G.ray_range(tris))
    assert (oids < 0).all()


@pytest.mark.parametrize("case", CASES)
def test_domain_bvh_equals_linear_scan(case):
    """The oracle BVH (the device build's leaf-box rule) against the linear
    scan: equal on the asserted families; the deviations beyond are printed
    (DESIGN.md "Scene query contract" holds the table)."""
    tris = tris_of(case)
    rng = G.ray_range(tris)
    bvh = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    lin = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    bad = []
    for family, rays in rays_of(case).items():
        ids, hits = bvh.hit_batch(rays, *rng)
        oids, ohits = scan_of(case, family) if family in asserted(case) else lin.hit_batch(rays, *rng)
        dev = np.nonzero(ids != oids)[0]
        print(f"{case} {family}: oracle BVH differs from the scan on {dev.size} of {len(rays)} rays")
        # sound wherever it is not equal: never closer than the scan, never a hit the scan misses
        assert (oids[ids >= 0] >= 0).all() and (hits[ids >= 0, 6] >= ohits[ids >= 0, 6]).all(), family
        if family not in asserted(case) and family != "in_plane":
            continue
        if dev.size:
            bad.append(f"{case} {family}: {dev.size} rays differ, first {dev[:5]} bvh {ids[dev[:5]]} "
                       f"scan {oids[dev[:5]]}")
        h = (ids >= 0) & (ids == oids)
        rec = np.nonzero((hits[h].view(np.uint32) != ohits[h].view(np.uint32)).any(1))[0]
        if rec.size:
            bad.append(f"{case} {family}: {rec.size} hit records differ")
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def obj_far_reference(name):
    """The far families of an OBJ scene (no octree) and the linear scan's answers
    at the reference's range: name -> {family: (rays, ids, hits)}."""
    tris, _, _ = oracle.load_scene(data(name + ".obj"))
    lin = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    out = {}
    for family, rays in R.families(tris, N, SEED).items():
        if family.startswith("far_"):
            out[family] = (rays,) + lin.hit_batch(rays, 0.001, 1.0e7)
            for a in out[family]:
                a.setflags(write=False)
    return tris, out


@pytest.mark.parametrize("name", ["suzanne", "teapot"])
def test_domain_obj_scenes(name):
    """The same domain on the reference's own meshes: the oracle BVH equals the
    scan from 10 and 100 diagonals away; the counts beyond are printed."""
    tris, fam = obj_far_reference(name)
    bvh = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX)
    for family, (rays, oids, ohits) in fam.items():
        ids, hits = bvh.hit_batch(rays, 0.001, 1.0e7)
        dev = np.nonzero(ids != oids)[0]
        print(f"{name} {family}: oracle BVH differs from the scan on {dev.size} of {len(rays)} rays; "
              f"scan hits {int((oids >= 0).sum())}")
        assert (oids[ids >= 0] >= 0).all() and (hits[ids >= 0, 6] >= ohits[ids >= 0, 6]).all(), family
        if family in R.ASSERTED:
            assert (oids >= 0).mean() >= 0.10
            assert dev.size == 0, (family, dev[:5], ids[dev[:5]], oids[dev[:5]])
            h = ids >= 0
            assert np.array_equal(hits[h].view(np.uint32), ohits[h].view(np.uint32)), family
