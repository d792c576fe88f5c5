"""The geometry and ray generator of the build tests (geometry_cases.py),
checked on the CPU by the oracle's linear scan alone: every case must give the
GPU tests rays that hit and rays that miss, or a comparison there says little."""
import numpy as np
import pytest

import geometry_cases as G
import oracle

N_RAYS = 4000
_CASES = G.cases()


def _scan(tris, rays, rng):
    return oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX).hit_batch(rays, *rng)


def test_case_list_is_complete():
    """The sweep covers every count of 3..272 and the large counts around the
    sort tile and the scan switch; the named families are all there."""
    assert [n for n in range(3, 273) if G.sweep_name(n) not in _CASES] == []
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4100):
        assert _CASES[G.sweep_name(n)].shape == (n, 3, 3)
    assert set(G.NON_SWEEP) <= set(_CASES) and len(_CASES) == 280 + len(G.SWEEP_NODES) + len(G.NON_SWEEP)
    for k in (3, 17, 64, 130, 200, 1000):
        assert _CASES[f"coincident{k}"].shape == (k, 3, 3)


def test_generator_is_deterministic():
    again = G.cases()
    assert list(again) == list(_CASES)
    for name, tris in _CASES.items():
        assert tris.dtype == np.float32 and tris.ndim == 3 and tris.shape[1:] == (3, 3), name
        assert np.isfinite(tris).all(), name
        assert np.array_equal(tris.view(np.uint32), again[name].view(np.uint32)), name
        assert np.array_equal(tris.view(np.uint32), G.case(name).view(np.uint32)), name
    for name in ("soup3", "coincident200", "translated_3e5"):
        a, ra = G.rays(_CASES[name], N_RAYS, 5)
        b, rb = G.rays(_CASES[name], N_RAYS, 5)
        assert ra == rb and a.dtype == np.float32 and a.shape == (N_RAYS, 6)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_case_structure():
    """What each family is built to have: identical boxes, zero extents, exact spacing."""
    c = _CASES
    for k in (3, 17, 64, 130, 200, 1000):
        assert (c[f"coincident{k}"] == c[f"coincident{k}"][0]).all()
    assert G.zero_area(c["points200"]).sum() == 200 and G.zero_area(c["segments200"]).sum() == 200
    fan = c["samebox_fan150"]
    assert (fan.min(1) == 0.0).all() and (fan.max(1) == 1.0).all()
    assert len(np.unique(fan.reshape(150, 9), axis=0)) == 150
    nest = c["nested200"]
    assert (np.diff(nest.max(1), axis=0) >= 0).all() and (np.diff(nest.min(1), axis=0) <= 0).all()
    assert c["degenerate_mix"].shape[0] == 330 and G.zero_area(c["degenerate_mix"]).sum() == 30
    assert not G.zero_area(c["soup272"]).any()
    for ax, nm in enumerate("xyz"):
        assert (c[f"flat_{nm}"][:, :, ax] == 0.0).all() and np.ptp(c[f"flat_{nm}"][:, :, (ax + 1) % 3]) > 0.5
    col = c["collinear_centroids"]
    centre = np.float32(0.5) * (col.min(1) + col.max(1))  # the build's centroid: the box centre
    assert (centre[:, :2] == 0.5).all() and np.ptp(centre[:, 2]) > 0.5
    for name, nq in (("uniform_strip", 256), ("uniform_sheet", 256)):
        q = c[name].reshape(nq, 6, 3)
        ext = q.max(1) - q.min(1)
        assert c[name].shape[0] == 512 and (ext == ext[0]).all()
    assert (np.diff(c["uniform_strip"].reshape(256, 6, 3).min(1)[:, 0]) == 1.0 / 16).all()
    assert c["one_cell"].shape[0] == 502
    assert G.ray_range(c["soup272"]) == (1e-3, 1e7) and G.ray_range(c["uniform_sheet"]) == (1e-3, 1e7)
    assert G.ray_range(c["scaled_1e-4"]) == (1e-5, 1e5) and G.ray_range(c["scaled_1e4"]) == (10.0, 1e11)


@pytest.mark.parametrize("group", range(8))
def test_rays_hit_and_miss(group):
    """By the linear scan alone: at least 20% of a case's rays hit and at least
    5% miss; coincident triangles answer index 0; a zero-area triangle is
    never the answer.  (The cases in eight groups, to keep the ids short.)"""
    names = list(_CASES)[group::8]
    for name in names:
        tris = _CASES[name]
        rays, rng = G.rays(tris, N_RAYS, 1)
        ids, hits = _scan(tris, rays, rng)
        frac = (ids >= 0).mean()
        assert 0.20 <= frac <= 0.95, (name, frac)
        if name.startswith("coincident"):
            assert (ids <= 0).all(), name
        assert not G.zero_area(tris)[ids[ids >= 0]].any(), name
