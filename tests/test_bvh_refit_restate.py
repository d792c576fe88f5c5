"""The restated refit (bvh_refit_restate.py) proved on the CPU, over the restated builds.

(a) identity: a refit with unchanged triangles reproduces the built node words, records
    and info bit for bit -- the refit's one right answer is the build's own encoding;
(b) every deformed refit passes all of bvh_check.check (leaf-greedy too: the rule counts
    triangles, not boxes), and no node extent lies near an exponent boundary,
    where the device's double-precision log2 could differ: the device comparison
    (test_gpu_scene_update.py) makes no exception for it;
(c) two wrong refits are seen by the checker as box-contain findings: one parent's
    planes left stale, and U taken from the unpadded boxes.
"""
import functools

import numpy as np
import pytest

import bvh_build_restate as R
import bvh_check as B
import bvh_refit_restate as F

CASES = ("soup3", "soup4", "soup64", "soup257", "soup1025", "soup4096", "coincident64", "one_cell", "nested200",
         "uniform_sheet", "translated_1e2")
OPTION_SETS = ({}, {"leaf_max": 4}, {"collapse": "sah"})


@functools.lru_cache(maxsize=None)
def _tris(name):
    t = R.case_tris(name)
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("name", CASES)
def test_identity_and_deformed_refits(name):
    tris = _tris(name)
    for opts in OPTION_SETS:
        built = R.cached_build(name, tris, opts)
        tag = f"{name} [{R.opt_id(opts)}]"
        same = F.refit(built, tris)
        assert np.array_equal(same["nodes"], built["nodes"]), f"{tag}: identity changes node words"
        assert np.array_equal(same["tris"], built["tris"]) and same["info"] == built["info"], tag
        for dname, deform in F.DEFORMATIONS.items():
            new = deform(tris)
            assert new.dtype == np.float32 and new.shape == tris.shape
            out = F.refit(built, new)
            bad = B.check(new, out, opts)
            assert not bad, f"{tag} {dname}: " + "\n".join(bad[:5])
            assert out["near_exponent_boundary"] == 0, f"{tag} {dname}: replace this case"
            # what a refit must not touch
            assert np.array_equal(out["nodes"][:, 12:16], built["nodes"][:, 12:16])
            assert np.array_equal(out["nodes"][:, 3] >> 24, built["nodes"][:, 3] >> 24)
            assert np.array_equal(out["tris"][:, 9:], built["tris"][:, 9:]) and out["info"] == built["info"]


def test_the_deformations_deform():
    tris = _tris("soup257")
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    tw = F.twist(tris)
    y = tris[..., 1]
    low, high = y == y.min(), y == y.max()
    assert np.array_equal(tw[low], tris[low])  # nothing at the bottom
    c = (0.5 * (lo.astype(np.float64) + hi)).astype(np.float64)
    top, was = tw[high][0].astype(np.float64) - c, tris[high][0].astype(np.float64) - c
    assert np.allclose([top[0], top[2]], [was[2], -was[0]], atol=1e-6)  # the quarter turn at the top
    assert np.array_equal(tw[..., 1], tris[..., 1])
    assert np.array_equal(F.twist(tris, 0.0), tris)
    j = F.jitter(tris)
    assert 0 < np.abs(j - tris).max() <= 0.05 * (hi - lo).max() * 1.0001
    p = F.permuted(tris)
    assert not np.array_equal(p, tris)
    assert np.array_equal(np.sort(p.reshape(-1, 9), 0), np.sort(tris.reshape(-1, 9), 0))
    assert len(np.unique(F.one_point(tris).reshape(-1, 3), axis=0)) == 1
    f = F.flat_y(tris)
    assert (f[..., 1] == np.float32(0.25)).all() and np.array_equal(f[..., [0, 2]], tris[..., [0, 2]])


@pytest.mark.parametrize("mut", sorted(F.MUTATIONS))
@pytest.mark.parametrize("dname", ("twist90", "jitter5"))
def test_the_checker_sees_a_wrong_refit(mut, dname):
    tris = _tris("soup257")
    built = R.cached_build("soup257", tris, {})
    new = F.DEFORMATIONS[dname](tris)
    assert B.check(new, F.refit(built, new), {}) == []
    bad = B.check(new, F.refit(built, new, mut=mut), {})
    assert any(b.startswith("box-contain") for b in bad), f"{mut}: {bad[:3]}"
