"""call_kinds.pin notices one flipped word, shown without a GPU for the kinds
whose pin is a comparison with a reference the CPU can compute: the result the
reference itself predicts passes its pin, and the same result with one bit of
one array flipped does not -- for every array of the result.  The kinds whose
pin needs device-made inputs or a fresh scene's dump (temporal,
temporal_clip_aux, sample_plan, denoise_moments, update_refit_back,
update_rebuild_back, octree_device_rebuild) are shown the same way on their
recorded baselines in test_gpu_call_order.py::test_pin_notices_one_flipped_word,
which covers these eight too.
"""
import numpy as np
import pytest

import adaptive_nb_restate
import call_kinds as K
import guided_restate
import noise_aware_restate
import render_restate
import temporal_restate
import toymeshpathtracer_amd as tm
from call_order import Result

f32 = np.float32


def _moments_result(want, col):
    n_p, rad, total, pass_pixels = want
    rad4 = np.concatenate([rad, np.ones(rad.shape[:2] + (1,), f32)], -1)
    stats = dict(passes=len(pass_pixels), samples=int(n_p.sum()), pass_pixels=tuple(pass_pixels))
    mom = noise_aware_restate.moments_expect(col, n_p)
    return Result({"radiance": rad4, "moments": mom, "image": render_restate.pack(rad4), "spp_map": n_p.astype(np.int32)},
                  total, stats)


def predicted(name, wd):
    """The Result the kind's reference predicts at the base size on the definition `wd`."""
    w, h, spp = K.BASE
    if name in ("moments_uniform", "moments_adaptive", "guided"):
        col, rays = K.sample_colours(wd.name, (w, h), spp + 8)
        if name == "moments_uniform":
            rad, total = render_restate.radiance_sum(col, rays, spp)
            return _moments_result((np.full((h, w), spp, np.int32), rad, total, [w * h]), col)
        if name == "moments_adaptive":
            return _moments_result(adaptive_nb_restate.adaptive_nb_expect(col, rays, *K.ADAPTIVE, 1, 4), col)
        prior = guided_restate.synthetic_prior(col[:, :, :8], K.GUIDED_N_MAX)
        res = _moments_result(guided_restate.guided_expect(col, rays, *K.GUIDED, prior), col)
        res.arrays["prior"] = prior
        return res
    if name == "motion_host_prev":
        rec = K.motion_expect(wd, wd.camera(w, h).as_array(), wd.prev_camera(w, h).as_array(), w, h, wd.moved)
        return Result({"records": rec.astype(tm.MOTION_DTYPE)}, w * h, dict(extend_rays=w * h, extend_launches=1))
    if name == "sample_waves6":
        img, rays = K.oracle_frame(wd.name, K.BASE, tm.SEED_SAMPLE)
        used = (6, 1) if wd.name == "coincident64" else (5, 0)
        return Result({"image": img}, rays, route=dict(path_waves_used=used[0], shadow_split_used=used[1], cam_rays_used=1))
    if name == "sample_based":
        col, rays = K.sample_colours(wd.name, (w, h), K.SAMPLE_BASE + spp)
        rad, total = render_restate.radiance_sum(col[:, :, K.SAMPLE_BASE:], rays[:, :, K.SAMPLE_BASE:])
        return Result({"image": render_restate.pack(rad)}, total)
    if name == "hit_device_closest":
        rays, (tmin, tmax), _ = wd.hit_rays
        ids, hits = wd.osc.hit_batch(rays, tmin, tmax)
        hits = np.where((ids >= 0)[:, None], hits, f32(0)).astype(f32)
        return Result({"ids": ids, "hits": hits, "uv": K.mt_uv(rays, wd.tris, ids)}, route=dict(query_sorted=0))
    assert name == "hit_device_any_sorted"
    _, _, r8 = wd.hit_rays
    hit = np.zeros(len(r8), np.uint8)
    for lo, hi in {(float(a), float(b)) for a, b in r8[:, 6:8]}:
        sel = np.nonzero((r8[:, 6] == f32(lo)) & (r8[:, 7] == f32(hi)))[0]
        hit[sel] = wd.osc.hit_batch(r8[sel, :6], lo, hi)[0] >= 0
    return Result({"hit": hit}, route=dict(query_sorted=1))


CPU_KINDS = ("moments_uniform", "moments_adaptive", "guided", "motion_host_prev", "hit_device_closest",
             "hit_device_any_sorted", "sample_waves6", "sample_based")


def flipped(a):
    """A copy of the array with the lowest bit of its middle 4-byte word flipped."""
    b = np.array(a, copy=True)
    words = b.view(np.uint8).reshape(-1)
    words[(words.size // 2) & ~3] ^= 1
    return b


@pytest.mark.parametrize("name", CPU_KINDS)
def test_pin_passes_the_prediction_and_notices_one_flipped_word(name):
    wd = K.world(K.KINDS[name].world)
    res = predicted(name, wd)
    K.pin(name, res, wd.name, K.BASE)
    assert res.arrays
    for key, a in res.arrays.items():
        bad = Result(dict(res.arrays, **{key: flipped(a)}), res.rays, res.stats, res.route, res.seen)
        with pytest.raises(AssertionError):
            K.pin(name, bad, wd.name, K.BASE)
    if res.rays is not None:
        with pytest.raises(AssertionError):
            K.pin(name, Result(res.arrays, res.rays + 1, res.stats, res.route, res.seen), wd.name, K.BASE)


def test_the_guided_restatement_stops_some_pixels_at_two_and_not_others():
    """The guided kind's marker, from the restatement alone, on both definitions at the base size."""
    w, h, spp = K.BASE
    for wname in K.WORLDS:
        col, rays = K.sample_colours(wname, (w, h), spp + 8)
        prior = guided_restate.synthetic_prior(col[:, :, :8], K.GUIDED_N_MAX)
        n_p = guided_restate.guided_expect(col, rays, *K.GUIDED, prior)[0]
        assert (n_p == 2).any() and (n_p > 2).any(), (wname, np.unique(n_p))
        plain = guided_restate.guided_expect(col, rays, *K.GUIDED)[0]
        assert (n_p != plain).any(), wname  # and the prior decides some of them


def test_motion_expect_is_the_restatement_where_no_centre_ray_is_tied():
    w, h, _ = K.BASE
    wd = K.world("suzanne")
    cam, pcam = wd.camera(w, h).as_array(), wd.prev_camera(w, h).as_array()
    got = K.motion_expect(wd, cam, pcam, w, h, wd.moved)
    want = temporal_restate.motion(wd.tris, cam, pcam, w, h, wd.moved)
    assert got.tobytes() == want.tobytes() and (want["flags"] & 2).any() and (want["tri_id"] < 0).any()
