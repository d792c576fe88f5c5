"""The host form and the device form of every staged frame call agree bit for bit,
and a host-form call on a warmed scene leaves `live_device_objects` where it was.

The host form stages its frames on the device (DESIGN.md "Owners", Staging): in a
buffer of the call's own (the render calls, denoise, temporal) or in one the scene
keeps (temporal_clip and sample_plan, trace_motion's previous pose).  Shapes: the
render calls at 24 x 10, 4 spp, band_rows = 3 and two shards, each in turn (6 and 4
tile rows, the last band partial); the whole-frame calls at 24 x 10 and then at
8 x 4 on the same scene, so the kept buffer is reused by a smaller frame.
Tolerance: none.
"""
import numpy as np
import pytest

import toymeshpathtracer_amd as tm
from test_gpu_temporal import _mesh, synthetic

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, SPP = 24, 10, 4


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def blank(like):
    import torch

    return torch.full((like.nbytes,), 7, dtype=torch.uint8, device="cuda:0")


def same(t, want, what):
    assert t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes(), what


def steady(sc, call, what):
    """call() once to warm the scene, then again: the second leaves the live objects as they were."""
    call()
    before = sc.get_option("live_device_objects")
    res = call()
    assert sc.get_option("live_device_objects") == before, what
    return res


@pytest.mark.parametrize("shard", [0, 1])
def test_render_calls_host_and_device_agree(gpu, shard):
    import bvh_refit_restate as F

    tris, bmin, bmax = _mesh("cube.obj")
    cam = tm.Camera.for_scene(bmin, bmax, W, H)
    tile = dict(band_rows=3, shard=shard, num_shards=2)
    rows = tm.tile_rows(W, H, **tile)
    assert rows == (6, 4)[shard]
    rng = np.random.default_rng(5)
    prior = rng.random((H, W, 4)).astype(f32)
    prior[..., 2] = f32(1.0) - prior[..., 2] * f32(0.75)  # the blend factor, in (0.25, 1]
    prior[..., 3] = np.floor(prior[..., 3] * 4)            # the history length
    prev = F.twist(tris, 10.0)
    with tm.Scene(tris) as sc:
        img, rays = steady(sc, lambda: sc.trace_image(cam, W, H, SPP, seed_mode=tm.SEED_SAMPLE, **tile), "trace_image")
        assert img.shape == (rows, W, 4)
        t = blank(img)
        assert sc.trace_image(cam, W, H, SPP, seed_mode=tm.SEED_SAMPLE, out=t.data_ptr(), **tile) == (None, rays)
        same(t, img, "trace_image")

        rec, rays = steady(sc, lambda: sc.trace_aov(cam, W, H, SPP, **tile), "trace_aov")
        t = blank(rec)
        assert sc.trace_aov(cam, W, H, SPP, out=t.data_ptr(), **tile) == (None, rays)
        same(t, rec, "trace_aov")

        rad, img, rays = steady(sc, lambda: sc.trace_radiance(cam, W, H, SPP, **tile), "trace_radiance")
        t32, t8 = blank(rad), blank(img)
        assert sc.trace_radiance(cam, W, H, SPP, out=(t32.data_ptr(), t8.data_ptr()), **tile) == (None, None, rays)
        same(t32, rad, "trace_radiance")
        same(t8, img, "trace_radiance, bytes")
        t32 = blank(rad)
        sc.trace_radiance(cam, W, H, SPP, out=t32.data_ptr(), **tile)  # the library's own rgba8 tile
        same(t32, rad, "trace_radiance, float tile alone")

        ad = dict(spp_min=2, spp_step=1, threshold=0.02)
        rad, img, cnt, rays, info = steady(sc, lambda: sc.trace_adaptive(cam, W, H, SPP, **ad, **tile), "trace_adaptive")
        t32, t8, tn = blank(rad), blank(img), blank(cnt)
        res = sc.trace_adaptive(cam, W, H, SPP, out=(t32.data_ptr(), t8.data_ptr(), tn.data_ptr()), **ad, **tile)
        assert res == (None, None, None, rays, info)
        for got, want, what in ((t32, rad, "radiance"), (t8, img, "bytes"), (tn, cnt, "map")):
            same(got, want, "trace_adaptive, " + what)

        for name, call in (("trace_moments", lambda **kw: sc.trace_moments(cam, W, H, SPP, **ad, **tile, **kw)),
                           ("trace_guided", lambda **kw: sc.trace_guided(cam, W, H, SPP, prior, **ad, **tile, **kw))):
            rad, mom, img, cnt, rays, info = steady(sc, call, name)
            ts = [blank(a) for a in (rad, mom, img, cnt)]
            assert call(out=tuple(x.data_ptr() for x in ts)) == (None, None, None, None, rays, info)
            for got, want, what in zip(ts, (rad, mom, img, cnt), ("radiance", "moments", "bytes", "map")):
                same(got, want, f"{name}, {what}")

        rec, rays = steady(sc, lambda: sc.trace_motion(cam, cam, W, H, prev, **tile), "trace_motion")
        assert (rec["tri_id"] >= 0).any()
        t, t_prev = blank(rec), dev(prev)
        assert sc.trace_motion(cam, cam, W, H, t_prev.data_ptr(), out=t.data_ptr(), **tile) == (None, rays)
        same(t, rec, "trace_motion")


def test_frame_calls_host_and_device_agree(gpu):
    tris, bmin, bmax = _mesh("cube.obj")
    with tm.Scene(tris) as sc:
        for w, h in ((W, H), (8, 4)):  # the second, smaller frame reuses what the first one grew
            size = dict(width=w, height=h)
            cam = tm.Camera.for_scene(bmin, bmax, w, h)
            rad = sc.trace_moments(cam, w, h, SPP)
            rad, mom = rad[0], rad[1]
            aov = sc.trace_aov(cam, w, h, SPP)[0]
            cur, mot, pmot, hist = synthetic(w, h)
            rng = np.random.default_rng(w)
            stat, aux, aux_hist = ((rng.random((h, w, 4)) * 4).astype(f32) for _ in range(3))
            what = f"{w}x{h}"

            for name, call, args in (("denoise", sc.denoise, (rad, aov)), ("denoise_moments", sc.denoise_moments, (rad, aov, mom))):
                res, img = steady(sc, lambda: call(*args, SPP), name)
                t32, t8 = blank(res), blank(img)
                ins = [dev(a) for a in args]
                assert call(*[x.data_ptr() for x in ins], SPP, out=(t32.data_ptr(), t8.data_ptr()), **size) == (None, None)
                same(t32, res, f"{name} {what}")
                same(t8, img, f"{name} {what}, bytes")

            res, img = steady(sc, lambda: sc.temporal(cur, mot, pmot, hist), "temporal")
            t32, t8 = blank(res), blank(img)
            ins = [dev(a) for a in (cur, mot, pmot, hist)]
            assert sc.temporal(*[x.data_ptr() for x in ins], out=(t32.data_ptr(), t8.data_ptr()), **size) == (None, None)
            same(t32, res, f"temporal {what}")
            same(t8, img, f"temporal {what}, bytes")

            plan = steady(sc, lambda: sc.sample_plan(mot, pmot, hist), "sample_plan")
            tp = blank(plan)
            ins = [dev(a) for a in (mot, pmot, hist)]
            assert sc.sample_plan(*[x.data_ptr() for x in ins], out=tp.data_ptr(), **size) is None
            same(tp, plan, f"sample_plan {what}")

            for kw in (dict(stat=stat, aux=aux, aux_history=aux_hist), dict()):  # the most frames staged, and the fewest
                res, img, aux_res = steady(sc, lambda: sc.temporal_clip(cur, mot, pmot, hist, **kw), "temporal_clip")
                assert (aux_res is None) == (not kw)
                t32, t8, ta = blank(res), blank(img), blank(res) if kw else None
                ins = [dev(a) for a in (cur, mot, pmot, hist)]
                dkw = {k: dev(v) for k, v in kw.items()}
                out = (t32.data_ptr(), t8.data_ptr(), ta.data_ptr() if kw else None)
                assert sc.temporal_clip(*[x.data_ptr() for x in ins], out=out, **{k: v.data_ptr() for k, v in dkw.items()},
                                        **size) == (None, None, None)
                same(t32, res, f"temporal_clip {what} {sorted(kw)}")
                same(t8, img, f"temporal_clip {what} {sorted(kw)}, bytes")
                if kw:
                    same(ta, aux_res, f"temporal_clip {what}, aux")
