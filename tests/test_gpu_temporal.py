"""Temporal accumulation on the device: render option sample_base, the motion
pass (tmpt_render_motion / Scene.trace_motion) and the reprojected history
(tmpt_temporal / Scene.temporal).

1  sample_base is the stream's window: against the reference's own per-sample
   values (tests/golden/ref/trace_cube.npz, trace_room.npz), bit for bit;
2  motion records are bit for bit those of tests/temporal_restate.py (proved on
   the CPU by test_temporal_restate.py), on scenes without an octree, so that
   closest hits tied on t take the lowest index as the restatement's scan does;
3  the blend is bit for bit the restatement's, on synthetic and on real frames;
4  it accumulates: eight 1-spp frames blended in turn are closer to the 512-spp
   frame than one 1-spp frame, static and over a twist with refits;
5  neither call disturbs a progressive render; the CLI's --temporal; the checked
   build computes the same bits and reports no failed index check.

Tolerance: none, except in 4, which asserts an inequality.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bvh_refit_restate as F
import ref_cases as C
import temporal_restate as T
import toymeshpathtracer_amd as tm
from conftest import ROOT, data
from render_restate import aov_sums, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")


def _same_records(got, want, what):
    assert got.dtype == tm.MOTION_DTYPE and got.shape == want.shape, what
    for name in tm.MOTION_DTYPE.names:
        a = np.ascontiguousarray(got[name]).view(np.uint32)
        b = np.ascontiguousarray(want[name]).view(np.uint32)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}: {name}: {len(bad)} of {a.size} differ, first at {bad[0]}: " \
                              f"{got[name][tuple(bad[0])]!r} vs {want[name][tuple(bad[0])]!r}"


# ---------------------------------------------------------------- 1  sample_base
@functools.lru_cache(maxsize=None)
def _trace_case(name):
    fx = C.load_trace(name)
    w, h, spp = (int(v) for v in fx["size"])
    n = (h, w, spp)
    a = [float(v) for v in fx["cam"]]
    return dict(fx=fx, w=w, h=h, spp=spp, col=fx["s_col"].reshape(n + (3,)), rays=fx["s_rays"].reshape(n).astype(np.int64),
                hit=fx["s_hit"].reshape(n).astype(bool), t=fx["s_tn"][:, 0].reshape(n),
                nrm=fx["s_tn"][:, 1:4].reshape(n + (3,)),
                cam=tm.Camera.create(a[0:3], a[3:6], a[6:9], a[9], a[10], a[11], a[12]))


@pytest.mark.parametrize("name", ["cube", "room"])
def test_sample_base_is_the_streams_window(gpu, name):
    c = _trace_case(name)
    fx, w, h, cam = c["fx"], c["w"], c["h"], c["cam"]
    with tm.Scene(fx["tris"], bounds=(fx["bmin"], fx["bmax"])) as sc:
        assert sc.get_option("sample_base") == 0
        first, first8, first_rays = sc.trace_radiance(cam, w, h, 4)  # before the option is touched
        for k in range(c["spp"]):
            sc.set_option("sample_base", k)
            rad, _, rays = sc.trace_radiance(cam, w, h, 1)
            same_bits(rad[..., :3], c["col"][:, :, k], f"{name} sample_base {k}, spp 1")
            assert rays == int(c["rays"][:, :, k].sum()), (name, k)
            rec, arays = sc.trace_aov(cam, w, h, 1)
            nrm, depth, hits = aov_sums(c["hit"][:, :, k:k + 1], c["nrm"][:, :, k:k + 1], c["t"][:, :, k:k + 1], 1)
            assert np.array_equal(rec["hits"], hits), (name, k)
            same_bits(rec["depth"], depth, f"{name} aov depth at sample_base {k}")
            same_bits(rec["normal"], nrm, f"{name} aov normal at sample_base {k}")
            assert arays == w * h + int(hits.sum())
            img, irays = sc.trace_image(cam, w, h, 1, seed_mode=tm.SEED_SAMPLE)
            assert np.array_equal(img, T.pack(rad)) and irays == rays
        sc.set_option("sample_base", 3)
        rad, _, rays = sc.trace_radiance(cam, w, h, 4)
        col = c["col"]
        want = (((col[:, :, 3] + col[:, :, 4]) + col[:, :, 5]) + col[:, :, 6]) * f32(0.25)
        same_bits(rad[..., :3], want, f"{name} sample_base 3, spp 4")
        assert rays == int(c["rays"][:, :, 3:7].sum())
        sc.set_option("sample_base", 0)
        rad, img, rays = sc.trace_radiance(cam, w, h, 4)
        assert rad.tobytes() == first.tobytes() and np.array_equal(img, first8) and rays == first_rays
        # row and pixel seeding do not read the option
        px0 = sc.trace_image(cam, w, h, 2, seed_mode=tm.SEED_PIXEL)
        row0 = sc.trace_image(cam, w, h, 2, seed_mode=tm.SEED_ROW)
        sc.set_option("sample_base", 5)
        px5 = sc.trace_image(cam, w, h, 2, seed_mode=tm.SEED_PIXEL)
        row5 = sc.trace_image(cam, w, h, 2, seed_mode=tm.SEED_ROW)
        assert np.array_equal(px0[0], px5[0]) and px0[1] == px5[1]
        assert np.array_equal(row0[0], row5[0]) and row0[1] == row5[1]
        # a progressive pass does not continue across a change of base; a fresh sequence does
        passes = sc.trace_progressive(cam, w, h, 8, [3, 5], seed_mode=tm.SEED_SAMPLE)
        next(passes)
        sc.set_option("sample_base", 5)  # the same value: nothing is invalidated
        done, last, _ = next(passes)
        assert done == 8
        passes = sc.trace_progressive(cam, w, h, 8, [3, 5], seed_mode=tm.SEED_SAMPLE)
        next(passes)
        sc.set_option("sample_base", 6)
        with pytest.raises(tm.TmptError, match="does not continue"):
            next(passes)
        whole, _ = sc.trace_image(cam, w, h, 8, seed_mode=tm.SEED_SAMPLE)
        done = [p for p in sc.trace_progressive(cam, w, h, 8, [3, 5], seed_mode=tm.SEED_SAMPLE)]
        assert np.array_equal(done[-1][1], whole)
        for bad in (-1, 64513, 0.5):
            with pytest.raises(tm.TmptError):
                sc.set_option("sample_base", bad)
        sc.set_option("sample_base", 64512)
        assert sc.get_option("sample_base") == 64512
        far, _, _ = sc.trace_radiance(cam, w, h, 1)
        assert np.isfinite(far).all() and far[..., :3].tobytes() != c["col"][:, :, 0].tobytes()


# ---------------------------------------------------------------- 2  motion records
@functools.lru_cache(maxsize=None)
def _mesh(name):
    tris, bmin, bmax = tm.load_scene(data(name))
    tris.setflags(write=False)
    return tris, bmin, bmax


def _moved_camera(bmin, bmax, w, h):
    lo, hi = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
    c, s = 0.5 * (lo + hi), hi - lo
    return tm.Camera.create(list(c + s * [0.45, 0.5, 1.25]), list(c + s * [0.05, -0.05, 0.0]), [0.0, 1.0, 0.0], 60.0, w / h,
                            0.0, 1.0)


MOTION_CASES = {
    # name: (obj, w, h, twist degrees or None, moved previous camera, scene options)
    "cube_static": ("cube.obj", 32, 18, None, False, None),
    "suzanne_twist": ("suzanne.obj", 64, 36, 10.0, False, None),
    "suzanne_camera": ("suzanne.obj", 64, 36, None, True, None),
    "cube_1x1": ("cube.obj", 1, 1, None, True, None),
    "cube_5x3": ("cube.obj", 5, 3, 10.0, True, None),
    "suzanne_soa": ("suzanne.obj", 64, 36, 10.0, True, {"layout": "soa"}),
}


@functools.lru_cache(maxsize=None)
def _motion_case(name):
    obj, w, h, deg, moved, opts = MOTION_CASES[name]
    rest, bmin, bmax = _mesh(obj)
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    prev_cam = _moved_camera(bmin, bmax, w, h) if moved else cam
    now = F.twist(rest, deg) if deg else rest
    want = T.motion(now, cam.as_array(), prev_cam.as_array(), w, h, rest if deg else None)
    want.setflags(write=False)
    return rest, now, cam, prev_cam, want


@pytest.mark.parametrize("name", list(MOTION_CASES))
def test_motion_records_bit_for_bit(gpu, name):
    obj, w, h, deg, moved, opts = MOTION_CASES[name]
    rest, now, cam, prev_cam, want = _motion_case(name)
    hit = want["tri_id"] >= 0
    if w * h > 1:
        assert hit.any() and ((want["flags"] & 2) != 0).any()
    with tm.Scene(rest, options=opts) as sc:  # no octree: ties take the lowest index
        if deg:
            sc.update(now, "refit")
        prev = rest if deg else None
        for tile in (-1, 0, 1):
            sc.set_option("motion_tile", tile)
            rec, rays = sc.trace_motion(cam, prev_cam, w, h, prev)
            _same_records(rec, want, f"{name} motion_tile {tile}")
            st = sc.stats()
            assert rays == w * h and st.extend_rays == w * h and st.extend_launches == 1 and st.shadow_rays == 0
            assert st.render_ms > 0 and st.extend_ms == st.render_ms
        sc.set_option("sample_base", 9)  # the pass draws nothing
        rec, _ = sc.trace_motion(cam, prev_cam, w, h, prev)
        _same_records(rec, want, f"{name} sample_base 9")


def test_motion_tiles_assemble(gpu):
    name = "suzanne_twist"
    _, w, h, _, _, _ = MOTION_CASES[name]
    rest, now, cam, prev_cam, want = _motion_case(name)
    with tm.Scene(rest) as sc:
        sc.update(now, "refit")
        for band, ns in ((4, 3), (1, 2), (5, 4)):
            got = np.zeros((h, w), tm.MOTION_DTYPE)
            seen = np.zeros(h, int)
            for shard in range(ns):
                for tile in (0, 1):
                    sc.set_option("motion_tile", tile)
                    rec, rays = sc.trace_motion(cam, prev_cam, w, h, rest, band_rows=band, shard=shard, num_shards=ns)
                    ys = tm.tile_row_to_y(w, h, band, shard, ns)
                    assert rec.shape == (len(ys), w) and rays == len(ys) * w
                    got[ys] = rec
                seen[ys] += 1
            assert (seen == 1).all()
            _same_records(got, want, f"band_rows {band}, {ns} shards")


def test_motion_device_pointers_and_owners(gpu):
    import torch

    name = "suzanne_twist"
    _, w, h, _, _, _ = MOTION_CASES[name]
    rest, now, cam, prev_cam, want = _motion_case(name)
    with tm.Scene(rest) as probe:
        live0 = probe.get_option("live_device_objects")
        with tm.Scene(rest) as sc:
            sc.update(now, "refit")
            sc.trace_motion(cam, prev_cam, w, h)  # no upload: no kept buffer
            live1 = sc.get_option("live_device_objects")
            rec, _ = sc.trace_motion(cam, prev_cam, w, h, rest)
            live2 = sc.get_option("live_device_objects")
            assert live2 == live1 + 1  # the kept copy of the previous pose
            for _ in range(3):
                again, _ = sc.trace_motion(cam, prev_cam, w, h, rest)
                assert sc.get_option("live_device_objects") == live2
            assert again.tobytes() == rec.tobytes()
            t_prev = torch.from_numpy(np.ascontiguousarray(rest, f32).reshape(-1, 9).copy()).to("cuda:0")
            t_out = torch.full((h, w, 8), 7.0, dtype=torch.float32, device="cuda:0")
            none, rays = sc.trace_motion(cam, prev_cam, w, h, t_prev.data_ptr(), out=t_out.data_ptr())
            assert none is None and rays == w * h
            assert t_out.cpu().numpy().tobytes() == rec.tobytes() == want.tobytes()
            # a device pose is read where it lies (no copy); the one new object is the scene's
            # wait event of TMPT_FLAG_WAIT_STREAM, made once
            live3 = sc.get_option("live_device_objects")
            assert live3 == live2 + 1
            sc.trace_motion(cam, prev_cam, w, h, t_prev.data_ptr(), out=t_out.data_ptr())
            sc.trace_motion(cam, prev_cam, w, h, rest)
            assert sc.get_option("live_device_objects") == live3
            with pytest.raises(tm.TmptError, match="prev_n"):
                sc.trace_motion(cam, prev_cam, w, h, rest[:-1])
            with pytest.raises(tm.TmptError, match="aligned"):
                sc.trace_motion(cam, prev_cam, w, h, t_prev.data_ptr(), out=t_out.data_ptr() + 8)
        assert probe.get_option("live_device_objects") == live0


# ---------------------------------------------------------------- 3  the blend
def synthetic(w, h, seed=1):
    """Random frames and records with every branch of the blend: reprojections
    that are NaN, +-inf, far outside, on the frame's edges and range ends, exactly
    on pixel centres and in between; depths that match, mismatch, sit at the
    tolerance and are NaN; flags 0, 1 and 3 in both frames' records; history
    lengths 1 .. 40."""
    rng = np.random.default_rng(seed * 1000 + w * 37 + h)
    n = w * h
    cur = (rng.random((h, w, 4)) * 4).astype(f32)
    hist = (rng.random((h, w, 4)) * 4).astype(f32)
    hist[..., 3] = rng.integers(1, 41, (h, w)).astype(f32)
    y, x = np.mgrid[0:h, 0:w]
    mot, pmot = np.zeros((h, w), tm.MOTION_DTYPE), np.zeros((h, w), tm.MOTION_DTYPE)
    mot["px"] = (x + 0.5 + rng.normal(0, 1.5, (h, w))).astype(f32)
    mot["py"] = (y + 0.5 + rng.normal(0, 1.5, (h, w))).astype(f32)
    centre = rng.random((h, w)) < 0.2  # exactly on a pixel centre, this one's or a neighbour's
    mot["px"][centre] = (x + 0.5 + rng.integers(-1, 2, (h, w)))[centre].astype(f32)
    mot["py"][centre] = (y + 0.5 + rng.integers(-1, 2, (h, w)))[centre].astype(f32)
    depth = (3 + rng.random((h, w))).astype(f32)
    pmot["depth"] = depth
    mot["depth"] = (depth * (1 + rng.normal(0, 0.01, (h, w)))).astype(f32)
    dp = depth * (1 + rng.normal(0, 0.03, (h, w)))  # around the 5 % tolerance of the default
    mot["depth_prev"] = dp.astype(f32)
    mot["flags"] = rng.choice([0, 1, 3, 3, 3, 3], (h, w)).astype(np.uint32)
    pmot["flags"] = rng.choice([0, 1, 3, 3, 3, 3], (h, w)).astype(np.uint32)
    mot["tri_id"] = rng.integers(-1, 50, (h, w))
    mot["u"], mot["v"] = rng.random((h, w)).astype(f32), rng.random((h, w)).astype(f32)
    specials = [(np.nan, 1.5), (1.5, np.nan), (np.inf, 1.5), (-np.inf, 1.5), (1.5, np.inf), (1e9, 1.5), (1.5, -1e9),
                (-1.0, 0.5), (-1.0000001, 0.5), (w + 1.0, 0.5), (np.nextafter(f32(w + 1), f32(0)), 0.5), (0.0, 0.0),
                (0.5, h + 1.0), (0.5, np.nextafter(f32(h + 1), f32(0))), (w, h), (w + 0.5, h + 0.5), (w - 0.5, h - 0.5),
                (0.5, 0.5), (-0.5, -0.5), (-0.999, -0.999), (0.25, h - 0.25)]
    flat = rng.permutation(n)
    for k, (sx, sy) in enumerate(specials):
        p = np.unravel_index(flat[k % n], (h, w))
        mot["px"][p], mot["py"][p], mot["flags"][p] = sx, sy, 3
    q = np.unravel_index(flat[(len(specials)) % n], (h, w))
    pmot["depth"][q] = np.nan
    mot["depth_prev"][np.unravel_index(flat[(len(specials) + 1) % n], (h, w))] = np.nan
    return cur, mot, pmot, hist


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (37, 23), (130, 9)])
def test_synthetic_blend_bit_for_bit(gpu, w, h):
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as sc:
        for seed in (1, 2, 3) if w * h < 100 else (1,):
            cur, mot, pmot, hist = synthetic(w, h, seed)
            for n_max, sigma in ((0.0, 0.0), (8.0, 0.02), (1.0, 0.5), (64.0, 0.0)):
                want = T.blend(cur, mot, pmot, hist, n_max, sigma)
                got, img = sc.temporal(cur, mot, pmot, hist, n_max=n_max, sigma_depth=sigma)
                what = f"{w}x{h} seed {seed} n_max {n_max} sigma_depth {sigma}"
                same_bits(got, want, what)
                assert np.array_equal(img, T.pack(want)), what
                assert (got[..., 3] <= (n_max or float(T.N_MAX_DEFAULT))).all()
                buf = cur.copy()
                res, img2 = sc.temporal(buf, mot, pmot, hist, n_max=n_max, sigma_depth=sigma, out=buf)  # out = cur
                assert res is buf and buf.tobytes() == got.tobytes() and np.array_equal(img2, img)
            if w * h > 100:  # the branches are all there
                want = T.blend(cur, mot, pmot, hist)
                reset = (want[..., 3] == 1) & (want[..., :3] == cur[..., :3]).all(-1)
                cap = T.N_MAX_DEFAULT
                assert reset.any() and not reset.all() and (want[..., 3] == cap).any()
                assert ((want[..., 3] > 1) & (want[..., 3] < cap)).any()
            same_bits(sc.temporal(cur, mot, pmot, hist)[0], T.blend(cur, mot, pmot, hist, 3.0, 0.05), "defaults spelled out")
        with pytest.raises(tm.TmptError, match="overlaps"):
            sc.temporal(cur, mot, pmot, hist, out=hist)


@functools.lru_cache(maxsize=None)
def _twist_pair():
    """suzanne at rest and twisted by 10 degrees, 64 x 36: radiance at 2 spp (sample_base 0 and 2), motion records."""
    w, h, spp = 64, 36, 2
    rest, bmin, bmax = _mesh("suzanne.obj")
    now = F.twist(rest, 10.0)
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(rest) as sc:
        rad0, _, _ = sc.trace_radiance(cam, w, h, spp)
        mot0, _ = sc.trace_motion(cam, cam, w, h)
        sc.update(now, "refit")
        sc.set_option("sample_base", spp)
        rad1, _, _ = sc.trace_radiance(cam, w, h, spp)
        mot1, _ = sc.trace_motion(cam, cam, w, h, rest)
    return w, h, rad0, mot0, rad1, mot1


def test_real_frames_blend_bit_for_bit(gpu):
    import torch

    w, h, rad0, mot0, rad1, mot1 = _twist_pair()
    want = T.blend(rad1, mot1, mot0, rad0)
    moved = (mot1["flags"] & 2 != 0) & (np.abs(mot1["px"] - (np.arange(w) + 0.5)) > 0.1)
    assert moved.sum() > 20 and (want[..., 3] == 2).any() and (want[..., 3] == 1).any()
    tris, _, _ = _mesh("cube.obj")
    with tm.Scene(tris) as sc:  # any scene: it lends its device and stream
        got, img = sc.temporal(rad1, mot1, mot0, rad0)
        same_bits(got, want, "suzanne twist pair")
        assert np.array_equal(img, T.pack(want))
        again = T.blend(rad0, mot0, mot0, want)  # and once more, on a history of mixed lengths
        same_bits(sc.temporal(rad0, mot0, mot0, got)[0], again, "second step")
        # device pointers: the same bytes, out = cur, the bytes alone
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(h, w, -1).copy()).to("cuda:0")
        t_cur, t_hist, t_m, t_pm = dev(rad1), dev(rad0), dev(mot1), dev(mot0)
        t_out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        t_8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda:0")
        size = dict(width=w, height=h)
        assert sc.temporal(t_cur.data_ptr(), t_m.data_ptr(), t_pm.data_ptr(), t_hist.data_ptr(),
                           out=(t_out.data_ptr(), t_8.data_ptr()), **size) == (None, None)
        assert t_out.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(t_8.cpu().numpy(), img)
        t_8.fill_(9)
        sc.temporal(t_cur.data_ptr(), t_m.data_ptr(), t_pm.data_ptr(), t_hist.data_ptr(), out=(None, t_8.data_ptr()), **size)
        assert np.array_equal(t_8.cpu().numpy(), img)
        assert t_cur.cpu().numpy().tobytes() == rad1.tobytes() and t_hist.cpu().numpy().tobytes() == rad0.tobytes()
        sc.temporal(t_cur.data_ptr(), t_m.data_ptr(), t_pm.data_ptr(), t_hist.data_ptr(), out=(t_cur.data_ptr(), None), **size)
        assert t_cur.cpu().numpy().tobytes() == want.tobytes()
        with pytest.raises(tm.TmptError, match="overlaps"):
            sc.temporal(t_cur.data_ptr(), t_m.data_ptr(), t_pm.data_ptr(), t_hist.data_ptr(),
                        out=(t_hist.data_ptr() + 16 * w, None), **size)
        st = sc.stats()
        assert st.render_ms > 0


# ---------------------------------------------------------------- 4  it accumulates
def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize("name", ["suzanne.obj", "teapot.obj"])
def test_it_accumulates(gpu, name):
    """RMSE against the 512-spp frame, over r, g, b, with the defaults: eight
    1-spp frames at sample_base 0 .. 7 blended in turn are closer than the last
    1-spp frame alone -- with a static scene, and over a 0 .. 20 degree twist
    with a refit per frame, against each pose's own 512-spp frame."""
    w, h, frames = 96, 54, 8
    rest, bmin, bmax = _mesh(name)
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    for what, top in (("static", 0.0), ("twist", 20.0)):
        with tm.Scene(rest, bounds=(bmin, bmax)) as sc:
            acc = pmot = prev = None
            for f in range(frames):
                pose = F.twist(rest, top * f / (frames - 1)) if top else rest
                if top:
                    sc.update(pose, "refit")
                sc.set_option("sample_base", f)
                rad, _, _ = sc.trace_radiance(cam, w, h, 1)
                mot, _ = sc.trace_motion(cam, cam, w, h, prev if top else None)
                acc = rad if f == 0 else sc.temporal(rad, mot, pmot, acc)[0]
                pmot, prev = mot, pose
            sc.set_option("sample_base", 0)
            truth, _, _ = sc.trace_radiance(cam, w, h, 512)
        e_one, e_acc = _rmse(rad, truth), _rmse(acc, truth)
        print(f"{name} {w}x{h} {what}: E_1spp = {e_one:.5f}  E_accumulated = {e_acc:.5f}  ratio {e_acc / e_one:.3f}  "
              f"mean history length {float(acc[..., 3].mean()):.2f}")
        assert e_acc < e_one, (name, what)


# ---------------------------------------------------------------- 5  state, CLI, checked build
def test_motion_and_blend_leave_the_progressive_state_alone(gpu):
    w, h, spp = 32, 18, 8
    tris, bmin, bmax = _mesh("suzanne.obj")
    cam = tm.Camera.for_scene(bmin, bmax, w, h)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        once, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        rad, _, _ = sc.trace_radiance(cam, w, h, 2)
        mot_alone, _ = sc.trace_motion(cam, cam, w, h)
        acc_alone, _ = sc.temporal(rad, mot_alone, mot_alone, rad)
        passes = sc.trace_progressive(cam, w, h, spp, [3, 5], seed_mode=tm.SEED_SAMPLE)
        done, _, r_a = next(passes)
        mot, _ = sc.trace_motion(cam, cam, w, h)
        acc, _ = sc.temporal(rad, mot, mot, rad)
        done, last, r_b = next(passes)
    assert done == spp and np.array_equal(last, once) and r_a + r_b == rays
    assert mot.tobytes() == mot_alone.tobytes() and acc.tobytes() == acc_alone.tobytes()


def test_cli_temporal_pngs(gpu, tmp_path):
    from PIL import Image

    w, h, spp = 32, 18, 2
    cli = os.path.join(os.path.dirname(tm.lib_path), "tmpt")
    stem = str(tmp_path / "tw")
    args = [cli, str(w), str(h), str(spp), data("suzanne.obj"), "--seed", "sample", "--twist", "20,3", "--out", stem + ".png"]
    r = subprocess.run(args + ["--temporal"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(tmp_path))
    assert names == ["tw_000.png", "tw_001.png", "tw_002.png", "tw_temporal_000.png", "tw_temporal_001.png",
                     "tw_temporal_002.png"], names
    load = lambda n: np.asarray(Image.open(str(tmp_path / n)).convert("RGBA"))
    assert np.array_equal(load("tw_temporal_000.png"), load("tw_000.png"))  # frame 0 is its own history
    assert not np.array_equal(load("tw_temporal_002.png"), load("tw_002.png"))
    plain0 = load("tw_000.png")
    # without --temporal the output is what it was: the same frame 0 (sample_base 0), no temporal file
    for n in names:
        os.remove(str(tmp_path / n))
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["tw_000.png", "tw_001.png", "tw_002.png"]
    assert np.array_equal(load("tw_000.png"), plain0)


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import bvh_refit_restate as F
import toymeshpathtracer_amd as tm
rest, bmin, bmax = tm.load_scene(sys.argv[2])
now = F.twist(rest, 10.0)
out = {}
sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
try:
    cam = tm.Camera.for_scene(bmin, bmax, 64, 36)
    with tm.Scene(rest) as sc:
        rad0, _, _ = sc.trace_radiance(cam, 64, 36, 2)
        mot0, _ = sc.trace_motion(cam, cam, 64, 36)
        sc.update(now, "refit")
        sc.set_option("sample_base", 2)
        rad1, _, _ = sc.trace_radiance(cam, 64, 36, 2)
        for tile in (0, 1):
            sc.set_option("motion_tile", tile)
            mot1, _ = sc.trace_motion(cam, cam, 64, 36, rest)
            out["motion%d" % tile] = sha(mot1)
        acc, img = sc.temporal(rad1, mot1, mot0, rad0)
        out["blend"] = [sha(acc), sha(img)]
    with tm.Scene(rest, bounds=(bmin, bmax)) as sc:  # with the octree: its root test and tie rule
        out["octree"] = sha(sc.trace_motion(cam, cam, 64, 36)[0])
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_temporal_checked_build(gpu):
    """The checked library computes the same motion records and the same blend, and no index check fails."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got
    w, h, rad0, mot0, rad1, mot1 = _twist_pair()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    rest, bmin, bmax = _mesh("suzanne.obj")
    with tm.Scene(rest, bounds=(bmin, bmax)) as sc:
        acc, img = sc.temporal(rad1, mot1, mot0, rad0)
        oct_rec, _ = sc.trace_motion(tm.Camera.for_scene(bmin, bmax, w, h), tm.Camera.for_scene(bmin, bmax, w, h), w, h)
    assert got == {"motion0": sha(mot1), "motion1": sha(mot1), "blend": [sha(acc), sha(img)], "octree": sha(oct_rec)}
