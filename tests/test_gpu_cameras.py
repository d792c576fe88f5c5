"""Frames through cameras the reference's placement never makes.

All but one frame of the suite is rendered through Camera.for_scene
(main.cpp:295-307: aperture 0.03, about one scene size away).  Here
Camera.create places a pinhole, a lens twice the scene's size, a camera inside
the scene, one looking away from it, one a hundred diagonals off behind a
0.5 degree lens, fields of view of 1 and 170 degrees, a camera whose basis is
the exact axes and one whose aspect disagrees with the frame -- each over a
scene without an octree (soup272, against the oracle's linear scan) and one
with it (suzanne, against the oracle's octree), through every path engine and
seeding.  Tolerance: none -- image bytes and ray counts.
"""
import functools

import numpy as np
import pytest

import geometry_cases as G
import oracle
import toymeshpathtracer_amd as tm
from conftest import data
from render_restate import aov_expect, pack, radiance_expect, same_bits, same_records
from test_gpu_build_geometry import _ENGINE, RENDER_CONFIGS, _config_id

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 27, 4
CONFIGS = RENDER_CONFIGS + [("megakernel", "row", None, None), ("persistent", "row", None, None)]
SEEDS = {"pixel": (tm.SEED_PIXEL, oracle.SEED_PIXEL), "sample": (tm.SEED_SAMPLE, oracle.SEED_SAMPLE),
         "row": (tm.SEED_ROW, oracle.SEED_ROW)}
CAMERAS = ("pinhole", "wide_lens", "inside", "away", "far", "fov_1", "fov_170", "axis_aligned", "aspect_3")
SCENES = ("soup272", "suzanne")


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> (triangles, box min, box max, octree bounds or None)"""
    if name == "suzanne":
        tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
        return tris, bmin, bmax, (bmin, bmax)
    tris = G.case(name)
    v = tris.reshape(-1, 3)
    return tris, v.min(0), v.max(0), None


def _oracle(name):
    tris, bmin, bmax, bounds = _scene(name)
    if bounds is None:
        return oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    return oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)


def _camera(scene, cam):
    _, lo, hi, _ = _scene(scene)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    c, D, asp = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo)), W / H
    d = np.array([0.6, 0.35, 0.72]) / np.linalg.norm([0.6, 0.35, 0.72])
    near, up = c + 1.2 * D * d, [0.0, 1.0, 0.0]
    if cam == "axis_aligned":
        # the centre on a 1/64 grid and a power-of-two distance: from - at = (0, 0, 2^k)
        # exactly, so normalize() gives w = (0, 0, 1), u = (1, 0, 0), v = (0, 1, 0)
        at = np.round(c * 64.0) / 64.0
        dist = 2.0 ** np.ceil(np.log2(1.5 * D))
        return tm.Camera.create(at + [0.0, 0.0, dist], at, up, 40.0, asp, 0.0, dist)
    args = {"pinhole": (near, c, up, 40.0, asp, 0.0, 1.2 * D),
            "wide_lens": (near, c, up, 40.0, asp, 2.0 * D, 1.2 * D),
            "inside": (c, c + d[::-1], up, 60.0, asp, 0.0, 1.0),
            "away": (near, near + D * d, up, 40.0, asp, 0.0, D),
            "far": (c + 100.0 * D * d, c, up, 0.5, asp, 0.0, 100.0 * D),
            "fov_1": (near, c, up, 1.0, asp, 0.0, 1.2 * D),
            "fov_170": (c + 0.55 * D * d, c, up, 170.0, asp, 0.0, 0.55 * D),  # close: the scene fills some of it
            "aspect_3": (near, c, up, 40.0, 3.0, 0.0, 1.2 * D)}[cam]
    return tm.Camera.create(*args)


@functools.lru_cache(maxsize=None)
def _reference_frame(scene, cam, seed):
    img, rays = _oracle(scene).render(_camera(scene, cam).as_array(), W, H, SPP, seed_mode=SEEDS[seed][1])
    img.setflags(write=False)
    return img, rays


def test_axis_aligned_basis_is_exact():
    for scene in SCENES:
        cam = _camera(scene, "axis_aligned")
        assert cam.u.tolist() == [1, 0, 0] and cam.v.tolist() == [0, 1, 0] and cam.w.tolist() == [0, 0, 1]
        assert cam.lens_radius == 0


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_camera_frames(gpu, scene, cam):
    """48x27 at 4 spp through every engine configuration of
    test_gpu_build_geometry.py and row seeding on the megakernel and the
    persistent engine: image and ray count equal the oracle's byte for byte."""
    tris, _, _, bounds = _scene(scene)
    camera = _camera(scene, cam)
    bad = []
    with tm.Scene(tris, bounds=bounds) as sc:
        defaults = sc.get_option("path_waves"), sc.get_option("help")
        for config in CONFIGS:
            engine, seed, waves, help_ = config
            ref, ref_rays = _reference_frame(scene, cam, seed)
            sc.set_option("path_waves", waves or defaults[0])
            sc.set_option("help", defaults[1] if help_ is None else help_)
            img, rays = sc.trace_image(camera, W, H, SPP, engine=_ENGINE[engine], seed_mode=SEEDS[seed][0])
            st = sc.stats()
            tag = f"{scene} {cam} {_config_id(config)}"
            if rays != ref_rays:
                bad.append(f"{tag}: rays {rays} != {ref_rays}")
            diff = np.nonzero((img != ref).any(-1))
            if diff[0].size:
                bad.append(f"{tag}: {diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}")
            if cam == "away" and scene == "soup272" and rays != W * H * SPP:
                bad.append(f"{tag}: {rays} rays, every sample should miss ({W * H * SPP})")
            if cam == "away" and (engine, seed) == ("persistent", "row") and (st.row_engine, st.stream_fallbacks) != (3, 0):
                bad.append(f"{tag}: row_engine {st.row_engine} stream_fallbacks {st.stream_fallbacks}, not the "
                           "streaming engine without a fallback")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cam", ["pinhole", "wide_lens", "away"])
@pytest.mark.parametrize("scene", SCENES)
def test_camera_aov_and_radiance(gpu, scene, cam):
    """The AOV records and the float radiance of the same cameras against the
    restatements of test_gpu_aov.py and test_gpu_radiance.py, bit for bit."""
    tris, _, _, bounds = _scene(scene)
    camera = _camera(scene, cam)
    osc = _oracle(scene)
    want, n = aov_expect(osc, camera.as_array(), W, H, SPP)
    print(scene, cam, n)
    if cam == "away" and scene == "soup272":
        assert n["hits"] == 0
    if cam == "pinhole":
        assert n["hits"] >= 200 and n["misses"] >= 100
    with tm.Scene(tris, bounds=bounds) as sc:
        got, rays = sc.trace_aov(camera, W, H, SPP)
        same_records(got, want)
        assert rays == W * H * SPP + n["hits"]
        for seed in (tm.SEED_SAMPLE, tm.SEED_PIXEL):
            rwant, rrays = radiance_expect(osc, camera.as_array(), W, H, SPP, seed)
            rad, img, rays = sc.trace_radiance(camera, W, H, SPP, seed_mode=seed)
            same_bits(rad[..., :3], rwant, f"{scene} {cam} seed {seed}")
            assert (rad[..., 3].view(np.uint32) == np.float32(1).view(np.uint32)).all()
            assert rays == rrays
            assert np.array_equal(img, pack(rad))
