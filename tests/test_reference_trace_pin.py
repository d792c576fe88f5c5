"""The oracle's shading chain against the reference itself, sample by sample and
float by float (CPU; no GPU).

tests/golden/ref/trace_<case>.npz hold what the compiled, unmodified reference
answered through oracle/ref/ref_trace.cpp (tests/golden/make_ref_fixtures.py;
cases and format in tests/ref_cases.py): for every sample of a 32x18x8 frame in
sample seeding and in pixel seeding, Camera::GetRay's ray and the RNG state
after it, Scene::HitScene's first hit, and the colour, state and ray count of
main.cpp's own Trace() -- the lens draw, RandomUnitVector, Scatter's light term
with its normal flip, the depth cap and the backward recurrence, none of which
the 8-bit frames of test_reference_pin.py resolve.

Tolerance: none.  Floats are compared as bits, and the first mismatch is named
by case, pixel and sample.  test_gpu_reference_trace.py holds the library to the
same files.
"""
import functools
import os

import numpy as np
import pytest

import oracle
import ref_cases as C
import toymeshpathtracer_amd as tm
from render_restate import chain_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_TRACE = os.path.join(ROOT, "oracle", "_ref", "ref_trace")
CAMERA_FIELDS = ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w", "lens_radius")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cam_args(cam13):
    c = [float(v) for v in cam13]
    return c[0:3], c[3:6], c[6:9], c[9], c[10], c[11], c[12]


def _first_bad(fx, bad):
    """'pixel (x, y) sample s' of the first sample flagged in bad (n,), or None."""
    idx = np.nonzero(bad)[0]
    if not idx.size:
        return None
    w, h, spp = (int(v) for v in fx["size"])
    i = int(idx[0])
    return f"{idx.size} samples differ, first at pixel ({i // spp % w}, {i // spp // w}) sample {i % spp}"


def _differs(a, b):
    """Per sample: any word of a differs from b's."""
    x, y = _u32(a), _u32(b)
    assert x.shape == y.shape, (x.shape, y.shape)
    return (x != y).reshape(len(x), -1).any(1)


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    fx = C.load_trace(name)
    return oracle.Scene(fx["tris"], accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=fx["bmin"], bmax=fx["bmax"])


def test_trace_fixture_list_is_complete():
    """Every trace case has its fixture: the size, the chains of today's seeds, the box of main.cpp:312."""
    w, h, spp = C.TRACE_SIZE
    n = w * h * spp
    chains = {True: C.seed_chains(w, h, spp, True), False: C.seed_chains(w, h, spp, False)}
    for name in C.TRACE_CASES:
        fx = C.load_trace(name)
        assert tuple(fx["size"]) == C.TRACE_SIZE
        assert np.array_equal(fx["chains_sample"], chains[True]) and np.array_equal(fx["chains_pixel"], chains[False])
        assert np.array_equal(_u32(fx["box"]), _u32(C.octree_box(fx["bmin"], fx["bmax"])))
        assert fx["cam"].shape == (13,) and fx["cam"].dtype == np.float32
        for key, shape in (("s_ray", (n, 6)), ("s_state_ray", (n,)), ("s_hit", (n,)), ("s_tn", (n, 4)),
                           ("s_col", (n, 3)), ("s_state", (n,)), ("s_rays", (n,)), ("p_col", (n, 3)),
                           ("p_state", (n,)), ("p_rays", (n,))):
            assert fx[key].shape == shape, (name, key, fx[key].shape)
        assert os.path.getsize(C.trace_path(name)) <= os.path.getsize(C.hits_path("crack_wall"))


@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_case_generators_give_the_fixture(name):
    """The scene and camera ref_cases.trace_scene makes today are the fixture's, bit for bit."""
    fx = C.load_trace(name)
    tris, bmin, bmax, cam = C.trace_scene(name)
    for key, a in (("tris", tris), ("bmin", bmin), ("bmax", bmax), ("cam", cam)):
        assert np.array_equal(_u32(np.asarray(a, np.float32)), _u32(fx[key])), key


def test_reference_camera_arguments():
    """ref_cases.ref_camera_args restates main.cpp:296-307: through Camera::Camera
    (the oracle's) they give the camera the oracle places for the scene itself."""
    w, h, _ = C.TRACE_SIZE
    _, bmin, bmax = C.hit_scene("cube")
    got = oracle.camera(*_cam_args(C.ref_camera_args(bmin, bmax, w, h, 0.03)))
    assert np.array_equal(_u32(got), _u32(oracle.camera_for_scene(bmin, bmax, w, h)))


@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_library_camera_equals_the_oracles(name):
    """tm.Camera.create over the stored arguments: the oracle's camera, field by field (host code)."""
    fx = C.load_trace(name)
    want = oracle.camera(*_cam_args(fx["cam"]))
    cam = tm.Camera.create(*_cam_args(fx["cam"]))
    got = cam.as_array()
    assert got.shape == want.shape == (22,)
    for k, field in enumerate(CAMERA_FIELDS):
        a, b = got[3 * k:3 * k + 3] if k < 7 else got[21:], want[3 * k:3 * k + 3] if k < 7 else want[21:]
        assert np.array_equal(_u32(a), _u32(b)), (name, field, a, b)
    assert np.float32(cam.lens_radius) == np.float32(fx["cam"][11]) * np.float32(0.5)


@pytest.mark.parametrize("seeding", ["sample", "pixel"])
@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_oracle_samples_equal_reference(name, seeding):
    """oracle.get_ray's ray and state, Scene.hit_batch's first hit, Scene.trace's
    colour, state out and ray count of every sample (pixel seeding: the fixture
    keeps colour, state and count)."""
    fx = C.load_trace(name)
    w, h, spp = (int(v) for v in fx["size"])
    osc = _oracle_scene(name)
    cam = oracle.camera(*_cam_args(fx["cam"]))
    pre = seeding[0] + "_"
    got = chain_samples(osc, cam, w, h, fx["chains_" + seeding])
    what = f"{name}, {seeding} seeding"
    if seeding == "sample":
        bad = _differs(got["ray"], fx["s_ray"])
        assert not bad.any(), f"{what}: camera rays: " + _first_bad(fx, bad)
        bad = got["state_ray"] != fx["s_state_ray"]
        assert not bad.any(), f"{what}: state after GetRay: " + _first_bad(fx, bad)
        ids, hits = osc.hit_batch(fx["s_ray"], *C.REF_RANGE)
        hit = fx["s_hit"].astype(bool)
        bad = (ids >= 0) != hit
        assert not bad.any(), f"{what}: first-hit flags: " + _first_bad(fx, bad)
        tn = np.concatenate([hits[:, 6:7], hits[:, 3:6]], 1)
        bad = hit & _differs(tn, fx["s_tn"])
        assert not bad.any(), f"{what}: first hit {{t, normal}}: " + _first_bad(fx, bad)
        assert not _u32(fx["s_tn"])[~hit].any()
    bad = _differs(got["col"], fx[pre + "col"])
    assert not bad.any(), f"{what}: Trace's colour: " + _first_bad(fx, bad)
    bad = got["state"] != fx[pre + "state"]
    assert not bad.any(), f"{what}: state after Trace: " + _first_bad(fx, bad)
    bad = got["rays"] != fx[pre + "rays"]
    assert not bad.any(), f"{what}: ray counts: " + _first_bad(fx, bad)


@pytest.mark.parametrize("name", C.TRACE_CASES)
def test_fresh_reference_trace_equals_fixture(name, tmp_path):
    """With the compiled reference at hand: it answers today what the fixture holds."""
    if not os.path.exists(REF_TRACE):
        pytest.skip("oracle/_ref/ref_trace not built (make -C oracle/ref, needs a reference checkout)")
    fx = C.load_trace(name)
    w, h, _ = (int(v) for v in fx["size"])
    for pre, keys in (("s", ("ray", "state_ray", "hit", "tn", "col", "state", "rays")), ("p", ("col", "state", "rays"))):
        chains = fx["chains_sample" if pre == "s" else "chains_pixel"]
        got = C.run_ref_trace(REF_TRACE, fx["tris"], fx["box"], fx["cam"], w, h, chains, tmp_path)
        for k in keys:
            assert got[k].dtype == fx[f"{pre}_{k}"].dtype and got[k].tobytes() == fx[f"{pre}_{k}"].tobytes(), (pre, k)


def test_trace_fixtures_are_not_vacuous():
    """From the reference's answers alone (ref_cases.TRACE_FLOORS): over all cases
    at least 500 samples of exactly 20 rays, 200 that leave to the sky after three
    or more bounces, 300 first hits seen from behind, 1000 camera rays that miss;
    in each case at least 100 pixels of which 1 .. 7 of the 8 samples hit; no
    colour that is not finite."""
    assert C.TRACE_FLOORS == dict(full_depth=500, late_sky=200, back_face=300, camera_miss=1000, partial_pixels=100)
    counts = {name: C.trace_counts(C.load_trace(name)) for name in C.TRACE_CASES}
    print(counts)
    C.check_trace_counts(counts)
