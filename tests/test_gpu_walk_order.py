"""The any-hit child order (option shadow_order): an any-hit query visits a
node's children longest-overlap or largest-exit first instead of nearest first.
That changes which occluder a shadow query meets first and never its hit bit,
the only thing used of it, so every frame and ray count equals the oracle's
octree frame -- equal, not close -- for every order, in every seeding, with 4
and 5 waves per SIMD and with ties deferred or settled in the main loop; the
batched any-hit HitScene's bit equals the oracle's closest hit's; and the
closest-hit walk does not move at all (equal visit counts)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_cases as G
import oracle
import toymeshpathtracer_amd as tm
from conftest import data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")

FRAMES = {"triangle": (64, 36, 4), "cube": (64, 36, 4), "suzanne": (160, 90, 4), "sponza": (96, 54, 8)}
SEEDS = {"sample": (tm.SEED_SAMPLE, oracle.SEED_SAMPLE), "pixel": (tm.SEED_PIXEL, oracle.SEED_PIXEL),
         "row": (tm.SEED_ROW, oracle.SEED_ROW)}
ORDERS = (0, 1, 2)  # nearest first, longest overlap first, largest exit first

_cache = {}


def _loaded(name, sponza_path):
    """(camera, GPU scene with the octree, oracle scene), once per scene."""
    if name not in _cache:
        w, h, _ = FRAMES[name]
        tris, bmin, bmax = tm.load_scene(sponza_path if name == "sponza" else data(name + ".obj"))
        cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=name == "sponza")
        sc = tm.Scene(tris, bounds=(bmin, bmax))
        osc = oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)
        _cache[name] = (cam, sc, osc)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for entry in _cache.values():
        entry[1].close()
    _cache.clear()


def test_option_range_and_default(gpu):
    tris, _, _ = tm.load_scene(data("triangle.obj"))
    with tm.Scene(tris) as sc:
        assert sc.get_option("shadow_order") == -1
        for v in ORDERS + (-1,):
            sc.set_option("shadow_order", v)
            assert sc.get_option("shadow_order") == v
        for bad in (3, -2, 1.5):
            with pytest.raises(tm.TmptError):
                sc.set_option("shadow_order", bad)


@pytest.mark.parametrize("seed", list(SEEDS))
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_parity(gpu, sponza_path, name, seed):
    """Frame and ray count identical to the oracle's octree frame for every
    shadow_order, with 4 and 5 waves per SIMD (and ties deferred or
    settled in the main loop in sample seeding)."""
    cam, sc, osc = _loaded(name, sponza_path)
    w, h, spp = FRAMES[name]
    sd, osd = SEEDS[seed]
    ref, ref_rays = osc.render(cam.as_array(), w, h, spp, seed_mode=osd)
    try:
        for waves in (4, 5):
            sc.set_option("path_waves", waves)
            for defer in ((1, 0) if seed == "sample" else (-1,)):
                sc.set_option("tie_defer", defer)
                for order in ORDERS:
                    sc.set_option("shadow_order", order)
                    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=sd, engine=tm.ENGINE_PERSISTENT)
                    where = (name, seed, waves, defer, order)
                    assert rays == ref_rays, where
                    diff = np.nonzero((img != ref).any(-1))
                    assert diff[0].size == 0, f"{where}: {diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}"
    finally:
        sc.set_option("path_waves", 0)
        sc.set_option("tie_defer", -1)
        sc.set_option("shadow_order", -1)


@pytest.mark.parametrize("engine", ["wavefront", "megakernel"])
def test_other_engines_and_aov(gpu, sponza_path, engine):
    """The wavefront and mega engines step the same function: the suzanne frame
    in pixel seeding equals the oracle's for every order; and the AOV pass's
    records do not move with the option."""
    cam, sc, osc = _loaded("suzanne", sponza_path)
    w, h, spp = FRAMES["suzanne"]
    ref, ref_rays = osc.render(cam.as_array(), w, h, spp, seed_mode=oracle.SEED_PIXEL)
    eng = tm.ENGINE_WAVEFRONT if engine == "wavefront" else tm.ENGINE_MEGAKERNEL
    aov = None
    try:
        for order in ORDERS:
            sc.set_option("shadow_order", order)
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_PIXEL, engine=eng)
            assert rays == ref_rays and np.array_equal(img, ref), (engine, order)
            if engine == "wavefront":
                rec, arays = sc.trace_aov(cam, w, h, spp)
                if aov is None:
                    aov = (rec, arays)
                assert arays == aov[1] and rec.tobytes() == aov[0].tobytes(), order
    finally:
        sc.set_option("shadow_order", -1)


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
cam = tm.Camera.for_scene(bmin, bmax, 160, 90)
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        for order in (0, 1, 2):
            sc.set_option("shadow_order", order)
            for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
                img, rays = sc.trace_image(cam, 160, 90, 4, seed_mode=sm, engine=tm.ENGINE_PERSISTENT)
                out[f"{order}/{sm}"] = [hashlib.sha256(img.tobytes()).hexdigest(), int(rays)]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_checked_build_no_index_fails(gpu):
    """The checked library (device index tests in the traversal) renders the
    three seedings under every order: no check fails, and the frames and ray
    counts are the same for all of them."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got["error"]
    assert "device index check failed" not in r.stderr
    for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
        for order in ORDERS:
            assert got[f"{order}/{sm}"] == got[f"0/{sm}"], (order, sm)


# ---------------------------------------------------------------- the batched any-hit HitScene
N_RAYS = 50_000
# meshes, and adversarial builds of geometry_cases.py: every hit tied on t,
# trees on both sides of the LDS top copy, a chain of nested boxes, and a soup
# whose stack outgrows its LDS part
HIT_CASES = ("suzanne", "teapot", "coincident3", "coincident64", "coincident1000", "soup272", "soup330", "soup480",
             "nested200", "soup4100")
RANGES = np.array([(0.001, 1e7), (0.0, 1e7), (-2.0, 1e7), (0.001, 1.5), (0.5, 4.0), (2.0, 2.0001),
                   (3.0, 1.0), (0.001, 0.001), (-1e7, 0.0), (-0.5, 0.25)], np.float32)


@functools.lru_cache(maxsize=None)
def _hit_case(name):
    """(tris, bmin, bmax, rays, the oracle BVH's closest-hit ids), once per case."""
    if name in ("suzanne", "teapot"):
        tris, bmin, bmax = tm.load_scene(data(name + ".obj"))
    else:
        tris = G.case(name)
        v = tris.reshape(-1, 3)
        bmin, bmax = v.min(0), v.max(0)
    rays, _ = G.rays(tris, N_RAYS, seed=31)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_BVH, tie=oracle.TIE_INDEX, bmin=bmin, bmax=bmax)
    oids, _ = osc.hit_batch(rays, 0.001, 1.0e7)
    for a in (rays, oids):
        a.setflags(write=False)
    return tris, bmin, bmax, rays, oids


@pytest.mark.parametrize("name", HIT_CASES)
def test_any_hit_bit(gpu, name):
    """k_intersect<ANY>: for every order the hit bit equals the oracle's
    (closest-hit id >= 0; which triangle a tie goes to does not matter to it),
    without an octree and -- where the reference's octree can be built in
    reasonable time -- with it (flat triangles and cracks answered over it);
    the closest-hit ids themselves do not move with the option."""
    tris, bmin, bmax, rays, oids = _hit_case(name)
    assert (oids >= 0).sum() > 1000 and (oids < 0).sum() > 1000
    for bounds in ((None,) if name == "coincident1000" else (None, (bmin, bmax))):
        with tm.Scene(tris, bounds=bounds) as sc:
            ids0 = None
            for order in ORDERS:
                sc.set_option("shadow_order", order)
                aids, _ = sc.hit_scene_batch(rays, 0.001, 1.0e7, any_hit=True)
                ids, _ = sc.hit_scene_batch(rays, 0.001, 1.0e7)
                if ids0 is None:
                    ids0 = ids
                assert np.array_equal(ids, ids0), (name, bounds is not None, order)
                # with the octree the reference drops rays its root box test rejects: the bit
                # follows the scene's own closest-hit answer, which equals the oracle's without it
                want = (ids >= 0) if bounds is not None else (oids >= 0)
                bad = np.nonzero((aids >= 0) != want)[0]
                assert bad.size == 0, f"{name} order {order}: {bad.size} hit bits differ, first rays {bad[:5]}"


def test_any_hit_ranged(gpu):
    """Ranged any-hit queries (the range per ray, mixed in one batch): the ten
    ranges of test_gpu_parity.test_hitscene_per_ray_ranges, those behind the
    origin and the empty ones included -- there tn and tf are negative and the
    far slack is applied by magnitude.  The bit equals the linear scan's."""
    tris, bmin, bmax, rays, _ = _hit_case("suzanne")
    rng = np.random.default_rng(21)
    k = rng.integers(0, len(RANGES), len(rays))
    r8 = np.concatenate([rays, RANGES[k]], 1).astype(np.float32)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX, bmin=bmin, bmax=bmax)
    want = np.zeros(len(rays), bool)
    for j in range(len(RANGES)):
        sel = np.nonzero(k == j)[0]
        want[sel] = osc.hit_batch(rays[sel], float(RANGES[j, 0]), float(RANGES[j, 1]))[0] >= 0
    assert want.sum() > 1000 and (~want).sum() > 1000
    with tm.Scene(tris) as sc:
        for order in ORDERS:
            sc.set_option("shadow_order", order)
            aids, _ = sc.hit_scene_batch(r8, any_hit=True)
            for j in range(len(RANGES)):
                sel = k == j
                assert np.array_equal(aids[sel] >= 0, want[sel]), (order, RANGES[j])


COUNT_FRAMES = {"suzanne": (160, 90, 4), "sponza": (96, 54, 8)}
KEYS = ("node_visits", "tri_tests", "shadow_node_visits", "shadow_tri_tests", "extend_rays", "shadow_rays")


@pytest.mark.parametrize("name", list(COUNT_FRAMES))
def test_visit_counts(gpu, sponza_path, name):
    """The counting kernels: closest-hit node visits and triangle tests, the ray
    counts and the frame do not move with shadow_order, in the persistent and
    the wavefront engine, which walk alike; the shadow queries' visits do move
    (on sponza, whose occluders are mostly far, both other orders visit fewer
    nodes than nearest first)."""
    w, h, spp = COUNT_FRAMES[name]
    tris, bmin, bmax = tm.load_scene(sponza_path if name == "sponza" else data(name + ".obj"))
    cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=name == "sponza")
    got = {}
    with tm.Scene(tris) as sc:
        for engine in (tm.ENGINE_PERSISTENT, tm.ENGINE_WAVEFRONT):
            for order in ORDERS:
                sc.set_option("shadow_order", order)
                img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_PIXEL, engine=engine, count_visits=True)
                st = sc.stats()
                got[engine, order] = (img, rays, {k: getattr(st, k) for k in KEYS})
                print(name, engine, order, got[engine, order][2])
    base_img, base_rays, base = got[tm.ENGINE_PERSISTENT, 0]
    assert base["node_visits"] > 0 and base["shadow_node_visits"] > 0
    for (engine, order), (img, rays, c) in got.items():
        where = (name, engine, order)
        assert rays == base_rays and np.array_equal(img, base_img), where
        for k in ("node_visits", "tri_tests", "extend_rays", "shadow_rays"):
            assert c[k] == base[k], (where, k)
        if name == "sponza" and order:
            assert c["shadow_node_visits"] < got[engine, 0][2]["shadow_node_visits"], where
