"""Top-walk rounds of the persistent path kernels (option top_walk, k_path):
at the end of a shading round the lanes standing on a BVH node of the block's
LDS copy of the top levels take up to top_walk node rounds that hold no global
load.  Each lane steps the same function on the same state in the same order,
so the frame, the ray count and every visit count are those of the voted rounds
alone -- equal, not close -- for every cap, and the frame is the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import toymeshpathtracer_amd as tm
from conftest import data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "toymeshpathtracer_amd", "_lib_check", "libtmpt.so")

# scene -> frame: a tree far smaller than the LDS copy, a whole tree inside it
# (only the cap bounds the walk), more nodes than the copy, the bench scene
FRAMES = {"triangle": (64, 36, 4), "cube": (64, 36, 4), "suzanne": (160, 90, 4), "sponza": (96, 54, 8)}
SEEDS = {"sample": (tm.SEED_SAMPLE, oracle.SEED_SAMPLE), "pixel": (tm.SEED_PIXEL, oracle.SEED_PIXEL),
         "row": (tm.SEED_ROW, oracle.SEED_ROW)}
CAPS = (0, 1, -1, 8)  # off, one round, the seeding's default, the largest cap

_cache = {}


def _loaded(name, sponza_path):
    """(tris, bmin, bmax, camera, GPU scene with the octree, oracle scene), once per scene."""
    if name not in _cache:
        w, h, _ = FRAMES[name]
        tris, bmin, bmax = tm.load_scene(sponza_path if name == "sponza" else data(name + ".obj"))
        cam = tm.Camera.for_scene(bmin, bmax, w, h, is_sponza=name == "sponza")
        sc = tm.Scene(tris, bounds=(bmin, bmax))
        osc = oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bmin, bmax=bmax)
        _cache[name] = (tris, bmin, bmax, cam, sc, osc)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for entry in _cache.values():
        entry[4].close()
    _cache.clear()


def test_option_range_and_default(gpu):
    tris, _, _ = tm.load_scene(data("triangle.obj"))
    with tm.Scene(tris) as sc:
        assert sc.get_option("top_walk") == -1
        for v in (0, 1, 8, -1):
            sc.set_option("top_walk", v)
            assert sc.get_option("top_walk") == v
        for bad in (9, -2, 1.5):
            with pytest.raises(tm.TmptError):
                sc.set_option("top_walk", bad)


@pytest.mark.parametrize("seed", list(SEEDS))
@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_parity(gpu, sponza_path, name, seed):
    """Frame and ray count byte-identical across top_walk 0 / 1 / default / 8,
    with 4 and 5 waves per SIMD (and ties deferred or settled in the main loop
    in sample seeding), and identical to the oracle's octree frame."""
    _, _, _, cam, sc, osc = _loaded(name, sponza_path)
    w, h, spp = FRAMES[name]
    sd, osd = SEEDS[seed]
    ref, ref_rays = osc.render(cam.as_array(), w, h, spp, seed_mode=osd)
    try:
        for waves in (4, 5):
            sc.set_option("path_waves", waves)
            for defer in ((1, 0) if seed == "sample" else (-1,)):
                sc.set_option("tie_defer", defer)
                for cap in CAPS:
                    sc.set_option("top_walk", cap)
                    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=sd, engine=tm.ENGINE_PERSISTENT)
                    where = (name, seed, waves, defer, cap)
                    assert rays == ref_rays, where
                    diff = np.nonzero((img != ref).any(-1))
                    assert diff[0].size == 0, f"{where}: {diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}"
    finally:
        sc.set_option("path_waves", 0)
        sc.set_option("tie_defer", -1)
        sc.set_option("top_walk", -1)


@pytest.mark.parametrize("seed", ["sample", "pixel"])
@pytest.mark.parametrize("name", ["suzanne", "sponza"])
def test_visit_counts_equal(gpu, sponza_path, name, seed):
    """The counting kernels: the same node visits, triangle tests and rays, of
    closest-hit and shadow queries apart, with the walk off and at its largest
    cap -- the traversal order is the same, so the counts are equal."""
    _, _, _, cam, sc, _ = _loaded(name, sponza_path)
    w, h, spp = FRAMES[name]
    got = {}
    try:
        for cap in (0, 8):
            sc.set_option("top_walk", cap)
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=SEEDS[seed][0], engine=tm.ENGINE_PERSISTENT,
                                       count_visits=True)
            st = sc.stats()
            got[cap] = (img, rays, {k: getattr(st, k) for k in
                                    ("node_visits", "tri_tests", "shadow_node_visits", "shadow_tri_tests",
                                     "extend_rays", "shadow_rays")})
    finally:
        sc.set_option("top_walk", -1)
    assert got[0][2]["node_visits"] > 0 and got[0][2]["shadow_node_visits"] > 0
    assert got[8][2] == got[0][2]
    assert got[8][1] == got[0][1] and np.array_equal(got[8][0], got[0][0])


CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
cam = tm.Camera.for_scene(bmin, bmax, 160, 90)
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        for cap in (0, 8):
            sc.set_option("top_walk", cap)
            for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
                img, rays = sc.trace_image(cam, 160, 90, 4, seed_mode=sm, engine=tm.ENGINE_PERSISTENT)
                out[f"{cap}/{sm}"] = [hashlib.sha256(img.tobytes()).hexdigest(), int(rays)]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_checked_build_no_index_fails(gpu):
    """The checked library (device index tests in the traversal) renders the
    three seedings with the walk off and at its largest cap: no check fails,
    and the frames and ray counts are the same for both caps."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("suzanne.obj")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got["error"]
    assert "device index check failed" not in r.stderr
    for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
        assert got[f"8/{sm}"] == got[f"0/{sm}"]
