"""Pop culling with the key in a stack entry's spare bits (options pop_cull,
pop_key_cap, pop_key_bits).

A pushed child carries the top K bits of its entry distance in the bits its
link leaves free; a closest-hit lane that pops an entry whose key already
exceeds the best hit discards it unvisited.  The child's own box test would
reject it, so nothing a query answers may move: frames, ray counts, hit
records, tie flags and tie_queries are equal -- not close -- with culling on
and off, at 13 key bits, at 9 (pop_key_cap) and at none; only the closest-hit
visit counts fall.  The hit records of hit_scene_batch (position, normal, t)
stand for (t, u, v): the position is formed from u and v."""
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

FRAMES = {"sponza": (96, 54, 4), "teapot": (64, 36, 4)}
# (pop_cull, pop_key_cap): off (the frame the others must equal), on with the scene's
# full key, on with 9 key bits, on with no key at all
VARIANTS = ((0, -1), (1, -1), (1, 9), (1, 0))
# (engine, seeding, shard, num_shards); the oracle renders whole frames in sample and pixel seeding
RENDERS = (("persistent", "sample", 0, 1), ("persistent", "pixel", 0, 1), ("persistent", "row", 0, 1),
           ("wavefront", "pixel", 0, 1), ("megakernel", "pixel", 0, 1), ("persistent", "sample", 1, 3))
ENGINES = {"persistent": tm.ENGINE_PERSISTENT, "wavefront": tm.ENGINE_WAVEFRONT, "megakernel": tm.ENGINE_MEGAKERNEL}
SEEDS = {"sample": (tm.SEED_SAMPLE, oracle.SEED_SAMPLE), "pixel": (tm.SEED_PIXEL, oracle.SEED_PIXEL),
         "row": (tm.SEED_ROW, oracle.SEED_ROW)}

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


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, seed, sponza_path):
    cam, _, osc = _loaded(name, sponza_path)
    w, h, spp = FRAMES[name]
    img, rays = osc.render(cam.as_array(), w, h, spp, seed_mode=SEEDS[seed][1])
    img.setflags(write=False)
    return img, rays


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for entry in _cache.values():
        entry[1].close()
    _cache.clear()


def _set(sc, cull, cap):
    sc.set_option("pop_cull", cull)
    sc.set_option("pop_key_cap", cap)


def test_options(gpu):
    tris, _, _ = tm.load_scene(data("triangle.obj"))
    with tm.Scene(tris) as sc:
        assert sc.get_option("pop_cull") == -1 and sc.get_option("pop_key_cap") == -1
        for v in (0, 1, -1):
            sc.set_option("pop_cull", v)
            assert sc.get_option("pop_cull") == v
        for bad in (2, -2, 0.5):
            with pytest.raises(tm.TmptError):
                sc.set_option("pop_cull", bad)
        for bad in (17, -2):
            with pytest.raises(tm.TmptError):
                sc.set_option("pop_key_cap", bad)
        with pytest.raises(tm.TmptError):  # read-only
            sc.set_option("pop_key_bits", 9)
        assert sc.get_option("pop_key_bits") == 16  # a tiny scene: the cap of 16 bits
        sc.set_option("pop_key_cap", 11)
        assert sc.get_option("pop_key_bits") == 11


@pytest.mark.parametrize("render", RENDERS, ids=lambda r: "-".join(map(str, r)))
@pytest.mark.parametrize("name", list(FRAMES))
def test_frames(gpu, sponza_path, name, render):
    """Frames and ray counts byte-identical to pop_cull=0 for every variant; the
    whole sample- and pixel-seeded frames also to the oracle's."""
    engine, seed, shard, shards = render
    cam, sc, _ = _loaded(name, sponza_path)
    w, h, spp = FRAMES[name]
    base = None
    try:
        for cull, cap in VARIANTS:
            _set(sc, cull, cap)
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=SEEDS[seed][0], engine=ENGINES[engine],
                                       band_rows=1 if shards > 1 else 0, shard=shard, num_shards=shards)
            if base is None:
                base = (img, rays)
            where = (name, render, cull, cap)
            assert rays == base[1], where
            diff = np.nonzero((img != base[0]).any(-1))
            assert diff[0].size == 0, f"{where}: {diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}"
    finally:
        _set(sc, -1, -1)
    if seed != "row" and shards == 1:
        ref, ref_rays = _oracle_frame(name, seed, sponza_path)
        assert base[1] == ref_rays and np.array_equal(base[0], ref), (name, render)


COUNT_KEYS = ("extend_rays", "shadow_rays", "shadow_node_visits", "shadow_tri_tests", "node_visits", "tri_tests")


@pytest.mark.parametrize("engine", ["persistent", "wavefront"])
def test_counts(gpu, sponza_path, engine):
    """The counting kernels on sponza 96x54x4: ray counts and the shadow
    queries' visits equal with culling on and off; the closest-hit node visits
    and triangle tests strictly smaller with it on, and no larger at 9 bits
    than with it off."""
    cam, sc, _ = _loaded("sponza", sponza_path)
    w, h, spp = FRAMES["sponza"]
    got = {}
    try:
        for cull, cap in VARIANTS:
            _set(sc, cull, cap)
            img, _ = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_PIXEL, engine=ENGINES[engine],
                                    count_visits=True)
            st = sc.stats()
            got[cull, cap] = (img, {k: getattr(st, k) for k in COUNT_KEYS})
            print(engine, cull, cap, got[cull, cap][1])
    finally:
        _set(sc, -1, -1)
    off = got[0, -1][1]
    assert off["node_visits"] > 0 and off["shadow_node_visits"] > 0
    for (cull, cap), (img, c) in got.items():
        assert np.array_equal(img, got[0, -1][0]), (cull, cap)
        for k in COUNT_KEYS[:4]:
            assert c[k] == off[k], (cull, cap, k)
    on, cap9, none = got[1, -1][1], got[1, 9][1], got[1, 0][1]
    for k in ("node_visits", "tri_tests"):
        assert on[k] < off[k], k
        assert cap9[k] <= off[k], k
        assert none[k] == off[k], k


# ---------------------------------------------------------------- the batched HitScene on every build
N_RAYS = 4000
RANGES = np.array([(0.001, 1e7), (0.0, 1e7), (-2.0, 1e7), (0.001, 1.5), (0.5, 4.0), (2.0, 2.0001),
                   (3.0, 1.0), (0.001, 0.001), (-1e7, 0.0), (-0.5, 0.25)], np.float32)
GROUPS = {"3-68": range(3, 69), "69-136": range(69, 137), "137-204": range(137, 205), "205-272": range(205, 273),
          "large": G.SWEEP_NODES + G.SWEEP_LARGE}


@functools.lru_cache(maxsize=None)
def _cases():
    return G.cases()


def _answers(sc, rays, tmin, tmax):
    """{variant: (ids, hit records, tie_queries)}; options restored."""
    out = {}
    for cull, cap in VARIANTS:
        _set(sc, cull, cap)
        ids, hits = sc.hit_scene_batch(rays, tmin, tmax)
        out[cull, cap] = (ids, hits, sc.stats().tie_queries)
    _set(sc, -1, -1)
    return out


def _check_case(name, opts=None, octree=False):
    """-> what is wrong with the case's answers (empty: nothing)."""
    tris = _cases()[name]
    rays, (tmin, tmax) = G.rays(tris, N_RAYS, seed=3)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    oids, ohits = osc.hit_batch(rays, tmin, tmax)
    v = tris.reshape(-1, 3)
    bad = []
    with tm.Scene(tris, options=opts, bounds=(v.min(0), v.max(0)) if octree else None) as sc:
        got = _answers(sc, rays, tmin, tmax)
        ids0, hits0, ties0 = got[0, -1]
        for var, (ids, hits, ties) in got.items():
            if not np.array_equal(ids, ids0) or hits.tobytes() != hits0.tobytes():
                bad.append(f"{name} {var}: answers differ from pop_cull=0 at rays {np.nonzero(ids != ids0)[0][:5]}")
            if ties != ties0:
                bad.append(f"{name} {var}: tie_queries {ties} != {ties0}")
            if not octree:  # (with the octree the reference's visit order picks among ties)
                mism = np.nonzero(ids != oids)[0]
                h = (ids >= 0) & (ids == oids)
                if mism.size or (hits[h].view(np.uint32) != ohits[h].view(np.uint32)).any():
                    bad.append(f"{name} {var}: differs from the linear scan, first rays {mism[:5]}")
    return bad


@pytest.mark.parametrize("group", list(GROUPS))
def test_answers_sweep(gpu, group):
    bad = []
    for n in GROUPS[group]:
        bad += _check_case(G.sweep_name(n))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", G.NON_SWEEP)
def test_answers_families(gpu, name):
    """Every family, the duplicated and coincident faces among them: id and hit
    record equal the linear scan's and pop_cull=0's for every variant."""
    bad = _check_case(name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["coincident3", "coincident17", "coincident64", "samebox_fan150", "uniform_sheet"])
def test_ties_keep_their_flag(gpu, name):
    """With the reference's octree every closest hit tied on t is flagged and
    answered over it: the flagged queries (tie_queries) and the answers equal
    pop_cull=0's -- an entry is discarded only when its key exceeds the best
    hit, never on equality."""
    tris = _cases()[name]
    rays, (tmin, tmax) = G.rays(tris, N_RAYS, seed=3)
    v = tris.reshape(-1, 3)
    with tm.Scene(tris, bounds=(v.min(0), v.max(0))) as sc:
        got = _answers(sc, rays, tmin, tmax)
    ids0, hits0, ties0 = got[0, -1]
    if name.startswith("coincident"):
        assert ties0 > 0
    for var, (ids, hits, ties) in got.items():
        assert ties == ties0, (name, var)
        assert np.array_equal(ids, ids0) and hits.tobytes() == hits0.tobytes(), (name, var)


def test_negative_tmin_unchanged(gpu):
    """Ranged queries, ranges behind the origin and empty ones among them (the
    NEG instantiation pushes no key and discards nothing): the linear scan's
    answers for every variant."""
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    rays, _ = G.rays(tris, 20000, seed=31)
    k = np.random.default_rng(21).integers(0, len(RANGES), len(rays))
    r8 = np.concatenate([rays, RANGES[k]], 1).astype(np.float32)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX, bmin=bmin, bmax=bmax)
    want = np.full(len(rays), -1, np.int32)
    for j in range(len(RANGES)):
        sel = np.nonzero(k == j)[0]
        want[sel] = osc.hit_batch(rays[sel], float(RANGES[j, 0]), float(RANGES[j, 1]))[0]
    assert (want >= 0).sum() > 1000
    with tm.Scene(tris) as sc:
        base = None
        for cull, cap in VARIANTS:
            _set(sc, cull, cap)
            ids, hits = sc.hit_scene_batch(r8)
            assert np.array_equal(ids, want), (cull, cap)
            base = base or (hits.tobytes(),)
            assert hits.tobytes() == base[0], (cull, cap)
            one, _ = sc.hit_scene_batch(rays, -2.0, 1.0e7)  # one range with t_min < 0: NEG too
            assert np.array_equal(one[k == 2], want[k == 2]), (cull, cap)


@pytest.mark.parametrize("name", ["coincident200", "coincident1000"])
def test_deep_stacks(gpu, name):
    """Identical boxes give a deep tree: its depth x 3 entries pass the LDS part
    of the stack (12 entries in the 5-wave path kernels; coincident1000 also
    the 16 of the batched queries), so keyed entries go through the global
    overflow area and come
    back: answers equal the linear scan's, and a frame through the 5-wave
    persistent kernel equals pop_cull=0's."""
    tris = _cases()[name]
    with tm.Scene(tris) as sc:
        depth = sc.stats().bvh4_depth
        print(name, "bvh4_depth", depth)
        assert 3 * depth > (16 if name == "coincident1000" else 12)
        cam = tm.Camera.for_scene(tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0), 48, 27)
        sc.set_option("path_waves", 5)
        frames = []
        for cull, cap in VARIANTS:
            _set(sc, cull, cap)
            frames.append(sc.trace_image(cam, 48, 27, 4, seed_mode=tm.SEED_SAMPLE, engine=tm.ENGINE_PERSISTENT))
        for img, rays in frames[1:]:
            assert rays == frames[0][1] and np.array_equal(img, frames[0][0])
    assert not _check_case(name)


# ---------------------------------------------------------------- layout
def test_key_bits(gpu, sponza_path):
    """13 key bits on the stand-in sponza at leaf_max 2 (17 record bits, one
    count bit), fewer at leaf_max 16 (four count bits), none under pop_key_cap=0."""
    tris, _, _ = tm.load_scene(sponza_path)
    with tm.Scene(tris) as sc:
        assert sc.stats().leaf_max == 2 and sc.get_option("pop_key_bits") == 13
        sc.set_option("pop_key_cap", 9)
        assert sc.get_option("pop_key_bits") == 9
        sc.set_option("pop_key_cap", 0)
        assert sc.get_option("pop_key_bits") == 0
    with tm.Scene(tris, options={"leaf_max": 16}) as sc:
        assert sc.get_option("pop_key_bits") == 10


@pytest.mark.parametrize("leaf_max", [1, 2, 4, 16])
def test_leaf_max_layouts(gpu, leaf_max):
    """The count field is as wide as leaf_max needs: every width decodes."""
    bad = []
    for name in ("soup480", "coincident64", "samebox_fan150", "soup4100"):
        bad += _check_case(name, {"leaf_max": leaf_max})
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- checked build
CHILD = r'''
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import toymeshpathtracer_amd as tm
tris, bmin, bmax = tm.load_scene(sys.argv[2])
cam = tm.Camera.for_scene(bmin, bmax, 64, 36)
out = {}
try:
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        for cull in (0, 1):
            sc.set_option("pop_cull", cull)
            for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
                img, rays = sc.trace_image(cam, 64, 36, 4, seed_mode=sm, engine=tm.ENGINE_PERSISTENT)
                out[f"{cull}/{sm}"] = [hashlib.sha256(img.tobytes()).hexdigest(), int(rays)]
except tm.TmptError as e:
    out["error"] = str(e)
print(json.dumps(out))
'''


@pytest.mark.skipif(not os.path.exists(CHECK_LIB),
                    reason="checked build not built (make -C toymeshpathtracer_amd/csrc CHECK=1)")
def test_checked_build(gpu):
    """The teapot frame under the checked library (device index tests on every
    node, leaf range and stack depth): no chk code is set with culling on or
    off, and the frames agree."""
    env = dict(os.environ, TMPT_NO_TORCH="1", TMPT_LIB_PATH=CHECK_LIB)
    env.pop("TMPT_CHECK_SELFTEST", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, data("teapot.obj")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert "error" not in got, got["error"]
    assert "device index check failed" not in r.stderr
    for sm in (tm.SEED_SAMPLE, tm.SEED_PIXEL, tm.SEED_ROW):
        assert got[f"1/{sm}"] == got[f"0/{sm}"], sm
