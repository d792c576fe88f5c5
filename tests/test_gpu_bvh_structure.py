"""The device-built BVH (tmpt_bvh.hip) checked exhaustively from a host dump.

The ray tests (test_gpu_build_geometry.py, test_gpu_ray_cases.py) see the tree
only through sampled rays.  Here every build is dumped (Scene.dump_bvh) and
bvh_check.check() goes through every node, slot, leaf range, triangle record
and box face -- in exact integers, with no tolerance; bvh_check.py states the
rules.  An error no sampled ray meets (a face short by one quantum, a leaf
range off by one triangle) and one that changes no answer (a loose box, nodes
not numbered level by level, a leaf the collapse should have merged) both show
up as findings.

Also here: the dump tied to what the kernels read (a numpy linear scan over
the dumped leaves gives the ids and t bits of hit_scene_batch), the canonical
form of two builds of one scene, and the tree quality (surface-area cost)
against the median-split reference tree and against builder=lbvh.
"""
import functools

import numpy as np
import pytest

import bvh_check as B
import geometry_cases as G
import mt_numpy as mt
import toymeshpathtracer_amd as tm
from conftest import data
from test_gpu_build_geometry import OPTION_SETS, SWEEP_GROUPS, _opt_id

pytestmark = pytest.mark.gpu

FAMILY_OPTIONS = [{}] + OPTION_SETS + [{"collapse": "sah", "leaf_max": 4}, {"layout": "soa", "leaf_max": 16}]


@functools.lru_cache(maxsize=None)
def _cases():
    return G.cases()


def _findings(name, tris, opts, sc, flat=None):
    """Dump the scene and check it -> (findings, each prefixed with the case; the dump)."""
    dump = sc.dump_bvh()
    soa = sc.dump_bvh("soa") if opts.get("layout") == "soa" else None
    bad = B.check(tris, dump, opts, stats=sc.stats(), pop_key=sc.get_option("pop_key_bits"), flat=flat, soa=soa)
    if bool(dump["info"]["soa"]) != (opts.get("layout") == "soa"):
        bad.append(f"info: soa {dump['info']['soa']} on a scene built with {opts}")
    return [f"{name} [{_opt_id(opts)}]: {b}" for b in bad], dump


def _build_and_check(name, opts):
    """name: a case of geometry_cases, or the triangles themselves."""
    tris = _cases()[name] if isinstance(name, str) else name
    label = name if isinstance(name, str) else f"array{len(tris)}"
    try:
        with tm.Scene(tris, options=opts or None) as sc:
            bad, dump = _findings(label, tris, opts, sc)
    except tm.TmptError as e:
        return [f"{label}: {e}"], None
    return bad, dump


@pytest.mark.parametrize("group", list(SWEEP_GROUPS))
def test_count_sweep(gpu, group):
    """Soup of every count the ray tests sweep, default build: partial blocks, tiles and
    waves in the sort, the scans and every per-level launch of the collapse."""
    bad = []
    for n in SWEEP_GROUPS[group]:
        bad += _build_and_check(G.sweep_name(n), {})[0]
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_arrays(gpu, n):
    """n = 0: no node and the one null record; n = 1, 2 (within leaf_max): one node whose
    only child is the leaf of all records -- the one tree where nc = 1."""
    tris = G.soup(n, 11) if n else np.zeros((0, 3, 3), np.float32)
    bad, dump = _build_and_check(tris, {})
    assert not bad, "\n".join(bad)
    info = dump["info"]
    assert (info["n_nodes4"], info["depth4"]) == ((0, 0) if n == 0 else (1, 1))
    assert dump["nodes"].shape == (info["n_nodes4"], 16) and dump["tris"].shape == (n + 1, 12)
    if n:
        assert dump["nodes"][0, 3] >> 24 == 1 and dump["nodes"][0, 12] == B.leaf_link(n, 0, info["count_shift"])


@pytest.mark.parametrize("name", G.NON_SWEEP)
@pytest.mark.parametrize("opts", FAMILY_OPTIONS, ids=_opt_id)
def test_families(gpu, opts, name):
    """Every adversarial family under the default build and every build option.  The
    coincident cases go through PLOC's second tie rule and nested200 through the LBVH
    fallback: both write nodes4 again after an abandoned collapse, so a link beyond
    n_nodes4 (rule tree-reach) would be a leftover of the abandoned one."""
    bad, dump = _build_and_check(name, opts)
    assert not bad, "\n".join(bad[:20])
    lbvh = opts.get("builder") == "lbvh" or name == "nested200"
    assert (dump["info"]["builder_iters"] == 0) == lbvh, dump["info"]


def test_dump_argument_errors(gpu):
    import ctypes
    with tm.Scene(G.soup(5, 1)) as sc:
        with pytest.raises(tm.TmptError, match="without layout=soa"):
            sc.dump_bvh("soa")
        with pytest.raises(ValueError):
            sc.dump_bvh("planes")
        fn = tm._lib.tmpt_scene_dump_bvh
        info = (ctypes.c_int32 * 8)()
        dump = sc.dump_bvh()
        n4, n = dump["info"]["n_nodes4"], 5
        nodes, tris = np.zeros(16 * n4, np.uint32), np.zeros(12 * (n + 1), np.uint32)
        for args, msg in (((sc._h, 0, nodes.ctypes.data, 16 * n4 - 1, tris.ctypes.data, tris.size, info), "short buffer"),
                          ((sc._h, 0, nodes.ctypes.data, nodes.size, tris.ctypes.data, 12 * n, info), "short buffer"),
                          ((sc._h, 0, nodes.ctypes.data, nodes.size, None, 0, info), "both buffers"),
                          ((sc._h, 2, None, 0, None, 0, info), "layout"), ((sc._h, 0, None, 0, None, 0, None), "null")):
            assert fn(*args) == -22 and msg in tm._last_error().decode(), (msg, tm._last_error())
        assert not nodes.any() and not tris.any()  # a refused call writes nothing
        # and the dump changes nothing: a second one is the same, word for word
        again = sc.dump_bvh()
        assert np.array_equal(again["nodes"], dump["nodes"]) and np.array_equal(again["tris"], dump["tris"])


# ---------------------------------------------------------------- OBJ scenes, with the octree
def _load(name, sponza_path):
    return tm.load_scene(sponza_path if name == "sponza" else data(name + ".obj"))


def _flat(tris, box):
    """The triangles flat on a plane of the octree over `box`: tm.octree_flags bit 1 for one
    synthetic query per triangle."""
    n = tris.shape[0]
    rays = np.zeros((n, 6), np.float32)
    rays[:, 5] = 1.0
    flags, _ = tm.octree_flags(tris, box[0], box[1], rays, np.ones(n, np.float32), np.arange(n, dtype=np.int32))
    return (flags & 1).astype(bool)


@pytest.mark.parametrize("name", ["suzanne", "teapot", "sponza"])
def test_obj_scenes_with_octree(gpu, sponza_path, name):
    """The flat marks follow the scene's octree: none before it is built, the set
    octree_flags reports after, and the other set after a second build over another box."""
    tris, bmin, bmax = _load(name, sponza_path)
    with tm.Scene(tris) as sc:
        bad, _ = _findings(name, tris, {}, sc)
        box = tm.octree_bounds(bmin, bmax)
        sc.build_octree(*box)
        flat = _flat(tris, box)
        assert sc.stats().octree_flat == flat.sum()
        bad += _findings(name + "+octree", tris, {}, sc, flat)[0]
        # the second box: wider in x and z, and in y centred on the floor (y = bmin.y, the last
        # two triangles) with a power-of-two half size, so the root's middle plane is the floor's
        half = np.float32(2.0 ** np.ceil(np.log2(2.0 * float(box[1][1] - box[0][1]))))
        lo2 = box[0] - np.float32(0.37) * (box[1] - box[0])
        hi2 = box[1].copy()
        lo2[1], hi2[1] = bmin[1] - half, bmin[1] + half
        sc.build_octree(lo2, hi2)
        flat2 = _flat(tris, (lo2, hi2))
        assert sc.stats().octree_flat == flat2.sum()
        bad += _findings(name + "+octree2", tris, {}, sc, flat2)[0]
        print(f"{name}: n {len(tris)} flat {flat.sum()} -> {flat2.sum()} under the second box")
    assert not bad, "\n".join(bad[:20])
    assert flat2[-2:].all() and not flat[-2:].any()  # the marks moved: the floor is flat under the second box only


@pytest.mark.parametrize("name", ["soup4096", "sponza"])
def test_two_builds_are_equal_in_canonical_form(gpu, sponza_path, name):
    """k_bvh4_level numbers the nodes of a level with an atomic counter, so two builds of one
    input need not be equal raw; renumbered breadth-first in slot order they must be.  The
    triangle records (leaf order) do not depend on that numbering and are equal raw."""
    tris = _cases()[name] if name.startswith("soup") else _load(name, sponza_path)[0]
    dumps = []
    for _ in range(2):
        with tm.Scene(tris) as sc:
            dumps.append(sc.dump_bvh())
    a, b = dumps
    assert a["info"] == b["info"]
    assert np.array_equal(a["tris"], b["tris"])
    raw = np.array_equal(a["nodes"], b["nodes"])
    print(f"{name}: two builds equal raw: {raw} ({int((a['nodes'] != b['nodes']).any(1).sum())} of "
          f"{a['info']['n_nodes4']} node records differ)")
    assert np.array_equal(B.canonical(a), B.canonical(b))


# ---------------------------------------------------------------- the dump is what the kernels read
@pytest.mark.parametrize("name", ["soup272", "degenerate_mix", "one_cell"])
def test_linear_scan_over_the_dumped_leaves(gpu, name):
    """A numpy closest hit (Moller-Trumbore, mt_numpy's order of operations) over every record
    a dumped leaf names gives the ids and t bits hit_scene_batch returns, for 2,000 rays."""
    tris = _cases()[name]
    rays, (tmin, tmax) = G.rays(tris, 2000, seed=3)
    with tm.Scene(tris) as sc:
        dump = sc.dump_bvh()
        ids, hits = sc.hit_scene_batch(rays, tmin, tmax)
    want_ids, want_t = B.closest_hit(dump, rays, tmin, tmax, mt)
    assert (want_ids >= 0).sum() > 200
    w = np.nonzero(ids != want_ids)[0]
    assert w.size == 0, f"{w.size} ids differ, first rays {w[:5]}: gpu {ids[w[:5]]} dump scan {want_ids[w[:5]]}"
    h = ids >= 0
    assert np.array_equal(hits[h, 6].view(np.uint32), want_t[h].view(np.uint32))


# ---------------------------------------------------------------- quality
QUALITY_SCENES = ["soup4096", "suzanne", "teapot", "sponza"]


@functools.lru_cache(maxsize=None)
def _costs(name, sponza_path):
    """-> {"ploc", "lbvh", "median"}: the surface-area cost (bvh_check.cost) of the default
    build, of builder=lbvh and of the median-split reference tree, each dump checked."""
    tris = _cases()[name] if name.startswith("soup") else _load(name, sponza_path)[0]
    out = {}
    for key, opts in (("ploc", {}), ("lbvh", {"builder": "lbvh"})):
        bad, dump = _build_and_check(tris, opts)
        assert not bad, "\n".join(bad[:20])
        out[key] = B.cost(dump, tris)
        out[key + "_nodes"] = dump["info"]["n_nodes4"]
    ref = B.reference_dump(tris)
    out["median"], out["median_nodes"] = B.cost(ref, tris), ref["info"]["n_nodes4"]
    print(f"cost {name}: n {len(tris)} ploc {out['ploc']:.3f} ({out['ploc_nodes']} nodes) lbvh {out['lbvh']:.3f} "
          f"({out['lbvh_nodes']}) median split {out['median']:.3f} ({out['median_nodes']})")
    return out


@pytest.mark.parametrize("name", QUALITY_SCENES)
def test_default_build_is_no_worse_than_the_median_split(gpu, sponza_path, name):
    """cost = sum over valid child slots of area(decoded box) / area(root union) x (1 for a
    node, count for a leaf).  An ordering, not a tolerance."""
    c = _costs(name, sponza_path)
    assert c["ploc"] <= c["median"], c


@pytest.mark.parametrize("name", QUALITY_SCENES)
def test_ploc_costs_less_than_lbvh(gpu, sponza_path, name):
    """DESIGN.md's reason for PLOC as the default builder."""
    c = _costs(name, sponza_path)
    assert c["ploc"] < c["lbvh"], c
