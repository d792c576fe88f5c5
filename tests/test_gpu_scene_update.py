"""Scene updates in place (tmpt_scene_update, Scene.update) on the device.

1  a refit equals the restatement (bvh_refit_restate.refit) raw, word for word: nodes,
   records and info, over the sizes at which the kernels change path, seven option sets
   and the five deformations, chained on one scene (the restated refit reads only the
   links and the records' order of the dump before, which a refit keeps);
2  an update with the scene's own triangles changes no word of either dump;
3  the octree is dropped as if none had been built, and comes back with build_octree;
4  the batched queries after a refit and after a rebuild equal a fresh scene's bit for
   bit, the closest hits the oracle's linear scan;
5  every call kind of call_kinds.KINDS after an update equals the kind on a fresh scene
   of the new triangles (call_order.compare), the fresh image kinds the oracle's frames;
6  a progressive pass cannot continue across an update; a full sequence after it can;
7  a rebuild to another triangle count and back;
9  option bvh_cost against bvh_check.cost.
(8, a failed rebuild: no case of geometry_cases fails its build -- test_gpu_build_geometry.py
builds every one -- so there is no device test of it.)

No tolerance anywhere but in 9, whose 1e-9 is the issue's (two float64 sums of the same
at most 4 * n_nodes4 non-negative terms in another order: < 1e-12 relative).
"""
import functools

import numpy as np
import pytest

import bvh_check as B
import bvh_refit_restate as F
import call_kinds as K
import geometry_cases as G
import oracle
import ref_cases
import toymeshpathtracer_amd as tm
from call_order import Result, compare, first_difference
from conftest import data

pytestmark = pytest.mark.gpu
f32 = np.float32

SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257)
CASES = tuple(f"soup{n}" for n in SIZES) + ("soup1025", "coincident64", "nested200")
OPTION_SETS = ({}, {"leaf_max": 1}, {"leaf_max": 4}, {"leaf_max": 16}, {"collapse": "sah"}, {"builder": "lbvh"},
               {"layout": "soa"})


def opt_id(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


@functools.lru_cache(maxsize=None)
def case_tris(name):
    t = np.zeros((0, 3, 3), f32) if name == "soup0" else G.case(name)
    t.setflags(write=False)
    return t


def same_dump(got, want, tag):
    """-> differences between two dumps, raw."""
    bad = []
    if got["info"] != want["info"]:
        bad.append(f"{tag}: info {got['info']} != {want['info']}")
    for part in ("nodes", "tris"):
        d = first_difference(got[part], np.asarray(want[part], np.uint32))
        if d:
            bad.append(f"{tag}: {part}: {d}")
    return bad


# ---------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("name", CASES)
def test_refit_equals_the_restatement(gpu, name):
    tris = case_tris(name)
    bad = []
    for opts in OPTION_SETS:
        with tm.Scene(tris, options=opts or None) as sc:
            before = sc.dump_bvh()
            soa = before["info"]["soa"] == 1  # the empty scene has no planes
            assert soa == (opts.get("layout") == "soa" and len(tris) > 0)
            assert sc.get_option("update_kind") == 0
            # identity first: the scene's own triangles change nothing
            sc.update(tris, "refit")
            assert sc.get_option("update_kind") == 1 and sc.get_option("update_ms") >= 0.0
            now = sc.dump_bvh()
            bad += same_dump(now, before, f"{name} [{opt_id(opts)}] identity")
            for dname, deform in F.DEFORMATIONS.items():
                tag = f"{name} [{opt_id(opts)}] {dname}"
                new = deform(tris)
                want = F.refit(now, new)
                assert want["near_exponent_boundary"] == 0, f"{tag}: replace this case"
                sc.update(new, "refit")
                now = sc.dump_bvh()
                bad += same_dump(now, want, tag)
                soa_dump = sc.dump_bvh("soa") if soa else None
                bad += [f"{tag}: {b}" for b in B.check(new, now, opts, stats=sc.stats(),
                                                       pop_key=sc.get_option("pop_key_bits"), soa=soa_dump)]
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("opts", [{}, {"layout": "soa"}, {"leaf_max": 16, "collapse": "sah"}], ids=opt_id)
def test_identity(gpu, opts):
    """A refit with the scene's own triangles keeps every word of both dumps, raw; after a
    deformation and back again they are the built ones."""
    tris = case_tris("soup257")
    soa = opts.get("layout") == "soa"
    with tm.Scene(tris, options=opts) as sc:
        first = sc.dump_bvh(), (sc.dump_bvh("soa") if soa else None)
        for step in (tris, F.twist(tris), tris):
            sc.update(step, "refit")
        bad = same_dump(sc.dump_bvh(), first[0], "aos")
        if soa:
            bad += same_dump(sc.dump_bvh("soa"), first[1], "soa")
    assert not bad, "\n".join(bad)


def test_refit_with_another_n_is_refused(gpu):
    tris = case_tris("soup64")
    with tm.Scene(tris) as sc:
        before = sc.dump_bvh()
        with pytest.raises(tm.TmptError, match=r"\(-22\).*a refit keeps the triangle count"):
            sc.update(case_tris("soup65"), "refit")
        assert sc.get_option("update_kind") == 0 and sc.n == 64
        assert not same_dump(sc.dump_bvh(), before, "after the refused call")


# ---------------------------------------------------------------- 3
def _flat(tris, box):
    n = tris.shape[0]
    rays = np.zeros((n, 6), f32)
    rays[:, 5] = 1.0
    flags, _ = tm.octree_flags(tris, box[0], box[1], rays, np.ones(n, f32), np.arange(n, dtype=np.int32))
    return (flags & 1).astype(bool)


def _bounds(tris):
    """The OBJ bounds of a scene whose last two triangles are the floor (ref_cases.with_floor)."""
    v = np.asarray(tris, f32)[:-2].reshape(-1, 3)
    return v.min(0), v.max(0)


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_octree_state(gpu, mode):
    tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    new = F.twist(tris)
    nb = _bounds(new)
    box = tm.octree_bounds(*nb)
    with tm.Scene(tris, bounds=(bmin, bmax)) as sc:
        st = sc.stats()
        assert st.octree_nodes > 0 and st.octree_flat > 0 and st.tie_rule == 0
        assert (sc.dump_bvh()["tris"][:-1, 9] & 1).sum() == st.octree_flat
        sc.update(new, mode)
        st = sc.stats()
        assert (st.octree_nodes, st.octree_leaves, st.octree_refs, st.octree_depth, st.octree_flat) == (0, 0, 0, 0, 0)
        assert st.tie_rule == 1
        dump = sc.dump_bvh()
        assert not (dump["tris"][:, 9] & 1).any()
        assert B.check(new, dump, {}, stats=st, pop_key=sc.get_option("pop_key_bits")) == []
        # a box whose middle plane is the floor's (test_gpu_bvh_structure.py's second box): the two
        # floor triangles are flat there, so the marks are seen to come back; then the new bounds' box
        half = f32(2.0 ** np.ceil(np.log2(2.0 * float(box[1][1] - box[0][1]))))
        lo2, hi2 = box[0].copy(), box[1].copy()
        lo2[1], hi2[1] = new[-1, 0, 1] - half, new[-1, 0, 1] + half
        for bx in ((lo2, hi2), box):
            sc.build_octree(*bx)
            flat = _flat(new, bx)
            st = sc.stats()
            assert st.octree_flat == flat.sum() and st.tie_rule == 0
            assert B.check(new, sc.dump_bvh(), {}, stats=st, flat=flat) == []
            assert flat[-2:].all() == (bx is not box)
        want = tm.octree_digest(new, *box)
        assert (st.octree_nodes, st.octree_leaves, st.octree_refs, st.octree_depth) == \
            (want["nodes"], want["leaves"], want["refs"], want["depth"])
        # and the octree's answers are the new triangles': the frame of a fresh scene's
        w, h, spp = K.TINY
        cam = tm.Camera.for_scene(*nb, w, h)
        got = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_ROW)
    osc = oracle.Scene(new, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=nb[0], bmax=nb[1])
    assert want["digest"] == osc.octree_digest()
    ref = osc.render(cam.as_array(), w, h, spp, seed_mode=oracle.SEED_ROW)
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]


# ---------------------------------------------------------------- 4
def quarter_turn(tris):
    """(x, y, z) -> (z, y, -x): exact in float32, so every coincidence survives bit for bit."""
    t = np.asarray(tris, f32)
    return np.stack([t[..., 2], t[..., 1], -t[..., 0]], -1).astype(f32)


def half_turn(tris):
    """(x, y, z) -> (-x, y, -z): the quarter turn twice, as exact."""
    t = np.asarray(tris, f32)
    return np.stack([-t[..., 0], t[..., 1], -t[..., 2]], -1).astype(f32)


def _answers(sc, rays, rng, r8):
    out = {}
    for any_hit in (False, True):
        ids, hits = sc.hit_scene_batch(rays, *rng, any_hit=any_hit)
        ids8, hits8 = sc.hit_scene_batch(r8, any_hit=any_hit)
        if any_hit:  # only the hit bit of an any-hit answer is defined
            out["any"], out["any ranged"] = (ids >= 0), (ids8 >= 0)
        else:
            out.update({"ids": ids, "hits": hits, "ids ranged": ids8, "hits ranged": hits8})
    return out


@pytest.mark.parametrize("name, deform", [("soup257", F.twist), ("soup1025", F.jitter), ("coincident64", quarter_turn)],
                         ids=["soup257-twist", "soup1025-jitter", "coincident64-turn"])
def test_answers(gpu, name, deform):
    tris = case_tris(name)
    new = deform(tris)
    rays, rng = G.rays(new, 256, seed=7)
    diag = float(np.linalg.norm(new.reshape(-1, 3).max(0) - new.reshape(-1, 3).min(0)))
    ranges = np.array([rng, (rng[0], 0.5 * diag), (0.3 * diag, rng[1])], f32)
    r8 = np.concatenate([rays, ranges[np.arange(len(rays)) % 3]], 1).astype(f32)
    with tm.Scene(new) as sc:
        fresh = _answers(sc, rays, rng, r8)
    oids, ohits = oracle.Scene(new, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX).hit_batch(rays, *rng)
    assert np.array_equal(fresh["ids"], oids)
    hit = oids >= 0
    assert np.array_equal(fresh["hits"][hit, 6].view(np.uint32), ohits[hit, 6].view(np.uint32))
    assert hit.sum() >= 64 and fresh["any"].sum() >= 64
    for mode in ("refit", "rebuild"):
        with tm.Scene(tris) as sc:
            _answers(sc, *G.rays(tris, 256, seed=7), r8)  # the old scene answers first
            sc.update(new, mode)
            got = _answers(sc, rays, rng, r8)
        for key, want in fresh.items():
            d = first_difference(got[key], want)
            assert d is None, f"{name} after a {mode}: {key}: {d}"


# ---------------------------------------------------------------- 5
def _world(name):
    """The updated definitions, named as the original ones (the denoise kind looks its fixed
    inputs up by that name and reads no geometry; nothing else here goes by the name):
    suzanne twisted by 90 degrees, floor included (the floor lies at the bottom: it stays);
    coincident64 with its floor under the exact half turn (x, y, z) -> (-x, y, -z).  Bounds and
    cameras from the new triangles, as call_kinds.world derives them from the old.
    Not the quarter turn (x, y, z) -> (z, y, -x): it has no flat triangle either, but it
    exchanges the x and z extents of the bounds (0.058 and 0.141), and call_kinds.world's camera,
    half a diagonal along +z from the centre, then stands outside the octree's root box (the
    bounds + 0.7 of their size a side): the camera rays need the root-box test, the render keeps
    the ties in the main loop (tie_path 1, tmpt_render.hip `defer`), and sample_deferred would
    not defer.  The half turn keeps the extents, so the camera stays inside and every route
    marker holds; test_answers keeps the quarter turn, where no camera is involved."""
    old = K.world(name)
    if name == "suzanne":
        new = F.twist(old.tris)
        lo, hi = _bounds(new)
        return K.World(name, new, lo, hi, lambda w, h: tm.Camera.for_scene(lo, hi, w, h))
    new = half_turn(old.tris)
    lo, hi = _bounds(new)

    def camera(w, h):  # call_kinds.world's, over the new bounds
        a, b = lo.astype(np.float64), hi.astype(np.float64)
        at, dist = 0.5 * (a + b), 0.5 * float(np.linalg.norm(b - a))
        d = np.array((0.1, 0.15, 1.0)) / np.linalg.norm((0.1, 0.15, 1.0))
        return tm.Camera.create(at + dist * d, at, [0.0, 1.0, 0.0], 40.0, w / h, 0.02 * dist, dist)

    return K.World(name, new, lo, hi, camera)


@functools.lru_cache(maxsize=None)
def new_world(name):
    return _world(name)


@pytest.fixture(scope="module")
def fresh(gpu):
    """fresh[world][kind]: every kind at the base size on a fresh scene of the new triangles,
    once; the image kinds pinned to the oracle's octree scene of the new triangles."""
    out = {}
    for wname in K.WORLDS:
        wd = new_world(wname)
        out[wname] = {}
        for name, kind in K.KINDS.items():
            with wd.scene() as sc:
                res = kind.fn(sc, K.BASE)
            for a in res.arrays.values():
                a.setflags(write=False)
            out[wname][name] = res
    return out


@pytest.mark.parametrize("wname", K.WORLDS)
def test_fresh_results_of_the_new_triangles(fresh, wname):
    """The comparison's other side pinned: every image kind against the oracle's render of the
    new triangles with their octree, bytes and ray counts; on the half-turned coincident64 the route
    markers, so that test_every_kind_after_an_update cannot pass on the fused route alone."""
    wd = new_world(wname)
    w, h, spp = K.BASE
    bad = []
    frames = {}
    for name, seed in K.IMAGE_SEED.items():
        res = fresh[wname][name]
        index = name == "sample_soa_count" and wname != "suzanne"  # call_kinds: an instrumented render's rule
        if (seed, index) not in frames:
            frames[seed, index] = (wd.osc_index if index else wd.osc).render(wd.camera(w, h).as_array(), w, h, spp,
                                                                             seed_mode=K.OSEED[seed])
        ref, ref_rays = frames[seed, index]
        if res.rays != ref_rays:
            bad.append(f"{name} on {wname}: rays {res.rays} != the oracle's {ref_rays}")
        d = first_difference(res.arrays["image"], ref)
        if d:
            bad.append(f"{name} on {wname}: {d}")
    assert not bad, "\n".join(bad)
    if wname == "coincident64":
        assert fresh[wname]["sample_default"].route["shadow_split_used"] >= 1
        assert fresh[wname]["sample_deferred"].seen["tie_path"] == 2
        assert fresh[wname]["sample_default"].seen["octree_flat"] == 0


OWN_DUMP = ("octree_rebuild", "octree_device_rebuild", "update_refit_back")


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("wname", K.WORLDS)
def test_every_kind_after_an_update(fresh, wname, mode):
    """On one scene created from the ORIGINAL triangles: sample_default at 1024 spp on the tiny
    frame (the matrix's buffer-warming A), update(new, mode, bounds=...), then every kind of
    call_kinds.KINDS in table order at the base size; each equals the kind on a fresh scene of
    the new triangles.  No kind is left out: each reads the scene's geometry through
    scene.world, which is the new definition from the update on.

    After a rebuild every part of every result is compared.  After a refit two parts are
    functions of the tree's shape, which a refit keeps and a fresh build of the new triangles
    does not share, so they are compared with what they must be instead:
      sample_soa_count  node_visits, tri_tests, shadow_node_visits, shadow_tri_tests count the
                        steps of the walk over this tree; they must be positive.  Its bytes,
                        rays and every other statistic are compared with the fresh scene's
      octree_rebuild, octree_device_rebuild, update_refit_back (OWN_DUMP)
                        their result holds the BVH dump: it must be the scene's own dump from
                        straight after the update (which test_refit_equals_the_restatement pins
                        to the restated refit), the flat marks the kind clears and sets again
                        included; the rest of the result (the statistic, the octree dump, the
                        route markers) is compared with the fresh scene's.  update_rebuild_back
                        builds the tree anew: its dump, and the dumps of the kinds after it,
                        are the fresh scene's"""
    old, wd = K.world(wname), new_world(wname)
    bad = []
    visits = ("node_visits", "tri_tests", "shadow_node_visits", "shadow_tri_tests")
    with old.scene() as sc:
        K.KINDS["sample_default"].fn(sc, K.SPP1024)
        sc.update(wd.tris, mode, bounds=(wd.bmin, wd.bmax))
        sc.world = wd
        assert sc.get_option("update_kind") == (1 if mode == "refit" else 2)
        own = sc.dump_bvh()
        for name, kind in K.KINDS.items():
            got, want = kind.fn(sc, K.BASE), fresh[wname][name]
            if mode == "refit" and name == "sample_soa_count":
                assert all(got.stats[v] > 0 for v in visits), got.stats
                keep = lambda r: Result(r.arrays, r.rays, {k: v for k, v in r.stats.items() if k not in visits}, r.route)
                got, want = keep(got), keep(want)
            if mode == "refit" and name in OWN_DUMP:
                want = Result(dict(want.arrays, nodes=B.canonical(own), tris=own["tris"]), want.rays, want.stats, want.route)
            if name == "update_rebuild_back":  # from here on the tree is a build of the new triangles
                own = sc.dump_bvh()
            bad += [f"{name} after a {mode} on {wname}: {d}" for d in compare(got, want)]
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------- 6
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_progressive_state_is_invalidated(gpu, mode):
    old, wd = K.world("suzanne"), new_world("suzanne")
    w, h, spp = K.BASE
    with old.scene() as sc:
        sc.trace_image(old.camera(w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE, spp_begin=0, spp_count=2)
        sc.update(wd.tris, mode, bounds=(wd.bmin, wd.bmax))
        with pytest.raises(tm.TmptError, match=r"\(-22\).*does not continue the previous pass"):
            sc.trace_image(old.camera(w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE, spp_begin=2, spp_count=spp - 2)
        cam = wd.camera(w, h)
        passes = list(sc.trace_progressive(cam, w, h, spp, [2, 3, 1], seed_mode=tm.SEED_SAMPLE))
        full, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
    assert np.array_equal(passes[-1][1], full) and sum(p[2] for p in passes) == rays


# ---------------------------------------------------------------- 7
def test_rebuild_with_another_n(gpu):
    suz, bmin, bmax = tm.load_scene(data("suzanne.obj"))
    soup, slo, shi = ref_cases.with_floor(case_tris("soup64"))
    w, h, spp = K.BASE
    render_options = {"shadow_order": 1.0, "aov_group": 4.0, "sample_block": 2.0, "pop_cull": 0.0}

    def frame(sc, lo, hi):
        return sc.trace_image(tm.Camera.for_scene(lo, hi, w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE)

    def fresh_of(tris, lo, hi):
        with tm.Scene(tris, bounds=(lo, hi)) as sc:
            for k, v in render_options.items():
                sc.set_option(k, v)
            return sc.dump_bvh(), frame(sc, lo, hi)

    want = {"soup": fresh_of(soup, slo, shi), "suz": fresh_of(suz, bmin, bmax)}
    with tm.Scene(suz, bounds=(bmin, bmax)) as sc:
        for k, v in render_options.items():
            sc.set_option(k, v)
        frame(sc, bmin, bmax)
        for key, tris, lo, hi in (("soup", soup, slo, shi), ("suz", suz, bmin, bmax)):
            sc.update(tris, "rebuild", bounds=(lo, hi))
            assert sc.n == len(tris) and sc.stats().n_tris == len(tris) and sc.get_option("update_kind") == 2
            dump, (img, rays) = sc.dump_bvh(), frame(sc, lo, hi)
            fd, (fimg, frays) = want[key]
            assert dump["info"] == fd["info"] and np.array_equal(dump["tris"], fd["tris"])
            assert np.array_equal(B.canonical(dump), B.canonical(fd))
            assert np.array_equal(img, fimg) and rays == frays
            assert {k: sc.get_option(k) for k in render_options} == render_options
        # to the empty scene and back to one triangle
        sc.update(np.zeros((0, 3, 3), f32), "rebuild")
        assert sc.dump_bvh()["info"]["n_nodes4"] == 0 and sc.get_option("bvh_cost") == 0.0
        one = case_tris("soup1")
        sc.update(one, "rebuild")
        assert B.check(one, sc.dump_bvh(), {}, stats=sc.stats()) == []
        sc.update(F.jitter(one), "refit")
        assert B.check(F.jitter(one), sc.dump_bvh(), {}, stats=sc.stats()) == []


# ---------------------------------------------------------------- 9
@pytest.mark.parametrize("name, opts", [("soup1025", {}), ("soup257", {"leaf_max": 16}), ("soup1", {}),
                                        ("soup1025", {"layout": "soa", "collapse": "sah"})],
                         ids=["soup1025", "soup257-leaf16", "soup1", "soup1025-soa-sah"])
def test_bvh_cost(gpu, name, opts):
    """Option bvh_cost = bvh_check.cost(dump, tris) within 1e-9 relative after the build and after
    each of the five refits, cached between updates.  On the all-on-one-point refit the root
    box is not empty -- every triangle box is padded by 1e-5 |coordinate| + 1e-30 on each side
    -- so the option is a finite number there too, the same quotient as everywhere (a root of
    area 0, which no padded box gives, would return IEEE's inf or NaN from the division)."""
    tris = case_tris(name)
    with tm.Scene(tris, options=opts or None) as sc:
        steps = [("built", tris)] + [(d, f(tris)) for d, f in F.DEFORMATIONS.items()]
        costs = {}
        for dname, new in steps:
            if dname != "built":
                sc.update(new, "refit")
            got, want = sc.get_option("bvh_cost"), B.cost(sc.dump_bvh(), new)
            print(f"{name} [{opt_id(opts)}] {dname}: bvh_cost {got!r} bvh_check.cost {want!r}")
            assert np.isfinite(want) and want > 0
            assert abs(got - want) <= 1e-9 * want, (dname, got, want)
            assert sc.get_option("bvh_cost") == got  # the cached value
            costs[dname] = got
        if len(tris) > 1:
            # what the option is for: a tree fitted to triangles it was not built for is worse (the
            # twist is no such case: the cost is relative to the root's area, which the twist grows)
            assert costs["permuted"] > 2.0 * costs["built"]
