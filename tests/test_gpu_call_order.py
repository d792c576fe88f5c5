"""Every ordered pair of scene calls against fresh-scene results.

include/tmpt.h promises that a call's result is a function of its arguments,
the options in force and the scene's triangles and octree, never of earlier
calls on the handle -- whatever those left in the grow-only buffers of struct
Scene (ws, sbuf, cam_rays, split_buf, split_carry, redo, redo_state, rs_buf,
rs_list, rss_buf, adapt_buf, prog, jt and jt2, motion_prev, clip_stage,
query_buf with its sort events, oct_scratch and oct_flags, the wait event) or
in its mode words (row_render / pixel_render, the adaptive and split pass flags,
prog_key / prog_cam, jt_spp under option sample_base, redo_cap, path_waves_used,
cam_rays_used, split_used, query_sorted, update_kind / cost_known, the triangle
records' flat bit, the last render's statistics).  Here, for every ordered
pair of call kinds (A, B) of tests/call_kinds.py, B after A on one scene equals
B on a fresh scene: bytes, ray count, the whitelisted statistics and the route
markers (call_order.compare) -- on a suzanne scene and on a coincident64 scene
(call_kinds.WORLDS), since the shadow split, its passes and the deferred ties run
only on the second (call_kinds' docstring); A's route there is asserted.  Every fresh-scene result is itself pinned to the
oracle or to the restatement the suite already has for it (call_kinds.pin), so
each equality is, transitively, one with an independent reference.
Tolerance: none.

Sizes: B always at base (40, 22, 6): 880 pixels, ragged against 64 lanes and
256-thread blocks, spp even so that sbuf_pair applies.  A at big (96, 54, 8) and
at tiny (7, 3, 2); the sample-seeded renders also at (8, 4, 1024), which grows
the jump tables to the largest spp and leaves the colour buffer with a
1024-sample stride -- and whose frame against the oracle is the suite's only
check of sample seeding above sample index 63.
"""
import numpy as np
import pytest

import bvh_check
import call_kinds as K
import toymeshpathtracer_amd as tm
from call_order import Kind, Result, compare, first_difference, run_pairs

pytestmark = pytest.mark.gpu


def _device_error(e):
    """Whether a TmptError can mean a device fault: the library's internal error code (-1: a
    failed HIP call is reported so, tmpt_internal.h TMPT_HIP, in the message as "failed (-1)")
    or the name of a HIP call in its text.  A refused argument (-22), memory that does not
    fit (-12) and the like are host-side answers."""
    text = str(e)
    return "failed (-1)" in text or "hip" in text.lower() or "failed (" not in text


def _guard(kind):
    """No call of the matrix may fail (arg_errors catches its own three).  A TmptError that can
    mean a device fault ends the session: nothing more is started on a device that may have
    faulted.  Any other one fails the test it is raised in."""
    def fn(scene, size):
        try:
            return kind.fn(scene, size)
        except tm.TmptError as e:
            if not _device_error(e):
                raise
            pytest.exit(f"{kind.name}{tuple(size)} failed, no further GPU work is started: {e}", returncode=3)
    fn.__doc__ = kind.fn.__doc__
    return Kind(kind.name, fn, kind.world, kind.sample)


KINDS = {name: _guard(k) for name, k in K.KINDS.items()}
NAMES = list(KINDS)
PAIR_CASES = [(a, size, world) for a in NAMES for size in ("big", "tiny") for world in K.WORLDS] + \
             [(a, "spp1024", world) for a in NAMES if KINDS[a].sample for world in K.WORLDS]


class Baselines(dict):
    """baseline[kind, world, size]: the kind's result on a fresh scene of that scene
    definition, computed once, pinned once (call_kinds.pin) and left unchanged.
    A pin that failed fails every test that needs the baseline."""

    def __missing__(self, key):
        name, world, size = key
        with K.world(world).scene() as sc:
            res = KINDS[name].fn(sc, size)
        for a in res.arrays.values():
            a.setflags(write=False)
        try:
            K.pin(name, res, world, size)
            self[key] = res
        except AssertionError as e:
            self[key] = e
        return self[key]

    def __getitem__(self, key):
        v = super().__getitem__(key)
        if isinstance(v, AssertionError):
            raise AssertionError(f"the fresh-scene baseline of {key[0]}{key[2]} on {key[1]} misses its pin: {v}") from v
        return v


@pytest.fixture(scope="module")
def baseline(gpu):
    return Baselines()


def _make_scene(world_name):
    return K.world(world_name).scene()


@pytest.mark.parametrize("world", K.WORLDS)
@pytest.mark.parametrize("name", NAMES)
def test_baseline_equals_its_reference(baseline, name, world):
    """The fresh-scene result of every kind at the base size, on either scene definition,
    against the oracle or its restatement there, with the kind's route marker (call_kinds.pin)."""
    res = baseline[name, world, K.BASE]
    print(name, "rays", res.rays, res.stats, res.route)


@pytest.mark.parametrize("a,a_size,world", PAIR_CASES, ids=[f"{a}-{s}-{wn}" for a, s, wn in PAIR_CASES])
def test_pairs(baseline, a, a_size, world):
    """On one scene of the definition `world` (suzanne, coincident64), for every kind
    B in table order: A at a_size, then B at the base size, the scene never rebuilt
    between the B's; B equals its baseline on that definition.  Where A returns a frame of
    tmpt_render's, each of its frames equals the oracle's too, and the split,
    split-passes and deferring renders take, as A, the route of the definition
    (call_kinds.a_route): on coincident64 the one they are named for."""
    size = K.SIZES[a_size]

    def a_check(res, scene):
        if a not in K.IMAGE_SEED:
            return []
        return K.a_route(a, res, scene.world.name, size) + K.image_against_oracle(a, res, scene.world.name, size)

    bad = run_pairs(_make_scene, KINDS, a, size, K.BASE, baseline, a_check, worlds=[world])
    assert not bad, "\n".join(bad)


#: the kinds that end a pending progressive sequence, by include/tmpt.h
ENDS_SEQUENCE = {
    "sample_based": "option sample_base: 'A new value drops the tables and invalidates the progressive state'",
    "update_refit_back": "tmpt_scene_update: 'The progressive state is invalidated'",
    "update_rebuild_back": "tmpt_scene_update: 'The progressive state is invalidated'",
}


@pytest.mark.parametrize("seed", ["pixel", "sample"])
@pytest.mark.parametrize("a", NAMES)
def test_between_progressive_passes(baseline, a, seed):
    """Progressive pass 1 (2 of 6 samples) at the base size, A at big, pass 2: the
    last preview is the full render's frame and the rays add up.  On A's own scene
    definition, so the split, split-passes and deferring renders run between the
    passes as such (their route is asserted).  No kind here ends a pending sequence:
    by include/tmpt.h only a pass that does not continue it does ("A call with
    spp_begin > 0 continues the per-pixel state the previous call on this scene left
    for the same shard"), and a refused continuation must leave the valid one alone:
    arg_errors' (spp_begin 7 of 8 at another size), and one that differs from the
    pending pass in spp_begin alone (3 for 2, same camera, size and seeding).
    The three kinds of ENDS_SEQUENCE are the calls the header says invalidate the
    progressive state: after them the continuation is refused with -22, and a new
    sequence on the same scene gives the full render's frame and rays."""
    sd, full = {"pixel": (tm.SEED_PIXEL, "pixel_ordered"), "sample": (tm.SEED_SAMPLE, "sample_fused_w4")}[seed]
    wd = K.world(K.KINDS[a].world)
    want = baseline[full, wd.name, K.BASE]
    w, h, spp = K.BASE
    cam = wd.camera(w, h)
    with wd.scene() as sc:
        _, r1 = sc.trace_image(cam, w, h, spp, seed_mode=sd, spp_begin=0, spp_count=2)
        res = KINDS[a].fn(sc, K.BIG)
        if a == "arg_errors":
            with pytest.raises(tm.TmptError, match="does not continue the previous pass"):
                sc.trace_image(cam, w, h, spp, seed_mode=sd, spp_begin=3, spp_count=spp - 3)
        if a in ENDS_SEQUENCE:  # the header's exceptions: refused as after a camera change, and a new sequence runs
            with pytest.raises(tm.TmptError, match=r"\(-22\).*does not continue the previous pass"):
                sc.trace_image(cam, w, h, spp, seed_mode=sd, spp_begin=2, spp_count=spp - 2)
            _, r1 = sc.trace_image(cam, w, h, spp, seed_mode=sd, spp_begin=0, spp_count=2)
        last, r2 = sc.trace_image(cam, w, h, spp, seed_mode=sd, spp_begin=2, spp_count=spp - 2)
    route = K.a_route(a, res, wd.name, K.BIG)
    assert not route, "\n".join(route)
    d = first_difference(last, want.arrays["image"])
    assert d is None, f"{a} between the passes ({seed} seeding) on {wd.name}: bytes of the last preview: {d}"
    assert r1 + r2 == want.rays, f"{a} between the passes ({seed} seeding) on {wd.name}: rays {r1} + {r2} != {want.rays}"


@pytest.mark.parametrize("rebuild", [False, True], ids=["raw", "canonical-with-rebuild"])
@pytest.mark.parametrize("world_name", ["suzanne", "coincident64"])
def test_bvh_words_survive_everything(gpu, world_name, rebuild):
    """Every kind once at big and once at base, in table order and then in
    reverse: the nodes and triangle records of the scene's BVH are the same words
    afterwards, the flat bit that octree_rebuild cleared and set again included.
    Raw over every kind but update_rebuild_back, whose rebuild renumbers the nodes
    within a level (include/tmpt.h, tmpt_scene_dump_bvh "order"); with it, the nodes
    renumbered breadth-first (bvh_check.canonical), the records raw, info equal."""
    names = [n for n in NAMES if rebuild or n != "update_rebuild_back"]
    assert len(names) == len(NAMES) - (not rebuild)
    with K.world(world_name).scene() as sc:
        before = sc.dump_bvh()
        for name in names + names[::-1]:
            for size in (K.BIG, K.BASE):
                KINDS[name].fn(sc, size)
        after = sc.dump_bvh()
    assert after["info"] == before["info"]
    nodes = (bvh_check.canonical(after), bvh_check.canonical(before)) if rebuild else (after["nodes"], before["nodes"])
    parts = {"nodes": nodes, "tris": (after["tris"], before["tris"])}
    for part, (a, b) in parts.items():
        d = first_difference(a, b)
        assert d is None, f"{world_name} {part}: {d}"


@pytest.mark.parametrize("name", NAMES)
def test_close_after_every_kind(baseline, name):
    """A fresh scene, one call, close(); a second fresh scene's same call equals
    the baseline: destroying a scene after each kind of buffer was allocated leaves
    the device usable.  (No assertion on free memory: other work shares the device.)"""
    wd = K.world(K.KINDS[name].world)
    want = baseline[name, wd.name, K.BASE]
    sc = wd.scene()
    KINDS[name].fn(sc, K.BIG)
    sc.close()
    sc.close()  # and a second close is harmless
    with wd.scene() as sc:
        bad = compare(KINDS[name].fn(sc, K.BASE), want)
    assert not bad, "\n".join(bad)


NEW_NAMES = NAMES[25:]


@pytest.mark.parametrize("name", NEW_NAMES)
def test_pin_notices_one_flipped_word(baseline, name):
    """Every array of the baseline of a kind added after the first 25, on the kind's own
    definition: with one bit of one word flipped (the middle word; for the spp map, the
    hit bits and the packed frames the lowest bit, for floats the lowest mantissa bit)
    call_kinds.pin raises.  The pins of these kinds are comparisons, and each array of
    a result is compared."""
    wd = K.KINDS[name].world
    res = baseline[name, wd, K.BASE]
    K.pin(name, res, wd, K.BASE)
    assert res.arrays
    for key, a in res.arrays.items():
        b = a.copy()
        words = b.view(np.uint8).reshape(-1)
        words[(words.size // 2) & ~3] ^= 1
        flipped = Result(dict(res.arrays, **{key: b}), res.rays, res.stats, res.route, res.seen)
        with pytest.raises(AssertionError):
            K.pin(name, flipped, wd, K.BASE)
