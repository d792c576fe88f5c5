"""Nothing the library takes from HIP outlives its owner (csrc/tmpt_device.h):
the process-wide count of live device allocations, pinned allocations, events
and streams (read-only option live_device_objects) is read through a witness
scene of one triangle, made before anything else here, and must come back to
where it was after every scene that is closed -- whatever calls the scene took,
failed and fallen-back ones included -- and must not move when a call is
repeated (the kept buffers are kept, the temporaries released).

The calls are tests/call_kinds.py's 40 kinds on its two scene definitions at
TINY (7x3x2) and BASE (40x22x6).  Every "does not fit" goes through an option
cap; nothing exhausts device memory and no call here faults."""
import gc

import numpy as np
import pytest

import call_kinds as K
import toymeshpathtracer_amd as tm

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (K.TINY, K.BASE)


@pytest.fixture(scope="module")
def witness(gpu):
    with tm.Scene(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)) as a:
        yield a


def live(witness):
    gc.collect()  # a scene another test left unclosed goes now, not in the middle of a count
    return int(witness.get_option("live_device_objects"))


def make_scene(wd, soa=False, octree=True):
    sc = tm.Scene(wd.tris, options="layout=soa" if soa else None, bounds=(wd.bmin, wd.bmax) if octree else None)
    sc.world = wd
    return sc


def test_the_count_counts(witness):
    """The witness itself holds its stream and four build products; a second scene adds
    as many, its octree three more (nodes, leaf lists, the device view) plus the
    counters it makes for them (device, pinned, two events)."""
    base = live(witness)
    assert base >= 5
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)
    with tm.Scene(tri) as b:
        assert live(witness) == base + 5  # stream, nodes4, tri_pre, tri_orig, node_box
        b.build_octree(*tm.octree_bounds([0, 0, 0], [1, 1, 0]))
        assert live(witness) >= base + 5 + 3 + 4  # (the checked build makes its check words too)
    assert live(witness) == base


@pytest.mark.parametrize("octree", (True, False), ids=("octree", "no-octree"))
@pytest.mark.parametrize("soa", (False, True), ids=("aos", "soa"))
@pytest.mark.parametrize("wname", K.WORLDS)
def test_everything_is_released(witness, wname, soa, octree):
    """Every kind once, at both sizes, on a scene of its own; after close() the count is the
    witness's again."""
    base = live(witness)
    for size in SIZES:
        with make_scene(K.world(wname), soa, octree) as sc:
            for kind in K.KINDS.values():
                kind.fn(sc, size)
            assert live(witness) > base
        assert live(witness) == base, (wname, size)


@pytest.mark.parametrize("size", SIZES, ids=("tiny", "base"))
@pytest.mark.parametrize("wname", K.WORLDS)
def test_kept_buffers_are_kept_and_temporaries_released(witness, wname, size):
    """A call repeated with the same arguments leaves the count where the first left it: what
    the first made and kept (grown on demand, reused across calls) the second reuses or
    replaces one for one, and what either made for itself alone it released."""
    base = live(witness)
    bad = []
    with make_scene(K.world(wname)) as sc:
        for kind in K.KINDS.values():
            kind.fn(sc, size)
            first = live(witness)
            kind.fn(sc, size)
            if live(witness) != first:
                bad.append(f"{kind.name}: {first - base} objects after the first call, {live(witness) - base} after the second")
    assert not bad, "\n".join(bad)
    assert live(witness) == base


def test_failure_and_fallback_paths_release(witness):
    """The calls that fail or fall back, each with the result the suite asserts for it elsewhere,
    then close(): the count is the witness's again."""
    base = live(witness)
    w, h, spp = K.BASE
    suz, tied = K.world("suzanne"), K.world("coincident64")
    with make_scene(tied) as sc:
        cam = tied.camera(w, h)
        want = K.oracle_frame("coincident64", K.BASE, tm.SEED_SAMPLE)
        # a sample-seeded progressive pass without its colour buffer (tests/test_gpu_adaptive.py: -12)
        with K.options(sc, sbuf_max=1):
            with pytest.raises(tm.TmptError, match=r"\(-12\).*colour buffer"):
                sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, spp_begin=0, spp_count=2)
        # the camera pre-pass's buffer does not fit: the render runs without it, the same frame
        res = K.prepass_fallback(sc, K.BASE)
        K.pin("prepass_fallback", res, "coincident64", K.BASE)
        # nor the shadow split's: the fused kernel, the same frame
        with K.options(sc, shadow_split_max=1):
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
            assert sc.get_option("shadow_split_used") == 0
        assert (rays, img.tobytes()) == (want[1], want[0].tobytes())
        # a redo list of one entry overflows: regrown, the frame rendered again (tests/test_gpu_parity.py)
        with K.options(sc, tie_defer=1, shadow_split=0):
            img1, rays1 = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
            redo = sc.stats().redo_samples
            assert redo > 1 and sc.stats().tie_path == 2
            with K.options(sc, redo_cap=1):
                img2, rays2 = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
                assert sc.stats().redo_samples == redo
        assert (rays1, img1.tobytes()) == (want[1], want[0].tobytes()) == (rays2, img2.tobytes())
        # the streaming row engine aborts, the iterated one renders the frame (tests/test_gpu_parity.py)
        ref_row = K.oracle_frame("coincident64", K.BASE, tm.SEED_ROW)
        with K.options(sc, rowstream_test_abort=1):
            img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_ROW)
            st = sc.stats()
            assert st.stream_fallbacks == 1 and st.row_engine == 2
        assert (rays, img.tobytes()) == (ref_row[1], ref_row[0].tobytes())
        K.pin("arg_errors", K.arg_errors(sc, K.BASE), "coincident64", K.BASE)
        lo, hi = tm.octree_bounds(tied.bmin, tied.bmax)
        sc.build_octree(lo, hi)
        sc.build_octree(lo, hi)
        assert sc.stats().octree_nodes > 0
        # updates: a rebuild with another triangle count, to no triangles, back, and a refit
        sc.update(suz.tris, "rebuild", bounds=(suz.bmin, suz.bmax))
        assert sc.stats().n_tris == len(suz.tris.reshape(-1, 9)) and sc.get_option("update_kind") == 2
        sc.update(np.zeros((0, 3, 3), f32), "rebuild")
        assert sc.dump_bvh()["info"]["n_nodes4"] == 0 and sc.get_option("bvh_cost") == 0.0
        sc.update(tied.tris, "rebuild")
        sc.update(tied.tris, "refit", bounds=(tied.bmin, tied.bmax))
        assert sc.get_option("update_kind") == 1 and sc.get_option("bvh_cost") > 0.0
        img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE)
        assert (rays, img.tobytes()) == (want[1], want[0].tobytes())
        K.pin("radix_sort", K.radix_sort(sc, K.BASE), "coincident64", K.BASE)
        assert sc.dump_bvh("aos")["info"]["n"] == len(tied.tris.reshape(-1, 9))
        with pytest.raises(tm.TmptError, match="without layout=soa"):
            sc.dump_bvh("soa")
    with make_scene(tied, soa=True) as sc:
        a, b = sc.dump_bvh("aos"), sc.dump_bvh("soa")
        assert a["info"] == b["info"] and a["info"]["soa"] == 1 and b["nodes"].any() and b["tris"].any()
    # one frame over "two" devices, both device 0: the gather without RCCL
    cam = suz.camera(w, h)
    ref = K.oracle_frame("suzanne", K.BASE, tm.SEED_SAMPLE)
    img, rays, _ = tm.render_multi(suz.tris, cam, w, h, spp, [0, 0], seed_mode=tm.SEED_SAMPLE, bounds=(suz.bmin, suz.bmax))
    assert (rays, img.tobytes()) == (ref[1], ref[0].tobytes())
    with pytest.raises(tm.TmptError, match="device"):
        tm.render_multi(suz.tris, cam, w, h, spp, [0, 99])
    assert live(witness) == base


#: what tmpt_scene_update changes in the count (tmpt_internal.h): the dropped Octree's three
#: buffers (oct, oct_refs, oct_view); a refit's rec_box, made by the first refit of a tree and
#: gone with the tree a rebuild replaces; the two update events, made by a scene's first update.
#: A rebuild's new Bvh has the old one's four buffers (nodes4, tri_pre, tri_orig, node_box), and
#: soa_buf where the scene has layout=soa: no change.  The scene's stream is not among them.
OCTREE_OBJECTS, REC_BOX, UPDATE_EVENTS = 3, 1, 2


@pytest.mark.parametrize("soa", (False, True), ids=("aos", "soa"))
def test_a_rebuild_keeps_the_stream_and_swaps_one_for_one(witness, soa):
    base = live(witness)
    w, h, spp = K.BASE
    suz, tied = K.world("suzanne"), K.world("coincident64")
    want = K.oracle_frame("suzanne", K.BASE, tm.SEED_SAMPLE)
    with make_scene(tied, soa=soa) as sc:
        sc.trace_image(tied.camera(w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE)
        before = live(witness)
        sc.update(tied.tris, "refit")  # the scene's first update: drops the octree
        assert live(witness) == before + UPDATE_EVENTS + REC_BOX - OCTREE_OBJECTS
        sc.build_octree(*tm.octree_bounds(tied.bmin, tied.bmax))
        before = live(witness)
        sc.update(suz.tris, "rebuild")  # another triangle count; the refitted tree and the octree go
        assert live(witness) == before - REC_BOX - OCTREE_OBJECTS
        before = live(witness)
        sc.update(suz.tris, "rebuild")  # nothing to drop: one for one
        assert live(witness) == before
        sc.build_octree(*tm.octree_bounds(suz.bmin, suz.bmax))
        assert live(witness) == before + OCTREE_OBJECTS
        # the scene's own stream still runs its renders: a fresh scene's frame (the oracle's)
        img, rays = sc.trace_image(suz.camera(w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE)
        assert (rays, img.tobytes()) == (want[1], want[0].tobytes())
    assert live(witness) == base
