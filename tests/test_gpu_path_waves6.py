"""Six waves per SIMD for the shadow split's path kernels (render option
path_waves=6: the OCC 6 lines of kPathVariants, their LDS layout kPathSL6 /
kTopNodes6, the closest-hit-only node step) -- a render with it against the
same render at path_waves=5 and with shadow_split=0 on one scene object, and
where it says so against the oracle's sample-seeded frame.
Tolerance: none -- frame bytes, ray totals (closest-hit and shadow apart) and
the tie / crack / redo counts.
"""
import functools
import os

import numpy as np
import pytest

import geometry_cases as G
import oracle
import ref_cases as C
import toymeshpathtracer_amd as tm
from conftest import data

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 36
SL6 = 12  # kPathSL6 (tmpt_path.h): the 6-wave kernels' LDS stack entries per lane
KEYS = ("extend_rays", "shadow_rays", "tie_queries", "crack_queries", "root_misses", "redo_samples", "redo_late",
        "tie_path")


def _render(sc, cam, spp, waves, split=1, w=W, h=H, seed_mode=tm.SEED_SAMPLE, **kw):
    sc.set_option("shadow_split", split)
    sc.set_option("path_waves", waves)
    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=seed_mode, **kw)
    st = sc.stats()
    return (img.tobytes(), rays, {k: getattr(st, k) for k in KEYS}, int(sc.get_option("path_waves_used")),
            int(sc.get_option("shadow_split_used")), st)


def _six_five_fused(sc, cam, what, spp=4, passes=1, **kw):
    """path_waves 6 against path_waves 5 and against shadow_split 0 on the same
    scene object: byte-identical frames, equal ray totals, equal tie, crack and
    redo counts; the 6-wave render ran the 6-wave twin under the split.
    -> the 6-wave render's (frame bytes, rays, stats)"""
    fused = _render(sc, cam, spp, 5, split=0, **kw)
    five = _render(sc, cam, spp, 5, **kw)
    six = _render(sc, cam, spp, 6, **kw)
    print(what, "waves used", five[3], six[3], "split passes", five[4], six[4], "rays", six[1], six[2])
    assert fused[3:5] == (5, 0) and five[3:5] == (5, passes), what
    assert six[3:5] == (6, passes), f"{what}: path_waves_used, shadow_split_used = {six[3:5]}"
    for other, nm in ((five, "path_waves 5"), (fused, "shadow_split 0")):
        assert six[1] == other[1] and six[2] == other[2], f"{what}: rays / counts {six[1:3]} != {nm}'s {other[1:3]}"
        assert six[0] == other[0], f"{what}: frame differs from {nm}'s"
    return six[0], six[1], six[5]


def _obj_scene(path):
    tris, bmin, bmax = tm.load_scene(path)
    return tris, (bmin, bmax), tm.Camera.for_scene(bmin, bmax, W, H)


def _look_camera(lo, hi, d, k, fov):
    """Camera.create at k box diagonals from the box centre along d (test_gpu_shadow_split's placement)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    at, dist = 0.5 * (lo + hi), k * float(np.linalg.norm(hi - lo))
    d = np.array(d) / np.linalg.norm(d)
    return tm.Camera.create(at + dist * d, at, [0.0, 1.0, 0.0], fov, W / H, 0.02 * dist, dist)


@functools.lru_cache(maxsize=None)
def _case_scene(name):
    tris, lo, hi = C.with_floor(G.case(name))
    tris.setflags(write=False)
    return tris, lo, hi


@pytest.mark.gpu
def test_blocks_and_tail_units(gpu):
    """cube at 4, 5 and 7 spp: blocks of one sample and single-sample tail
    units; its 3 BVH4 nodes are fewer than the LDS top copy holds.  The frame
    is also the oracle's sample-seeded one (octree, visit-order ties)."""
    tris, bounds, cam = _obj_scene(data("cube.obj"))
    osc = oracle.Scene(tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=bounds[0], bmax=bounds[1])
    with tm.Scene(tris, bounds=bounds) as sc:
        assert sc.stats().bvh4_nodes < 64
        for spp in (4, 5, 7):
            frame, rays, _ = _six_five_fused(sc, cam, f"cube x{spp}", spp=spp)
            ref, ref_rays = osc.render(cam.as_array(), W, H, spp, seed_mode=oracle.SEED_SAMPLE)
            assert rays == ref_rays and frame == ref.tobytes(), f"cube x{spp}: not the oracle's frame"


@pytest.mark.gpu
def test_tree_larger_than_the_top_cache(gpu):
    """soup4096 (geometry_cases): 1,227 BVH4 nodes, so most of the walk is
    below the 64 nodes of the 6-wave kernels' LDS copy."""
    tris = G.case("soup4096")
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        assert sc.stats().bvh4_nodes > 1000
        _six_five_fused(sc, tm.Camera.for_scene(lo, hi, W, H), "soup4096")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid", "samebox_fan150"])
def test_every_line_launches(gpu, name):
    """The three tie modes' lines.  samebox_fan150 (tests/golden/ref) with
    tie_defer 1 and 0 (TIES 1 through the second camera, whose render defers
    samples, TIES 2 otherwise) and built without the octree (TIES 0).  grid has triangles flat on
    octree planes, so with the octree its shadow answers can need it and there
    is no split to run at 6 waves (path_waves_used 5); without the octree it
    runs the TIES 0 line."""
    tris, bounds, cam = _obj_scene(os.path.join(ROOT, "tests", "golden", "ref", f"{name}.obj"))
    near = {"grid": ((0.5, 0.5, 0.5), 0.8, 40.0), "samebox_fan150": ((0.1, 0.15, 1.0), 0.6, 50.0)}[name]
    cams = (cam, _look_camera(bounds[0], bounds[1], *near))
    with tm.Scene(tris, bounds=bounds) as sc:
        for defer in (1, 0):
            sc.set_option("tie_defer", defer)
            for k, c in enumerate(cams):
                what = f"{name}, tie_defer {defer}, camera {k}"
                if name == "grid":
                    five, six = _render(sc, c, 4, 5), _render(sc, c, 4, 6)
                    assert six[3:5] == (5, 0) and six[5].octree_flat > 0, what
                    assert six[:3] == five[:3], what
                else:
                    _, _, st = _six_five_fused(sc, c, what)
                    # (the loader's camera stands outside the octree's root box: its rays need
                    # the root-box test, so that render answers its ties in the main loop)
                    if defer and k == 1:
                        assert st.tie_path == 2 and st.redo_samples > 0 and st.redo_late == 0, what
                    else:
                        assert st.tie_path == 1, what
    with tm.Scene(tris) as sc:  # no octree: the lowest index takes a tie (TIES 0)
        for k, c in enumerate(cams):
            _, _, st = _six_five_fused(sc, c, f"{name}, no octree, camera {k}")
            assert st.tie_path == 0


@pytest.mark.gpu
def test_deferral_and_k_redo(gpu):
    """coincident64 (geometry_cases): every hit is a tie, so the redo list
    fills.  redo_inline 1: the 6-wave launch's own waves trace every entry
    (its grid is co-resident: none is left, redo_late 0); redo_inline 0: all
    are left to the k_redo launch after it."""
    tris, lo, hi = _case_scene("coincident64")
    cam = _look_camera(lo, hi, (0.1, 0.15, 1.0), 0.5, 40.0)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        sc.set_option("tie_defer", 1)
        _, _, st = _six_five_fused(sc, cam, "coincident64")
        assert st.tie_path == 2 and st.redo_samples > 0 and st.redo_late == 0
        sc.set_option("redo_inline", 0)
        _, _, st = _six_five_fused(sc, cam, "coincident64, redo_inline 0")
        assert st.redo_late == st.redo_samples > 0


@pytest.mark.gpu
def test_stacks_beyond_the_lds_part(gpu):
    """coincident200 (geometry_cases): identical boxes give a deep tree, and a
    ray through them finds every child of every node, so a lane's stack passes
    the kPathSL6 entries it has in LDS and goes through the spill area, which
    is sized for the 6-wave grid.  The split stays on (asserted by
    _six_five_fused: shadow_split_used 1)."""
    tris, lo, hi = _case_scene("coincident200")
    cam = _look_camera(lo, hi, (0.1, 0.15, 1.0), 0.5, 40.0)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        depth = sc.stats().bvh4_depth
        print("coincident200 bvh4_depth", depth)
        assert 3 * depth > SL6
        for defer in (1, 0):
            sc.set_option("tie_defer", defer)
            _six_five_fused(sc, cam, f"coincident200, tie_defer {defer}")


@pytest.mark.gpu
def test_passes_and_shards(gpu):
    """shadow_split_pass=2 at 7 spp (four passes, each a 6-wave launch), and a
    1/2 shard into a device tile."""
    import torch

    tris, bounds, cam = _obj_scene(data("cube.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        sc.set_option("shadow_split_pass", 2)
        _, _, st = _six_five_fused(sc, cam, "cube x7, 2 samples per pass", spp=7, passes=4)
        assert st.shadow_launches == 4 and st.extend_launches == 4
        sc.set_option("shadow_split_pass", 0)
        for shard in range(2):
            kw = dict(band_rows=1, shard=shard, num_shards=2)
            host = _six_five_fused(sc, cam, f"shard {shard}/2", **kw)
            rows = len(host[0]) // (W * 4)
            tile = torch.empty((rows, W, 4), dtype=torch.uint8, device="cuda:0")
            tile.fill_(7)
            sc.set_option("path_waves", 6)
            none, rays = sc.trace_image(cam, W, H, 4, seed_mode=tm.SEED_SAMPLE, out=tile.data_ptr(), **kw)
            assert none is None and rays == host[1]
            assert sc.get_option("path_waves_used") == 6 and sc.get_option("shadow_split_used") == 1
            assert tile.cpu().numpy().tobytes() == host[0]


@pytest.mark.gpu
def test_where_no_six_wave_kernel_exists(gpu):
    """path_waves=6 runs what 5 runs in pixel seeding, with shadow_split=0 and
    on flat_z (a shadow answer can need the octree: the fused kernel): the same
    frame and counts, and path_waves_used is 5."""
    tris, bounds, cam = _obj_scene(data("cube.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        for what, kw in (("pixel seeding", dict(seed_mode=tm.SEED_PIXEL, engine=tm.ENGINE_PERSISTENT)),
                         ("shadow_split 0", dict(split=0))):
            five, six = _render(sc, cam, 4, 5, **kw), _render(sc, cam, 4, 6, **kw)
            assert five[3:5] == (5, 0) and six[3:5] == (5, 0), what
            assert six[:3] == five[:3], what
    tris, lo, hi = _case_scene("flat_z")
    cam = tm.Camera.for_scene(lo, hi, W, H)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        five, six = _render(sc, cam, 4, 5), _render(sc, cam, 4, 6)
        assert five[3:5] == (5, 0) and six[3:5] == (5, 0)
        assert six[:3] == five[:3]


@pytest.mark.gpu
def test_options(gpu):
    """path_waves takes 0, 4, 5 and 6 and nothing else; path_waves_used is read-only."""
    tris, bounds, _ = _obj_scene(data("cube.obj"))
    for bad in ("path_waves=7", "path_waves=3", "path_waves=1", "path_waves=-1", "path_waves_used=6"):
        with pytest.raises(tm.TmptError):
            tm.Scene(tris, bounds=bounds, options=bad)
    with tm.Scene(tris, bounds=bounds) as sc:
        with pytest.raises(tm.TmptError):
            sc.set_option("path_waves", 7)
        for v in (0, 4, 5, 6):
            sc.set_option("path_waves", v)
            assert sc.get_option("path_waves") == v
