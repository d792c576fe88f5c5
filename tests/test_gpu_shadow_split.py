"""The shadow split of sample seeding (render option shadow_split: the 5-wave
sample kernel queues its shadow queries, k_shadow answers them from the queue,
k_split_resolve runs each sample's backward recurrence from its record) --
a render with it against the same render without it on one scene object, and
on the CPU the resolve's arithmetic restated from the oracle's pieces against
the oracle's frame.
Tolerance: none -- frame bytes, ray totals and the tie / crack / redo counts.
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
from render_restate import LIGHT, light_cosine, normalize, pack

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 36
KEYS = ("extend_rays", "shadow_rays", "tie_queries", "crack_queries", "root_misses", "redo_samples", "redo_late",
        "tie_path")


def _render(sc, cam, w, h, spp, on, **kw):
    sc.set_option("shadow_split", on)
    img, rays = sc.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, **kw)
    st = sc.stats()
    return img.tobytes(), rays, {k: getattr(st, k) for k in KEYS}, int(sc.get_option("shadow_split_used")), st


def _on_off(sc, cam, what, w=W, h=H, spp=4, **kw):
    """shadow_split 1 against 0 on the same scene object: byte-identical
    frames, equal ray totals (closest-hit and shadow apart), equal tie, crack
    and redo counts.  -> (passes the split ran in, the split render's stats)"""
    off = _render(sc, cam, w, h, spp, 0, **kw)
    on = _render(sc, cam, w, h, spp, 1, **kw)
    assert off[3] == 0, what
    assert on[1] == off[1] and on[2] == off[2], f"{what}: rays / counts {on[1:3]} != {off[1:3]}"
    assert on[0] == off[0], f"{what}: frames differ"
    return on[3], on[4]


def _obj_scene(path):
    tris, bmin, bmax = tm.load_scene(path)
    return tris, (bmin, bmax), tm.Camera.for_scene(bmin, bmax, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "suzanne"])
def test_full_blocks_and_tail_units(gpu, name):
    """4, 5 and 7 spp at 64x36: blocks of one sample and single-sample tail
    units.  cube really runs the split; suzanne has triangles flat on octree
    planes, so its shadow answers can need the octree and it keeps the fused
    kernel (asserted in test_flat_triangles_fall_back for a flat case)."""
    tris, bounds, cam = _obj_scene(data(f"{name}.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        for spp in (4, 5, 7):
            used, st = _on_off(sc, cam, f"{name} x{spp}", spp=spp)
            if name == "cube":
                assert used == 1 and st.shadow_launches == 1 and st.shadow_ms > 0.0


@pytest.mark.gpu
def test_nearly_empty_queue(gpu):
    """triangle.obj: nearly every path misses, so the queue is almost empty."""
    tris, bounds, cam = _obj_scene(data("triangle.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        used, _ = _on_off(sc, cam, "triangle")
        assert used == 1


def _rotated_box():
    """A closed box around the origin, turned so that no face lies on an octree
    plane, its normals pointing inwards: Scatter aims along the stored normal
    (main.cpp:71-72), so a path from inside stays inside."""
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    a, b = 0.37, 0.61
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    c = c @ (rx @ rz).T
    tris = np.array([[c[q[0]], c[q[2]], c[q[1]]] for q in quads] + [[c[q[0]], c[q[3]], c[q[2]]] for q in quads], f32)
    return tris, tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)


@pytest.mark.gpu
def test_camera_inside_a_closed_box(gpu):
    """Nearly every ray hits (one that scatters from an edge may slip out), so
    the paths reach kMaxDepth: ten bounces per sample, the tenth's shadow query
    queued in the round that ends the path."""
    tris, lo, hi = _rotated_box()
    cam = tm.Camera.create([0.1, 0.05, -0.2], [0.4, 0.3, 1.0], [0.0, 1.0, 0.0], 60.0, W / H, 0.01, 1.0)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        used, st = _on_off(sc, cam, "closed box")
        assert used == 1
        assert st.extend_rays >= 0.99 * 10 * W * H * 4 and st.shadow_rays >= 0.99 * 10 * W * H * 4


@pytest.mark.gpu
def test_no_triangles(gpu):
    with tm.Scene(np.zeros((0, 3, 3), f32), bounds=(np.full(3, -1, f32), np.full(3, 1, f32))) as sc:
        cam = tm.Camera.for_scene(np.full(3, -1, f32), np.full(3, 1, f32), W, H)
        _, st = _on_off(sc, cam, "no triangles")
        assert st.shadow_rays == 0 and st.extend_rays == W * H * 4


def _look_camera(lo, hi, d, k, fov):
    """Camera.create at k box diagonals from the box centre along d (test_gpu_reference_mode's placement)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    at, dist = 0.5 * (lo + hi), k * float(np.linalg.norm(hi - lo))
    d = np.array(d) / np.linalg.norm(d)
    return tm.Camera.create(at + dist * d, at, [0.0, 1.0, 0.0], fov, W / H, 0.02 * dist, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid", "samebox_fan150"])
def test_tied_scenes(gpu, name):
    """tests/golden/ref/grid.obj and samebox_fan150.obj, tie_defer on, through
    the loader's camera and test_gpu_reference_mode's.  samebox_fan150 runs the
    split, and through the second camera, which stands inside the octree's
    root box, the deferral too (redo_samples > 0).  grid cannot defer a sample
    from any camera: it has triangles flat on octree planes
    (tmpt_stats.octree_flat), so a shadow answer can need the octree, tie_defer
    is off by its own rule and the render keeps the fused kernel, its ties
    answered in the main loop (tie_queries > 0).
    test_deferral_runs_under_the_split has a scene whose every hit is a tie."""
    tris, bounds, cam = _obj_scene(os.path.join(ROOT, "tests", "golden", "ref", f"{name}.obj"))
    near = {"grid": ((0.5, 0.5, 0.5), 0.8, 40.0), "samebox_fan150": ((0.1, 0.15, 1.0), 0.6, 50.0)}[name]
    with tm.Scene(tris, bounds=bounds) as sc:
        sc.set_option("tie_defer", 1)
        for k, c in enumerate((cam, _look_camera(bounds[0], bounds[1], *near))):
            used, st = _on_off(sc, c, name)
            print(name, "used", used, "tie_path", st.tie_path, "tie_queries", st.tie_queries, "redo_samples",
                  st.redo_samples, "octree_flat", st.octree_flat)
            if name == "grid":
                assert used == 0 and st.octree_flat > 0 and st.tie_queries > 0
            else:
                assert used == 1 and st.octree_flat == 0
                if k == 1:
                    assert st.tie_path == 2 and st.redo_samples > 0


@functools.lru_cache(maxsize=None)
def _case_scene(name):
    tris, lo, hi = C.with_floor(G.case(name))
    tris.setflags(write=False)
    return tris, lo, hi


@pytest.mark.gpu
def test_deferral_runs_under_the_split(gpu):
    """coincident64 (geometry_cases): every hit on its 64 triangles is a tie and
    none is flat, so the deferral applies and its redo list fills -- the
    re-traces resume behind shadow queries that are already queued."""
    tris, lo, hi = _case_scene("coincident64")
    cam = _look_camera(lo, hi, (0.1, 0.15, 1.0), 0.5, 40.0)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        sc.set_option("tie_defer", 1)
        used, st = _on_off(sc, cam, "coincident64")
        assert used == 1 and st.tie_path == 2 and st.redo_samples > 0
        sc.set_option("redo_inline", 0)  # every re-trace left to the k_redo launch
        used, st = _on_off(sc, cam, "coincident64, redo_inline 0")
        assert used == 1 and st.redo_late == st.redo_samples > 0
        sc.set_option("redo_inline", 1)


@pytest.mark.gpu
def test_flat_triangles_fall_back(gpu):
    """flat_z (geometry_cases): a shadow answer can need the octree there
    (PathCtl::oct_shadow), so the render keeps the fused kernel."""
    tris, lo, hi = _case_scene("flat_z")
    cam = tm.Camera.for_scene(lo, hi, W, H)
    with tm.Scene(tris, bounds=(lo, hi)) as sc:
        used, st = _on_off(sc, cam, "flat_z")
        assert used == 0 and st.shadow_launches == 0


@pytest.mark.gpu
def test_several_passes(gpu):
    """64x36x7 with at most 2 samples of every pixel per pass: four passes, the
    pixels' sums carried between them."""
    tris, bounds, cam = _obj_scene(data("cube.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        sc.set_option("shadow_split_pass", 2)
        used, st = _on_off(sc, cam, "cube x7, 2 samples per pass", spp=7)
        assert used == 4 and st.shadow_launches == 4 and st.extend_launches == 4
        sc.set_option("shadow_split_pass", 0)
        used, _ = _on_off(sc, cam, "cube x7", spp=7)
        assert used == 1


@pytest.mark.gpu
def test_shards_and_device_tile(gpu):
    """num_shards = 3 in bands of 1 row, and out = a device tile."""
    import torch

    tris, bounds, cam = _obj_scene(data("cube.obj"))
    with tm.Scene(tris, bounds=bounds) as sc:
        for shard in range(3):
            used, _ = _on_off(sc, cam, f"shard {shard}/3", band_rows=1, shard=shard, num_shards=3)
            assert used == 1
        host = _render(sc, cam, W, H, 4, 0)
        tile = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
        tile.fill_(7)
        sc.set_option("shadow_split", 1)
        none, rays = sc.trace_image(cam, W, H, 4, seed_mode=tm.SEED_SAMPLE, out=tile.data_ptr())
        assert none is None and rays == host[1] and sc.get_option("shadow_split_used") == 1
        assert tile.cpu().numpy().tobytes() == host[0]


@pytest.mark.gpu
def test_options(gpu):
    """shadow_split, shadow_split_max and shadow_split_pass are in the option
    table with their ranges; shadow_split_used is read-only."""
    tris, bounds, _ = _obj_scene(data("cube.obj"))
    for bad in ("shadow_split=2", "shadow_split=-1", "shadow_split_max=-1", "shadow_split_pass=-1",
                "shadow_split_used=1"):
        with pytest.raises(tm.TmptError):
            tm.Scene(tris, bounds=bounds, options=bad)


# ---------------------------------------------------------------- the resolve's arithmetic, on the CPU
def _sky(d):
    t = f32(0.5) * (d[:, 1] + f32(1))
    one, blue = np.ones(3, f32), np.array([0.5, 0.7, 1.0], f32)
    return ((f32(1) - t)[:, None] * one + t[:, None] * blue) * f32(0.5)


def _backward_step(color, cosine):
    albedo = np.array([0.7, 0.7, 0.7], f32) * np.array([0.7, 0.6, 0.5], f32)
    le = np.zeros(3, f32) + albedo * cosine[:, None]
    return le + np.array([0.7, 0.7, 0.7], f32) * color


def test_resolve_restated_equals_the_oracle():
    """One 16x9x4 frame of cube.obj: every sample's record as the split leaves
    it -- the end colour, the depth and the per-bounce light cosines, zeroed
    where the oracle's shadow query hits -- then the backward recurrence from
    the record, the pixel's sum in sample order and the pixel, in numpy float32;
    equal to oracle.Scene.render's frame and ray count."""
    w, h, spp, max_depth = 16, 9, 4, 10
    tris, bmin, bmax = oracle.load_scene(data("cube.obj"))
    osc = oracle.Scene(tris, bmin=bmin, bmax=bmax)
    cam = oracle.camera_for_scene(bmin, bmax, w, h)
    n = w * h * spp
    o, d, state = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, np.uint32)
    inv_w, inv_h = f32(1) / f32(w), f32(1) / f32(h)
    i = 0
    for y in range(h):
        for x in range(w):
            seed = oracle.pixel_seed(x, y, w)
            for s in range(spp):
                st = oracle.sample_seed(seed, s)
                r = oracle.float01_seq(st, 2)
                st = int(oracle.xorshift_seq(st, 2)[1])
                o[i], d[i], state[i] = oracle.get_ray(cam, float((f32(x) + r[0]) * inv_w),
                                                      float((f32(y) + r[1]) * inv_h), st)
                i += 1
    cosines = np.zeros((n, max_depth), f32)
    depth = np.zeros(n, np.int64)
    end = np.zeros((n, 3), f32)
    alive = np.ones(n, bool)
    rays = 0
    with np.errstate(all="ignore"):
        for k in range(max_depth):
            idx = np.nonzero(alive)[0]
            if not len(idx):
                break
            ids, hits = osc.hit_batch(np.concatenate([o[idx], d[idx]], 1), 0.001, 1.0e7)
            rays += len(idx)
            miss = idx[ids < 0]
            end[miss] = _sky(d[miss])
            alive[miss] = False
            hit = idx[ids >= 0]
            pos, nrm = hits[ids >= 0, 0:3], hits[ids >= 0, 3:6]
            rays += len(hit)  # the shadow ray, counted whatever the cosine
            lc = light_cosine(nrm, d[hit])
            sids, _ = osc.hit_batch(np.concatenate([pos, np.broadcast_to(LIGHT, pos.shape)], 1), 0.001, 1.0e7)
            cosines[hit, k] = np.where((lc > 0) & (sids >= 0), f32(0), lc)  # k_shadow's store
            depth[hit] = k + 1
            for j, sample in enumerate(hit):
                rnd, nxt = oracle.unit_vector_seq(int(state[sample]), 1)
                state[sample] = nxt
                target = (pos[j] + nrm[j]) + rnd[0]
                d[sample] = normalize(target - pos[j])
                o[sample] = pos[j]
        # (a path with max_depth hits keeps the end colour 0)
        color = end.copy()
        for k in range(max_depth - 1, -1, -1):
            m = depth > k
            color[m] = _backward_step(color[m], cosines[m, k])
        col = np.zeros((h, w, 3), f32)
        per = color.reshape(h, w, spp, 3)
        for s in range(spp):
            col = col + per[:, :, s]
        got = pack(col * (f32(1) / f32(spp)))
    want, want_rays = osc.render(cam, w, h, spp, seed_mode=oracle.SEED_SAMPLE)
    assert int(depth.max()) >= 2 and int((cosines > 0).sum()) > 0 and rays == want_rays
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"
