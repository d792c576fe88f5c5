"""The kinds of call a scene handle takes, as a table for the call-order matrix
(tests/test_gpu_call_order.py): each kind is a function (scene, size) -> Result
(tests/call_order.py) with size = (w, h, spp), and each has a pin, the check of
its fresh-scene result against the independent reference the suite already has
for it, with the route marker that shows the call took the path it is named for.

Every kind reads the options it needs through get_option, sets them, and puts
them back in a `finally` (options()), so the option flips are part of a scene's
history too.

Scenes.  One definition for nearly every kind: data/suzanne.obj with its floor,
built with bounds= so that the octree answers, through Camera.for_scene.  Three
kinds cannot show their route there: suzanne has triangles flat on octree
planes (tmpt_stats.octree_flat), so a shadow answer can need the octree and the
library keeps the fused kernel and settles ties in the main loop
(tests/test_gpu_shadow_split.py::test_full_blocks_and_tail_units says the
same).  tests/golden/ref/grid.obj has flat triangles too
(test_gpu_shadow_split.py::test_tied_scenes: "grid cannot defer a sample from
any camera"), so it does not help.  sample_default, sample_split_passes and
sample_deferred therefore take their baseline on geometry_cases' coincident64
with its floor, through test_gpu_shadow_split.py's camera inside the root box:
no flat triangle, every hit on its 64 triangles a tie: that definition is those
three kinds' own (Kind.world).
Every kind runs, and is pinned, on both definitions (WORLDS): in the matrix each
kind plays A and B on a suzanne scene and on a coincident64 scene, so the split,
split-passes and deferring renders touch split_buf, split_carry, redo and
redo_state before every B, and every B follows them.  A kind's route marker is
asserted on both definitions; where the route is another one there, that one is
asserted (_marker): on suzanne the three kinds above keep the fused kernel
(shadow_split_used 0, tie_path 1, redo_samples 0).  The markers that are a
property of the frame, not of the route (MARKER_HOME_ONLY), hold on the kind's
own definition.  An instrumented render (count_visits) keeps the lowest-index
leaf even with the octree built (include/tmpt.h TMPT_FLAG_COUNT_VISITS), so on
coincident64, where ties decide pixels, sample_soa_count is pinned to the
oracle's octree scene with TIE_INDEX; on suzanne both tie rules give the
oracle's TIE_VISIT frame, which is the one asserted there.

Statistics compared (Result.stats), each a function of the call and the scene
(read in tmpt_render.hip render(), tmpt_adaptive.hip, tmpt_aov.hip and
tmpt_hitscene.hip): extend_rays, shadow_rays, tie_queries, root_misses,
crack_queries, row_engine, stream_fallbacks, tie_path, redo_samples,
chain_pixels, octree_flat; node_visits, tri_tests, shadow_node_visits and
shadow_tri_tests for the counting kind.  After a call that is not a render only
what include/tmpt.h says the call writes: the AOV pass its rays, extend_launches
and the three octree counters, a HitScene batch tie_queries and root_misses,
tmpt_render_adaptive the summed rays, redo_samples, the octree counters and
tie_path; denoise, camera_rays, radix_sort, the octree rebuild and the refused
calls none.
Left out, and why:
  render_ms, extend_ms, shadow_ms, redo_ms, build_ms, octree_build_ms  times
  redo_late, redo_launches, redo_rays  how many re-traces the main launch's tail
                     took before it ended: residency and timing
  iterations, extend_launches, shadow_launches  counts of launches, not of
                     queries: where the streaming row engine's watchdog falls
                     back (timing) they are the iterated engine's, whose own
                     count follows the windows it sizes by the resident lanes
                     (extend_launches stays where it is the route marker or
                     the header's promise: pixel_ordered, aov; row_iter's
                     iterations > 1 is asserted on its baseline alone)
  tie_queries, root_misses, crack_queries of row_stream: the octree counts every
                     query it answers (tmpt_traverse.h), the speculative units'
                     too, and how far the streaming engine speculates follows the
                     rows still chasing -- timing.  (row_iter and pixel_chains keep
                     them: the iterated engine plans its windows on the device
                     from the frame and the occupancy grid, tmpt_rows.hip
                     render_rowspec, a fixed number of iterations between the
                     host's checks.)
  the build's fields (bvh_nodes ...): the scene's, not a call's
"""
import contextlib
import functools
import math

import numpy as np

import adaptive_nb_restate
import adaptive_restate
import bvh_check
import geometry_cases as G
import oracle
import ref_cases
import render_restate
import toymeshpathtracer_amd as tm
from call_order import Kind, Result
from cam_rays_restate import camera_samples_expect
from conftest import data
from test_gpu_denoise import np_denoise
from test_gpu_denoise import pack as pack_denoised

f32 = np.float32

BASE, BIG, TINY, SPP1024 = (40, 22, 6), (96, 54, 8), (7, 3, 2), (8, 4, 1024)
SIZES = {"base": BASE, "big": BIG, "tiny": TINY, "spp1024": SPP1024}

RENDER_STATS = ("extend_rays", "shadow_rays", "tie_queries", "root_misses", "crack_queries", "row_engine",
                "stream_fallbacks", "tie_path", "redo_samples", "chain_pixels", "octree_flat")
OCTREE_COUNTS = ("tie_queries", "root_misses", "crack_queries")
STREAMING_STATS = tuple(f for f in RENDER_STATS if f not in OCTREE_COUNTS)
COUNT_STATS = RENDER_STATS + ("node_visits", "tri_tests", "shadow_node_visits", "shadow_tri_tests")
AOV_STATS = ("extend_rays", "shadow_rays", "extend_launches") + OCTREE_COUNTS
ADAPTIVE_STATS = ("extend_rays", "shadow_rays", "redo_samples", "tie_path") + OCTREE_COUNTS
HIT_STATS = ("tie_queries", "root_misses")
ROUTE_OPTIONS = ("cam_rays_used", "shadow_split_used")

OSEED = {tm.SEED_ROW: oracle.SEED_ROW, tm.SEED_PIXEL: oracle.SEED_PIXEL, tm.SEED_SAMPLE: oracle.SEED_SAMPLE}


# ----------------------------------------------------------------------------- scene definitions
class World:
    """A scene definition: the triangles, the OBJ bounds the octree is built over,
    the camera of a frame size, and the oracle's scene of the same."""

    def __init__(self, name, tris, bmin, bmax, camera):
        self.name, self.tris, self.bmin, self.bmax, self.camera = name, tris, bmin, bmax, camera
        self.tris.setflags(write=False)

    def scene(self):
        sc = tm.Scene(self.tris, bounds=(self.bmin, self.bmax))
        sc.world = self
        return sc

    @functools.cached_property
    def osc(self):
        return oracle.Scene(self.tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_VISIT, bmin=self.bmin, bmax=self.bmax)

    @functools.cached_property
    def osc_index(self):
        """The oracle's octree scene with ties to the lowest index: an instrumented render's rule."""
        return oracle.Scene(self.tris, accel=oracle.ACCEL_OCTREE, tie=oracle.TIE_INDEX, bmin=self.bmin, bmax=self.bmax)

    @functools.cached_property
    def hit_rays(self):
        """256 fixed rays around the box (geometry_cases.rays: half aimed at triangles, edges and
        vertices among them) and their range; the same with a range of its own per ray."""
        rays, (tmin, tmax) = G.rays(self.tris, 256, seed=7)
        diag = float(np.linalg.norm(self.tris.reshape(-1, 3).max(0) - self.tris.reshape(-1, 3).min(0)))
        ranges = np.array([(tmin, tmax), (tmin, 0.5 * diag), (0.3 * diag, tmax)], f32)
        r8 = np.concatenate([rays, ranges[np.arange(len(rays)) % 3]], 1).astype(f32)
        for a in (rays, r8):
            a.setflags(write=False)
        return rays, (tmin, tmax), r8


@functools.lru_cache(maxsize=None)
def world(name):
    if name == "suzanne":
        tris, bmin, bmax = tm.load_scene(data("suzanne.obj"))
        return World(name, tris, bmin, bmax, lambda w, h: tm.Camera.for_scene(bmin, bmax, w, h))
    assert name == "coincident64"
    tris, lo, hi = ref_cases.with_floor(G.case("coincident64"))

    def camera(w, h):  # test_gpu_shadow_split.py _look_camera: inside the octree's root box
        a, b = lo.astype(np.float64), hi.astype(np.float64)
        at, dist = 0.5 * (a + b), 0.5 * float(np.linalg.norm(b - a))
        d = np.array((0.1, 0.15, 1.0)) / np.linalg.norm((0.1, 0.15, 1.0))
        return tm.Camera.create(at + dist * d, at, [0.0, 1.0, 0.0], 40.0, w / h, 0.02 * dist, dist)

    return World(name, tris, lo, hi, camera)


WORLDS = ("suzanne", "coincident64")


@functools.lru_cache(maxsize=None)
def oracle_frame(world_name, size, seed, tie_index=False):
    """(image, rays) of the oracle's octree scene, computed once and left unchanged."""
    w, h, spp = size
    wd = world(world_name)
    img, rays = (wd.osc_index if tie_index else wd.osc).render(wd.camera(w, h).as_array(), w, h, spp, seed_mode=OSEED[seed])
    img.setflags(write=False)
    return img, rays


@functools.lru_cache(maxsize=None)
def sample_colours(world_name, size_wh, cap):
    wd = world(world_name)
    w, h = size_wh
    col, rays = adaptive_restate.sample_colours(wd.osc, wd.camera(w, h).as_array(), w, h, cap)
    col.setflags(write=False)
    rays.setflags(write=False)
    return col, rays


@functools.lru_cache(maxsize=None)
def denoise_inputs(world_name, size):
    """The denoise kind's inputs: one radiance / AOV pair per size, computed once on a
    fresh scene -- data, not part of any history."""
    wd = world(world_name)
    w, h, spp = size
    with wd.scene() as sc:
        rad, _, _ = sc.trace_radiance(wd.camera(w, h), w, h, spp)
        aov, _ = sc.trace_aov(wd.camera(w, h), w, h, spp)
    rad.setflags(write=False)
    aov.setflags(write=False)
    return rad, aov


# ----------------------------------------------------------------------------- the calls
@contextlib.contextmanager
def options(scene, **kv):
    """The options read back first, set for the call, and put back afterwards."""
    old = {k: scene.get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            scene.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            scene.set_option(k, v)


def _stats(scene, fields, route=ROUTE_OPTIONS, markers=()):
    st = scene.stats()
    seen = {f: getattr(st, f) for f in st.__dataclass_fields__}
    r = {k: int(scene.get_option(k)) for k in route}
    r.update({m: seen[m] for m in markers})
    return {f: seen[f] for f in fields}, r, seen


def _image(scene, size, seed, engine=tm.ENGINE_PERSISTENT, fields=RENDER_STATS, count=False, markers=(), **opts):
    w, h, spp = size
    with options(scene, **opts):
        img, rays = scene.trace_image(scene.world.camera(w, h), w, h, spp, seed_mode=seed, engine=engine,
                                      count_visits=count)
        stats, route, seen = _stats(scene, fields, markers=markers)
    return Result({"image": img}, rays, stats, route, seen)


def row_stream(scene, size):
    """trace_image SEED_ROW, persistent: the streaming speculative row engine."""
    return _image(scene, size, tm.SEED_ROW, fields=STREAMING_STATS, rowspec=1, rowspec_stream=1)


def row_iter(scene, size):
    """The same with rowspec_stream=0: host-driven iterations."""
    return _image(scene, size, tm.SEED_ROW, rowspec=1, rowspec_stream=0)


def row_mega(scene, size):
    """SEED_ROW on the megakernel: one lane per row."""
    return _image(scene, size, tm.SEED_ROW, engine=tm.ENGINE_MEGAKERNEL)


def pixel_ordered(scene, size):
    """SEED_PIXEL, persistent, pilot=2: the cost-ordered supply (the workspace takes the pilot's
    state, the sort, its histogram and the registration words).  tmpt_stats.extend_launches
    reports the two k_path launches, so it is this kind's route marker."""
    return _image(scene, size, tm.SEED_PIXEL, markers=("extend_launches",), pilot=2, pixel_chains=0)


def pixel_chains(scene, size):
    """SEED_PIXEL, pixel_chains=200: the heaviest pixels run as speculative chains."""
    return _image(scene, size, tm.SEED_PIXEL, pilot=2, pixel_chains=200)


def pixel_wavefront(scene, size):
    """SEED_PIXEL on the wavefront engine."""
    return _image(scene, size, tm.SEED_PIXEL, engine=tm.ENGINE_WAVEFRONT)


def pixel_mega(scene, size):
    """SEED_PIXEL on the megakernel."""
    return _image(scene, size, tm.SEED_PIXEL, engine=tm.ENGINE_MEGAKERNEL)


def sample_default(scene, size):
    """SEED_SAMPLE, persistent, the defaults: the camera pre-pass and the shadow split.
    Its own definition is coincident64: suzanne's flat triangles keep the fused kernel (module docstring)."""
    return _image(scene, size, tm.SEED_SAMPLE, cam_pre=-1, shadow_split=1, shadow_split_pass=0, path_waves=0)


def sample_split_passes(scene, size):
    """The same with shadow_split_pass=2: the split in ceil(spp / 2) passes, the sums carried
    in Scene::split_carry.  Its own definition is coincident64, as sample_default's."""
    return _image(scene, size, tm.SEED_SAMPLE, cam_pre=-1, shadow_split=1, shadow_split_pass=2, path_waves=0)


def sample_fused_w4(scene, size):
    """SEED_SAMPLE with shadow_split=0, cam_pre=0, path_waves=4, sample_block=1: the fused 4-wave kernel."""
    return _image(scene, size, tm.SEED_SAMPLE, shadow_split=0, cam_pre=0, path_waves=4, sample_block=1)


def sample_deferred(scene, size):
    """SEED_SAMPLE with tie_defer=1, redo_inline=0, shadow_split=0: tied samples dropped and traced
    again by k_redo.  Its own definition is coincident64 (every hit a tie; suzanne defers nothing,
    module docstring)."""
    return _image(scene, size, tm.SEED_SAMPLE, tie_defer=1, redo_inline=0, shadow_split=0)


def sample_soa_count(scene, size):
    """SEED_SAMPLE with count_visits=True: the instrumented instantiation (in place of a second,
    layout=soa scene).  Its visit counts show a pop_cull or shadow_order default that leaked."""
    return _image(scene, size, tm.SEED_SAMPLE, fields=COUNT_STATS, count=True)


def prepass_fallback(scene, size):
    """SEED_SAMPLE with cam_pre_max=1: the camera pre-pass's buffer does not fit."""
    return _image(scene, size, tm.SEED_SAMPLE, cam_pre=-1, cam_pre_max=1)


def aov(scene, size):
    """trace_aov."""
    w, h, spp = size
    rec, rays = scene.trace_aov(scene.world.camera(w, h), w, h, spp)
    stats, _, seen = _stats(scene, AOV_STATS, route=())
    return Result({"records": rec}, rays, stats, {}, seen)


def _radiance(scene, size, seed):
    w, h, spp = size
    rad, img, rays = scene.trace_radiance(scene.world.camera(w, h), w, h, spp, seed_mode=seed)
    stats, route, seen = _stats(scene, RENDER_STATS)
    return Result({"radiance": rad, "image": img}, rays, stats, route, seen)


def radiance_sample(scene, size):
    """trace_radiance, SEED_SAMPLE."""
    return _radiance(scene, size, tm.SEED_SAMPLE)


def radiance_pixel(scene, size):
    """trace_radiance, SEED_PIXEL."""
    return _radiance(scene, size, tm.SEED_PIXEL)


ADAPTIVE = (4, 4, 0.02)  # spp_min, spp_step, threshold; the cap is spp + 8


def _adaptive(scene, size, **kw):
    w, h, spp = size
    rad, img, cnt, rays, info = scene.trace_adaptive(scene.world.camera(w, h), w, h, spp + 8, *ADAPTIVE, **kw)
    stats, route, seen = _stats(scene, ADAPTIVE_STATS)
    stats.update(passes=info["passes"], samples=info["samples"], pass_pixels=tuple(info["pass_pixels"]))
    return Result({"radiance": rad, "image": img, "spp_map": cnt}, rays, stats, route, seen)


def adaptive(scene, size):
    """trace_adaptive(cap = spp + 8, 4, 4, 0.02)."""
    return _adaptive(scene, size)


def adaptive_nb(scene, size):
    """The same with radius=1, band_rows=4: the neighbourhood rule, band-clipped."""
    return _adaptive(scene, size, radius=1, band_rows=4)


DENOISE_LEVELS = 3


def denoise(scene, size):
    """denoise, levels=3, over the fixed radiance / AOV pair of the size (denoise_inputs)."""
    rad, aov_rec = denoise_inputs(scene.world.name, tuple(size))
    with options(scene, denoise_lds=-1):
        out, img = scene.denoise(rad, aov_rec, size[2], levels=DENOISE_LEVELS)
    return Result({"filtered": out, "image": img})


def hit_closest(scene, size):
    """hit_scene_batch, closest hits of the world's 256 rays in one range."""
    rays, (tmin, tmax), _ = scene.world.hit_rays
    ids, hits = scene.hit_scene_batch(rays, tmin, tmax)
    stats, _, seen = _stats(scene, HIT_STATS, route=())
    return Result({"ids": ids, "hits": hits}, None, stats, {}, seen)


def hit_any_ranged(scene, size):
    """hit_scene_batch, any_hit=True, a range per ray: the hit bits (nothing else of an any-hit answer is defined)."""
    _, _, r8 = scene.world.hit_rays
    ids, _ = scene.hit_scene_batch(r8, any_hit=True)
    stats, _, seen = _stats(scene, HIT_STATS, route=())
    return Result({"hit": (ids >= 0).astype(np.uint8)}, None, stats, {}, seen)


def camera_rays(scene, size):
    """camera_rays: the camera pre-pass alone."""
    w, h, spp = size
    return Result({"entries": scene.camera_rays(scene.world.camera(w, h), w, h, spp)})


@functools.lru_cache(maxsize=None)
def radix_pairs():
    rng = np.random.default_rng(5000)
    keys = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    keys[::7] = keys[3]  # equal keys: stability shows in the values
    vals = np.arange(5000, dtype=np.uint32)
    keys.setflags(write=False)
    vals.setflags(write=False)
    return keys, vals


def radix_sort(scene, size):
    """radix_sort on 5000 fixed pairs, 32 bits."""
    k, v = scene.radix_sort(*radix_pairs(), 32)
    return Result({"keys": k, "vals": v})


def octree_rebuild(scene, size):
    """build_octree with the box moved by +0.25, then with the original box again; the
    result is the BVH dump, whose flat marks the two builds rewrite in place -- the
    triangle records raw, the nodes renumbered breadth-first (bvh_check.canonical): within a
    level two builds of one scene number their nodes differently (include/tmpt.h,
    tmpt_scene_dump_bvh "order"), and the baseline's scene is another build."""
    wd = scene.world
    lo, hi = tm.octree_bounds(wd.bmin, wd.bmax)
    try:
        scene.build_octree(lo + f32(0.25), hi + f32(0.25))
    finally:
        scene.build_octree(lo, hi)
    dump = scene.dump_bvh()
    stats, _, seen = _stats(scene, ("octree_flat",), route=())
    return Result({"nodes": bvh_check.canonical(dump), "tris": dump["tris"]}, None, stats, {}, seen)


ARG_ERRORS = (("spp_1025", "invalid samplesPerPixel"), ("spp_begin", "does not continue the previous pass"),
              ("radius_9", "radius outside 0 .. 8"))


def arg_errors(scene, size):
    """Three calls that host-side validation refuses, launching nothing: spp 1025, an spp_begin
    (spp - 1) that continues no pass, adaptive radius=9.  The result is the messages."""
    w, h, spp = size
    cam = scene.world.camera(w, h)
    calls = (lambda: scene.trace_image(cam, w, h, 1025, seed_mode=tm.SEED_SAMPLE),
             lambda: scene.trace_image(cam, w, h, spp, seed_mode=tm.SEED_SAMPLE, spp_begin=spp - 1),
             lambda: scene.trace_adaptive(cam, w, h, spp + 8, *ADAPTIVE, radius=9))
    route = {}
    for (name, _), call in zip(ARG_ERRORS, calls):
        try:
            call()
            route[name] = "no error"
        except tm.TmptError as e:
            route[name] = str(e)
    return Result(route=route)


KINDS = {k.name: k for k in (
    Kind("row_stream", row_stream), Kind("row_iter", row_iter), Kind("row_mega", row_mega),
    Kind("pixel_ordered", pixel_ordered), Kind("pixel_chains", pixel_chains),
    Kind("pixel_wavefront", pixel_wavefront), Kind("pixel_mega", pixel_mega),
    Kind("sample_default", sample_default, world="coincident64", sample=True),
    Kind("sample_split_passes", sample_split_passes, world="coincident64", sample=True),
    Kind("sample_fused_w4", sample_fused_w4, sample=True),
    Kind("sample_deferred", sample_deferred, world="coincident64", sample=True),
    Kind("sample_soa_count", sample_soa_count, sample=True),
    Kind("aov", aov), Kind("radiance_sample", radiance_sample), Kind("radiance_pixel", radiance_pixel),
    Kind("adaptive", adaptive), Kind("adaptive_nb", adaptive_nb), Kind("denoise", denoise),
    Kind("hit_closest", hit_closest), Kind("hit_any_ranged", hit_any_ranged), Kind("camera_rays", camera_rays),
    Kind("radix_sort", radix_sort), Kind("octree_rebuild", octree_rebuild), Kind("arg_errors", arg_errors),
    Kind("prepass_fallback", prepass_fallback, sample=True))}

#: the seeding of the kinds that return a frame of tmpt_render's
IMAGE_SEED = {"row_stream": tm.SEED_ROW, "row_iter": tm.SEED_ROW, "row_mega": tm.SEED_ROW,
              "pixel_ordered": tm.SEED_PIXEL, "pixel_chains": tm.SEED_PIXEL, "pixel_wavefront": tm.SEED_PIXEL,
              "pixel_mega": tm.SEED_PIXEL, "sample_default": tm.SEED_SAMPLE, "sample_split_passes": tm.SEED_SAMPLE,
              "sample_fused_w4": tm.SEED_SAMPLE, "sample_deferred": tm.SEED_SAMPLE, "sample_soa_count": tm.SEED_SAMPLE,
              "prepass_fallback": tm.SEED_SAMPLE}


# ----------------------------------------------------------------------------- the pins
def image_against_oracle(name, res, world_name, size):
    """-> the differences between an image kind's result and the oracle's frame (the octree's
    with TIE_VISIT; for the instrumented render away from suzanne with TIE_INDEX, module docstring)."""
    ref, ref_rays = oracle_frame(world_name, tuple(size), IMAGE_SEED[name],
                                 tie_index=name == "sample_soa_count" and world_name != "suzanne")
    bad = []
    if res.rays != ref_rays:
        bad.append(f"{name}{tuple(size)} on {world_name}: rays {res.rays} != the oracle's {ref_rays}")
    diff = np.nonzero((res.arrays["image"] != ref).any(-1))
    if diff[0].size:
        bad.append(f"{name}{tuple(size)} on {world_name}: {diff[0].size} pixels differ from the oracle's, first at "
                   f"{list(zip(*diff))[:5]}")
    return bad


#: route markers that are a property of the frame rather than of the route the call takes:
#: asserted on the kind's own definition (the issue's), not on the other one
MARKER_HOME_ONLY = {
    "row_iter": "iterations > 1 follows the frame's rows and windows",
    "pixel_chains": "chain_pixels > 0 needs pixels heavy enough to chain",
}


def a_route(name, res, world_name, size):
    """-> what is wrong with the route of sample_default, sample_split_passes or sample_deferred
    playing A at any size (empty for every other kind): the route options and tie_path are
    functions of the options and the scene (tmpt_render.hip render_persistent: split_on, defer;
    the colour buffer both need is taken whenever a pixel has several blocks, spp >= 2 here)."""
    s, r, spp = res.seen, res.route, size[2]
    own = world_name == "coincident64"
    want = {"sample_default": (1, 1 if own else 0), "sample_split_passes": (1, math.ceil(spp / 2) if own else 0)}
    bad = []
    if name in want and (r["cam_rays_used"], r["shadow_split_used"]) != want[name]:
        bad.append(f"{name}{tuple(size)} on {world_name}: route (cam_rays_used, shadow_split_used) "
                   f"{(r['cam_rays_used'], r['shadow_split_used'])} != {want[name]}")
    if name == "sample_deferred" and s["tie_path"] != (2 if own else 1):
        bad.append(f"{name}{tuple(size)} on {world_name}: route tie_path {s['tie_path']} != {2 if own else 1}")
    return bad


def _marker(name, res, size, world_name):
    s, r, spp = res.seen, res.route, size[2]
    own = world_name == KINDS[name].world
    assert not a_route(name, res, world_name, size), a_route(name, res, world_name, size)
    if name == "row_stream":
        assert (s["row_engine"], s["stream_fallbacks"]) == (3, 0), (s["row_engine"], s["stream_fallbacks"])
    elif name == "row_iter":
        assert s["row_engine"] == 2 and (s["iterations"] > 1 or not own), (s["row_engine"], s["iterations"])
    elif name == "row_mega":
        assert s["row_engine"] == 1
    elif name == "pixel_ordered":
        assert r["extend_launches"] == 2, r
    elif name == "pixel_chains":
        assert s["chain_pixels"] > 0 or not own
    elif name == "sample_fused_w4":
        assert (r["cam_rays_used"], r["shadow_split_used"]) == (0, 0), r
    elif name == "sample_deferred":  # suzanne: oct_shadow_check() keeps the ties in the main loop
        assert (s["redo_samples"] > 0) == own, s["redo_samples"]
    elif name == "sample_soa_count":
        assert s["node_visits"] > 0 and s["tri_tests"] > 0 and s["shadow_node_visits"] > 0
    elif name == "prepass_fallback":
        assert r["cam_rays_used"] == 0, r


def _pin_adaptive(res, wd, size, radius, band_rows):
    w, h, spp = size
    col, rays = sample_colours(wd.name, (w, h), spp + 8)
    if radius:
        n_p, rad, total, pass_pixels = adaptive_nb_restate.adaptive_nb_expect(col, rays, *ADAPTIVE, radius, band_rows)
    else:
        n_p, rad, total, pass_pixels = adaptive_restate.adaptive_expect(col, rays, *ADAPTIVE)
    assert np.array_equal(res.arrays["spp_map"], n_p)
    render_restate.same_bits(res.arrays["radiance"][..., :3], rad, "adaptive radiance")
    assert np.array_equal(res.arrays["image"], render_restate.pack(res.arrays["radiance"]))
    assert res.rays == total and list(res.stats["pass_pixels"]) == pass_pixels
    assert res.stats["samples"] == int(n_p.sum())
    assert res.stats["passes"] >= 2 and len(np.unique(n_p)) >= 2, (res.stats["passes"], np.unique(n_p))


def pin(name, res, world_name, size):
    """The result of kind `name` at `size` on a fresh scene of the definition `world_name`
    against its independent reference there, and its route marker.  Raises AssertionError."""
    wd = world(world_name)
    w, h, spp = size
    cam = wd.camera(w, h).as_array()
    _marker(name, res, size, world_name)
    if name in IMAGE_SEED:
        bad = image_against_oracle(name, res, wd.name, size)
        assert not bad, "\n".join(bad)
    elif name == "aov":
        want, n = render_restate.aov_expect(wd.osc, cam, w, h, spp)
        render_restate.same_records(res.arrays["records"], want)
        assert res.rays == w * h * spp + n["hits"]
    elif name in ("radiance_sample", "radiance_pixel"):
        seed = tm.SEED_SAMPLE if name == "radiance_sample" else tm.SEED_PIXEL
        want, rays = render_restate.radiance_expect(wd.osc, cam, w, h, spp, seed)
        rad = res.arrays["radiance"]
        render_restate.same_bits(rad[..., :3], want, name)
        assert (rad[..., 3].view(np.uint32) == f32(1).view(np.uint32)).all() and res.rays == rays
        assert np.array_equal(res.arrays["image"], render_restate.pack(rad))
        assert np.array_equal(res.arrays["image"], oracle_frame(wd.name, tuple(size), seed)[0])
    elif name == "adaptive":
        _pin_adaptive(res, wd, size, 0, 0)
    elif name == "adaptive_nb":
        _pin_adaptive(res, wd, size, 1, 4)
    elif name == "denoise":
        rad, aov_rec = denoise_inputs(wd.name, tuple(size))
        want = np_denoise(rad, aov_rec, spp, levels=DENOISE_LEVELS)
        render_restate.same_bits(res.arrays["filtered"], want, "denoise")
        assert np.array_equal(res.arrays["image"], pack_denoised(want))
    elif name == "hit_closest":
        rays, (tmin, tmax), _ = wd.hit_rays
        oids, ohits = wd.osc.hit_batch(rays, tmin, tmax)
        ids, hits = res.arrays["ids"], res.arrays["hits"]
        assert np.array_equal(ids, oids), np.nonzero(ids != oids)[0][:8]
        render_restate.same_bits(hits[ids >= 0], ohits[ids >= 0], "hit records")
        assert (ids >= 0).sum() >= 64 and (ids < 0).any()
    elif name == "hit_any_ranged":
        _, _, r8 = wd.hit_rays
        want = np.zeros(len(r8), np.uint8)
        for lo, hi in {(float(a), float(b)) for a, b in r8[:, 6:8]}:
            sel = np.nonzero((r8[:, 6] == f32(lo)) & (r8[:, 7] == f32(hi)))[0]
            want[sel] = wd.osc.hit_batch(r8[sel, :6], lo, hi)[0] >= 0
        assert np.array_equal(res.arrays["hit"], want), np.nonzero(res.arrays["hit"] != want)[0][:8]
        assert want.sum() >= 64 and (want == 0).any()
    elif name == "camera_rays":
        want, _ = camera_samples_expect(cam, w, h, spp)
        got = res.arrays["entries"]
        assert got.shape == (w * h, spp, 8)
        assert np.array_equal(got[..., :7], want.reshape(w * h, spp, 7))
        assert not (got[..., 7] & ~np.uint32(3)).any()
    elif name == "radix_sort":
        keys, vals = radix_pairs()
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(res.arrays["keys"], keys[order]) and np.array_equal(res.arrays["vals"], vals[order])
    elif name == "octree_rebuild":
        with wd.scene() as sc:
            first = sc.dump_bvh()
        assert np.array_equal(res.arrays["tris"], first["tris"])
        assert np.array_equal(res.arrays["nodes"], bvh_check.canonical(first))
    elif name == "arg_errors":
        for key, text in ARG_ERRORS:
            assert text in res.route[key], (key, res.route[key])
    else:
        raise AssertionError(f"no pin for {name}")
