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

The kinds added after the first 25 (the entry points the handle gained since:
KINDS from moments_uniform on; COVERS maps every kind to the Scene methods and
options it exercises, and tests/test_call_kinds_cover.py holds Scene's public
methods to that map).  Their fixed inputs -- the two frames of a sequence the
image-to-image kinds read (temporal_inputs), the guided render's prior
(guided_prior) -- are made once per (definition, size) on fresh scenes and
marked read-only: data, as denoise_inputs is, not part of any scene's history.
  moments_uniform, moments_adaptive, guided   tmpt_render_moments / _guided are
      tmpt_render_adaptive "in every rule": ADAPTIVE_STATS and the info fields, pinned to
      the adaptive restatements over the oracle's per-sample colours with the moments of
      noise_aware_restate.moments_expect at each pixel's count.  guided's marker -- some
      pixel stops at 2, some runs on -- holds in the restatement alone on both
      definitions (test_call_kinds_pins.py shows it without a GPU)
  motion_host_prev   the host prev_tris form, which fills Scene::motion_prev; the
      statistics the header lists for the pass (MOTION_STATS); pinned to
      temporal_restate's pieces with the oracle octree's triangle where a centre ray is
      tied (motion_expect: the scenes here have the octree, the restatement's scan none)
  temporal, temporal_clip_aux, sample_plan, denoise_moments   host arrays, so the clip and
      the plan go through Scene::clip_stage; "the other fields keep the last render's"
      (include/tmpt.h), so no statistic is compared; pinned to temporal_restate.blend,
      temporal_clip_restate.clip, guided_restate.plan, noise_aware_restate.np_denoise_moments
  hit_device_closest, hit_device_any_sorted   a torch tensor of World.hit_rays on the
      scene's device, HIT_STATS, the read-only option query_sorted as the route marker;
      pinned as hit_closest / hit_any_ranged are, (u, v) to Moller-Trumbore's for the
      returned triangle (test_gpu_hit_device.mt_uv)
  sample_waves6   path_waves=6 under the shadow split: (path_waves_used,
      shadow_split_used) = (6, 1) on coincident64, its own definition, and (5, 0) on
      suzanne, whose flat triangles leave no split to run at six waves
  sample_based   option sample_base=24, put back to 0 afterwards: both changes drop the
      jump tables (Scene::jt_spp) and end a pending progressive sequence; pinned to samples
      [24, 24 + spp) of the oracle's per-sample colours
  update_refit_back, update_rebuild_back   an update to World.moved and back, bounds=
      building the octree again (on the device: profiles/call_order_durations.log has the
      host build's cost); route marker update_kind.  The result is the BVH dump
      (nodes canonical, records raw: update_refit_back's docstring says why not raw
      nodes across scenes, and what is compared raw instead) and the octree dump raw,
      pinned to a fresh scene's
  octree_device_rebuild   octree_rebuild under octree_build=device, with the octree
      dump, raw, against a fresh host-built scene's word for word
Left out, and why:
  every statistic after temporal, temporal_clip_aux, sample_plan and denoise_moments:
                     the header promises render_ms alone, a time
  shadow_rays after motion_host_prev: the header's list for the pass does not name it
  every statistic after the update kinds: the header names none (update_ms is a time,
                     bvh_cost is test_gpu_scene_update.py::test_bvh_cost's)
  any-hit ids, records and (u, v) of hit_device_any_sorted: only the hit bit is
                     specified across routes (include/tmpt.h); that a reported record
                     is the reported triangle's is test_gpu_hit_device.py's
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
import dataclasses
import functools
import math

import numpy as np

import adaptive_nb_restate
import adaptive_restate
import bvh_check
import geometry_cases as G
import guided_restate
import noise_aware_restate
import oracle
import ref_cases
import render_restate
import temporal_clip_restate
import temporal_restate
import toymeshpathtracer_amd as tm
from call_order import Kind, Result, first_difference
from cam_rays_restate import camera_samples_expect
from conftest import data
from test_gpu_denoise import np_denoise
from test_gpu_denoise import pack as pack_denoised
from test_gpu_hit_device import mt_uv

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
MOTION_STATS = ("extend_rays", "extend_launches") + OCTREE_COUNTS
ROUTE_OPTIONS = ("cam_rays_used", "shadow_split_used")
WAVES_OPTIONS = ROUTE_OPTIONS + ("path_waves_used",)

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
    def moved(self):
        """The pose of one frame ago, and the update kinds' other triangles: every third
        triangle moved by 0.01 along all three axes (test_gpu_hit_device.py's `moved`)."""
        t = self.tris.copy()
        t[::3] += f32(0.01)
        t.setflags(write=False)
        return t

    def prev_camera(self, w, h):
        """The camera of one frame ago: this frame's, moved by a fixed small offset --
        2 % of the bounds' diagonal along (1, 0.5, 0.25)."""
        c = self.camera(w, h)
        off = f32(0.02) * f32(np.linalg.norm(np.asarray(self.bmax, f32) - np.asarray(self.bmin, f32))) * \
            np.array([1.0, 0.5, 0.25], f32)
        return dataclasses.replace(c, origin=(c.origin + off).astype(f32), lower_left=(c.lower_left + off).astype(f32))

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


@functools.lru_cache(maxsize=None)
def temporal_inputs(world_name, size):
    """The inputs of the image-to-image kinds (temporal, temporal_clip_aux, sample_plan,
    denoise_moments): two frames of a sequence per size, computed once on fresh scenes --
    data, not part of any history.  Frame 0: the pose (World.moved) and the camera
    (World.prev_camera) of one frame ago, its radiance and moments at spp and its motion
    records.  Frame 1: the world's triangles and camera at sample_base = spp -- radiance,
    moments, AOV records, the motion records back to frame 0 -- and `stat`, the mean of the
    two radiance frames (a statistics frame that is neither the current frame nor the history)."""
    wd = world(world_name)
    w, h, spp = size
    cam, pcam = wd.camera(w, h), wd.prev_camera(w, h)
    with tm.Scene(wd.moved, bounds=(wd.bmin, wd.bmax)) as sc:
        rad0, mom0 = sc.trace_moments(pcam, w, h, spp)[:2]
        mot0, _ = sc.trace_motion(pcam, pcam, w, h)
    with wd.scene() as sc:
        with options(sc, sample_base=spp):
            rad1, mom1 = sc.trace_moments(cam, w, h, spp)[:2]
            aov1, _ = sc.trace_aov(cam, w, h, spp)
        mot1, _ = sc.trace_motion(cam, pcam, w, h, prev_triangles=wd.moved)
    out = dict(rad0=rad0, mom0=mom0, mot0=mot0, rad1=rad1, mom1=mom1, aov1=aov1, mot1=mot1,
               stat=((rad0 + rad1) * f32(0.5)).astype(f32))
    for a in out.values():
        a.setflags(write=False)
    return out


GUIDED_N_MAX = 3.0  # guided_restate.synthetic_prior's n_max: tmpt_temporal's default


@functools.lru_cache(maxsize=None)
def guided_prior(world_name, size_wh):
    """The guided kind's prior: guided_restate.synthetic_prior over the frame's per-sample
    colours 4 .. 7 (the only ones it reads), each a 1-spp radiance frame at sample_base = k of
    a fresh scene -- data, computed once per size.  At the base size pin() holds it to the same
    prior over the oracle's per-sample colours."""
    wd = world(world_name)
    w, h = size_wh
    col = np.zeros((h, w, 8, 3), f32)
    with wd.scene() as sc:
        for k in range(4, 8):
            with options(sc, sample_base=k):
                col[:, :, k] = sc.trace_radiance(wd.camera(w, h), w, h, 1)[0][..., :3]
    return guided_restate.synthetic_prior(col, GUIDED_N_MAX)


def motion_expect(wd, cam, prev_cam, w, h, prev_tris):
    """temporal_restate.motion for a scene WITH the octree: the restatement's centre rays, hit
    position and projection, with the closest hit's triangle taken from the oracle's octree
    scene (visit-order ties, the root test, flat triangles: include/tmpt.h "as tmpt_scene_hit
    answers it") where that differs from the restatement's lowest-index scan -- t, u and v are
    then the restated triangle test's for that triangle.  Where no centre ray is tied (suzanne)
    this is temporal_restate.motion word for word, which test_call_kinds_pins.py asserts."""
    T = temporal_restate
    tris = np.asarray(wd.tris, f32).reshape(-1, 3, 3)
    prev = np.asarray(prev_tris, f32).reshape(-1, 3, 3)
    o, d = T.centre_rays(cam, w, h)
    d = d.reshape(-1, 3)
    ids, t, u, v = T.scan(o, d, tris)
    rays = np.concatenate([np.broadcast_to(o, d.shape), d], 1).astype(f32)
    oids, _ = wd.osc.hit_batch(rays, float(T.TMIN), float(T.TMAX))
    for k in np.unique(oids[(oids != ids) & (oids >= 0)]):
        sel = np.nonzero((oids == k) & (oids != ids))[0]
        one, t[sel], u[sel], v[sel] = T.scan(o, d[sel], tris[k:k + 1])
        assert (one == 0).all(), f"the restated triangle test rejects the oracle's triangle {k}"
    miss = oids < 0
    t[miss], u[miss], v[miss] = 0, 0, 0
    hit = ~miss
    tp = prev[np.maximum(oids, 0)]
    px, py, dp, valid = T.project(prev_cam, T.hit_pos(tp[:, 0], tp[:, 1], tp[:, 2], u, v), w, h)
    valid &= hit
    rec = np.zeros(h * w, T.MOTION_DTYPE)
    rec["px"], rec["py"], rec["depth_prev"] = (np.where(valid, a, T.ZERO) for a in (px, py, dp))
    rec["depth"], rec["u"], rec["v"], rec["tri_id"] = t, u, v, oids
    rec["flags"] = hit.astype(np.uint32) | (valid.astype(np.uint32) << 1)
    return rec.reshape(h, w)


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


# ----------------------------------------------------------------------------- the calls added since the matrix
def _moments(scene, size, call, *args, **kw):
    """trace_moments / trace_guided -> Result; the statistics are tmpt_render_adaptive's (include/tmpt.h:
    "every rule of tmpt_render_adaptive" / "the statistics are unchanged")."""
    w, h, spp = size
    rad, mom, img, cnt, rays, info = call(scene.world.camera(w, h), w, h, *args, **kw)
    stats, route, seen = _stats(scene, ADAPTIVE_STATS)
    stats.update(passes=info["passes"], samples=info["samples"], pass_pixels=tuple(info["pass_pixels"]))
    return Result({"radiance": rad, "moments": mom, "image": img, "spp_map": cnt}, rays, stats, route, seen)


def moments_uniform(scene, size):
    """trace_moments(spp_min=None) at spp: the uniform schedule, one pass."""
    return _moments(scene, size, scene.trace_moments, size[2])


def moments_adaptive(scene, size):
    """trace_moments(cap = spp + 8, 4, 4, 0.02, radius=1, band_rows=4): adaptive_nb's schedule with the moments."""
    return _moments(scene, size, scene.trace_moments, size[2] + 8, *ADAPTIVE, radius=1, band_rows=4)


GUIDED = (2, 4, 0.02)  # spp_min, spp_step, threshold; the cap is spp + 8


def guided(scene, size):
    """trace_guided(cap = spp + 8, the size's fixed prior (guided_prior), 2, 4, 0.02).  The prior
    the call was given rides in the result, for pin()."""
    prior = guided_prior(scene.world.name, tuple(size[:2]))
    res = _moments(scene, size, scene.trace_guided, size[2] + 8, prior, *GUIDED)
    res.arrays["prior"] = prior
    return res


def motion_host_prev(scene, size):
    """trace_motion with the previous camera (World.prev_camera) and the previous pose as a HOST
    array (World.moved): the form that fills Scene::motion_prev."""
    w, h, _ = size
    wd = scene.world
    rec, rays = scene.trace_motion(wd.camera(w, h), wd.prev_camera(w, h), w, h, prev_triangles=wd.moved)
    stats, _, seen = _stats(scene, MOTION_STATS, route=())
    return Result({"records": rec}, rays, stats, {}, seen)


def temporal(scene, size):
    """temporal on host arrays: frame 1 of temporal_inputs over frame 0 as the history."""
    f = temporal_inputs(scene.world.name, tuple(size))
    out, img = scene.temporal(f["rad1"], f["mot1"], f["mot0"], f["rad0"])
    return Result({"frame": out, "image": img})


CLIP = dict(gamma=0.5, radius=2)


def temporal_clip_aux(scene, size):
    """temporal_clip(gamma=0.5, radius=2, stat=, aux=, aux_history=) on host arrays: seven frames
    through Scene::clip_stage, the moments frames as the aux pair."""
    f = temporal_inputs(scene.world.name, tuple(size))
    out, img, aux = scene.temporal_clip(f["rad1"], f["mot1"], f["mot0"], f["rad0"], stat=f["stat"], aux=f["mom1"],
                                        aux_history=f["mom0"], **CLIP)
    return Result({"frame": out, "image": img, "aux": aux})


def sample_plan(scene, size):
    """sample_plan on host arrays (staged through clip_stage too): frame 0's moments as the history."""
    f = temporal_inputs(scene.world.name, tuple(size))
    return Result({"prior": scene.sample_plan(f["mot1"], f["mot0"], f["mom0"])})


def denoise_moments(scene, size):
    """denoise_moments, levels=3, over frame 1 of temporal_inputs (radiance, AOV records, moments)."""
    f = temporal_inputs(scene.world.name, tuple(size))
    with options(scene, denoise_lds=-1):
        out, img = scene.denoise_moments(f["rad1"], f["aov1"], f["mom1"], size[2], levels=DENOISE_LEVELS)
    return Result({"filtered": out, "image": img})


def _device(scene, a):
    return tm.torch.from_numpy(np.array(a)).to(f"cuda:{scene.device}")  # (a writable copy: the fixed rays are read-only)


def hit_device_closest(scene, size):
    """hit_scene_device, closest hits of the world's 256 rays as a device tensor, uv=True,
    query_sort=0 (query_top at its default)."""
    rays, (tmin, tmax), _ = scene.world.hit_rays
    with options(scene, query_sort=0):
        ids, hits, uv = (t.cpu().numpy() for t in scene.hit_scene_device(_device(scene, rays), tmin, tmax, uv=True))
        stats, route, seen = _stats(scene, HIT_STATS, route=("query_sorted",))
    return Result({"ids": ids, "hits": hits, "uv": uv}, None, stats, route, seen)


def hit_device_any_sorted(scene, size):
    """hit_scene_device, any_hit=True, a range per ray, query_sort=1: the hit bits (nothing else
    of an any-hit answer is defined across routes)."""
    _, _, r8 = scene.world.hit_rays
    with options(scene, query_sort=1):
        ids, _, _ = scene.hit_scene_device(_device(scene, r8), any_hit=True, hits=False)
        stats, route, seen = _stats(scene, HIT_STATS, route=("query_sorted",))
    return Result({"hit": (ids.cpu().numpy() >= 0).astype(np.uint8)}, None, stats, route, seen)


def sample_waves6(scene, size):
    """SEED_SAMPLE with path_waves=6 under the shadow split: the six-wave path twins.  Its own
    definition is coincident64; suzanne's flat triangles keep the fused kernel at five waves."""
    w, h, spp = size
    with options(scene, cam_pre=-1, shadow_split=1, shadow_split_pass=0, path_waves=6):
        img, rays = scene.trace_image(scene.world.camera(w, h), w, h, spp, seed_mode=tm.SEED_SAMPLE)
        stats, route, seen = _stats(scene, RENDER_STATS, route=WAVES_OPTIONS)
    return Result({"image": img}, rays, stats, route, seen)


SAMPLE_BASE = 24


def sample_based(scene, size):
    """SEED_SAMPLE with option sample_base=24: samples [24, 24 + spp) of every pixel's stream.
    The option goes back to 0 afterwards, which drops the jump tables."""
    return _image(scene, size, tm.SEED_SAMPLE, sample_base=SAMPLE_BASE)


def _octree_arrays(scene):
    o = scene.dump_octree()
    return {"octree_nodes": o["nodes"], "octree_refs": o["refs"], "octree_grid": o["grid"]}, tuple(o["info"].items())


def _update_back(scene, mode):
    wd = scene.world
    before = scene.dump_bvh()
    with options(scene, octree_build=1):  # the host recursion over coincident64 costs 0.13 s a build
        try:
            scene.update(wd.moved, mode)
        finally:
            scene.update(wd.tris, mode, bounds=(wd.bmin, wd.bmax))
    route = {"update_kind": int(scene.get_option("update_kind"))}
    dump = scene.dump_bvh()
    arrays, route["octree_info"] = _octree_arrays(scene)
    if mode == "refit":
        route["raw_nodes"] = first_difference(dump["nodes"], before["nodes"]) or "unchanged"
    arrays.update(nodes=bvh_check.canonical(dump), tris=dump["tris"])
    return Result(arrays, None, {}, route, {"info": dump["info"]})


def update_refit_back(scene, size):
    """update(World.moved, "refit"), then update(the world's triangles, "refit", bounds=), the
    octree coming back through the device build (option octree_build=device, put back: word
    for word the host build's, which octree_rebuild runs and the pin compares with): the
    result is the BVH dump and the octree dump.  The triangle records and the octree raw; the
    nodes renumbered breadth-first (bvh_check.canonical), since two builds of one scene number
    their nodes differently within a level (octree_rebuild's docstring) and the baseline's
    scene is another build -- and, raw, against the SAME scene's dump from before the two
    refits (route marker raw_nodes: "unchanged", test_gpu_scene_update.py::test_identity)."""
    return _update_back(scene, "refit")


def update_rebuild_back(scene, size):
    """The same with "rebuild": the nodes canonical, the triangle records and the octree raw."""
    return _update_back(scene, "rebuild")


def octree_device_rebuild(scene, size):
    """octree_rebuild's two builds under option octree_build=device (put back afterwards): the
    BVH dump as octree_rebuild returns it, and the octree dump raw."""
    wd = scene.world
    lo, hi = tm.octree_bounds(wd.bmin, wd.bmax)
    with options(scene, octree_build=1):
        try:
            scene.build_octree(lo + f32(0.25), hi + f32(0.25))
        finally:
            scene.build_octree(lo, hi)
    dump = scene.dump_bvh()
    arrays, oct_info = _octree_arrays(scene)
    arrays.update(nodes=bvh_check.canonical(dump), tris=dump["tris"])
    stats, _, seen = _stats(scene, ("octree_flat",), route=())
    return Result(arrays, None, stats, {"octree_info": oct_info}, seen)


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
    Kind("prepass_fallback", prepass_fallback, sample=True),
    Kind("moments_uniform", moments_uniform), Kind("moments_adaptive", moments_adaptive), Kind("guided", guided),
    Kind("motion_host_prev", motion_host_prev), Kind("temporal", temporal), Kind("temporal_clip_aux", temporal_clip_aux),
    Kind("sample_plan", sample_plan), Kind("denoise_moments", denoise_moments),
    Kind("hit_device_closest", hit_device_closest), Kind("hit_device_any_sorted", hit_device_any_sorted),
    Kind("sample_waves6", sample_waves6, world="coincident64", sample=True),
    Kind("sample_based", sample_based, sample=True),
    Kind("update_refit_back", update_refit_back), Kind("update_rebuild_back", update_rebuild_back),
    Kind("octree_device_rebuild", octree_device_rebuild))}

#: the seeding of the kinds that return a frame of tmpt_render's
IMAGE_SEED = {"row_stream": tm.SEED_ROW, "row_iter": tm.SEED_ROW, "row_mega": tm.SEED_ROW,
              "pixel_ordered": tm.SEED_PIXEL, "pixel_chains": tm.SEED_PIXEL, "pixel_wavefront": tm.SEED_PIXEL,
              "pixel_mega": tm.SEED_PIXEL, "sample_default": tm.SEED_SAMPLE, "sample_split_passes": tm.SEED_SAMPLE,
              "sample_fused_w4": tm.SEED_SAMPLE, "sample_deferred": tm.SEED_SAMPLE, "sample_soa_count": tm.SEED_SAMPLE,
              "prepass_fallback": tm.SEED_SAMPLE, "sample_waves6": tm.SEED_SAMPLE}

#: kind -> the public Scene methods and the options (include/tmpt.h "Scene options") it exercises;
#: tests/test_call_kinds_cover.py holds toymeshpathtracer_amd.Scene's public methods to it
COVERS = {
    "row_stream": (("trace_image",), ("rowspec", "rowspec_stream")),
    "row_iter": (("trace_image",), ("rowspec", "rowspec_stream")),
    "row_mega": (("trace_image",), ()),
    "pixel_ordered": (("trace_image",), ("pilot", "pixel_chains")),
    "pixel_chains": (("trace_image",), ("pilot", "pixel_chains")),
    "pixel_wavefront": (("trace_image",), ()),
    "pixel_mega": (("trace_image",), ()),
    "sample_default": (("trace_image",), ("cam_pre", "shadow_split", "shadow_split_pass", "path_waves")),
    "sample_split_passes": (("trace_image",), ("cam_pre", "shadow_split", "shadow_split_pass", "path_waves")),
    "sample_fused_w4": (("trace_image",), ("shadow_split", "cam_pre", "path_waves", "sample_block")),
    "sample_deferred": (("trace_image",), ("tie_defer", "redo_inline", "shadow_split")),
    "sample_soa_count": (("trace_image",), ()),
    "aov": (("trace_aov",), ()),
    "radiance_sample": (("trace_radiance",), ()),
    "radiance_pixel": (("trace_radiance",), ()),
    "adaptive": (("trace_adaptive",), ()),
    "adaptive_nb": (("trace_adaptive",), ()),
    "denoise": (("denoise",), ("denoise_lds",)),
    "hit_closest": (("hit_scene_batch",), ()),
    "hit_any_ranged": (("hit_scene_batch",), ()),
    "camera_rays": (("camera_rays",), ()),
    "radix_sort": (("radix_sort",), ()),
    "octree_rebuild": (("build_octree", "dump_bvh"), ()),
    "arg_errors": (("trace_image", "trace_adaptive"), ()),
    "prepass_fallback": (("trace_image",), ("cam_pre", "cam_pre_max")),
    "moments_uniform": (("trace_moments",), ()),
    "moments_adaptive": (("trace_moments",), ()),
    "guided": (("trace_guided",), ()),
    "motion_host_prev": (("trace_motion",), ()),
    "temporal": (("temporal",), ()),
    "temporal_clip_aux": (("temporal_clip",), ()),
    "sample_plan": (("sample_plan",), ()),
    "denoise_moments": (("denoise_moments",), ("denoise_lds",)),
    "hit_device_closest": (("hit_scene_device",), ("query_sort", "query_sorted")),
    "hit_device_any_sorted": (("hit_scene_device",), ("query_sort", "query_sorted")),
    "sample_waves6": (("trace_image",), ("cam_pre", "shadow_split", "shadow_split_pass", "path_waves", "path_waves_used")),
    "sample_based": (("trace_image",), ("sample_base",)),
    "update_refit_back": (("update", "dump_bvh", "dump_octree"), ("update_kind", "octree_build")),
    "update_rebuild_back": (("update", "dump_bvh", "dump_octree"), ("update_kind", "octree_build")),
    "octree_device_rebuild": (("build_octree", "dump_bvh", "dump_octree"), ("octree_build",)),
}


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
    elif name == "hit_device_closest":
        assert r["query_sorted"] == 0, r
    elif name == "hit_device_any_sorted":
        assert r["query_sorted"] == 1, r
    elif name == "sample_waves6":  # suzanne: flat triangles, no split to run at six waves (include/tmpt.h path_waves)
        want = (6, 1) if world_name == "coincident64" else (5, 0)
        assert (r["path_waves_used"], r["shadow_split_used"]) == want, r
    elif name == "update_refit_back":
        assert r["update_kind"] == 1 and r["raw_nodes"] == "unchanged", r
    elif name == "update_rebuild_back":
        assert r["update_kind"] == 2, r


def _pin_moments(res, size, want):
    """A trace_moments / trace_guided result against (spp map, radiance, rays, pass_pixels) of a
    restatement over the frame's per-sample colours `col`: every output, the moments at each
    pixel's own count."""
    n_p, rad, total, pass_pixels, col = want
    assert np.array_equal(res.arrays["spp_map"], n_p)
    render_restate.same_bits(res.arrays["radiance"][..., :3], rad, "radiance")
    assert (res.arrays["radiance"][..., 3].view(np.uint32) == f32(1).view(np.uint32)).all()
    render_restate.same_bits(res.arrays["moments"], noise_aware_restate.moments_expect(col, n_p), "moments")
    assert np.array_equal(res.arrays["image"], render_restate.pack(res.arrays["radiance"]))
    assert res.rays == total and list(res.stats["pass_pixels"]) == pass_pixels
    assert res.stats["samples"] == int(n_p.sum()) and res.stats["passes"] == len(pass_pixels)


def _pin_dumps(res, wd):
    """The BVH and octree dumps of a result against a fresh (host-built) scene's."""
    with wd.scene() as sc:
        first, oct_first = sc.dump_bvh(), sc.dump_octree()
    assert np.array_equal(res.arrays["tris"], first["tris"])
    assert np.array_equal(res.arrays["nodes"], bvh_check.canonical(first))
    for key in ("nodes", "refs", "grid"):
        d = first_difference(res.arrays["octree_" + key], oct_first[key])
        assert d is None, f"octree {key}: {d}"
    assert res.route["octree_info"] == tuple(oct_first["info"].items()) and oct_first["info"]["nodes"] > 0
    if "info" in res.seen:
        assert res.seen["info"] == first["info"], (res.seen["info"], first["info"])


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
    elif name == "moments_uniform":
        col, rays = sample_colours(wd.name, (w, h), spp + 8)
        rad, total = render_restate.radiance_sum(col, rays, spp)
        _pin_moments(res, size, (np.full((h, w), spp, np.int32), rad, total, [w * h], col))
    elif name == "moments_adaptive":
        col, rays = sample_colours(wd.name, (w, h), spp + 8)
        want = adaptive_nb_restate.adaptive_nb_expect(col, rays, *ADAPTIVE, 1, 4)
        _pin_moments(res, size, want + (col,))
        assert res.stats["passes"] >= 2 and len(np.unique(want[0])) >= 2, (res.stats["passes"], np.unique(want[0]))
    elif name == "guided":
        col, rays = sample_colours(wd.name, (w, h), spp + 8)
        prior = guided_restate.synthetic_prior(col[:, :, :8], GUIDED_N_MAX)
        render_restate.same_bits(res.arrays["prior"], prior, "the prior the call was given")
        want = guided_restate.guided_expect(col, rays, *GUIDED, prior)
        _pin_moments(res, size, want + (col,))
        assert (want[0] == GUIDED[0]).any() and (want[0] > GUIDED[0]).any(), np.unique(want[0])
    elif name == "motion_host_prev":
        want = motion_expect(wd, cam, wd.prev_camera(w, h).as_array(), w, h, wd.moved)
        got = res.arrays["records"]
        assert got.dtype == tm.MOTION_DTYPE and got.shape == want.shape
        for field in tm.MOTION_DTYPE.names:
            d = first_difference(np.ascontiguousarray(got[field]), np.ascontiguousarray(want[field]))
            assert d is None, f"motion {field}: {d}"
        assert res.rays == w * h and res.stats["extend_rays"] == w * h and res.stats["extend_launches"] == 1
        assert ((want["flags"] & 2) != 0).any()
    elif name == "temporal":
        f = temporal_inputs(wd.name, tuple(size))
        want = temporal_restate.blend(f["rad1"], f["mot1"], f["mot0"], f["rad0"])
        render_restate.same_bits(res.arrays["frame"], want, "temporal")
        assert np.array_equal(res.arrays["image"], temporal_restate.pack(want))
        assert (want[..., 3] > 1).any() and (want[..., 3] == 1).any()  # histories taken up, and restarts
    elif name == "temporal_clip_aux":
        f = temporal_inputs(wd.name, tuple(size))
        want, want_aux = temporal_clip_restate.clip(f["rad1"], f["mot1"], f["mot0"], f["rad0"], stat=f["stat"],
                                                    aux=f["mom1"], aux_hist=f["mom0"], **CLIP)
        render_restate.same_bits(res.arrays["frame"], want, "temporal_clip")
        render_restate.same_bits(res.arrays["aux"], want_aux, "temporal_clip aux")
        assert np.array_equal(res.arrays["image"], temporal_restate.pack(want))
        assert (want[..., 3] > 1).any()
    elif name == "sample_plan":
        f = temporal_inputs(wd.name, tuple(size))
        want = guided_restate.plan(f["mot1"], f["mot0"], f["mom0"])
        render_restate.same_bits(res.arrays["prior"], want, "sample_plan")
        assert (want[..., 3] > 0).any()  # not the null prior everywhere
    elif name == "denoise_moments":
        f = temporal_inputs(wd.name, tuple(size))
        want = noise_aware_restate.np_denoise_moments(f["rad1"], f["aov1"], f["mom1"], spp, levels=DENOISE_LEVELS)
        render_restate.same_bits(res.arrays["filtered"], want, "denoise_moments")
        assert np.array_equal(res.arrays["image"], pack_denoised(want))
    elif name == "hit_device_closest":
        rays, (tmin, tmax), _ = wd.hit_rays
        oids, ohits = wd.osc.hit_batch(rays, tmin, tmax)
        ids, hits, uv = res.arrays["ids"], res.arrays["hits"], res.arrays["uv"]
        assert np.array_equal(ids, oids), np.nonzero(ids != oids)[0][:8]
        render_restate.same_bits(hits[ids >= 0], ohits[ids >= 0], "hit records")
        assert not hits[ids < 0].any() and not uv[ids < 0].any()  # rows of missed rays are not written
        render_restate.same_bits(uv, mt_uv(rays, wd.tris, ids), "(u, v) against Moller-Trumbore's for the returned triangle")
        assert (ids >= 0).sum() >= 64 and (ids < 0).any()
    elif name == "hit_device_any_sorted":
        _, _, r8 = wd.hit_rays
        want = np.zeros(len(r8), np.uint8)
        for lo, hi in {(float(a), float(b)) for a, b in r8[:, 6:8]}:
            sel = np.nonzero((r8[:, 6] == f32(lo)) & (r8[:, 7] == f32(hi)))[0]
            want[sel] = wd.osc.hit_batch(r8[sel, :6], lo, hi)[0] >= 0
        assert np.array_equal(res.arrays["hit"], want), np.nonzero(res.arrays["hit"] != want)[0][:8]
        assert want.sum() >= 64 and (want == 0).any()
    elif name == "sample_based":
        col, rays = sample_colours(wd.name, (w, h), SAMPLE_BASE + spp)
        rad, total = render_restate.radiance_sum(col[:, :, SAMPLE_BASE:], rays[:, :, SAMPLE_BASE:])
        assert res.rays == total, (res.rays, total)
        d = first_difference(res.arrays["image"], render_restate.pack(rad))
        assert d is None, f"samples [{SAMPLE_BASE}, {SAMPLE_BASE + spp}): {d}"
        assert not np.array_equal(res.arrays["image"], oracle_frame(wd.name, tuple(size), tm.SEED_SAMPLE)[0])
    elif name in ("update_refit_back", "update_rebuild_back"):
        _pin_dumps(res, wd)
    elif name == "octree_device_rebuild":
        _pin_dumps(res, wd)
        assert res.stats["octree_flat"] == int((res.arrays["tris"][:-1, 9] & 1).sum())
    else:
        raise AssertionError(f"no pin for {name}")
