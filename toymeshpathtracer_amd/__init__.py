"""toymeshpathtracer_amd -- MI355X-native (gfx950) hot path of pr0g/ToyMeshPathTracer.

Python face of ``libtmpt.so`` (C ABI: ``include/tmpt.h``), mirroring the
reference's host interface for the path (``/root/reference/source``):

==========================  ==============================================
reference                   here
==========================  ==============================================
``LoadScene`` main.cpp:122  :func:`load_scene`
``Camera`` maths.cpp:40     :class:`Camera` (+ :meth:`Camera.for_scene`, main.cpp:295-307)
``Scene`` scene.h:17        :class:`Scene` (LBVH on the GPU)
``BuildOctree`` scene.h:26  :meth:`Scene.build_octree` (+ :func:`octree_bounds`, main.cpp:312)
``Scene::HitScene`` :36     :meth:`Scene.hit_scene` / :meth:`Scene.hit_scene_batch`
``TraceImageBody`` :180     :meth:`Scene.trace_image` (parallel_for, main.cpp:329)
(none: guide buffers)       :meth:`Scene.trace_aov` (:data:`AOV_DTYPE` records: normal, depth, direct
                            light, triangle id, coverage of a sample-seeded frame's camera rays)
(none: float frame)         :meth:`Scene.trace_radiance` (the render's linear radiance beside its bytes)
(none: denoiser)            :meth:`Scene.denoise` (edge-avoiding a-trous filter guided by the AOV records)
(none: adaptive sampling)   :meth:`Scene.trace_adaptive` (per-pixel sample counts by a variance test)
(none: noise-aware filter)  :meth:`Scene.trace_moments` (the frame with each pixel's luminance moments) and
                            :meth:`Scene.denoise_moments` (the filter steered by them: wavelet shrinkage)
(none: device queries)      :meth:`Scene.hit_scene_device` (``HitScene`` over a torch tensor of rays on the scene's
                            device: ids, hit records and (u, v) as tensors, no host round trip)
(none: scene update)        :meth:`Scene.update` (new triangles in place: a device BVH refit, or a rebuild)
(none: temporal)            :meth:`Scene.trace_motion` (:data:`MOTION_DTYPE` records: where each pixel's surface
                            was one frame ago) and :meth:`Scene.temporal` (the reprojected, accumulated history);
                            render option ``sample_base`` gives every frame its own samples
``stbi_write_png`` :342     :func:`write_png`
==========================  ==============================================

The compute path is the HIP library only: if ``libtmpt.so`` is missing this
module raises on import -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

__all__ = [
    "Camera", "Scene", "Hit", "RenderStats", "load_scene", "write_png", "device_count",
    "SEED_ROW", "SEED_PIXEL", "SEED_SAMPLE", "ENGINE_WAVEFRONT", "ENGINE_MEGAKERNEL", "ENGINE_PERSISTENT", "lib_path", "TmptError",
    "tile_rows", "tile_row_to_y", "render_multi", "octree_bounds", "octree_digest", "octree_flags", "octree_arrays",
    "AOV_DTYPE", "MOTION_DTYPE", "query_keys", "query_plan",
]

SEED_ROW, SEED_PIXEL, SEED_SAMPLE = 0, 1, 2
ENGINE_WAVEFRONT, ENGINE_MEGAKERNEL, ENGINE_PERSISTENT = 0, 1, 2
UPDATE_REFIT, UPDATE_REBUILD = 0, 1
FLAG_OUT_DEVICE, FLAG_COUNT_VISITS, FLAG_WAIT_STREAM, FLAG_REQUIRE_RCCL = 1, 2, 4, 8

#: tmpt_aov_pixel (include/tmpt.h), one record of :meth:`Scene.trace_aov`, 32 bytes
AOV_DTYPE = np.dtype([("normal", np.float32, (3,)), ("depth", np.float32), ("direct", np.float32),
                      ("tri_id", np.int32), ("hits", np.uint32), ("lit", np.uint32)])
#: tmpt_motion_pixel (include/tmpt.h), one record of :meth:`Scene.trace_motion`, 32 bytes
MOTION_DTYPE = np.dtype([("px", np.float32), ("py", np.float32), ("depth", np.float32), ("depth_prev", np.float32),
                         ("u", np.float32), ("v", np.float32), ("tri_id", np.int32), ("flags", np.uint32)])

_HERE = os.path.dirname(os.path.abspath(__file__))
# TMPT_LIB_PATH: another in-tree build of the library (compiler-flag A/B in tools/)
lib_path = os.environ.get("TMPT_LIB_PATH") or os.path.join(_HERE, "_lib", "libtmpt.so")


class TmptError(RuntimeError):
    pass


if not os.path.exists(lib_path):
    raise ImportError(
        f"libtmpt.so not built ({lib_path}); run `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C toymeshpathtracer_amd/csrc`. There is no CPU fallback.")

# One HIP runtime per process: torch wheels bundle their own libamdhip64 /
# libhsa-runtime64 (same sonames as /opt/rocm's).  Importing torch first makes
# libtmpt bind to the runtime torch already loaded, so torch CUDA tensors,
# torch.distributed (RCCL) and our kernels share one device context.  Without
# torch, the system ROCm runtime is used.
# (TMPT_NO_TORCH=1: not even that -- the host sanitizer runs, tools/san_check.sh)
try:  # pragma: no cover - depends on the environment
    if os.environ.get("TMPT_NO_TORCH") == "1":
        raise ImportError("TMPT_NO_TORCH")
    import torch  # noqa: F401
except Exception:  # torch is optional for the C ABI itself
    torch = None

_lib = ctypes.CDLL(lib_path)

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)


class _Camera(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("lower_left", ctypes.c_float * 3),
                ("horizontal", ctypes.c_float * 3), ("vertical", ctypes.c_float * 3),
                ("u", ctypes.c_float * 3), ("v", ctypes.c_float * 3), ("w", ctypes.c_float * 3),
                ("lens_radius", ctypes.c_float)]


class _Desc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("seed_mode", ctypes.c_int32), ("band_rows", ctypes.c_int32),
                ("shard", ctypes.c_int32), ("num_shards", ctypes.c_int32),
                ("engine", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("spp_begin", ctypes.c_int32), ("spp_count", ctypes.c_int32),
                ("reserved0", ctypes.c_int32), ("wait_stream", ctypes.c_uint64),
                ("reserved", ctypes.c_int32 * 2)]


class _DenoiseDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("levels", ctypes.c_int32), ("normal_exp", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("sigma_depth", ctypes.c_float), ("sigma_direct", ctypes.c_float),
                ("wait_stream", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 4)]


class _TemporalDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("n_max", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("reserved0", ctypes.c_int32),
                ("wait_stream", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 4)]


class _TemporalClipDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("n_max", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("gamma", ctypes.c_float),
                ("radius", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("wait_stream", ctypes.c_uint64),
                ("reserved", ctypes.c_int32 * 4)]


class _HitDesc(ctypes.Structure):  # tmpt_hit_desc, 56 bytes
    _fields_ = [("n", ctypes.c_int64), ("ranged", ctypes.c_int32), ("any_hit", ctypes.c_int32),
                ("tmin", ctypes.c_float), ("tmax", ctypes.c_float), ("flags", ctypes.c_int32),
                ("reserved0", ctypes.c_int32), ("wait_stream", ctypes.c_uint64), ("reserved", ctypes.c_int32 * 4)]


class _AdaptiveDesc(ctypes.Structure):
    _fields_ = [("spp_min", ctypes.c_int32), ("spp_step", ctypes.c_int32), ("threshold", ctypes.c_float),
                ("radius", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


class _AdaptiveInfo(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("samples", ctypes.c_uint64),
                ("pass_pixels", ctypes.c_int64 * 64)]


class _Stats(ctypes.Structure):
    _fields_ = [("render_ms", ctypes.c_double), ("extend_ms", ctypes.c_double),
                ("shadow_ms", ctypes.c_double), ("extend_rays", ctypes.c_uint64),
                ("shadow_rays", ctypes.c_uint64), ("extend_launches", ctypes.c_int64),
                ("shadow_launches", ctypes.c_int64), ("iterations", ctypes.c_int64),
                ("node_visits", ctypes.c_uint64), ("tri_tests", ctypes.c_uint64),
                ("shadow_node_visits", ctypes.c_uint64), ("shadow_tri_tests", ctypes.c_uint64),
                ("build_ms", ctypes.c_double), ("bvh_nodes", ctypes.c_int32),
                ("bvh_depth", ctypes.c_int32), ("n_tris", ctypes.c_int32),
                ("device", ctypes.c_int32), ("bvh4_nodes", ctypes.c_int32),
                ("bvh4_depth", ctypes.c_int32), ("leaf_max", ctypes.c_int32),
                ("builder_iters", ctypes.c_int32), ("octree_nodes", ctypes.c_int32),
                ("octree_leaves", ctypes.c_int32), ("octree_refs", ctypes.c_int64),
                ("octree_build_ms", ctypes.c_double), ("tie_queries", ctypes.c_uint64),
                ("root_misses", ctypes.c_uint64), ("row_engine", ctypes.c_int32),
                ("stream_fallbacks", ctypes.c_int32), ("octree_depth", ctypes.c_int32),
                ("tie_rule", ctypes.c_int32), ("chain_pixels", ctypes.c_int64),
                ("redo_samples", ctypes.c_int64), ("redo_late", ctypes.c_int64),
                ("crack_queries", ctypes.c_uint64), ("octree_flat", ctypes.c_int32),
                ("redo_launches", ctypes.c_int32), ("redo_ms", ctypes.c_double),
                ("redo_rays", ctypes.c_uint64), ("tie_path", ctypes.c_int32), ("reserved_stats", ctypes.c_int32)]


def _sig(name, res, args):
    fn = getattr(_lib, name)
    fn.restype = res
    fn.argtypes = args
    return fn


_load_obj = _sig("tmpt_load_obj", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_f32p), _i32p, _f32p, _f32p])
_free = _sig("tmpt_free", None, [ctypes.c_void_p])
_cam_init = _sig("tmpt_camera_init", ctypes.c_int, [ctypes.POINTER(_Camera), _f32p, _f32p, _f32p,
                                                     ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                                     ctypes.c_float])
_cam_scene = _sig("tmpt_camera_for_scene", ctypes.c_int, [ctypes.POINTER(_Camera), _f32p, _f32p,
                                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int32])
_dev_count = _sig("tmpt_device_count", ctypes.c_int, [])
_scene_create = _sig("tmpt_scene_create", ctypes.c_int, [_f32p, ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.POINTER(ctypes.c_void_p)])
_scene_create_ex = _sig("tmpt_scene_create_ex", ctypes.c_int, [_f32p, ctypes.c_int32, ctypes.c_int32,
                                                               ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)])
_set_option = _sig("tmpt_scene_set_option", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double])
_get_option = _sig("tmpt_scene_get_option", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p,
                                                           ctypes.POINTER(ctypes.c_double)])
_scene_destroy = _sig("tmpt_scene_destroy", ctypes.c_int, [ctypes.c_void_p])
_scene_hit = _sig("tmpt_scene_hit", ctypes.c_int, [ctypes.c_void_p, _f32p, ctypes.c_int64,
                                                   ctypes.c_float, ctypes.c_float, ctypes.c_int32,
                                                   _f32p, _i32p])
_scene_hit_ranged = _sig("tmpt_scene_hit_ranged", ctypes.c_int, [ctypes.c_void_p, _f32p, ctypes.c_int64,
                                                                 ctypes.c_int32, _f32p, _i32p])
_render = _sig("tmpt_render", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera),
                                             ctypes.POINTER(_Desc), ctypes.c_void_p, _u64p])
_render_aov = _sig("tmpt_render_aov", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera),
                                                     ctypes.POINTER(_Desc), ctypes.c_void_p, _u64p])
_render_radiance = _sig("tmpt_render_radiance", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera),
                                                               ctypes.POINTER(_Desc), ctypes.c_void_p,
                                                               ctypes.c_void_p, _u64p])
_denoise = _sig("tmpt_denoise", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_DenoiseDesc), ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_build_octree = _sig("tmpt_scene_build_octree", ctypes.c_int, [ctypes.c_void_p, _f32p, _f32p])


def _scene_update(handle, tris, n, mode):
    # bound on first use, as tmpt_scene_dump_bvh is: a library from before the entry point still loads
    fn = _sig("tmpt_scene_update", ctypes.c_int, [ctypes.c_void_p, _f32p, ctypes.c_int32, ctypes.c_int32])
    return fn(handle, tris, n, mode)


_octree_bounds = _sig("tmpt_octree_bounds", ctypes.c_int, [_f32p, _f32p, _f32p])
_octree_digest = _sig("tmpt_octree_digest", ctypes.c_int, [_f32p, ctypes.c_int32, _f32p, _f32p, _u64p])
_octree_flags = _sig("tmpt_octree_flags", ctypes.c_int, [_f32p, ctypes.c_int32, _f32p, _f32p, _f32p, _f32p, _i32p,
                                                         ctypes.c_int64, ctypes.c_void_p, _f32p])
_render_multi = _sig("tmpt_render_multi", ctypes.c_int,
                     [_f32p, ctypes.c_int32, _f32p, ctypes.POINTER(_Camera), ctypes.POINTER(_Desc),
                      ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_void_p, _u64p,
                      ctypes.POINTER(ctypes.c_double)])
_tile_rows = _sig("tmpt_tile_rows", ctypes.c_int32, [ctypes.POINTER(_Desc)])
_tile_row_to_y = _sig("tmpt_tile_row_to_y", ctypes.c_int32, [ctypes.POINTER(_Desc), ctypes.c_int32])
_stats = _sig("tmpt_get_stats", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Stats)])
_write_png = _sig("tmpt_write_png", ctypes.c_int, [ctypes.c_char_p, _u8p, ctypes.c_int32, ctypes.c_int32])
_last_error = _sig("tmpt_last_error", ctypes.c_char_p, [])
_abi = _sig("tmpt_abi_version", ctypes.c_int, [])
_unit_sincos = _sig("tmpt_unit_sincos", ctypes.c_int, [ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32,
                                                       ctypes.c_void_p])
#: every symbol include/tmpt.h declares (checked by tests/test_abi.py)
EXPORTS = ("tmpt_load_obj", "tmpt_free", "tmpt_camera_init", "tmpt_camera_for_scene",
           "tmpt_device_count", "tmpt_scene_create", "tmpt_scene_create_ex", "tmpt_scene_set_option",
           "tmpt_scene_get_option", "tmpt_scene_destroy", "tmpt_scene_hit", "tmpt_scene_hit_ranged",
           "tmpt_render", "tmpt_render_multi", "tmpt_tile_rows", "tmpt_tile_row_to_y", "tmpt_get_stats",
           "tmpt_write_png", "tmpt_last_error", "tmpt_abi_version", "tmpt_unit_sincos",
           "tmpt_scene_build_octree", "tmpt_octree_bounds", "tmpt_octree_digest",
           "tmpt_octree_flags", "tmpt_render_aov", "tmpt_render_radiance", "tmpt_denoise", "tmpt_fastdiv",
           "tmpt_scene_dump_bvh", "tmpt_radix_sort", "tmpt_camera_rays", "tmpt_render_adaptive",
           "tmpt_scene_update", "tmpt_render_motion", "tmpt_temporal", "tmpt_render_moments",
           "tmpt_denoise_moments", "tmpt_temporal_clip", "tmpt_scene_dump_octree", "tmpt_octree_arrays",
           "tmpt_sample_plan", "tmpt_render_guided", "tmpt_scene_hit_device", "tmpt_query_keys", "tmpt_query_plan")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise TmptError(f"{what} failed ({rc}): {_last_error().decode(errors='replace')}")


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_f32p)


def unit_sincos(key0: int, n: int, device: int = 0) -> np.ndarray:
    """RandomUnitVector's (cos a, sin a) for RNG keys [key0, key0 + n) (maths.cpp:33-36),
    n x 2 float32: computed on `device`, or by the host restatement when device < 0."""
    out = np.empty((n, 2), dtype=np.float32)
    _check(_unit_sincos(device, key0, n, out.ctypes.data), "tmpt_unit_sincos")
    return out


def fastdiv(divisor: int, x: np.ndarray):
    """x // divisor by the path kernel's multiply-shift divider (tmpt_internal.h
    FastDiv; dividends below 2^31), evaluated on the host: (quotients, (mul, shift))."""
    # bound on first use: an earlier build of the library (TMPT_LIB_PATH, the A/B tools) has no such symbol
    fn = _sig("tmpt_fastdiv", ctypes.c_int, [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p])
    x = np.ascontiguousarray(x, dtype=np.uint32)
    out = np.empty_like(x)
    ms = np.zeros(2, dtype=np.uint32)
    _check(fn(divisor, x.ctypes.data, x.size, out.ctypes.data, ms.ctypes.data), "tmpt_fastdiv")
    return out, (int(ms[0]), int(ms[1]))


def query_keys(rays, box) -> np.ndarray:
    """The sort key of option ``query_sort`` (tmpt_query_keys, host only; include/tmpt.h
    states it) for rays float32 [n, 6] or [n, 8] and box = the six floats {min.xyz,
    max.xyz} of the BVH's root box: uint32 [n], 24 bits each, 0xFFFFFF for a ray with a
    NaN in its origin or direction."""
    fn = _sig("tmpt_query_keys", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_void_p])
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim != 2 or rays.shape[1] not in (6, 8):
        raise ValueError("query_keys: rays [n, 6] or [n, 8]")
    box = np.ascontiguousarray(box, np.float32).reshape(-1)
    if box.size != 6:
        raise ValueError("query_keys: box = {min.xyz, max.xyz}")
    keys = np.zeros(rays.shape[0], np.uint32)
    _check(fn(rays.ctypes.data, rays.shape[0], rays.shape[1], box.ctypes.data, keys.ctypes.data), "query_keys")
    return keys


def query_plan(n: int, sorted: bool, chunk: int = 1 << 22, grid_cap: int = 0, resident: int = 1024) -> dict:
    """The sizes of one :meth:`Scene.hit_scene_device` call (tmpt_query_plan, host only)."""
    fn = _sig("tmpt_query_plan", ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_void_p])
    out = np.zeros(6, np.int64)
    _check(fn(n, int(sorted), chunk, grid_cap, resident, out.ctypes.data), "query_plan")
    return dict(zip(("chunks", "chunk_n", "last_n", "grid", "ovf_bytes", "sort_bytes"), (int(v) for v in out)))


def device_count() -> int:
    return int(_dev_count())


def abi_version() -> int:
    return int(_abi())


# ----------------------------------------------------------------------------- scene ingest
def load_scene(path: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """LoadScene (main.cpp:122-170): returns (tris[n,3,3] float32 incl. the 2
    floor triangles, bounds_min[3], bounds_max[3]) -- bounds of the OBJ only."""
    p = _f32p()
    n = ctypes.c_int32()
    bmin = np.zeros(3, np.float32)
    bmax = np.zeros(3, np.float32)
    _check(_load_obj(path.encode(), ctypes.byref(p), ctypes.byref(n), _fp(bmin), _fp(bmax)),
           f"load_scene({path!r})")
    try:
        tris = np.ctypeslib.as_array(p, shape=(n.value * 9,)).copy().reshape(n.value, 3, 3)
    finally:
        _free(p)
    return tris, bmin, bmax


def octree_bounds(bmin, bmax) -> Tuple[np.ndarray, np.ndarray]:
    """The root box main.cpp:312 gives BuildOctree for a scene whose OBJ bounds
    are (bmin, bmax): bmin - extra, bmax + extra, extra = 0.7 x the size
    (main.cpp:296-297), in float32."""
    lo, hi = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
    box = np.zeros(6, np.float32)
    _check(_octree_bounds(_fp(lo), _fp(hi), _fp(box)), "octree_bounds")
    return box[:3].copy(), box[3:].copy()


def octree_digest(tris: np.ndarray, box_min, box_max) -> dict:
    """The octree Scene.build_octree(box_min, box_max) builds, summarised on
    the host (no GPU): nodes, leaves, triangle references, depth and an FNV-1a
    digest of its preorder walk -- the check hook tests compare with the oracle."""
    t = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    lo, hi = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    out = (ctypes.c_uint64 * 5)()
    _check(_octree_digest(_fp(t), t.shape[0], _fp(lo), _fp(hi), out), "octree_digest")
    return dict(zip(("nodes", "leaves", "refs", "depth", "digest"), (int(v) for v in out)))


_OCT_INFO = ("nodes", "leaves", "refs", "depth", "flat")


def _octree_result(nodes, refs, info, grid) -> dict:
    return {"nodes": nodes, "refs": refs, "info": dict(zip(_OCT_INFO, (int(v) for v in info))), "grid": grid}


def octree_arrays(tris: np.ndarray, box_min, box_max, method: int = 0) -> dict:
    """The octree Scene.build_octree(box_min, box_max) builds, as arrays, on the
    host (tmpt_octree_arrays, no GPU): ``nodes`` uint32[n, 8] in preorder (box
    min, skip link, box max, leaf-list offset or -1), ``refs`` int32 (per leaf
    its count, then its triangle ids), ``info`` (nodes, leaves, refs, depth,
    flat) and ``grid``, the 16 floats of the crack grid.  ``method=0``: the
    recursion of the host build; ``method=1``: the passes of the device build
    (option octree_build=device) run as host loops.  Both give the same words."""
    # bound on first use: an earlier build of the library (TMPT_LIB_PATH, the A/B tools) has no such symbol
    fn = _sig("tmpt_octree_arrays", ctypes.c_int, [_f32p, ctypes.c_int32, _f32p, _f32p, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p])
    t = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    lo, hi = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    info = np.zeros(5, np.int64)
    grid = np.zeros(16, np.float32)
    _check(fn(_fp(t), t.shape[0], _fp(lo), _fp(hi), method, None, 0, None, 0, info.ctypes.data, grid.ctypes.data),
           "octree_arrays")
    nodes = np.zeros((int(info[0]), 8), np.uint32)
    refs = np.zeros(int(info[2]), np.int32)
    _check(fn(_fp(t), t.shape[0], _fp(lo), _fp(hi), method, nodes.ctypes.data, nodes.size, refs.ctypes.data,
              refs.size, info.ctypes.data, grid.ctypes.data), "octree_arrays")
    return _octree_result(nodes, refs, info, grid)


def octree_flags(tris: np.ndarray, box_min, box_max, rays, t, ids):
    """Which answered queries the octree re-answers besides ties (host, no GPU):
    per ray 1 = the hit triangle lies flat on an octree plane, 2 = the hit may
    lie in a crack (the device's test), 0 = the BVH's answer stands; and the
    crack grid {r0, 1/cell, cell, band, reach}."""
    tr = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    lo, hi = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    r = np.ascontiguousarray(np.asarray(rays, np.float32)[:, :6])
    tt = np.ascontiguousarray(np.asarray(t, np.float32))
    ii = np.ascontiguousarray(np.asarray(ids, np.int32))
    out = np.zeros(r.shape[0], np.uint8)
    grid = np.zeros(13, np.float32)
    _check(_octree_flags(_fp(tr), tr.shape[0], _fp(lo), _fp(hi), _fp(r), _fp(tt), ii.ctypes.data_as(_i32p),
                         r.shape[0], out.ctypes.data, _fp(grid)), "octree_flags")
    return out, grid


# ----------------------------------------------------------------------------- camera
@dataclass
class Camera:
    """Camera of maths.h:83-112 (fields as computed by Camera::Camera)."""
    origin: np.ndarray
    lower_left: np.ndarray
    horizontal: np.ndarray
    vertical: np.ndarray
    u: np.ndarray
    v: np.ndarray
    w: np.ndarray
    lens_radius: float

    @staticmethod
    def _from_c(c: _Camera) -> "Camera":
        a = lambda f: np.array(list(f), np.float32)
        return Camera(a(c.origin), a(c.lower_left), a(c.horizontal), a(c.vertical), a(c.u),
                      a(c.v), a(c.w), float(c.lens_radius))

    def _to_c(self) -> _Camera:
        c = _Camera()
        for name in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w"):
            getattr(c, name)[:] = [float(x) for x in np.asarray(getattr(self, name), np.float32)]
        c.lens_radius = self.lens_radius
        return c

    @staticmethod
    def create(look_from, look_at, vup, vfov: float, aspect: float, aperture: float,
               focus_dist: float) -> "Camera":
        """Camera::Camera (maths.cpp:40-59)."""
        c = _Camera()
        lf, la, up = (np.asarray(x, np.float32) for x in (look_from, look_at, vup))
        _check(_cam_init(ctypes.byref(c), _fp(lf), _fp(la), _fp(up), vfov, aspect, aperture,
                         focus_dist), "Camera")
        return Camera._from_c(c)

    @staticmethod
    def for_scene(bmin, bmax, width: int, height: int, is_sponza: bool = False) -> "Camera":
        """Camera placement of main.cpp:295-307."""
        c = _Camera()
        lo, hi = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
        _check(_cam_scene(ctypes.byref(c), _fp(lo), _fp(hi), width, height, int(is_sponza)),
               "Camera.for_scene")
        return Camera._from_c(c)

    def as_array(self) -> np.ndarray:
        return np.concatenate([self.origin, self.lower_left, self.horizontal, self.vertical,
                               self.u, self.v, self.w, [self.lens_radius]]).astype(np.float32)


# ----------------------------------------------------------------------------- scene
@dataclass
class Hit:
    """Hit of maths.h:46-51."""
    pos: np.ndarray
    normal: np.ndarray
    t: float


@dataclass
class RenderStats:
    render_ms: float
    extend_ms: float
    shadow_ms: float
    extend_rays: int
    shadow_rays: int
    extend_launches: int
    shadow_launches: int
    iterations: int
    node_visits: int
    tri_tests: int
    shadow_node_visits: int
    shadow_tri_tests: int
    build_ms: float
    bvh_nodes: int
    bvh_depth: int
    n_tris: int
    device: int
    bvh4_nodes: int
    bvh4_depth: int
    leaf_max: int
    builder_iters: int
    octree_nodes: int
    octree_leaves: int
    octree_refs: int
    octree_build_ms: float
    tie_queries: int
    root_misses: int
    row_engine: int
    stream_fallbacks: int
    octree_depth: int
    tie_rule: int
    chain_pixels: int
    redo_samples: int
    redo_late: int
    crack_queries: int
    octree_flat: int
    redo_launches: int
    redo_ms: float
    redo_rays: int
    tie_path: int


def _desc(width, height, spp, seed_mode, band_rows=0, shard=0, num_shards=1,
          engine=ENGINE_PERSISTENT, flags=0, spp_begin=0, spp_count=0, wait_stream=None) -> _Desc:
    d = _Desc()
    d.width, d.height, d.spp, d.seed_mode = width, height, spp, seed_mode
    d.band_rows, d.shard, d.num_shards = band_rows, shard, num_shards
    d.engine, d.flags = engine, flags
    d.spp_begin, d.spp_count = spp_begin, spp_count
    if wait_stream is not None:
        d.flags |= FLAG_WAIT_STREAM
        d.wait_stream = int(wait_stream)
    return d


def _current_stream(device: int):
    """hipStream_t of torch's current stream on `device` (0 = its null stream),
    or None when torch has not initialised its GPU context (a caller whose
    device buffer does not come from torch has no torch work to wait for, and
    asking would initialise torch's context)."""
    if torch is None or not torch.cuda.is_initialized():
        return None
    return int(torch.cuda.current_stream(device).cuda_stream)


def _wait_stream(device: int, wait_stream):
    """A method's ``wait_stream`` as a hipStream_t or None: "current" is torch's current stream."""
    return _current_stream(device) if isinstance(wait_stream, str) else wait_stream


def _tile_desc(device, out, wait_stream, width, height, spp, seed_mode, band_rows, shard, num_shards,
               engine=ENGINE_PERSISTENT, flags=0, spp_begin=0, spp_count=0) -> _Desc:
    """The descriptor of one shard's render; with ``out`` (device pointers) the
    device form, ordered after ``wait_stream``."""
    if out is None:
        return _desc(width, height, spp, seed_mode, band_rows, shard, num_shards, engine, flags, spp_begin, spp_count)
    return _desc(width, height, spp, seed_mode, band_rows, shard, num_shards, engine, flags | FLAG_OUT_DEVICE, spp_begin,
                 spp_count, _wait_stream(device, wait_stream))


def _device_form(d, device: int, wait_stream) -> None:
    """A whole-frame descriptor's flags for device pointers, ordered after ``wait_stream``."""
    d.flags = FLAG_OUT_DEVICE
    ws = _wait_stream(device, wait_stream)
    if ws is not None:
        d.flags |= FLAG_WAIT_STREAM
        d.wait_stream = int(ws)


def _dptr(p):
    """A device pointer (an int, or None) as a C argument."""
    return None if p is None else ctypes.c_void_p(int(p))


def _hptr(a):
    """A numpy array (or None) as a C argument."""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _out_frame(what: str, out, h: int, w: int, tail: str = "") -> np.ndarray:
    """The float32 frame [h, w, 4] a whole-frame method writes: ``out``, checked, or a new one."""
    res = np.zeros((h, w, 4), np.float32) if out is None else out
    if not (isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == (h, w, 4)
            and res.flags.c_contiguous):
        raise ValueError(f"{what}: out must be a contiguous float32 array [h, w, 4]{tail}")
    return res


def _frames(what: str, frames, width, height, out, msg: str):
    """The input frames of a whole-frame method, (value, dtype) each, the radiance
    first.  Device pointers (ints) pass, ``width`` and ``height`` giving the size;
    arrays are made contiguous and must be [h, w, 4] (float32) or [h, w] (records)
    of one frame.  Returns (device form?, h, w, frames)."""
    if isinstance(frames[0][0], int):
        if width is None or height is None or out is None:
            raise ValueError(f"{what}: device pointers need width, height and out")
        return True, int(height), int(width), [f for f, _ in frames]
    arrays = [np.ascontiguousarray(f, t) for f, t in frames]
    h, w = arrays[0].shape[:2]
    if any(a.shape != ((h, w, 4) if a.dtype == np.float32 else (h, w)) for a in arrays):
        raise ValueError(f"{what}: {msg} of one whole frame")
    return False, h, w, arrays


def _filter_call(what: str, call, d, device: int, dev: bool, frames, out, wait_stream):
    """``call(d, *inputs, float out, rgba8 out)`` of denoise, denoise_moments and
    temporal, whose float output may be their radiance: returns (float32[h, w, 4],
    rgba8[h, w, 4]), or (None, None) in the device form."""
    if dev:
        _device_form(d, device, wait_stream)
        f32, u8 = out
        _check(call(ctypes.byref(d), *[ctypes.c_void_p(int(p)) for p in frames], _dptr(f32), _dptr(u8)), what)
        return None, None
    res = _out_frame(what, out, d.height, d.width, " (it may be radiance itself)")
    img = np.zeros((d.height, d.width, 4), np.uint8)
    _check(call(ctypes.byref(d), *[_hptr(a) for a in frames], _hptr(res), _hptr(img)), what)
    return res, img


def _adaptive_desc(spp_min, spp_step, threshold, radius):
    ad = _AdaptiveDesc()
    ad.spp_min, ad.spp_step, ad.threshold, ad.radius = spp_min, spp_step, threshold, radius
    return ctypes.byref(ad)


#: per output of the adaptive family, in ABI order: a pixel's shape and type
_TILES = {"f32": ((4,), np.float32), "u8": ((4,), np.uint8), "i32": ((), np.int32)}


def _adaptive_call(what: str, fn, head, kinds, d, out):
    """The tail trace_adaptive, trace_moments and trace_guided share: ``head`` the
    arguments before the outputs, ``kinds`` the outputs' :data:`_TILES`, ``out``
    their device pointers or None (then arrays are made).  Returns (*arrays or
    Nones, rays, info)."""
    rays, inf = ctypes.c_uint64(), _AdaptiveInfo()
    if out is not None:
        arrays, ptrs = [None] * len(kinds), [_dptr(p) for p in out]
    else:
        rows = int(_tile_rows(ctypes.byref(d)))
        arrays = [np.zeros((rows, d.width) + _TILES[k][0], _TILES[k][1]) for k in kinds]
        ptrs = [_hptr(a) for a in arrays]
    _check(fn(*head, *ptrs[:len(kinds)], ctypes.byref(inf), ctypes.byref(rays)), what)
    info = {"passes": int(inf.passes), "samples": int(inf.samples),
            "pass_pixels": [int(v) for v in inf.pass_pixels[:inf.passes]]}
    return (*arrays, int(rays.value), info)


def tile_rows(width, height, band_rows=0, shard=0, num_shards=1) -> int:
    return int(_tile_rows(ctypes.byref(_desc(width, height, 1, 0, band_rows, shard, num_shards))))


def tile_row_to_y(width, height, band_rows, shard, num_shards) -> np.ndarray:
    d = _desc(width, height, 1, 0, band_rows, shard, num_shards)
    n = int(_tile_rows(ctypes.byref(d)))
    return np.array([_tile_row_to_y(ctypes.byref(d), r) for r in range(n)], np.int64)


def _options_text(options) -> Optional[bytes]:
    if options is None:
        return None
    if isinstance(options, str):
        return options.encode()
    return ",".join(f"{k}={v}" for k, v in dict(options).items()).encode()


class Scene:
    """Scene (scene.h:17-43): triangles copied to the GPU, BVH built there.

    ``options``: build and render options (include/tmpt.h "Scene options"),
    a dict or "key=value,..." string, e.g. ``{"builder": "lbvh", "leaf_max": 4}``;
    render options can also be changed later with :meth:`set_option`.
    ``bounds``: the OBJ bounds (bmin, bmax) :func:`load_scene` returns; given,
    the reference's octree is built over them as main.cpp:312 does
    (:meth:`build_octree`), so tied closest hits get the reference's answer."""

    def __init__(self, triangles: np.ndarray, device: int = 0, options=None, bounds=None):
        tris = np.ascontiguousarray(np.asarray(triangles, np.float32).reshape(-1, 9))
        self._h = ctypes.c_void_p()
        self.n = tris.shape[0]
        self.device = device
        _check(_scene_create_ex(_fp(tris), self.n, device, _options_text(options), ctypes.byref(self._h)),
               "Scene")
        if bounds is not None:
            self.build_octree(*octree_bounds(*bounds))

    def build_octree(self, box_min, box_max) -> None:
        """Scene::BuildOctree(min, max) (scene.cpp:75-83): the reference's octree
        over the scene, kept on the device to answer closest hits tied on t in
        its visit order and to apply its root box test (include/tmpt.h)."""
        lo, hi = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
        _check(_build_octree(self._h, _fp(lo), _fp(hi)), "build_octree")

    def update(self, triangles: np.ndarray, mode: str = "refit", bounds=None) -> None:
        """New triangles for this scene (tmpt_scene_update, include/tmpt.h).

        ``mode="refit"``: the same number of triangles, triangle i in the slot
        triangle i had; the tree keeps its shape and every record, box and
        plane is made again on the device.  ``mode="rebuild"``: any number of
        triangles, the full build with the scene's build options; a failed
        rebuild raises and leaves the scene as it was.  Both drop the octree:
        ``bounds=(bmin, bmax)`` builds it again over the new bounds, as the
        constructor does.  ``get_option("bvh_cost")`` tells how far a refitted
        tree has degraded, ``get_option("update_ms")`` what the update took."""
        modes = {"refit": UPDATE_REFIT, "rebuild": UPDATE_REBUILD, UPDATE_REFIT: UPDATE_REFIT,
                 UPDATE_REBUILD: UPDATE_REBUILD}
        if mode not in modes:
            raise ValueError(f"Scene.update: mode is 'refit' or 'rebuild', not {mode!r}")
        tris = np.ascontiguousarray(np.asarray(triangles, np.float32).reshape(-1, 9))
        _check(_scene_update(self._h, _fp(tris), tris.shape[0], modes[mode]), f"update({mode})")
        self.n = tris.shape[0]
        if bounds is not None:
            self.build_octree(*octree_bounds(*bounds))

    def set_option(self, key: str, value: float) -> None:
        """A render option (include/tmpt.h); applies to the renders after it."""
        _check(_set_option(self._h, key.encode(), float(value)), f"set_option({key!r})")

    def get_option(self, key: str) -> float:
        v = ctypes.c_double()
        _check(_get_option(self._h, key.encode(), ctypes.byref(v)), f"get_option({key!r})")
        return v.value

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- Scene::HitScene (scene.cpp:86-97)
    def hit_scene_batch(self, rays: np.ndarray, t_min: Optional[float] = None, t_max: Optional[float] = None,
                        any_hit: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """rays [n,6] (orig, dir) with one [t_min, t_max] for all, or rays [n,8]
        (orig, dir, tmin, tmax: the range per ray, as HitScene takes it,
        scene.h:36-37) with t_min = t_max = None
        -> (ids[n] triangle index or -1, hits[n,7] pos/normal/t)."""
        rays = np.asarray(rays, np.float32)
        if (t_min is None) != (t_max is None):
            raise ValueError("hit_scene_batch: give both t_min and t_max, or neither (ranged rays [n,8])")
        ranged = t_min is None and t_max is None
        rays = np.ascontiguousarray(rays.reshape(-1, 8 if ranged else 6))
        n = rays.shape[0]
        hits = np.zeros((n, 7), np.float32)
        ids = np.full(n, -1, np.int32)
        if ranged:
            _check(_scene_hit_ranged(self._h, _fp(rays), n, int(any_hit), _fp(hits), ids.ctypes.data_as(_i32p)),
                   "hit_scene")
        else:
            _check(_scene_hit(self._h, _fp(rays), n, t_min, t_max, int(any_hit), _fp(hits),
                              ids.ctypes.data_as(_i32p)), "hit_scene")
        return ids, hits

    def hit_scene_device(self, rays, t_min: Optional[float] = None, t_max: Optional[float] = None,
                         any_hit: bool = False, hits: bool = True, uv: bool = False, out=None,
                         wait_stream="current"):
        """:meth:`hit_scene_batch` on a torch tensor that lives on the scene's device
        (tmpt_scene_hit_device): nothing is copied to or from the host and nothing
        is allocated by the library per call.  ``rays``: a contiguous float32 tensor
        [n, 6] with one [t_min, t_max], or [n, 8] (the range per ray) with both
        ``None``, on ``cuda:<scene.device>``; anything else is a ``ValueError`` --
        no silent copy or cast.  Returns ``(ids, hits, uv)`` on that device: ids
        int32 [n]; hits float32 [n, 7] (pos, normal, t), zero-initialised, or
        ``None`` (``hits=False``); uv float32 [n, 2], Moller-Trumbore's (u, v) of
        the hit, zero-initialised, or ``None`` (``uv=False``).  Rows of rays that
        missed are not written.  ``out=(ids, hits, uv)``: preallocated tensors of
        those shapes (``None`` for either optional one); they decide which outputs
        are made.  The answers are :meth:`hit_scene_batch`'s bit for bit, whatever
        the options ``query_sort`` / ``query_top`` say.  The work starts after the
        work enqueued on ``wait_stream`` ("current": torch's current stream on the
        scene's device) and the call returns when it is complete on the device."""
        what = "hit_scene_device"
        if torch is None:
            raise TmptError(f"{what}: needs torch (tensors on the scene's device); hit_scene_batch takes numpy arrays")
        if (t_min is None) != (t_max is None):
            raise ValueError(f"{what}: give both t_min and t_max, or neither (ranged rays [n, 8])")
        ranged = t_min is None
        dev = torch.device("cuda", self.device)

        def tensor(t, name, dtype, shape):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}: {name} must be a torch tensor, not {type(t).__name__}")
            if t.device != dev:
                raise ValueError(f"{what}: {name} is on {t.device}, the scene is on {dev}")
            if t.dtype != dtype:
                raise ValueError(f"{what}: {name} must be {dtype}, not {t.dtype}")
            if shape is not None and tuple(t.shape) != shape:
                raise ValueError(f"{what}: {name} must have shape {list(shape)}, not {list(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous")

        tensor(rays, "rays", torch.float32, None)
        if rays.dim() != 2 or rays.shape[1] != (8 if ranged else 6):
            raise ValueError(f"{what}: rays must have shape [n, {8 if ranged else 6}] "
                             f"({'ranged' if ranged else 'with t_min and t_max'}), not {list(rays.shape)}")
        n = int(rays.shape[0])
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 3:
                raise ValueError(f"{what}: out = (ids, hits, uv)")
            ids, h, w = out
            if ids is None:
                raise ValueError(f"{what}: out's ids must be a tensor")
            tensor(ids, "out ids", torch.int32, (n,))
            if h is not None:
                tensor(h, "out hits", torch.float32, (n, 7))
            if w is not None:
                tensor(w, "out uv", torch.float32, (n, 2))
        else:
            ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
            h = torch.zeros((n, 7), dtype=torch.float32, device=dev) if hits else None
            w = torch.zeros((n, 2), dtype=torch.float32, device=dev) if uv else None
        fn = _sig("tmpt_scene_hit_device", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_HitDesc), ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
        d = _HitDesc()
        d.n, d.ranged, d.any_hit = n, int(ranged), int(bool(any_hit))
        d.tmin, d.tmax = (0.0, 0.0) if ranged else (t_min, t_max)
        ws = _wait_stream(self.device, wait_stream)
        if ws is not None:
            d.flags |= FLAG_WAIT_STREAM
            d.wait_stream = int(ws)
        _check(fn(self._h, ctypes.byref(d), rays.data_ptr(), ids.data_ptr(), None if h is None else h.data_ptr(),
                  None if w is None else w.data_ptr()), what)
        return ids, h, w

    #: the sort key of option ``query_sort`` (:func:`query_keys`; host only, needs no scene)
    query_keys = staticmethod(query_keys)

    def hit_scene(self, orig, direction, t_min: float, t_max: float) -> Tuple[int, Optional[Hit]]:
        """Same contract as the reference: returns (-1, None) on a miss and
        (1, Hit) on a hit (scene.cpp:37 sets 1, not the index)."""
        ids, hits = self.hit_scene_batch(np.concatenate([orig, direction])[None], t_min, t_max)
        if ids[0] < 0:
            return -1, None
        h = hits[0]
        return 1, Hit(h[0:3].copy(), h[3:6].copy(), float(h[6]))

    # -- TraceImageBody over parallel_for (main.cpp:180-246, 329-331)
    def trace_image(self, camera: Camera, width: int, height: int, spp: int,
                    seed_mode: int = SEED_ROW, engine: int = ENGINE_PERSISTENT, band_rows: int = 0,
                    shard: int = 0, num_shards: int = 1, count_visits: bool = False,
                    out=None, spp_begin: int = 0, spp_count: int = 0,
                    wait_stream="current") -> Tuple[np.ndarray, int]:
        """Render one shard.  Returns (rgba[tile_rows, width, 4] uint8, rays).
        Row 0 is the lowest rendered row (main.cpp:229; flipped on PNG write).
        ``out`` may be a device pointer (int) with tile_rows*width*4 bytes; the
        render then starts after the work already enqueued on ``wait_stream``
        ("current": torch's current stream on the scene's device when torch's
        GPU context is up, so a fill of ``out`` or a collective still reading
        it is ordered before the render; an int: a raw hipStream_t; None: no
        ordering).  The call returns once
        the frame is complete on the device.
        ``spp_begin``/``spp_count``: one progressive pass (persistent engine,
        pixel or sample seeding) -- see :meth:`trace_progressive`."""
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, seed_mode, band_rows, shard, num_shards, engine,
                       FLAG_COUNT_VISITS if count_visits else 0, spp_begin, spp_count)
        img = np.zeros((int(_tile_rows(ctypes.byref(d))), width, 4), np.uint8) if out is None else None
        rays = ctypes.c_uint64()
        cam = camera._to_c()
        _check(_render(self._h, ctypes.byref(cam), ctypes.byref(d), _hptr(img) if out is None else _dptr(out),
                       ctypes.byref(rays)), "trace_image")
        return img, int(rays.value)

    def trace_progressive(self, camera: Camera, width: int, height: int, spp: int, passes,
                          band_rows: int = 0, shard: int = 0, num_shards: int = 1, seed_mode: int = SEED_PIXEL):
        """Progressive spp: yields (samples_done, preview rgba, rays of the pass) per
        pass; ``passes`` = samples per pass (int) or a list of them summing to spp.
        The last preview is the final image, bit-identical to one full render;
        pixel or sample seeding (the samples of a pass run side by side there)."""
        if isinstance(passes, int):
            passes = [min(passes, spp - b) for b in range(0, spp, passes)]
        if sum(passes) != spp or min(passes) < 1:
            raise ValueError("passes must be positive and sum to spp")
        done = 0
        for n in passes:
            img, rays = self.trace_image(camera, width, height, spp, seed_mode=seed_mode,
                                         engine=ENGINE_PERSISTENT, band_rows=band_rows, shard=shard,
                                         num_shards=num_shards, spp_begin=done, spp_count=n)
            done += n
            yield done, img, rays

    def trace_aov(self, camera: Camera, width: int, height: int, spp: int, band_rows: int = 0,
                  shard: int = 0, num_shards: int = 1, out=None, wait_stream="current"):
        """The AOV pass of one shard (tmpt_render_aov): returns (records[tile_rows,
        width] of :data:`AOV_DTYPE`, rays) -- per pixel the summed hit normal,
        depth and first-bounce light scalar (each times 1/spp), sample 0's
        triangle id and the hit / lit sample counts, from the camera rays a
        ``SEED_SAMPLE`` :meth:`trace_image` of the same size and spp traces.
        rays = one closest-hit query per sample + one shadow query per hit.
        ``out`` (a device pointer with tile_rows*width*32 bytes, 16-byte aligned;
        then records is None) and ``wait_stream`` as in :meth:`trace_image`.
        Render option ``aov_group`` sets the lanes that share a pixel."""
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, SEED_SAMPLE, band_rows, shard, num_shards)
        rec = np.zeros((int(_tile_rows(ctypes.byref(d))), width), AOV_DTYPE) if out is None else None
        rays = ctypes.c_uint64()
        cam = camera._to_c()
        _check(_render_aov(self._h, ctypes.byref(cam), ctypes.byref(d), _hptr(rec) if out is None else _dptr(out),
                           ctypes.byref(rays)), "trace_aov")
        return rec, int(rays.value)

    def trace_radiance(self, camera: Camera, width: int, height: int, spp: int, seed_mode: int = SEED_SAMPLE,
                       band_rows: int = 0, shard: int = 0, num_shards: int = 1, out=None, wait_stream="current"):
        """:meth:`trace_image` of one shard on the persistent engine (pixel or
        sample seeding) that also hands out the linear radiance
        (tmpt_render_radiance): returns (float32[tile_rows, width, 4], rgba8[tile_rows,
        width, 4], rays) -- per pixel the colour sum in sample order times 1/spp
        (before the square root of the 8-bit image) with alpha 1.0, the very
        bytes and ray count of :meth:`trace_image`.  ``out``: a device pointer
        for the float tile (16-byte aligned), or a pair (float tile, rgba8 tile
        or None); the arrays returned are then None.  ``wait_stream`` as in
        :meth:`trace_image`."""
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, seed_mode, band_rows, shard, num_shards)
        rays = ctypes.c_uint64()
        cam = camera._to_c()
        rad = img = None
        if out is not None:
            f32, u8 = out if isinstance(out, (tuple, list)) else (out, None)
            ptrs = ctypes.c_void_p(int(f32)), _dptr(u8)
        else:
            rows = int(_tile_rows(ctypes.byref(d)))
            rad, img = np.zeros((rows, width, 4), np.float32), np.zeros((rows, width, 4), np.uint8)
            ptrs = _hptr(rad), _hptr(img)
        _check(_render_radiance(self._h, ctypes.byref(cam), ctypes.byref(d), *ptrs, ctypes.byref(rays)), "trace_radiance")
        return rad, img, int(rays.value)

    def trace_adaptive(self, camera: Camera, width: int, height: int, spp: int, spp_min: int = 0, spp_step: int = 0,
                       threshold: float = -1.0, band_rows: int = 0, shard: int = 0, num_shards: int = 1, out=None,
                       wait_stream="current", radius: int = 0):
        """Adaptive sampling of one shard (tmpt_render_adaptive; include/tmpt.h
        states its arithmetic): sample seeding on the persistent engine, ``spp``
        the cap.  Every pixel gets ``spp_min`` samples, a pixel still active
        ``spp_step`` more per pass, until the standard error of its luminance
        falls under the limit ``threshold`` sets (0 / 0 / negative: the
        defaults).  Returns (radiance float32[tile_rows, width, 4], rgba8[tile_rows,
        width, 4], spp_map int32[tile_rows, width], rays, info) -- a pixel that
        stopped at n is bit for bit the pixel of :meth:`trace_radiance` at
        spp = n; info is a dict of ``passes``, ``samples`` (the sum of the map)
        and ``pass_pixels`` (the pixels each pass traced).  ``out``: a triple of
        device pointers or None (float tile 16-byte aligned, rgba8 tile, int32
        map), at least one given; the arrays returned are then None.
        ``wait_stream`` as in :meth:`trace_image`.

        ``radius`` (0 .. 8; 0: none) is the neighbourhood rule: a pixel still
        active stays active while the variance test holds for itself or for any
        pixel within ``radius`` columns and ``radius`` rows of it, inside the
        frame and inside its own band of ``band_rows`` rows (0: the whole
        height is one band).  A stopped pixel never resumes, so per-count
        identity holds as before.  The neighbourhood is clipped to the band so
        that the tiles of any ``shard`` / ``num_shards`` assemble bit for bit
        into the ``num_shards = 1`` result with the same ``band_rows``; with a
        radius the result depends on ``band_rows`` (1-row bands: horizontal
        reach only)."""
        # bound on first use, as tmpt_fastdiv is
        fn = _sig("tmpt_render_adaptive", ctypes.c_int,
                  [ctypes.c_void_p, ctypes.POINTER(_Camera), ctypes.POINTER(_Desc), ctypes.POINTER(_AdaptiveDesc),
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_AdaptiveInfo), _u64p])
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, SEED_SAMPLE, band_rows, shard, num_shards)
        cam = camera._to_c()
        head = (self._h, ctypes.byref(cam), ctypes.byref(d), _adaptive_desc(spp_min, spp_step, threshold, radius))
        return _adaptive_call("trace_adaptive", fn, head, ("f32", "u8", "i32"), d, out)

    def denoise(self, radiance, aov, spp: int, levels: int = 0, normal_exp: int = -1, sigma_depth: float = 0.0,
                sigma_direct: float = 0.0, out=None, width: Optional[int] = None, height: Optional[int] = None,
                wait_stream="current"):
        """The AOV-guided a-trous filter (tmpt_denoise; include/tmpt.h states its
        arithmetic) over a whole frame: ``radiance`` float32[h, w, 4]
        (:meth:`trace_radiance`; shards assembled first), ``aov`` the frame's
        :data:`AOV_DTYPE` records [h, w] at ``spp`` (:meth:`trace_aov`).
        Returns (float32[h, w, 4], rgba8[h, w, 4]).  0 / -1 / 0.0 select the
        defaults: 5 levels, the normal cosine to the 32nd power, sigma_depth =
        1 / h, sigma_direct = 0.05.  ``out``: a float32 array [h, w, 4] that takes
        the filtered frame (it may be ``radiance`` itself).  Device form: ``radiance`` and ``aov`` are
        device pointers (ints, 16-byte aligned), ``width`` and ``height`` give
        the size and ``out`` = (float frame pointer or None, rgba8 pointer or
        None) -- the float output may be the input itself; returns (None, None)."""
        dev, h, w, frames = _frames("denoise", [(radiance, np.float32), (aov, AOV_DTYPE)], width, height, out,
                                    "radiance [h, w, 4] and aov [h, w]")
        d = _DenoiseDesc()
        d.width, d.height, d.spp, d.levels, d.normal_exp = w, h, spp, levels, normal_exp
        d.sigma_depth, d.sigma_direct = sigma_depth, sigma_direct
        return _filter_call("denoise", lambda d, *p: _denoise(self._h, d, *p), d, self.device, dev, frames, out,
                            wait_stream)

    def trace_moments(self, camera: Camera, width: int, height: int, spp: int, spp_min: Optional[int] = None,
                      spp_step: int = 0, threshold: float = -1.0, radius: int = 0, band_rows: int = 0, shard: int = 0,
                      num_shards: int = 1, out=None, wait_stream="current"):
        """:meth:`trace_adaptive` that also hands out each pixel's luminance
        moments (tmpt_render_moments; include/tmpt.h states them): returns
        (radiance, moments float32[tile_rows, width, 4], rgba8, spp_map, rays,
        info) -- moments = {m1 / n, m2 / n, 1 / n, 1.0} over the pixel's n
        samples, everything else bit for bit what :meth:`trace_adaptive` returns.
        ``spp_min=None`` means uniform: one pass, every pixel at ``spp`` (>= 2);
        ``spp_min=0`` the adaptive default.  A moments tile is a frame as
        :meth:`temporal` reads one (alpha = a history of length one): accumulate
        it exactly as the colour frame, then hand both to
        :meth:`denoise_moments`.  ``out``: a 4-tuple of device pointers (float
        tile or None, moments tile, rgba8 tile or None, int32 map or None); the
        arrays returned are then None.  ``wait_stream`` as in :meth:`trace_image`."""
        # bound on first use, as tmpt_render_adaptive is
        fn = _sig("tmpt_render_moments", ctypes.c_int,
                  [ctypes.c_void_p, ctypes.POINTER(_Camera), ctypes.POINTER(_Desc), ctypes.POINTER(_AdaptiveDesc),
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_AdaptiveInfo),
                   _u64p])
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, SEED_SAMPLE, band_rows, shard, num_shards)
        cam = camera._to_c()
        ad = None if spp_min is None else _adaptive_desc(spp_min, spp_step, threshold, radius)
        return _adaptive_call("trace_moments", fn, (self._h, ctypes.byref(cam), ctypes.byref(d), ad),
                              ("f32", "f32", "u8", "i32"), d, out)

    def denoise_moments(self, radiance, aov, moments, spp: int, shrink: float = 0.0, levels: int = 0,
                        normal_exp: int = -1, sigma_depth: float = 0.0, sigma_direct: float = 0.0, out=None,
                        width: Optional[int] = None, height: Optional[int] = None, wait_stream="current"):
        """The noise-aware filter (tmpt_denoise_moments; include/tmpt.h states its
        arithmetic): :meth:`denoise` with the frame's ``moments`` float32[h, w, 4]
        (:meth:`trace_moments`, or that frame accumulated by :meth:`temporal`) --
        at every level each pixel takes back the part of its removed detail that
        the noise estimate cannot explain.  ``shrink`` > 0 scales the estimate
        (0.0: the default, 2.0; larger filters more, 3e38 is :meth:`denoise`).
        Everything else, the host and the device form (``moments`` then a device
        pointer too) as :meth:`denoise`."""
        # bound on first use, as tmpt_render_adaptive is
        fn = _sig("tmpt_denoise_moments", ctypes.c_int,
                  [ctypes.c_void_p, ctypes.POINTER(_DenoiseDesc), ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
        dev, h, w, frames = _frames("denoise_moments", [(radiance, np.float32), (aov, AOV_DTYPE), (moments, np.float32)],
                                    width, height, out, "radiance and moments [h, w, 4] and aov [h, w]")
        d = _DenoiseDesc()
        d.width, d.height, d.spp, d.levels, d.normal_exp = w, h, spp, levels, normal_exp
        d.sigma_depth, d.sigma_direct = sigma_depth, sigma_direct
        return _filter_call("denoise_moments", lambda d, *p: fn(self._h, d, shrink, *p), d, self.device, dev, frames, out,
                            wait_stream)

    def trace_motion(self, camera: Camera, prev_camera: Camera, width: int, height: int, prev_triangles=None,
                     band_rows: int = 0, shard: int = 0, num_shards: int = 1, out=None, wait_stream="current"):
        """The motion pass of one shard (tmpt_render_motion; include/tmpt.h states
        its arithmetic): returns (records[tile_rows, width] of :data:`MOTION_DTYPE`,
        rays) -- per pixel the closest hit of its centre ray (depth, barycentrics,
        triangle id) and where that surface point lay in the previous frame:
        ``prev_triangles`` [n, 3, 3] is the previous pose (``None``: the geometry
        did not move), ``prev_camera`` the previous camera; ``px``, ``py`` are
        continuous pixel coordinates of the whole frame.  rays = the tile's
        pixels.  Device form: ``out`` a device pointer with tile_rows*width*32
        bytes (16-byte aligned; then records is None), ``prev_triangles`` a
        device pointer to the scene's n x 9 floats or None, ``wait_stream`` as in
        :meth:`trace_image`."""
        # bound on first use, as tmpt_fastdiv is
        fn = _sig("tmpt_render_motion", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_Camera),
                                                       ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int32,
                                                       ctypes.POINTER(_Desc), ctypes.c_void_p, _u64p])
        d = _tile_desc(self.device, out, wait_stream, width, height, 1, SEED_SAMPLE, band_rows, shard, num_shards)
        rays = ctypes.c_uint64()
        cam, pcam = camera._to_c(), prev_camera._to_c()
        if out is not None:
            _check(fn(self._h, ctypes.byref(cam), ctypes.byref(pcam), _dptr(prev_triangles), self.n, ctypes.byref(d),
                      ctypes.c_void_p(int(out)), ctypes.byref(rays)), "trace_motion")
            return None, int(rays.value)
        pt, pn = None, 0
        if prev_triangles is not None:
            pt = np.ascontiguousarray(np.asarray(prev_triangles, np.float32).reshape(-1, 9))
            pn = pt.shape[0]
        rec = np.zeros((int(_tile_rows(ctypes.byref(d))), width), MOTION_DTYPE)
        _check(fn(self._h, ctypes.byref(cam), ctypes.byref(pcam), _hptr(pt), pn, ctypes.byref(d), _hptr(rec),
                  ctypes.byref(rays)), "trace_motion")
        return rec, int(rays.value)

    def temporal(self, radiance, motion, prev_motion, history, n_max: float = 0.0, sigma_depth: float = 0.0,
                 out=None, width: Optional[int] = None, height: Optional[int] = None, wait_stream="current"):
        """One step of temporal accumulation (tmpt_temporal; include/tmpt.h states
        its arithmetic) over a whole frame: ``radiance`` float32[h, w, 4] (this
        frame, :meth:`trace_radiance`), ``motion`` and ``prev_motion`` the
        :data:`MOTION_DTYPE` records [h, w] of this frame and the previous one
        (:meth:`trace_motion`), ``history`` float32[h, w, 4] the previous
        accumulation, whose alpha is its history length (a plain radiance frame
        is a history of length one).  Returns (float32[h, w, 4], rgba8[h, w, 4]):
        keep the float frame as the next history.  0.0 selects the defaults
        (n_max 3, sigma_depth 0.05; raise n_max where little moves).  ``out``: a float32 array [h, w, 4] that
        takes the frame (it may be ``radiance`` itself, never ``history``).
        Device form, as :meth:`denoise`: the four inputs are device pointers
        (ints, 16-byte aligned), ``width`` and ``height`` give the size and
        ``out`` = (float frame pointer or None, rgba8 pointer or None); returns
        (None, None)."""
        fn = _sig("tmpt_temporal", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_TemporalDesc), ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p])
        dev, h, w, frames = _frames("temporal", [(radiance, np.float32), (motion, MOTION_DTYPE),
                                                 (prev_motion, MOTION_DTYPE), (history, np.float32)], width, height, out,
                                    "radiance and history [h, w, 4], motion and prev_motion [h, w]")
        d = _TemporalDesc()
        d.width, d.height, d.n_max, d.sigma_depth = w, h, n_max, sigma_depth
        return _filter_call("temporal", lambda d, *p: fn(self._h, d, *p), d, self.device, dev, frames, out, wait_stream)

    def temporal_clip(self, radiance, motion, prev_motion, history, gamma: float = 0.0, radius: int = 0,
                      n_max: float = 0.0, sigma_depth: float = 0.0, stat=None, aux=None, aux_history=None, out=None,
                      width: Optional[int] = None, height: Optional[int] = None, wait_stream="current"):
        """:meth:`temporal` with history clipping (tmpt_temporal_clip; include/tmpt.h
        states its arithmetic): the reprojected history is pulled into the box
        mean +- ``gamma`` standard deviations of the (2 ``radius`` + 1)^2 window of
        ``stat`` (float32[h, w, 4]; ``None``: ``radiance`` itself) around the
        pixel, and loses length by how far it was pulled.  ``aux`` and
        ``aux_history`` (both or neither, float32[h, w, 4]: a moments frame of
        :meth:`trace_moments` and its accumulation) ride through the same taps and
        blend factor, unclipped.  Returns (float32[h, w, 4], rgba8[h, w, 4], aux
        frame or None).  0 selects the defaults.  ``out``: a float32 array
        [h, w, 4] that takes the frame; unlike :meth:`temporal` it may be neither
        ``radiance`` nor ``stat`` nor a history.
        Device form, as :meth:`temporal`: every frame a device pointer (int,
        16-byte aligned; ``stat`` may stay ``None``), ``width`` and ``height`` give
        the size and ``out`` = (float frame pointer or None, rgba8 pointer or
        None, aux frame pointer or None: given exactly when ``aux`` is); returns
        (None, None, None)."""
        # bound on first use, as tmpt_render_adaptive is
        fn = _sig("tmpt_temporal_clip", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_TemporalClipDesc)]
                  + [ctypes.c_void_p] * 10)
        if (aux is None) != (aux_history is None):
            raise ValueError("temporal_clip: aux and aux_history go together")
        given = {"radiance": (radiance, np.float32), "motion": (motion, MOTION_DTYPE),
                 "prev_motion": (prev_motion, MOTION_DTYPE), "history": (history, np.float32), "stat": (stat, np.float32),
                 "aux": (aux, np.float32), "aux_history": (aux_history, np.float32)}
        given = {k: v for k, v in given.items() if v[0] is not None}  # stat and the aux pair may be absent
        dev, h, w, frames = _frames("temporal_clip", list(given.values()), width, height, out,
                                    "radiance, history, stat, aux and aux_history [h, w, 4], motion and "
                                    "prev_motion [h, w]")
        f = dict(zip(given, frames))
        d = _TemporalClipDesc()
        d.width, d.height, d.n_max, d.sigma_depth, d.gamma, d.radius = w, h, n_max, sigma_depth, gamma, radius
        res = img = aux_res = None
        if dev:
            _device_form(d, self.device, wait_stream)
            ptr, (f32, u8, ao) = _dptr, out
        else:
            ptr, f32, u8 = _hptr, _out_frame("temporal_clip", out, h, w), np.zeros((h, w, 4), np.uint8)
            ao = None if aux is None else np.zeros((h, w, 4), np.float32)
            res, img, aux_res = f32, u8, ao
        order = ("radiance", "stat", "motion", "prev_motion", "history", "aux", "aux_history")  # the C signature's
        frames = [f.get(k) for k in order] + [ao, f32, u8]
        _check(fn(self._h, ctypes.byref(d), *[ptr(x) for x in frames]), "temporal_clip")
        return res, img, aux_res

    def sample_plan(self, motion, prev_motion, moments_history, n_max: float = 0.0, sigma_depth: float = 0.0, out=None,
                    width: Optional[int] = None, height: Optional[int] = None, wait_stream="current"):
        """The sample plan of history-guided sampling (tmpt_sample_plan;
        include/tmpt.h states its arithmetic) over a whole frame: the accumulated
        moments frame ``moments_history`` float32[h, w, 4] (the aux frame
        :meth:`temporal_clip` returns, or a moments frame through :meth:`temporal`)
        fetched where ``motion`` says each pixel's surface was and accepted where
        ``prev_motion`` shows the same depth, as :meth:`temporal` fetches a
        history, and turned into the per-pixel prior of :meth:`trace_guided`:
        returns float32[h, w, 4] = {history luminance, the history's share of the
        blended pixel's variance, the blend factor of this frame, history
        length}; {0, 0, 1, 0} (the null prior) where the history restarts.  Use
        the ``n_max`` and ``sigma_depth`` of the blend that will follow (0.0: the
        defaults of :meth:`temporal`).  ``out``: a float32 array [h, w, 4] that
        takes the prior (never ``moments_history``).  Torch tensors on the
        scene's device may be given in place of the three arrays (``motion`` and
        ``prev_motion`` as uint8 [h, w, 32] or any tensor of h*w*32 bytes): the
        prior is then a torch tensor too (``out``: a contiguous float32 tensor
        [h, w, 4], or None).  Device-pointer form, as :meth:`temporal`: three ints
        (16-byte aligned), ``width``, ``height`` and ``out`` = the prior's
        pointer; returns None."""
        # bound on first use, as tmpt_render_adaptive is
        fn = _sig("tmpt_sample_plan", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(_TemporalDesc)]
                  + [ctypes.c_void_p] * 4)
        d = _TemporalDesc()
        tens = hasattr(moments_history, "data_ptr")
        dev = tens or isinstance(moments_history, int)
        res = None
        if tens:
            if tuple(moments_history.shape[2:]) != (4,) or moments_history.dim() != 3:
                raise ValueError("sample_plan: moments_history [h, w, 4] of one whole frame")
            h, w = int(moments_history.shape[0]), int(moments_history.shape[1])
            for t, size, name in ((moments_history, 16, "moments_history"), (motion, 32, "motion"),
                                  (prev_motion, 32, "prev_motion")):
                if (not hasattr(t, "data_ptr") or not t.is_contiguous() or t.numel() * t.element_size() != h * w * size
                        or t.device != moments_history.device):
                    raise ValueError(f"sample_plan: {name} must be a contiguous tensor of one whole frame on the "
                                     "history's device")
            if moments_history.dtype != torch.float32:
                raise ValueError("sample_plan: moments_history must be float32")
            res = torch.empty((h, w, 4), dtype=torch.float32, device=moments_history.device) if out is None else out
            if not (hasattr(res, "data_ptr") and res.dtype == torch.float32 and tuple(res.shape) == (h, w, 4)
                    and res.is_contiguous() and res.device == moments_history.device):
                raise ValueError("sample_plan: out must be a contiguous float32 tensor [h, w, 4] on the history's device")
            ptrs = [t.data_ptr() for t in (motion, prev_motion, moments_history, res)]
        elif dev:
            if width is None or height is None or out is None:
                raise ValueError("sample_plan: device pointers need width, height and out")
            h, w = int(height), int(width)
            ptrs = [int(motion), int(prev_motion), int(moments_history), int(out)]
        else:
            moments_history = np.ascontiguousarray(moments_history, np.float32)
            motion = np.ascontiguousarray(motion, MOTION_DTYPE)
            prev_motion = np.ascontiguousarray(prev_motion, MOTION_DTYPE)
            h, w = moments_history.shape[:2]
            if moments_history.shape != (h, w, 4) or motion.shape != (h, w) or prev_motion.shape != (h, w):
                raise ValueError("sample_plan: moments_history [h, w, 4], motion and prev_motion [h, w] of one whole "
                                 "frame")
            res = _out_frame("sample_plan", out, h, w)
            ptrs = [a.ctypes.data for a in (motion, prev_motion, moments_history, res)]
        d.width, d.height, d.n_max, d.sigma_depth = w, h, n_max, sigma_depth
        if dev:
            _device_form(d, self.device, wait_stream)
        _check(fn(self._h, ctypes.byref(d), *[ctypes.c_void_p(p) for p in ptrs]), "sample_plan")
        return res

    def trace_guided(self, camera: Camera, width: int, height: int, spp: int, prior=None,
                     spp_min: Optional[int] = None, spp_step: int = 0, threshold: float = -1.0, radius: int = 0,
                     band_rows: int = 0, shard: int = 0, num_shards: int = 1, out=None, wait_stream="current"):
        """:meth:`trace_moments` whose stopping test reads a per-pixel ``prior``
        (tmpt_render_guided; include/tmpt.h states the test): the variance and the
        mean are judged as the temporal blend will leave them, so a pixel with a
        long, quiet history stops at ``spp_min`` (2 is the least) and a pixel
        whose history restarted runs on as in :meth:`trace_moments`.  Returns
        :meth:`trace_moments`' tuple (radiance, moments, rgba8, spp_map, rays,
        info).  ``prior`` is always the WHOLE frame float32[height, width, 4] of
        :meth:`sample_plan`, a numpy array or a torch tensor on the scene's
        device; the method hands the call the shard's rows
        (:func:`tile_row_to_y`), gathered on the device for a tensor.  ``None``
        (or a frame of {0, 0, 1, 0}) is :meth:`trace_moments` bit for bit.
        ``out``: a 4-tuple of device pointers, any of them None but not all (the
        moments tile is optional here); the arrays returned are then None.
        ``wait_stream`` as in :meth:`trace_image`."""
        # bound on first use, as tmpt_render_adaptive is
        fn = _sig("tmpt_render_guided", ctypes.c_int,
                  [ctypes.c_void_p, ctypes.POINTER(_Camera), ctypes.POINTER(_Desc), ctypes.POINTER(_AdaptiveDesc),
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.POINTER(_AdaptiveInfo), _u64p])
        d = _tile_desc(self.device, out, wait_stream, width, height, spp, SEED_SAMPLE, band_rows, shard, num_shards)
        tile = None  # the prior's rows of this shard, kept alive over the call
        if prior is not None:
            if tuple(prior.shape) != (height, width, 4):
                raise ValueError("trace_guided: prior is the whole frame [height, width, 4]")
            ys = tile_row_to_y(width, height, band_rows, shard, num_shards)
            whole = len(ys) == height and bool((ys == np.arange(height)).all())
            if hasattr(prior, "data_ptr"):
                if prior.dtype != torch.float32:
                    raise ValueError("trace_guided: prior must be float32")
                tile = prior if whole else prior.index_select(0, torch.as_tensor(ys, device=prior.device))
                tile = tile.contiguous()
                if out is None:
                    tile = tile.cpu().numpy()
            else:
                tile = np.ascontiguousarray(np.asarray(prior, np.float32)[ys])
                if out is not None:
                    if torch is None:
                        raise ValueError("trace_guided: device outputs need a torch prior")
                    tile = torch.from_numpy(tile).to(f"cuda:{self.device}")
        p_ptr = None
        if tile is not None:
            p_ptr = ctypes.c_void_p(tile.data_ptr() if hasattr(tile, "data_ptr") else tile.ctypes.data)
        ad = None if spp_min is None else _adaptive_desc(spp_min, spp_step, threshold, radius)
        cam = camera._to_c()
        if out is not None and tile is not None and not d.flags & FLAG_WAIT_STREAM:
            torch.cuda.current_stream(self.device).synchronize()  # the gathered rows are ready
        return _adaptive_call("trace_guided", fn, (self._h, ctypes.byref(cam), ctypes.byref(d), ad, p_ptr),
                              ("f32", "f32", "u8", "i32"), d, out)

    def camera_rays(self, camera: Camera, width: int, height: int, spp: int, spp_begin: int = 0,
                    spp_count: int = 0, band_rows: int = 0, shard: int = 0, num_shards: int = 1) -> np.ndarray:
        """The camera pre-pass of sample seeding run alone (tmpt_camera_rays; render
        option ``cam_pre``): uint32[slots, count, 8] -- per tile pixel slot and
        sample of the pass the ray's origin [0:3] and direction [3:6] as float32
        bits, the RNG state after the camera's draws [6] and the flag word [7]
        (include/tmpt.h)."""
        # bound on first use, as tmpt_fastdiv is
        fn = _sig("tmpt_camera_rays", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p])
        d = _desc(width, height, spp, SEED_SAMPLE, band_rows, shard, num_shards, ENGINE_PERSISTENT, 0,
                  spp_begin, spp_count)
        slots = int(_tile_rows(ctypes.byref(d))) * width
        count = spp_count if spp_count > 0 else spp - spp_begin
        out = np.zeros((slots, max(count, 0), 8), np.uint32)
        cam = camera._to_c()
        _check(fn(self._h, ctypes.byref(cam), ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p)), "camera_rays")
        return out

    def dump_bvh(self, layout: str = "aos") -> dict:
        """The built BVH as the kernels read it (tmpt_scene_dump_bvh; include/tmpt.h
        states the encoding and the invariants): ``nodes`` uint32[n_nodes4, 16],
        ``tris`` uint32[n + 1, 12] and ``info``, a dict of n, n_nodes4, depth4,
        leaf_max, count_shift, link_bits, builder_iters and soa.  ``layout="soa"``
        puts the two arrays together again from the SoA planes (an error on a
        scene built without ``layout=soa``).  Launches no kernel."""
        if layout not in ("aos", "soa"):
            raise ValueError("dump_bvh: layout is 'aos' or 'soa'")
        # bound on first use, as tmpt_fastdiv is
        fn = _sig("tmpt_scene_dump_bvh", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                        ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, _i32p])
        info = np.zeros(8, np.int32)
        lay = int(layout == "soa")
        _check(fn(self._h, lay, None, 0, None, 0, info.ctypes.data_as(_i32p)), "dump_bvh")
        nodes = np.zeros((int(info[1]), 16), np.uint32)
        tris = np.zeros((int(info[0]) + 1, 12), np.uint32)
        _check(fn(self._h, lay, nodes.ctypes.data, nodes.size, tris.ctypes.data, tris.size,
                  info.ctypes.data_as(_i32p)), "dump_bvh")
        keys = ("n", "n_nodes4", "depth4", "leaf_max", "count_shift", "link_bits", "builder_iters", "soa")
        return {"nodes": nodes, "tris": tris, "info": dict(zip(keys, (int(v) for v in info)))}

    def dump_octree(self) -> dict:
        """The octree the scene holds, as its kernels read it (tmpt_scene_dump_octree):
        the arrays of :func:`octree_arrays`; all empty on a scene without one.
        Synchronises the scene's stream, launches no kernel."""
        fn = _sig("tmpt_scene_dump_octree", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                           ctypes.c_void_p])
        info = np.zeros(5, np.int64)
        grid = np.zeros(16, np.float32)
        _check(fn(self._h, None, 0, None, 0, info.ctypes.data, grid.ctypes.data), "dump_octree")
        nodes = np.zeros((int(info[0]), 8), np.uint32)
        refs = np.zeros(int(info[2]), np.int32)
        if nodes.size:
            _check(fn(self._h, nodes.ctypes.data, nodes.size, refs.ctypes.data, refs.size, info.ctypes.data,
                      grid.ctypes.data), "dump_octree")
        return _octree_result(nodes, refs, info, grid)

    def radix_sort(self, keys, vals, bits: int = 32):
        """The device radix sort of the build and the pixel supply on caller data
        (tmpt_radix_sort): returns (keys, vals) uint32, stably ordered by the low
        8 * ceil(bits / 8) bits of the key; at most 2^22 pairs."""
        fn = _sig("tmpt_radix_sort", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_int64, ctypes.c_int32])
        k = np.array(keys, dtype=np.uint32).reshape(-1)
        v = np.array(vals, dtype=np.uint32).reshape(-1)
        if k.shape != v.shape:
            raise ValueError("radix_sort: keys and vals of one length")
        _check(fn(self._h, k.ctypes.data, v.ctypes.data, k.size, bits), "radix_sort")
        return k, v

    def stats(self) -> RenderStats:
        s = _Stats()
        _check(_stats(self._h, ctypes.byref(s)), "stats")
        return RenderStats(*[getattr(s, f) for f, _ in _Stats._fields_ if not f.startswith("reserved")])


def render_multi(tris: np.ndarray, camera: "Camera", width: int, height: int, spp: int, devices,
                 seed_mode: int = SEED_PIXEL, engine: int = ENGINE_PERSISTENT,
                 require_rccl: bool = False, bounds=None) -> Tuple[np.ndarray, int, float]:
    """One frame over several devices in this process (tmpt_render_multi: the
    tiles gathered to devices[0] by one RCCL gather): returns (rgba[height,
    width, 4], rays, seconds from the renders' start to the assembled frame).
    A device may repeat (then the gather is device-to-device copies; with
    require_rccl that is an error instead).  ``bounds`` (OBJ bounds): every
    device's scene builds the reference's octree (main.cpp:312)."""
    t = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 9))
    devs = (ctypes.c_int32 * len(devices))(*devices)
    img = np.zeros((height, width, 4), np.uint8)
    rays = ctypes.c_uint64()
    secs = ctypes.c_double()
    d = _desc(width, height, spp, seed_mode, 0, 0, 1, engine, FLAG_REQUIRE_RCCL if require_rccl else 0)
    cam = camera._to_c()
    box = None if bounds is None else np.concatenate(octree_bounds(*bounds)).astype(np.float32)
    _check(_render_multi(t.ctypes.data_as(_f32p), t.shape[0], None if box is None else _fp(box),
                         ctypes.byref(cam), ctypes.byref(d), devs,
                         len(devices), img.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rays),
                         ctypes.byref(secs)), "render_multi")
    return img, int(rays.value), float(secs.value)


def write_png(path: str, rgba: np.ndarray) -> None:
    """stbi_write_png with flip-on-write (main.cpp:341-342): rgba rows bottom-up."""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    _check(_write_png(path.encode(), rgba.ctypes.data_as(_u8p), w, h), "write_png")
