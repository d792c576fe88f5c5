"""The device BVH build (tmpt_bvh.hip) on adversarial geometry.

Every case of geometry_cases.py is built and queried, and the answers are
compared with the oracle's linear scan (no tree at all, lowest index on a tie
in t).  Tolerance: none -- triangle ids bit for bit, and the hit records
(position, normal, t) where a triangle was hit; the any-hit bit equals
id >= 0.  The scenes have no octree, so ties go to the lowest index.

What the cases are after: partial blocks and tiles of the sort and the scans
(the count sweep), key ties in the Karras hierarchy and area ties in PLOC
(coincident and same-box triangles, one Morton cell), zero Morton extents
(flat, collinear), PLOC's chains and the fallbacks from them (identical and
nested boxes), the per-axis exponent and the outward rounding of the
quantised child boxes and the relative box padding (translated, scaled,
anisotropic), and zero-area triangles, which no ray may be answered with.
"""
import functools

import numpy as np
import pytest

import geometry_cases as G
import oracle
import toymeshpathtracer_amd as tm

pytestmark = pytest.mark.gpu

STACK = 128  # kStackTotal (tmpt_internal.h): a BVH4 level costs the traversal at most 3 entries

OPTION_SETS = [{"builder": "lbvh"}, {"leaf_max": 1}, {"leaf_max": 16}, {"collapse": "sah"}, {"layout": "soa"},
               {"ploc_radius": 1}, {"ploc_radius": 256}]


def _opt_id(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


@functools.lru_cache(maxsize=None)
def _cases():
    return G.cases()


@functools.lru_cache(maxsize=None)
def _reference(name, nrays):
    """Rays of a case and the linear scan's answers: computed once, shared by
    every build of the case (arrays made read-only)."""
    tris = _cases()[name]
    rays, rng = G.rays(tris, nrays, seed=3)
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    oids, ohits = osc.hit_batch(rays, *rng)
    for a in (rays, oids, ohits):
        a.setflags(write=False)
    return rays, rng, oids, ohits


def _build_and_query(name, opts, nrays):
    """-> list of what is wrong with this build of the case (empty: nothing)."""
    tris = _cases()[name]
    n = tris.shape[0]
    rays, (tmin, tmax), oids, ohits = _reference(name, nrays)
    try:
        with tm.Scene(tris, options=opts or None) as sc:
            st = sc.stats()
            ids, hits = sc.hit_scene_batch(rays, tmin, tmax)
            aids, _ = sc.hit_scene_batch(rays, tmin, tmax, any_hit=True)
    except tm.TmptError as e:
        return [f"{name}: {e}"]
    print(f"{name} [{_opt_id(opts)}]: n {n} bvh4_nodes {st.bvh4_nodes} bvh4_depth {st.bvh4_depth} "
          f"builder_iters {st.builder_iters} hits {(oids >= 0).mean():.3f}")
    bad = []
    if st.n_tris != n:
        bad.append(f"{name}: n_tris {st.n_tris} != {n}")
    if 3 * st.bvh4_depth + 1 > STACK:
        bad.append(f"{name}: bvh4_depth {st.bvh4_depth} overruns the traversal stack")
    # PLOC passes; 0 = the scene holds the LBVH: asked for, or (nested200) fallen back to
    lbvh = opts.get("builder") == "lbvh" or name == "nested200"
    if n > 1 and (st.builder_iters != 0 if lbvh else not st.builder_iters > 0):
        bad.append(f"{name}: builder_iters {st.builder_iters}, {'LBVH' if lbvh else 'PLOC'} expected")
    mism = np.nonzero(ids != oids)[0]
    if mism.size:
        bad.append(f"{name}: {mism.size} id mismatches, first rays {mism[:5]} gpu {ids[mism[:5]]} "
                   f"scan {oids[mism[:5]]}")
    h = (ids >= 0) & (ids == oids)
    rec = np.nonzero((hits[h].view(np.uint32) != ohits[h].view(np.uint32)).any(1))[0]
    if rec.size:
        bad.append(f"{name}: {rec.size} hit records differ, first rays {np.nonzero(h)[0][rec[:5]]}")
    anyb = np.nonzero((aids >= 0) != (oids >= 0))[0]
    if anyb.size:
        bad.append(f"{name}: {anyb.size} any-hit bits differ, first rays {anyb[:5]}")
    if name.startswith("coincident") and not (ids <= 0).all():
        bad.append(f"{name}: a tie on t answered with index {ids.max()}, not 0")
    if G.zero_area(tris)[ids[ids >= 0]].any():
        bad.append(f"{name}: a zero-area triangle was the answer")
    return bad


SWEEP_GROUPS = {"3-68": range(3, 69), "69-136": range(69, 137), "137-204": range(137, 205),
                "205-272": range(205, 273), "large": G.SWEEP_NODES + G.SWEEP_LARGE}


@pytest.mark.parametrize("group", list(SWEEP_GROUPS))
def test_count_sweep(gpu, group):
    """Soup of every count of 3..272 and of the counts around the sort tile
    (1024, 2048) and the scan's switch (4096), and two counts whose BVH4 node
    counts pass the LDS top caches -- default build, 4,000 rays each."""
    bad = []
    for n in SWEEP_GROUPS[group]:
        bad += _build_and_query(G.sweep_name(n), {}, 4000)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", G.NON_SWEEP)
def test_case_default_build(gpu, name):
    """Every family under the default options (PLOC, greedy collapse, leaf_max 2), 20,000 rays."""
    bad = _build_and_query(name, {}, 20000)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", G.NON_SWEEP)
@pytest.mark.parametrize("opts", OPTION_SETS, ids=_opt_id)
def test_case_build_options(gpu, opts, name):
    """Every family under each build option: the tree changes, the answers do
    not.  coincident1000 with leaf_max=16 is the 1000-way tie on t in 16-wide
    leaves: index 0 must win."""
    bad = _build_and_query(name, opts, 20000)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- renders through the path kernels
# Unit-scale cases only: the path engines trace with the reference's constant
# range 0.001 .. 1e7.  The three soups put the default build's BVH4 node count
# below the 5-wave kernels' LDS top cache (kTopNodes5 = 80), between it and the
# 4-wave one's fill limit (kTopNodes - 4 = 116), and above the whole cache
# (kTopNodes = 120); the counts were read from test_count_sweep's printout.
RENDER_SOUPS = {"soup200": (0, 79), "soup330": (81, 116), "soup480": (121, 1 << 30)}
RENDER_CASES = list(RENDER_SOUPS) + ["coincident200", "degenerate_mix", "flat_z", "uniform_sheet"]
W, H, SPP = 48, 27, 4

RENDER_CONFIGS = [("persistent", "pixel", 4, 0), ("persistent", "pixel", 4, 1), ("persistent", "pixel", 5, 0),
                  ("persistent", "pixel", 5, 1), ("persistent", "sample", 4, None), ("persistent", "sample", 5, None),
                  ("wavefront", "pixel", None, None), ("megakernel", "pixel", None, None)]
_ENGINE = {"persistent": tm.ENGINE_PERSISTENT, "wavefront": tm.ENGINE_WAVEFRONT, "megakernel": tm.ENGINE_MEGAKERNEL}


def _config_id(c):
    engine, seed, waves, help_ = c
    return "-".join([engine, seed] + ([f"path_waves{waves}"] if waves else []) +
                    ([f"help{help_}"] if help_ is not None else []))


def _camera(tris):
    """The reference's placement (main.cpp:295-307) over the case's vertex box.
    It leaves most samples as misses: at 48x27x4 the linear scan counts 5,216 ..
    6,474 rays for the 5,184 camera samples of every case but two, so at most
    about a fifth of them hit anything.  test_gpu_reference_mode.py renders the
    same families through cameras that at least 40 % of the samples hit."""
    v = tris.reshape(-1, 3)
    return tm.Camera.for_scene(v.min(0), v.max(0), W, H)


@functools.lru_cache(maxsize=None)
def _reference_frame(name, seed):
    tris = _cases()[name]
    osc = oracle.Scene(tris, accel=oracle.ACCEL_LINEAR, tie=oracle.TIE_INDEX)
    img, rays = osc.render(_camera(tris).as_array(), W, H, SPP,
                           seed_mode=oracle.SEED_PIXEL if seed == "pixel" else oracle.SEED_SAMPLE)
    img.setflags(write=False)
    return img, rays


@pytest.mark.parametrize("name", RENDER_CASES)
@pytest.mark.parametrize("config", RENDER_CONFIGS, ids=_config_id)
def test_case_renders(gpu, config, name):
    """A 48x27 frame at 4 spp of each unit-scale case, through every path
    engine: the persistent one in pixel and sample seeding with the 4-wave and
    the 5-wave kernels (pixel seeding with and without the shadow offload),
    wavefront and megakernel in pixel seeding.  Image and ray count equal the
    linear scan's render byte for byte."""
    engine, seed, waves, help_ = config
    tris = _cases()[name]
    ref, ref_rays = _reference_frame(name, seed)
    with tm.Scene(tris) as sc:
        if name in RENDER_SOUPS:
            lo, hi = RENDER_SOUPS[name]
            assert lo <= sc.stats().bvh4_nodes <= hi, (name, sc.stats().bvh4_nodes)
        if waves:
            sc.set_option("path_waves", waves)
        if help_ is not None:
            sc.set_option("help", help_)
        img, rays = sc.trace_image(_camera(tris), W, H, SPP, engine=_ENGINE[engine],
                                   seed_mode=tm.SEED_PIXEL if seed == "pixel" else tm.SEED_SAMPLE)
    assert rays == ref_rays
    diff = np.nonzero((img != ref).any(-1))
    assert diff[0].size == 0, f"{diff[0].size} pixels differ, first at {list(zip(*diff))[:5]}"
