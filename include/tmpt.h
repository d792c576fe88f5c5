/*
 * tmpt.h -- C ABI of libtmpt.so, the MI355X-native (gfx950) hot path of
 * pr0g/ToyMeshPathTracer: Trace() -> Scatter() -> Scene::HitScene().
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes
 * (0 = ok, < 0 = error; message in tmpt_last_error(); -30 only from the
 * checked build, make CHECK=1: a device index test failed during the call),
 * no C++ exceptions and no
 * torch types cross this boundary.  Every entry point names the reference
 * interface it replaces (/root/reference/source/<file>:<line>); INTEGRATION.md
 * shows the reference-side binding.
 *
 * Threading: one scene per device.  Calls on different scenes may run from
 * different host threads at once; one scene handle is not re-entrant for
 * concurrent render calls.  Host buffers are caller-owned; device memory is
 * library-owned unless a flag says the caller passes a device pointer.
 */
#ifndef TMPT_H
#define TMPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMPT_ABI_VERSION 9  /* 2: progressive spp (spp_begin / spp_count); 3: tmpt_render_multi;
                              4: tmpt_unit_sincos; 5: wait_stream (TMPT_FLAG_WAIT_STREAM),
                              progressive continuation keyed on the camera,
                              TMPT_SEED_SAMPLE; 6: scene options (tmpt_scene_create_ex,
                              tmpt_scene_set_option / get_option) replace the
                              library's environment variables, tmpt_scene_hit_ranged
                              (per-ray tmin / tmax), tmpt_render_multi gathers over RCCL;
                              7: tmpt_scene_build_octree (the reference's octree: its answer
                              for closest hits tied on t and for rays its root box drops),
                              option tie_rule, tmpt_octree_digest, tmpt_stats octree / tie /
                              row-engine fields, tmpt_render_multi takes the octree box,
                              options tie_defer / redo_cap, tmpt_stats.redo_samples;
                              8: the octree answers crack queries and flat triangles too
                              (tmpt_stats.crack_queries, octree_flat), tmpt_stats.redo_launches /
                              redo_ms (k_redo apart from the k_path launches);
                              9: tmpt_stats.tie_path (how the last render answered the
                              octree's queries, and whether the deferred form fell back);
                              still 9, additive: tmpt_render_aov and tmpt_aov_pixel (the AOV pass) and
                              the render option aov_group -- no struct above changed, so the version
                              did not: callers detect the entry point by its symbol;
                              still 9, additive: tmpt_render_radiance (the float frame of a render),
                              tmpt_denoise and tmpt_denoise_desc (the AOV-guided a-trous filter) and the
                              render option denoise_lds -- again no struct above changed;
                              still 9, additive: the check hooks tmpt_scene_dump_bvh and tmpt_radix_sort;
                              still 9, additive: tmpt_render_adaptive with tmpt_adaptive_desc and
                              tmpt_adaptive_info (adaptive sampling) -- no struct above changed;
                              still 9, additive: tmpt_adaptive_desc.radius (the neighbourhood rule of
                              adaptive sampling) in the place of reserved[0] -- size and offsets kept,
                              0 = the rule as it was;
                              still 9, additive: tmpt_scene_update (a device BVH refit, or a rebuild, of a
                              scene in place) and the read-only options update_kind, update_ms and
                              bvh_cost -- no struct above changed;
                              still 9, additive: the read-only option live_device_objects;
                              still 9, additive: temporal accumulation -- the render option sample_base,
                              tmpt_render_motion with tmpt_motion_pixel (the motion pass) and
                              tmpt_temporal with tmpt_temporal_desc (the reprojected history) -- no
                              struct above changed;
                              still 9, additive: tmpt_temporal_clip with tmpt_temporal_clip_desc (the
                              reprojected history clipped to the current frame's local statistics);
                              still 9, additive: the render options octree_build and octree_dev_max (the
                              reference's octree built on the device) and the check hooks
                              tmpt_scene_dump_octree and tmpt_octree_arrays, TMPT_FLAG_OCTREE_DEVICE for
                              tmpt_render_multi -- no struct above changed;
                              still 9, additive: history-guided sampling -- tmpt_sample_plan (the
                              accumulated moments reprojected into a per-pixel prior) and
                              tmpt_render_guided (tmpt_render_moments with that prior in its test);
                              still 9, additive: device-resident batched queries -- tmpt_scene_hit_device with
                              tmpt_hit_desc, the render options query_sort, query_top, query_max, query_chunk and
                              query_grid, and the check hooks tmpt_query_keys and tmpt_query_plan -- no struct
                              above changed */

typedef struct tmpt_scene tmpt_scene; /* opaque, device-resident */

/* Camera, field for field maths.h:106-111 */
typedef struct {
    float origin[3], lower_left[3], horizontal[3], vertical[3], u[3], v[3], w[3];
    float lens_radius;
} tmpt_camera;

/* RNG seeding of the xorshift32 stream (maths.cpp:5-13):
 *   ROW    the reference: seed y*9781+1 per row, threaded along the row
 *          (main.cpp:204) -- one lane per row
 *   PIXEL  seed (y*W+x)*9781+1 per pixel (0 remapped), its samples in sequence
 *   SAMPLE the pixel's seed as in PIXEL, sample s starting 2^16 * s steps into
 *          that stream (a GF(2) jump), so the samples of a pixel are
 *          independent work; the sum stays in sample order */
enum { TMPT_SEED_ROW = 0, TMPT_SEED_PIXEL = 1, TMPT_SEED_SAMPLE = 2 };

/* render engines */
enum {
    TMPT_ENGINE_WAVEFRONT = 0,  /* generate/extend/shade/shadow kernels over compacted queues */
    TMPT_ENGINE_MEGAKERNEL = 1, /* one lane per pixel (pixel mode) or per row (row mode) */
    TMPT_ENGINE_PERSISTENT = 2  /* pixel mode: one persistent kernel per frame, lanes own pixels and
                                   schedule extend / shadow / shade per wave (row mode: the speculative
                                   row engine -- every even RNG offset of a window traced, the chain
                                   walked through it; instrumented row renders: megakernel) */
};

/* render flags */
enum {
    TMPT_FLAG_OUT_DEVICE = 1,    /* rgba_out is a device pointer on the scene's device */
    TMPT_FLAG_COUNT_VISITS = 2,  /* instrumented traversal: node visits / triangle tests.  The
                                    persistent engine's instrumented kernels keep the lowest-index
                                    leaf: closest hits tied on t go to the lowest triangle index
                                    even with the octree built, so on a scene whose ties decide
                                    pixels the image is the one of tie_rule = index */
    TMPT_FLAG_WAIT_STREAM = 4,   /* the render starts after the work enqueued on desc->wait_stream */
    TMPT_FLAG_REQUIRE_RCCL = 8,  /* tmpt_render_multi: fail unless the gather runs over RCCL */
    TMPT_FLAG_OCTREE_DEVICE = 16 /* tmpt_render_multi: its scenes build their octree on the device (option
                                    octree_build = device); every other call refuses it as it did */
};

/* One render call = one shard of one frame (TraceImageBody over its rows,
 * main.cpp:180-246).  Rows are grouped in bands of band_rows rows; this call
 * renders the bands b with b % num_shards == shard, in increasing b, into a
 * compact tile of full-width rows (RGBA8, row 0 = the lowest rendered row,
 * as in the reference's in-memory image, main.cpp:229).  band_rows = 0 means
 * one band of the whole height. */
typedef struct {
    int32_t width, height, spp;
    int32_t seed_mode;  /* TMPT_SEED_ROW (main.cpp:204), TMPT_SEED_PIXEL or TMPT_SEED_SAMPLE */
    int32_t band_rows;
    int32_t shard, num_shards;
    int32_t engine;
    int32_t flags;
    /* Progressive spp (persistent engine, pixel or sample seeding): this call runs samples
     * [spp_begin, spp_begin + spp_count) of every pixel (spp_count 0 = to spp).
     * A call with spp_begin > 0 continues the per-pixel state (RNG, colour sum)
     * the previous call on this scene left for the same shard, so the passes
     * together equal one full render bit for bit; each pass writes a preview
     * (colour sum / samples so far, main.cpp:221-233 at that count) and the
     * pass that reaches spp writes the final image.  The continuation must use
     * the same camera, size, spp and shard as the pass before it (checked). */
    int32_t spp_begin, spp_count;
    int32_t reserved0;
    /* Stream ordering (TMPT_FLAG_WAIT_STREAM): a hipStream_t of the caller on
     * the scene's device (0 = its null stream).  The render's kernels run on
     * the scene's own non-blocking stream; with the flag they start only
     * after everything enqueued on wait_stream before the call -- e.g. a
     * collective still reading the device buffer a previous render wrote, or
     * the caller's fill of it.  The call returns once the render is complete
     * on the device, so work the caller enqueues afterwards sees the result. */
    uint64_t wait_stream;
    int32_t reserved[2];
} tmpt_render_desc;

/* Statistics of the last render on a scene (HIP-event timed on the scene's
 * stream, i.e. the stream the kernels are launched on). */
typedef struct {
    double render_ms;             /* first kernel to last kernel of the call */
    double extend_ms, shadow_ms;  /* summed closest-hit / any-hit kernel time (persistent engine:
                                     extend_ms = its k_path launches, both query kinds) */
    uint64_t extend_rays, shadow_rays;
    int64_t extend_launches, shadow_launches, iterations;
    uint64_t node_visits, tri_tests; /* extend (closest-hit) kernel, with TMPT_FLAG_COUNT_VISITS */
    uint64_t shadow_node_visits, shadow_tri_tests; /* shadow (any-hit) kernel, same flag */
    double build_ms;                 /* LBVH build of the scene */
    int32_t bvh_nodes, bvh_depth, n_tris, device;
    int32_t bvh4_nodes, bvh4_depth, leaf_max, builder_iters; /* 4-wide tree; PLOC passes (0 = LBVH) */
    /* the reference's octree (tmpt_scene_build_octree; 0 when none) */
    int32_t octree_nodes, octree_leaves;
    int64_t octree_refs;             /* triangle references in its leaves */
    double octree_build_ms;          /* the whole tmpt_scene_build_octree call, host or device build */
    /* the last render or HitScene call: closest-hit queries whose t two or more
     * triangles share, answered again in the octree's visit order; and queries
     * the reference's root box test rejected (answered as misses) */
    uint64_t tie_queries, root_misses;
    int32_t row_engine;       /* last render in row seeding: 0 none, 1 one lane per row (megakernel),
                                 2 iterated speculative engine, 3 streaming speculative engine */
    int32_t stream_fallbacks; /* 1: the streaming engine's launch aborted (no chain progress) and the
                                 frame was rendered again by the iterated engine */
    int32_t octree_depth;
    int32_t tie_rule;         /* in effect: 0 octree visit order, 1 lowest index (no octree / option) */
    int64_t chain_pixels;     /* pixel seeding: pixels the last render ran as speculative chains */
    int64_t redo_samples;     /* sample seeding, tie_defer: samples the last render traced again */
    int64_t redo_late;        /* of them, left to the second launch (the main launch's tail did not take them) */
    /* (ABI 8) closest-hit queries answered over the octree because they may run in one of its
     * cracks (a hit near an octree plane on a ray nearly parallel to it) or hit a triangle
     * lying flat on a plane (octree_flat of them in the scene); see tmpt_scene_build_octree */
    uint64_t crack_queries;
    int32_t octree_flat;
    int32_t redo_launches;    /* sample seeding, tie_defer: k_redo launches of the last render (0 or 1) */
    double redo_ms;           /* their time; extend_ms holds the main k_path launches only */
    uint64_t redo_rays;       /* their queries (part of the render's ray count) */
    /* (ABI 9) how the last render answered the queries the octree decides: 0 none (no octree,
     * tie_rule = index, or not a k_path render), 1 in the main loop (the wave's octree walk or
     * the serial walk), 2 deferred (tie_defer: dropped samples traced again in the launch's
     * tail), 3 deferral chosen but its list could not be allocated: answered in the main loop */
    int32_t tie_path;
    int32_t reserved_stats;
} tmpt_stats;

/* One pixel of the AOV pass (tmpt_render_aov), 32 B: the guide buffers of a
 * sample-seeded frame, from the camera rays that frame traces.  The camera ray
 * of sample s of pixel (x, y) is the one TraceImageBody forms (main.cpp:209-221)
 * from the sample's own RNG state, sample_seed(s, pixel_seed(x, y, width))
 * (TMPT_SEED_SAMPLE above); it is answered as HitScene answers the beauty
 * render's camera ray (main.cpp:91), and a hit takes Scatter's shadow query
 * and light term (main.cpp:53-72).  Every sum is float32, starts at 0.0f, is
 * taken in sample order s = 0 .. spp-1 (part of the contract, as the colour
 * sum's order is), a miss adding nothing, and is then multiplied by
 * spp_recip = 1.0f / (float)spp, as the colour is (main.cpp:188, 221-223). */
typedef struct {
    float    normal[3]; /* sum over the pixel's samples of the hit normal exactly as HitScene returns it
                           (geometric, not flipped towards the ray), times spp_recip */
    float    depth;     /* sum of the hit t, times spp_recip */
    float    direct;    /* sum of the first bounce's light scalar, times spp_recip: fmax(0, dot(kLightDir, nl))
                           (main.cpp:66-67) where it is > 0 and the shadow query (main.cpp:59) misses,
                           else nothing.  Times albedo * kLightColor this is bounce 0's outLightE (main.cpp:67) */
    int32_t  tri_id;    /* closest triangle of sample 0, or -1 */
    uint32_t hits;      /* samples whose camera ray hit (coverage = hits / spp) */
    uint32_t lit;       /* of them, those that added to `direct` */
} tmpt_aov_pixel;

/* tmpt_denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010)
 * over a float radiance frame (tmpt_render_radiance), guided by the frame's AOV
 * records (tmpt_render_aov): `direct` stops it at the hard shadow edges, `normal`
 * and `depth` at the geometry's.  The arithmetic below IS the contract, as the
 * renders' is: every operation is float32 and rounds once (no contraction into
 * fused multiply-adds, `/` and sqrtf correctly rounded), in the order written;
 * there is no exp or pow in it.  dot(a, b) = (ax*bx + ay*by) + az*bz.
 *
 * Guides, per pixel, once per call:
 *   cov = hits > 0
 *   nh  = normal * (1.0f / sqrtf(fmaxf(dot(normal, normal), 1e-30f)))   (each component times the scalar)
 *   zb  = depth * ((float)spp / (float)hits)      the mean hit t; formed and read only where cov
 *   dl  = direct
 * Level L = 0 .. levels-1, stride s = 1 << L; level 0 reads rgba32f_in, level L > 0
 * the output of level L-1.  For pixel p = (x, y), with h = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *   wsum = 0, csum = {0, 0, 0}
 *   for j = -2 .. 2 (outer), for i = -2 .. 2 (inner): the tap q = p + s * (i, j)
 *     q outside the frame: skipped;  cov_q != cov_p: skipped
 *     i == 0 and j == 0:  w = h[2] * h[2]
 *     else                w = h[i+2] * h[j+2], and if cov_p then, in this order,
 *       w = w * wn   c = fmaxf(0.0f, dot(nh_p, nh_q)), then normal_exp times c = c * c;  wn = c
 *       w = w * wz   wz = 1.0f / (1.0f + rz*rz),
 *                    rz = (zb_p - zb_q) / ((sigma_depth * fminf(zb_p, zb_q)) * (float)(s * max(|i|, |j|)))
 *       w = w * wd   wd = 1.0f / (1.0f + rd*rd),  rd = (dl_p - dl_q) / sigma_direct
 *     csum.k = csum.k + in_q.k * w   for k = r, g, b;   wsum = wsum + w
 *   out_p.k = csum.k / wsum,  out_p.w = in_p.w        (wsum >= 9/64: the centre tap always counts)
 * rgba32f_out = the last level's output; rgba8_out = its pixels packed as the renders
 * pack theirs (main.cpp:224-233): uint8(saturate(sqrtf(k)) * 255) per channel, alpha 255.
 * fmaxf / fminf return the other operand for a NaN; which NaN comes out of NaN inputs is
 * not specified.  Nothing screens the input: a radiance value that is not finite reaches
 * every pixel whose taps reach it, level after level.
 * The two sigma defaults were tuned by RMSE against 512-spp frames (DESIGN.md "Denoiser").
 *
 * The filter works on a WHOLE frame, width x height pixels with contiguous rows, row 0 at
 * the bottom: a caller who rendered banded shards assembles the frame (radiance and AOV
 * records alike, tmpt_tile_row_to_y) before the call. */
typedef struct {
    int32_t width, height, spp;   /* spp of the AOV records (for the mean depth) */
    int32_t levels;               /* 1..6, 0 = 5 */
    int32_t normal_exp;           /* squarings of the normal cosine, 0..8, -1 = 5 (c^32) */
    int32_t flags;                /* TMPT_FLAG_OUT_DEVICE: all four pointers are device pointers;
                                     TMPT_FLAG_WAIT_STREAM + wait_stream as in tmpt_render */
    float sigma_depth;            /* 0 = auto: 1.0f / (float)height */
    float sigma_direct;           /* 0 = 0.05f */
    uint64_t wait_stream;
    int32_t reserved[4];
} tmpt_denoise_desc;

/* ---- host side: scene ingest and camera (not kernels) ------------------- */

/* LoadScene (main.cpp:122-170) over objParseFile (objparser.cpp:304-355):
 * positions of every face, fan-triangulated, plus the 2 floor triangles.
 * *out_tris = n*9 floats (caller frees with tmpt_free); bounds are of the OBJ
 * triangles only (main.cpp:132-151).  Returns 0, or <0 if the file can't be read. */
int tmpt_load_obj(const char* path, float** out_tris, int32_t* out_n, float out_bmin[3],
                  float out_bmax[3]);
void tmpt_free(void* p);

/* Camera::Camera (maths.cpp:40-59) */
int tmpt_camera_init(tmpt_camera* cam, const float look_from[3], const float look_at[3],
                     const float vup[3], float vfov, float aspect, float aperture,
                     float focus_dist);
/* camera placement of main.cpp:295-307 (is_sponza: strstr(path,"sponza.obj")) */
int tmpt_camera_for_scene(tmpt_camera* cam, const float bmin[3], const float bmax[3],
                          int32_t width, int32_t height, int32_t is_sponza);

/* ---- device side --------------------------------------------------------- */

int tmpt_device_count(void);

/* Scene::Scene (scene.h:19, scene.cpp:54-57) + Scene::BuildOctree
 * (scene.h:26, scene.cpp:75-83): copies n triangles (n*9 floats, v0 v1 v2)
 * to `device` and builds the BVH there.  The caller keeps ownership of tris.
 * tmpt_scene_create = tmpt_scene_create_ex with no options. */
int tmpt_scene_create(const float* tris, int32_t n, int32_t device, tmpt_scene** out);

/* Scene options: the library's whole control plane (no environment variables;
 * the reference has no counterpart -- its constants are compiled in).  Every
 * option has a default that reproduces the measured-best configuration; all of
 * them change speed, never the image or the HitScene answers (tie_rule aside).
 * `options` = "key=value,key=value" (NULL or "" = defaults); an unknown key or
 * a value out of range is an error (-22).
 * Build options (only at creation):
 *   builder      ploc (0, default) | lbvh (1): PLOC (Meister & Bittner 2018) or
 *                Karras 2012 LBVH over the same 30-bit Morton order
 *   layout       aos (0, default) | soa (1): the sample-seeding path kernel and the
 *                batched HitScene also get the nodes and triangle records as
 *                planes (56 B / 40 B per node / triangle in 4 / 3 separate
 *                lines) -- the measured A/B of DESIGN.md section 3
 *   leaf_max     triangles per BVH4 leaf, 1..16 (default 2)
 *   collapse     greedy (0, default) | sah (1): BVH2 -> BVH4 collapse
 *   ploc_radius  PLOC search radius, 1..256 (default 32)
 *   sah_c_leaf, sah_c_tri  SAH collapse costs (defaults 0.7, 0.5; inner node 1)
 * Render options (tmpt_scene_set_option; apply to later renders on the scene):
 *   sample_base      sample seeding: an integer B, 0 .. 64512 (default 0).  Sample s of every
 *                    sample-seeded call on the scene (tmpt_render, tmpt_render_radiance,
 *                    tmpt_render_aov, tmpt_render_adaptive, tmpt_camera_rays) starts
 *                    2^16 (s + B) xorshift steps into the pixel's stream instead of 2^16 s:
 *                    a call at spp = n traces samples [B, B + n) of the stream, summed from
 *                    zero, so frame f of a sequence at B = f * spp draws numbers no earlier
 *                    frame drew (B + 1024 <= 65536 keeps the windows inside the period).
 *                    Host only: the jump tables hold J_(s + B).  A new value drops the tables
 *                    and invalidates the progressive state as a camera change does (a render
 *                    with spp_begin > 0 straight after fails with -22).  Row and pixel
 *                    seeding and tmpt_render_motion (which draws nothing) do not read it.
 *   sample_block    sample seeding: samples per work unit, power of two (0 = auto)
 *   sample_tail      sample seeding: the frame's last sample_tail x (resident lanes) blocks run
 *                    as single-sample units, so the frame ends on one sample, not one block
 *                    (-1 = auto: a quarter of a lane's samples, at most 64; 0 = off)
 *   sbuf_max         sample seeding: cap in bytes on the per-sample colour
 *                    buffer (0 = 3/4 of free HBM); over the cap a pixel is one unit
 *   sbuf_pair        sample seeding: a unit's samples 2k and 2k+1 written back to back into
 *                    one 32-B sector of the colour buffer (1) or each on its own (0)
 *   cam_pre          sample seeding, persistent engine at 5 waves per SIMD: the pass's camera
 *                    samples (ray and RNG state, a function of pixel and sample there) are made
 *                    by a pre-pass on full waves in every such render call, 32 B per sample in a
 *                    buffer the scene keeps, and the path kernel reads them (-1 = the measured
 *                    default: on; 0 = off; 1 = on).  Where the buffer does not fit -- over
 *                    cam_pre_max, over half of the device memory still free, or not
 *                    allocated -- the call runs the kernels that make their own camera samples;
 *                    the image, the ray counts and every statistic are the same either way
 *   cam_pre_max      cam_pre: cap in bytes on that buffer (0 = half of the free HBM alone)
 *   cam_rays_used    read-only (tmpt_scene_get_option): 1 if the last render ran the pre-pass
 *   shadow_split     sample seeding, where the pre-pass runs (cam_pre), a plain tmpt_render: the
 *                    path kernel queues every shadow query (16 B) instead of tracing it and
 *                    leaves a record per sample (64 B); a second kernel answers the queue, a
 *                    third runs the samples' backward recurrences and packs the pixels
 *                    (1 = the default, 0 = the fused kernel).  The fused kernel also runs where
 *                    a shadow answer can need the octree (a triangle flat on one of its planes),
 *                    in progressive and adaptive passes and tmpt_render_radiance, and where not
 *                    even one sample of every pixel fits; the image, the ray counts and every
 *                    statistic but the kernel times are the same either way (tmpt_stats:
 *                    extend_ms the path kernel's, shadow_ms and shadow_launches the queue kernel's)
 *   shadow_split_max shadow_split: cap in bytes on its queue and records, which are sized for
 *                    the worst case of 10 queries per sample (0 = half of the free HBM alone);
 *                    a render whose samples do not fit runs in several passes of samples
 *   shadow_split_pass  shadow_split: at most this many samples of every pixel per pass (0 = what fits)
 *   shadow_split_used  read-only: the passes of the last render that ran the split (0: fused)
 *   shadow_split_resolve_ms  read-only: the third kernel's time in the last render
 *   pilot            pixel seeding: pilot samples of the cost-ordered supply (-1 = auto, 0 = off)
 *   help, pair       pixel seeding: shadow offload to idle lanes (-1 = auto, 0, 1)
 *                    and expensive ranks per 64-rank chunk (-1 = auto, 0..63)
 *   balance, dprio   pixel seeding: SIMD-balanced first chunks (1), longest-
 *                    remaining-first wave priority in cost-ordered passes (1)
 *   wave_cap         pixel seeding: pixels a wave holds at once (0 = auto, 1..64)
 *   pixel_chains     pixel seeding, cost-ordered: the heaviest pixels per 1024 that run as
 *                    speculative chains (every even RNG offset past the pilot traced,
 *                    the chain walked through them) instead of in pass 2 (-1 = auto, 0 = off)
 *   rowspec          row seeding on the persistent engine: 1 = speculative row
 *                    engine, 0 = one lane per row chain
 *   rowspec_wmax, rowspec_windows, rowspec_spread, rowspec_groups,
 *   rowspec_noshadow, rowspec_chase, rowspec_stream, rowstream_dynamic
 *                    speculative row engine: units per window (0 = auto),
 *                    windows per row and iteration (0 = auto, 1..32), window
 *                    spread in pixels (-1 = auto), row groups/streams (1..8),
 *                    shadow-free speculation + one full re-trace (1), the
 *                    chase over LDS-staged units, one wave per row (1), the
 *                    streaming engine: one launch, chains walked on the device
 *                    as units finish (1, the default; 0 = host-driven iterations,
 *                    also the fallback when the streaming engine does not apply),
 *                    its windows and spread following the rows still chasing
 *                    (1; 0 = fixed at the launch's load)
 *   row_flag_leaves  row seeding, streaming, with the octree answering ties: the
 *                    leaves only flag a tie (1; 0 = lowest-index bookkeeping, A/B)
 *   row_occ          row seeding, streaming: worker waves per SIMD (0 = by load:
 *                    5 at full load, 4 with room; or 4, 5)
 *   rowstream_test_abort  test hook (0): 1 makes the streaming engine's chaser
 *                    blocks leave at once, so its watchdog (~2 ms then, ~1 s
 *                    normally) aborts the launch and the iterated engine renders
 *                    the frame -- the abort-and-fallback path, reported in
 *                    tmpt_stats.stream_fallbacks
 *   wf_bins          wavefront engine: each segment's extend queue split by the
 *                    rays' direction octant into 1, 2, 4 or 8 sub-queues (1)
 *   tie_rule         visit (0, default) | index (1): closest hits tied on t take the
 *                    reference's octree visit order (needs tmpt_scene_build_octree)
 *                    or the lowest triangle index -- the one option that can change
 *                    an answer, by design: index is the exact-semantics contract
 *   tie_defer        sample seeding with the colour buffer: a sample whose closest hit
 *                    is a tie is dropped by the main loop (built without the octree
 *                    walk) and traced again, ties settled, by the launch's waves once
 *                    their main loop is done (-1 = auto, 0 = off: ties settled in the
 *                    main loop, 1 = on); the image and ray counts are the same either way
 *   redo_lanes       tie_defer: lanes per wave that take the re-traces (1..64, default 4)
 *   path_waves       waves per SIMD of the persistent path kernels (0 = auto, 4, 5 or 6; 5: a 12-entry LDS
 *                    stack and 80 LDS top nodes, 30 KB of LDS per block and 96 VGPRs per lane; 6: the
 *                    shadow split's kernels only -- a 12-entry stack and 64 top nodes, 26 KB and 80 VGPRs
 *                    -- and what 5 runs wherever the split does not run: pixel and row seeding, a
 *                    progressive or adaptive pass, the float sums, shadow_split=0, cam_pre=0, a scene
 *                    whose shadow answers can need the octree).  Auto: 5 in sample seeding and the row
 *                    engine's re-trace -- 6 where the split runs with deferred ties (tie_defer) and the
 *                    pass has at least 150 samples per lane of the 5-wave grid --, 5 in pixel seeding
 *                    from 3 pixels per 4-wave lane.  The image and every count are the same for every
 *                    value
 *   path_waves_used  read-only: the waves per SIMD the last tmpt_render's path kernel ran at (4, 5 or
 *                    6; 0 where the row engines rendered)
 *   top_walk         persistent path kernels: at the end of a shading round, up to top_walk node
 *                    rounds for the lanes standing on a BVH node of the block's LDS copy of the top
 *                    levels (every query starts there), with no global load in them (-1 = the
 *                    seeding's measured default, 0 = off, 1..8 = the round cap); each lane's
 *                    traversal order, and so the image and every count, is the same for every value
 *   shadow_order     any-hit (shadow) queries, every engine: the order in which a BVH node's children
 *                    that the ray meets are visited (-1 = the measured default: 2, in row seeding 0; 0 = nearest entry
 *                    first, as closest-hit queries always go; 1 = longest overlap tf - tn first;
 *                    2 = largest exit distance first, by the key tn - 1024 tf); only the hit / miss
 *                    bit of such a query is used, so the image and the ray counts are the same for
 *                    every value, and closest-hit queries do not change at all
 *   pop_cull         closest-hit queries, every engine: a traversal stack entry carries, in the bits its
 *                    child link leaves free, the top bits of its child's entry distance (a lower bound);
 *                    an entry popped once the best hit is already nearer than that is discarded
 *                    unvisited and one more entry popped (-1 = the seeding's measured default: on in
 *                    every seeding mode and for the batched queries; 0 = off; 1 = on); the child's own box test would reject it, so every answer, tie flag, image
 *                    and ray count is the same for every value; only node_visits and tri_tests fall
 *   pop_key_bits     read-only (tmpt_scene_get_option): the width K of that key on this scene, 31 less
 *                    the bits of a child link (the record count's and leaf_max's widths), at most 16 and
 *                    at most pop_key_cap; 0, and nothing culled, where fewer than 9 would be left
 *   update_kind      read-only: the scene's last tmpt_scene_update -- 0 none since creation, 1 refit,
 *                    2 rebuild
 *   update_ms        read-only: the device time of that update, between two events on the scene's
 *                    stream (a refit: the upload through the last kernel)
 *   bvh_cost         read-only: the surface-area cost of the tree as it stands -- the sum over every
 *                    valid child slot of the decoded box's area x (1 for a node, the triangle count
 *                    for a leaf), over the area of the root's box (the union of the padded triangle
 *                    boxes), in float64 (tests/bvh_check.py cost()); computed on demand by a
 *                    reduction kernel and kept until the next update; 0 for the empty scene.  It
 *                    tells when a refitted tree has degraded enough to rebuild; the library applies
 *                    no policy of its own
 *   live_device_objects  read-only, of the process, not of the scene: the device allocations, pinned
 *                    allocations, events and streams the library holds at this moment, over every
 *                    scene and call (csrc/tmpt_device.h); it returns to its earlier value when a
 *                    scene is destroyed, and a call repeated with the same arguments does not move it
 *   pop_key_cap      test hook (-1 = no cap): at most this many key bits (0..16; 0..8 give no key)
 *   redo_cap        test hook (0 = auto): the capacity of tie_defer's sample list; a
 *                    frame that overflows it is rendered again with the list grown
 *   redo_inline      test hook (1): 0 leaves every dropped sample to the second launch
 *                    that otherwise takes only those the main launch's tail did not
 *   aov_group        tmpt_render_aov: lanes that share a pixel, each tracing every aov_group-th
 *                    sample (0 = auto: the largest of them that spp fills; or 1, 2, 4, 8, 16); the
 *                    records are the same for every value
 *   denoise_lds      tmpt_denoise: how a level reads its taps -- 1: the levels of stride 1 and 2 stage
 *                    their block's tile and halo (colour and guides) in LDS, the wider strides read
 *                    global memory directly; 0: every level reads directly; -1 (default): the measured
 *                    choice per stride; the output is the same for every value
 *   motion_tile      tmpt_render_motion: the 64 pixels a wave takes at a time -- 1: an 8 x 8 block,
 *                    0: 64 consecutive pixels of a row, -1 (default): the measured choice (the row); the
 *                    records are the same for every value
 *   query_sort       tmpt_scene_hit_device: 1 = the rays of a batch are traced in the order of a 24-bit key of
 *                    their origin's cell and direction (tmpt_query_keys states it), sorted on the device in
 *                    chunks of query_chunk rays; 0 = in the order given; -1 (default): the measured rule
 *                    ("Device-resident queries": off).  The answers are the same
 *                    for every value
 *   query_top        tmpt_scene_hit_device: 1 = the top levels of the BVH are read from an LDS copy, 0 = from
 *                    global memory, -1 (default): the measured choice.  The answers are the same for every value
 *   query_max        tmpt_scene_hit_device: cap in bytes on the scene's query scratch (overflow stacks, sort
 *                    buffers; kept by the scene between calls; 0 = half of the free device memory).  A call
 *                    whose scratch would pass it returns -12 with a message and changes nothing
 *   query_chunk      test hook (2^22): rays per sorted chunk, 64 .. 2^22
 *   query_grid       test hook (0 = the occupancy grid): cap on the blocks a query launch has
 *   query_legacy     tool hook (0): 1 = tmpt_scene_hit_device runs tmpt_scene_hit's kernel on the caller's
 *                    device data (d_hits required, d_uv must be NULL), for kernel-to-kernel timing
 *   query_ms, query_sort_ms, query_chunks, query_sorted
 *                    read-only, of the last tmpt_scene_hit_device: its device time between two events on the
 *                    scene's stream; the keys' and the sorts' share of it (timed on the first 32 chunks, their
 *                    mean taken for the rest); the chunks run (1 when unsorted); 1 if it sorted
 *   octree_build     tmpt_scene_build_octree: where the octree is built -- 0 or "host" (default): the
 *                    recursion on the host, uploaded; 1 or "device": a level-order build on the scene's
 *                    stream from the triangles the scene keeps on the device, nothing uploaded.  The
 *                    octree, its grid and the flat marks are the same word for word, and so are images,
 *                    hits, ray counts and every statistic but octree_build_ms
 *   octree_dev_max   octree_build=device: cap in bytes on the build's scratch (kept by the scene
 *                    between builds) plus its result (0 = half of the free device memory).  A build
 *                    that would pass it, or whose allocation fails, returns -12 with a message and
 *                    the scene keeps its previous octree, flat marks and statistics exactly */
int tmpt_scene_create_ex(const float* tris, int32_t n, int32_t device, const char* options, tmpt_scene** out);
int tmpt_scene_set_option(tmpt_scene* scene, const char* key, double value);
int tmpt_scene_get_option(const tmpt_scene* scene, const char* key, double* value);
/* Scene::BuildOctree (scene.h:26, scene.cpp:75-83; called by main.cpp:312
 * with the OBJ bounds +- 0.7 x their size): builds the reference's octree
 * (scene.cpp:99-160, host) over the scene's triangles and keeps it on the
 * device.  The BVH answers every query; the octree answers the kinds of
 * query where the reference's answer can differ from the BVH's closest hit: a
 * closest hit whose t two or more triangles share (the reference keeps the
 * first in its depth-first visit order, scene.cpp:29-48), a ray its root
 * box test rejects (scene.cpp:25), and a hit the reference's octree can miss
 * through a crack between neighbouring subtrees (their boxes' faces differ by
 * the rounding of min + half + half): a hit point near an octree plane on a
 * ray nearly parallel to that plane, or a triangle lying flat on one (stats
 * crack_queries, octree_flat).  Without it (or with option tie_rule = index)
 * ties go to the lowest triangle index and no ray is rejected.
 * Must not run while a render or HitScene call on the scene is in flight on
 * another host thread: it synchronises the scene's stream and frees the old
 * octree (a caller's wait_stream is not waited on). */
int tmpt_scene_build_octree(tmpt_scene* scene, const float bmin[3], const float bmax[3]);
/* The root box main.cpp:312 gives BuildOctree: sceneMin - extra, sceneMax + extra
 * with extra = (sceneMax - sceneMin) * 0.7 (main.cpp:296-297); bmin / bmax
 * are tmpt_load_obj's OBJ bounds.  box = {min.xyz, max.xyz}. */
int tmpt_octree_bounds(const float bmin[3], const float bmax[3], float box[6]);
/* Check hook (host only, no device): the octree tmpt_scene_build_octree would
 * build: out = {nodes, leaves, triangle references, depth, FNV-1a digest of
 * the preorder walk (box bits, leaf lists)}.  Tests compare it with the
 * oracle's octree. */
int tmpt_octree_digest(const float* tris, int32_t n, const float bmin[3], const float bmax[3], uint64_t out[5]);
/* Check hook: the octree a scene holds, as its kernels read it, copied to host memory.
 *   nodes  info[0] records of 8 words (32 B) in depth-first preorder: box min.xyz (f32 bits), [3] the
 *          skip link (the index of the node after this subtree), box max.xyz, [7] the offset of the
 *          leaf's list in refs, or -1 for an inner node
 *   refs   info[2] words: per leaf in preorder its count, then its triangle ids in the scene's order
 *   info   {nodes, leaves, reference words (counts included), depth, triangles marked flat}; all 0
 *          on a scene without an octree
 *   grid   (may be NULL) the 16 floats of the crack grid: reach, drift.xyz, r0.xyz, 1/cell.xyz,
 *          cell.xyz, band.xyz
 * nodes = refs = NULL: only info (and grid) are written (the sizes to allocate).  The call
 * synchronises the scene's stream and launches nothing.  -22 with a message, checked in this order
 * before any device call: a null scene, a null info, one buffer without the other, node_words below
 * 8 * nodes, ref_words below the reference words. */
int tmpt_scene_dump_octree(const tmpt_scene* scene, uint32_t* nodes, uint64_t node_words, uint32_t* refs,
                           uint64_t ref_words, int64_t info[5], float grid[16]);
/* Check hook (host only, no device): the same arrays for n triangles and a root box, made by
 *   method 0  the recursion tmpt_scene_build_octree runs under octree_build=host
 *   method 1  the passes of the device build (octree_build=device) run as host loops, one loop per
 *             kernel: level-order lists, counts, prefix sums, bottom-up sizes, top-down preorder
 *             indices
 * info[4] and grid come from the arrays by the scene's own rules; the two methods give the same
 * words.  nodes = refs = NULL: only info (and grid) are written.  -22 with a message, checked in
 * this order: n < 0, null tris with n > 0, a null bmin or bmax, a method other than 0 / 1, a null
 * info, one buffer without the other; then, once the sizes are known, node_words below 8 * nodes or
 * ref_words below the reference words; an octree past INT32_MAX nodes or reference words. */
int tmpt_octree_arrays(const float* tris, int32_t n, const float bmin[3], const float bmax[3], int32_t method,
                       uint32_t* nodes, uint64_t node_words, uint32_t* refs, uint64_t ref_words, int64_t info[5],
                       float grid[16]);
/* Check hook (host only, no device): which of n_rays answered queries the
 * octree re-answers besides ties -- rays n_rays x {o.xyz, d.xyz}, t and ids the
 * closest (or first) hit of each (ids < 0: a miss, never flagged):
 * flags[i] = 1 the hit triangle lies flat on an octree plane, | 2 the hit may
 * lie in a crack (the device's own octree_crack test).  grid (may be NULL) =
 * {r0.xyz, 1/cell.xyz, cell.xyz, band.xyz, reach} of that octree. */
int tmpt_octree_flags(const float* tris, int32_t n, const float bmin[3], const float bmax[3], const float* rays,
                      const float* t, const int32_t* ids, int64_t n_rays, uint8_t* flags, float grid[13]);
/* Scene::~Scene (scene.h:20) */
int tmpt_scene_destroy(tmpt_scene* scene);

/* Scene::HitScene (scene.h:36-37, scene.cpp:86-97), batched:
 * rays = n x {orig.xyz, dir.xyz} (dir normalised), hits = n x {pos.xyz,
 * normal.xyz, t} written where ids[i] >= 0; ids[i] = index of the closest
 * triangle or -1 (the reference returns 1 instead of the index).  any_hit != 0
 * stops at the first accepted triangle (the shadow query's semantics: only
 * ids[i] >= 0 is meaningful).  Host pointers.
 *
 * Domain.  "The closest triangle" is the linear scan over all triangles with
 * RayIntersectTriangleImproved (maths.cpp:339-380), lowest index on a tie.  The
 * answers equal it for ray origins within 100 scene diagonals of the scene's
 * box.  This does not hold for a scene one of whose extents is thousands of
 * times smaller than another (tests/geometry_cases.py `anisotropic`: 1e3 x 1
 * x 1e-3).  Cause: Moller-Trumbore's acceptance region widens with distance
 * (the error of u and v grows with |orig - v0|), the padded leaf box
 * (kBoxPadRel) does not, so from afar the scan accepts rays that miss the box.
 * Beyond the domain an answer is still sound: a returned triangle is one the
 * scan accepts, with its t bits, never nearer than the scan's; only hits can be
 * lost.  Rays of 40,000 (20,000 from a sphere, 20,000 from an axis, at that many
 * diagonals) whose answer differs from the scan's, oracle BVH / GPU:
 *                        10     100      1000         10000
 *   12 cases (below)    0 / 0   0 / 0   <= 2 / <= 5   <= 73 / <= 88
 *   anisotropic         0 / 0  95 / 87  2490 / 2438   6333 / 6307
 * (below: the other ten cases of tests/test_ray_cases.py, suzanne and teapot,
 * no octree; oracle BVH counts printed by
 * tests/test_ray_cases.py::test_domain_*, GPU counts by
 * tests/test_gpu_ray_cases.py::test_beyond_the_domain_is_sound and
 * ::test_obj_scenes_from_afar, seed 5; DESIGN.md section 2 has every row.) */
int tmpt_scene_hit(const tmpt_scene* scene, const float* rays, int64_t n, float tmin, float tmax,
                   int32_t any_hit, float* hits, int32_t* ids);
/* The same with the range per ray, as each HitScene call takes it
 * (scene.h:36-37: HitScene(ray, tMin, tMax, hit)): rays8 = n x {orig.xyz,
 * dir.xyz, tmin, tmax}.  t is accepted in [tmin, tmax]. */
int tmpt_scene_hit_ranged(const tmpt_scene* scene, const float* rays8, int64_t n, int32_t any_hit,
                          float* hits, int32_t* ids);

/* The same queries on data that lives on the device: nothing is uploaded, copied back or
 * allocated per call.  d_rays = n x 6 floats {orig.xyz, dir.xyz} with desc's one [tmin, tmax]
 * (ranged = 0), or n x 8 {orig.xyz, dir.xyz, tmin, tmax} (ranged = 1, desc's tmin / tmax not read).
 * All four pointers are device pointers on the scene's device, 4-byte aligned (a d_rays that is
 * 16-byte aligned takes the wider loads).
 *   d_ids[i]       as tmpt_scene_hit's ids[i]
 *   d_hits[7 i..]  as tmpt_scene_hit's hits, written only where d_ids[i] >= 0 and untouched elsewhere;
 *                  may be NULL: no hit record is formed
 *   d_uv[2 i..]    (may be NULL) Moller-Trumbore's (u, v) of the hit (maths.cpp:339-380; the record's
 *                  position is v0 (1 - u - v) + v1 u + v2 v), written where d_ids[i] >= 0, so a caller
 *                  can interpolate vertex attributes without intersecting again
 * The answers are tmpt_scene_hit's ray for ray and bit for bit -- closest ids, hit records, t bits;
 * with the octree its answers for ties, root misses, cracks and flat triangles -- whatever the
 * options query_sort, query_top, query_chunk and query_grid say, and the Domain paragraph above applies
 * unchanged.  any_hit: only the bit d_ids[i] >= 0 is specified, as there; in addition, where a hit is
 * reported, the record and (u, v) are those of triangle d_ids[i] for that ray.
 * The work runs on the scene's own stream, after the work enqueued on desc->wait_stream when
 * TMPT_FLAG_WAIT_STREAM is set, and the call returns when it is complete on the device, as the renders
 * do.  tmpt_get_stats afterwards reports tie_queries, root_misses and crack_queries as after
 * tmpt_scene_hit.  The scratch (overflow stacks; with query_sort the keys, the permutation and the
 * sort's buffers) belongs to the scene, grows on demand, is reused and is freed with the scene: the
 * option live_device_objects does not move when a call is repeated with the same arguments.  The
 * progressive state, the octree and every render buffer are left alone; like tmpt_render_aov the
 * call may run between two progressive passes.
 * -22 with a message, checked in this order before any device call: a null scene; a null desc;
 * n < 0; n > 0 with a null d_rays or d_ids; a flag other than TMPT_FLAG_WAIT_STREAM; ranged or
 * any_hit outside 0 / 1.  A non-finite tmin or tmax (ranged = 0) is accepted, as tmpt_scene_hit
 * accepts it: the range is compared as given (a NaN bound accepts no hit, tmax = +inf bounds nothing).
 * n = 0 returns 0 and launches nothing.  -12: the scratch does not fit (option query_max); the scene
 * is unchanged. */
typedef struct {
    int64_t  n;            /* rays */
    int32_t  ranged;       /* 0: rays n x 6 and one [tmin, tmax]; 1: rays n x 8, tmin / tmax not read */
    int32_t  any_hit;
    float    tmin, tmax;
    int32_t  flags;        /* TMPT_FLAG_WAIT_STREAM only; any other bit: -22 */
    int32_t  reserved0;
    uint64_t wait_stream;
    int32_t  reserved[4];
} tmpt_hit_desc;
int tmpt_scene_hit_device(tmpt_scene* scene, const tmpt_hit_desc* desc, const float* d_rays,
                          int32_t* d_ids, float* d_hits /* may be NULL */, float* d_uv /* may be NULL */);
/* Check hook (host only, no device): the sort key of option query_sort for n rays of `stride`
 * floats (6 or 8: {orig.xyz, dir.xyz[, tmin, tmax]}) and box = {min.xyz, max.xyz}, the root box of
 * the scene's BVH.  Every operation is float32 and rounds once; per axis a:
 *   inv[a] = 32.0f / fmaxf(box.max[a] - box.min[a], 1e-30f)
 *   c[a]   = (int)fminf(fmaxf((o[a] - box.min[a]) * inv[a], 0.0f), 31.0f)
 *   q[a]   = (int)fminf(fmaxf((d[a] + 1.0f) * 4.0f, 0.0f), 7.0f)
 *   key    = morton3(c.x, c.y, c.z) << 9 | q.x << 6 | q.y << 3 | q.z
 * (morton3 interleaves with x in the lowest bit of each triple: 24 bits in all); a ray with a NaN
 * anywhere in its origin or direction gets 0xFFFFFF and sorts last.  The device's key kernel
 * compiles the same function (csrc/tmpt_query_key.h).  -22 with a message, checked in this order:
 * n < 0; a null rays or keys with n > 0; a stride other than 6 or 8; a null box. */
int tmpt_query_keys(const float* rays, int64_t n, int32_t stride /* 6 or 8 */, const float box[6], uint32_t* keys);
/* Check hook (host only, no device): the sizes of one tmpt_scene_hit_device call of n rays -- sorted
 * (0 / 1), chunk = option query_chunk, grid_cap = option query_grid, resident = the blocks the device
 * holds at once: out = {chunks, rays per chunk, rays of the last chunk, blocks of the largest
 * launch, bytes of overflow stacks, bytes of sort buffers}.  -22: n < 0, sorted outside 0 / 1, a
 * chunk outside 64 .. 2^22, grid_cap < 0, resident < 1, a null out. */
int tmpt_query_plan(int64_t n, int32_t sorted, int64_t chunk, int64_t grid_cap, int64_t resident, int64_t out[6]);

/* tbb::parallel_for(rows, TraceImageBody) (main.cpp:329-331, 180-246):
 * renders desc's shard into rgba_out (tmpt_tile_rows(desc) * width * 4 bytes).
 * *ray_count = every HitScene call (main.cpp:57,91), counted in uint64. */
int tmpt_render(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                uint8_t* rgba_out, uint64_t* ray_count);
/* The AOV pass of desc's shard: one tmpt_aov_pixel per pixel into out
 * (tmpt_tile_rows(desc) * width records, the compact tile layout of
 * tmpt_render, row 0 = the lowest rendered row).  One closest-hit query per
 * sample and one shadow query per hit -- the primary rays of a
 * TMPT_SEED_SAMPLE render of the same desc, with its jitter, lens samples,
 * octree root test and tie rule, so the buffers line up with that frame.
 * Reads width, height, spp, band_rows, shard, num_shards, flags and
 * wait_stream (TMPT_FLAG_OUT_DEVICE: out is a device pointer, 16-byte aligned;
 * TMPT_FLAG_WAIT_STREAM as in tmpt_render); engine is not read.  -22 unless
 * seed_mode is TMPT_SEED_SAMPLE (the only seeding where the primary rays are
 * a function of pixel and sample), spp_begin and spp_count are 0,
 * TMPT_FLAG_COUNT_VISITS is clear and the sizes are within tmpt_render's
 * limits.  *ray_count = pixels * spp closest-hit queries + one shadow query
 * per hit (counted even where a zero cosine skips it, as main.cpp:57 counts).
 * tmpt_get_stats afterwards: render_ms, extend_ms, extend_rays, shadow_rays,
 * extend_launches = 1, tie_queries, root_misses, crack_queries.  The call
 * leaves the scene's progressive state alone: it may run between two passes
 * of a progressive render.  Render option aov_group sets the lanes per pixel. */
int tmpt_render_aov(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                    tmpt_aov_pixel* out, uint64_t* ray_count);
/* The float frame of a render: tmpt_render of the same desc, which also hands
 * out the linear radiance.  rgba32f_out (tmpt_tile_rows(desc) * width * 4
 * floats, the compact tile layout of tmpt_render): per pixel {r, g, b} = the
 * colour sum taken in sample order times spp_recip = 1.0f / (float)spp -- the
 * value of main.cpp:221, before the sqrtf of :224 -- and .w = 1.0f.
 * rgba8_out (may be NULL): exactly the bytes tmpt_render writes; they are also
 * what packing the float tile gives: uint8(saturate(sqrtf(k)) * 255), alpha 255.
 * The call traces the paths tmpt_render traces, with the same kernels but for
 * the stores of the float sums, so *ray_count and tmpt_get_stats are
 * tmpt_render's.  Persistent engine, TMPT_SEED_PIXEL or TMPT_SEED_SAMPLE, whole
 * renders only: -22 for TMPT_SEED_ROW, another engine, TMPT_FLAG_COUNT_VISITS or
 * spp_begin / spp_count other than 0.  TMPT_FLAG_OUT_DEVICE: both outputs are
 * device pointers (rgba32f_out 16-byte aligned); TMPT_FLAG_WAIT_STREAM as in
 * tmpt_render.  The call leaves the scene's progressive state alone, as
 * tmpt_render_aov does: it may run between two passes of a progressive render. */
int tmpt_render_radiance(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                         float* rgba32f_out, uint8_t* rgba8_out, uint64_t* ray_count);
/* Adaptive sampling: per-pixel sample counts by a variance test.  In sample
 * seeding sample s of a pixel is a function of the pixel and s alone, so a pixel
 * may stop at any count n and then holds exactly the pixel of an n-spp frame.
 * desc->spp is the cap S.  The arithmetic below IS the contract, as
 * tmpt_denoise's is: every operation is float32 and rounds once (no contraction
 * into fused multiply-adds, `/` correctly rounded), in the order written.
 *
 * Pass schedule: n_0 = spp_min, n_(k+1) = min(n_k + spp_step, S).  Pass 0 traces
 * samples [0, n_0) of every pixel of the tile, pass k+1 samples [n_k, n_(k+1)) of
 * the pixels still active after pass k.  The call ends when no pixel is active
 * or n_k = S.  A schedule of more than 64 passes is -22.
 * Per pixel, carried over the samples it has, in sample order, from 0.0f:
 *   sum.k = sum.k + c_s.k  for k = r, g, b; c_s = what Trace returned for sample s
 *   Y_s = (0.2126f * c_s.r + 0.7152f * c_s.g) + 0.0722f * c_s.b
 *   m1 = m1 + Y_s
 *   m2 = m2 + Y_s * Y_s
 * The test after a pass ending at n, for a pixel active through it (tau = threshold):
 *   fn   = (float)n
 *   mean = m1 / fn
 *   var  = fmaxf(0.0f, m2 / fn - mean * mean)
 *   se2  = var / (fn - 1.0f)
 *   lim  = (4.0f * (tau * tau)) * fmaxf(mean, 1.0f / 256.0f)
 *   the pixel stays active iff n < S and se2 > lim
 * To first order: the standard error of the packed value sqrtf(mean) exceeds tau,
 * in units of full scale.  fmaxf returns the other operand for a NaN and a NaN
 * compares false, so a pixel with a sample that is not finite stops at the count
 * where it appears; nothing is screened, as in tmpt_denoise.  With radius = 0 the
 * decision reads the pixel's own samples only (no neighbourhood rule), so shard
 * tiles assemble into the whole frame's outputs bit for bit, whatever band_rows.
 *
 * The neighbourhood rule, radius = r in 1 .. 8: only the stay-active rule changes;
 * the schedule, the sums, m1, m2 and the test's arithmetic do not.
 *   own_p  = the test above (n < S and se2 > lim), after the pass ending at n, for
 *            a pixel active through that pass; false for every pixel that was not
 *   N_r(p) = the pixels q with |q.x - p.x| <= r and |q.y - p.y| <= r (global
 *            rows), inside the frame and in p's band: q.y / band_rows ==
 *            p.y / band_rows (band_rows = 0: the whole height is one band);
 *            p itself is a member
 *   p stays active iff it was active through the pass, n < S, and own_q is true
 *   for some q in N_r(p).  A pixel that has stopped never resumes: its samples
 *   stay the prefix [0, n_p).
 * What follows from it:
 *   - per-count identity holds as before: a pixel that stopped at n is bit for
 *     bit the pixel of tmpt_render_radiance at spp = n, and n_p is one of the
 *     schedule's ends;
 *   - the neighbourhood is clipped to the band, so the tiles of any shard /
 *     num_shards with one band_rows assemble bit for bit into the num_shards = 1
 *     result with that band_rows.  The result now depends on band_rows (with
 *     1-row bands the reach is horizontal only); with radius = 0 it does not;
 *   - a pixel with a sample that is not finite no longer necessarily stops where
 *     that sample appears: its own test is false, but a neighbour can carry it
 *     on.  Nothing is screened, as before;
 *   - monotone in r: for r >= r' every pixel's count at r is >= its count at r'
 *     (own_p depends on p's samples alone; by induction over the passes).
 * Result, n_p the count at which the pixel stopped:
 *   rgba32f_out = {sum.rgb * (1.0f / (float)n_p), 1.0f}
 *   rgba8_out   = that pixel packed as every render packs its own (main.cpp:224-233)
 *   spp_out     = n_p
 * -- bit for bit the pixel of tmpt_render_radiance at spp = n_p. */
typedef struct {
    int32_t spp_min;    /* samples every pixel gets, 2 .. desc->spp; 0 = default: min(24, desc->spp) */
    int32_t spp_step;   /* samples a still-active pixel gets per further pass, >= 1; 0 = default: 8 */
    float   threshold;  /* tau >= 0 and finite; < 0 = default: 0.015f; NaN / inf: -22 */
    int32_t radius;     /* the neighbourhood rule's reach in pixels, 0 .. 8; 0 = none: the own test alone */
    int32_t reserved[4];
} tmpt_adaptive_desc;

typedef struct {
    int32_t  passes, reserved;
    uint64_t samples;          /* sum of n_p over the tile */
    int64_t  pass_pixels[64];  /* pixels pass k traced; 0 past the last pass */
} tmpt_adaptive_info;

/* The adaptive render of desc's shard (tmpt_adaptive_desc above; ad NULL = all
 * defaults).  The outputs use the compact tile layout of tmpt_render:
 * rgba32f_out tmpt_tile_rows(desc) * width * 4 floats, rgba8_out * 4 bytes,
 * spp_out one int32 per pixel.  Any of the three and info may be NULL; at
 * least one output is given.  TMPT_FLAG_OUT_DEVICE: all three are device
 * pointers (rgba32f_out 16-byte aligned, rgba8_out and spp_out 4-byte);
 * TMPT_FLAG_WAIT_STREAM as in tmpt_render.
 * *ray_count = every HitScene call of every traced sample.  tmpt_get_stats
 * afterwards: render_ms covers the whole call (the passes, the update, the
 * neighbourhood rule's and the compaction kernels, the host's wait after each
 * pass and the final kernel);
 * extend_ms, redo_ms, extend_rays, shadow_rays, extend_launches, redo_launches,
 * redo_samples, redo_late, redo_rays, tie_queries, root_misses and
 * crack_queries are summed over the passes; iterations = the passes;
 * tie_path is the first pass's.
 * TMPT_SEED_SAMPLE and the persistent engine only: -22 for another seeding or
 * engine, for spp_begin / spp_count other than 0, for TMPT_FLAG_COUNT_VISITS,
 * for spp_min outside 2 .. desc->spp (after the defaults), a negative
 * spp_step, a threshold that is NaN or infinite, a radius outside 0 .. 8, a
 * schedule of more than 64 passes, and a call without any output.  The call needs the per-sample colour buffer (16 B per
 * sample of the tile at the cap): -12 where that does not fit (render option
 * sbuf_max), as for a progressive pass.  It leaves the scene's progressive state
 * alone, as tmpt_render_aov does: it may run between two passes of a
 * progressive render.  Additive, the ABI version stays. */
int tmpt_render_adaptive(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                         const tmpt_adaptive_desc* ad, float* rgba32f_out, uint8_t* rgba8_out,
                         int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count);
/* The filter of tmpt_denoise_desc above, `levels` a-trous levels over the
 * whole frame: rgba32f_in and aov hold width * height pixels / records (the AOV
 * pass at desc->spp); rgba32f_out (may be NULL; may be rgba32f_in itself, else
 * must not overlap it) takes the filtered frame, rgba8_out (may be NULL) its
 * packed pixels; at least one of the two is given.  The scene supplies the
 * device, the stream, the workspace and the error channel -- no geometry is
 * read, and the progressive state is left alone.  Device pointers
 * (TMPT_FLAG_OUT_DEVICE) are 16-byte aligned (rgba8_out: 4).  -22 for a size
 * outside tmpt_render's limits, levels outside 0..6, normal_exp outside -1..8,
 * a negative or non-finite sigma, other flags, or a missing pointer.
 * tmpt_get_stats afterwards: render_ms is the filter's time on the device
 * (guide preparation and the levels); the other fields keep the last render's. */
int tmpt_denoise(tmpt_scene* scene, const tmpt_denoise_desc* desc, const float* rgba32f_in,
                 const tmpt_aov_pixel* aov, float* rgba32f_out, uint8_t* rgba8_out);

/* ---- The noise-aware filter: luminance moments and wavelet shrinkage.
 *
 * tmpt_render_moments is tmpt_render_adaptive with the same arguments, plus each
 * pixel's luminance moments.  Every output but moments_out, the ray count, info,
 * the statistics, the restrictions (sample seeding, the persistent engine,
 * spp_min >= 2, the per-sample colour buffer and its -12) and every rule of
 * tmpt_render_adaptive hold bit for bit: the radius rule, shards and bands, the
 * option sample_base, TMPT_FLAG_OUT_DEVICE, TMPT_FLAG_WAIT_STREAM.
 *   ad NULL  means the UNIFORM schedule spp_min = desc->spp: one pass, every pixel
 *            at n_p = desc->spp (so desc->spp >= 2).  It does NOT mean the
 *            adaptive defaults, as it does in tmpt_render_adaptive; pass a zeroed
 *            tmpt_adaptive_desc with threshold = -1 for those.
 *   moments_out  is required (-22 without it; the other three outputs may then
 *            all be NULL): 4 floats per pixel in the compact tile layout, 16-byte
 *            aligned where it is a device pointer.  With m1, m2 the sums stated
 *            above (carried in sample order over the pixel's n_p samples) and
 *            fn = (float)n_p:
 *              mom = { m1 / fn,  m2 / fn,  1.0f / fn,  1.0f }
 * A moments tile is a frame in the sense tmpt_temporal uses: its .w is a history
 * of length one.  Temporal use needs no call of its own: pass the moments frame
 * through tmpt_temporal exactly as the colour frame goes (as rgba32f_cur, the
 * previous accumulated moments as rgba32f_history), with the same motion records,
 * n_max and sigma_depth; the result is {mean mu1, mean mu2, mean 1/n, history
 * length} over the same taps.  rgba8_out of that call is meaningless and may be NULL.
 * Additive, the ABI version stays. */
int tmpt_render_moments(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                        const tmpt_adaptive_desc* ad, float* rgba32f_out, float* moments_out,
                        uint8_t* rgba8_out, int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count);

/* tmpt_denoise_moments: tmpt_denoise steered by a moments frame.  desc is read
 * exactly as tmpt_denoise reads it; moments holds width * height float4 (a whole
 * frame, like the other inputs: tmpt_render_moments' tiles assembled, or that
 * frame accumulated by tmpt_temporal).  shrink > 0; 0 selects the default, 2.0f;
 * negative, NaN or infinite is -22.  The validation order (shrink after the
 * sigmas, moments with the other pointers), the aliasing rule (rgba32f_out may be
 * rgba32f_in), the alignment of device pointers and the statistics are
 * tmpt_denoise's.
 *
 * The arithmetic IS the contract: float32, one rounding per operation, no
 * contraction, `/` correctly rounded, in the order written.  The guides, the 25
 * taps, their skip rules, their weights w (the centre's h[2]*h[2] included), csum
 * and wsum are tmpt_denoise's own (tmpt_denoise_desc above).  c_0 = rgba32f_in,
 * and c_(L+1) is that filter's level L over c_L: the bits tmpt_denoise produces.
 * Once per call, per pixel (mom = the pixel's moments):
 *   ne   = mom.w / mom.z                                  effective sample count
 *   v_0  = fmaxf(0.0f, mom.y - mom.x * mom.x) / fmaxf(ne - 1.0f, 1.0f)
 *                                                         variance of the pixel's mean luminance
 *   keep = {0, 0, 0}
 * Level L = 0 .. levels-1, stride s = 1 << L, pixel p:
 *   vsum = 0;  for every tap q that counts, in the taps' order:  vsum = vsum + v_L(q) * (w * w)
 *   v_(L+1)(p) = vsum / (wsum * wsum)
 *   gsum = 0, ksum = 0                                    a 3x3 Gaussian of v_L, distance 1 at every level
 *   for j = -1 .. 1 (outer), i = -1 .. 1 (inner): q = p + (i, j)
 *       skipped: q outside the frame;  cov_q != cov_p
 *       k = k3[i+1] * k3[j+1], k3 = {0.25f, 0.5f, 0.25f}
 *       gsum = gsum + v_L(q) * k;   ksum = ksum + k
 *   g    = gsum / ksum                                    ksum >= 0.25: the centre counts
 *   d.k  = c_L(p).k - c_(L+1)(p).k           k = r, g, b  the detail this level removed
 *   dY   = (0.2126f * d.r + 0.7152f * d.g) + 0.0722f * d.b
 *   e = dY * dY;   n = shrink * g
 *   gain = e > n ? (e - n) / e : 0.0f                     a NaN compares false
 *   keep.k = keep.k + d.k * gain
 * After the last level N = levels:
 *   out.k = c_N(p).k + keep.k;   out.w = in.w
 *   rgba8_out packs out as every render packs its pixels
 * In words: the filter runs as before, and at every level each pixel takes back
 * the part of its removed detail that the noise estimate cannot explain.  Nothing
 * is screened, as in tmpt_denoise; fmaxf returns the other operand for a NaN; sky
 * pixels follow the same statements with their plain weights.  What follows:
 *   - on a frame of positive finite values with v_0 > 0 everywhere and
 *     shrink = 3e38f every gain is 0: the output is tmpt_denoise's, bit for bit;
 *   - a pixel whose taps are all skipped but the centre has c_(L+1) = c_L, d = 0,
 *     and passes through.
 * The render option denoise_lds selects the staged or the direct kernels as for
 * tmpt_denoise; the output is the same for every value.  Additive, the ABI
 * version stays. */
int tmpt_denoise_moments(tmpt_scene* scene, const tmpt_denoise_desc* desc, float shrink,
                         const float* rgba32f_in, const tmpt_aov_pixel* aov, const float* moments,
                         float* rgba32f_out, uint8_t* rgba8_out);

/* ---- Temporal accumulation: the motion pass and the reprojected history.
 * Everything below is float32 arithmetic that rounds once per operation and is
 * not contracted; '/' and sqrtf are correctly rounded; operations happen in the
 * order written; dot(a, b) = (ax*bx + ay*by) + az*bz.  This statement is the
 * contract (tests/temporal_restate.py restates it in numpy).
 *
 * The motion record of one pixel: where the surface point its centre ray hits
 * was one frame ago.  A refit keeps triangle i in slot i (tmpt_scene_update), so
 * the hit's triangle id and barycentrics name the same material point in the
 * previous pose. */
typedef struct {          /* 32 B, two 16-byte stores */
    float    px, py;      /* where this pixel's surface point was in the previous frame, in continuous
                             pixel coordinates of the whole frame (pixel (x, y)'s centre is (x+0.5, y+0.5)) */
    float    depth;       /* t of this frame's centre ray */
    float    depth_prev;  /* distance of the previous point from the previous camera's origin */
    float    u, v;        /* barycentrics of the hit, the bits the triangle test returns */
    int32_t  tri_id;      /* closest triangle, or -1 */
    uint32_t flags;       /* 1 = hit, 2 = px, py, depth_prev are valid */
} tmpt_motion_pixel;
/* The motion pass of desc's shard (tmpt_tile_rows(desc) * width records, the
 * compact tile layout of tmpt_render; y below is the global row).  desc is read as
 * tmpt_render_aov reads it -- width, height, band_rows, shard, num_shards, flags
 * (TMPT_FLAG_OUT_DEVICE: out, and prev_tris if given, are device pointers, out
 * 16-byte aligned; TMPT_FLAG_WAIT_STREAM), wait_stream; spp, seed_mode and engine
 * are not read.
 *
 * Centre ray: one ray per pixel (x, y), no random draw, from the lens centre:
 *   s = ((float)x + 0.5f) * invW,  t = ((float)y + 0.5f) * invH
 *       (invW = 1.0f / (float)width, invH = 1.0f / (float)height)
 *   o = cam.origin
 *   d = normalize(((lower_left + s*horizontal) + t*vertical) - origin)
 * This is the camera's ray expression with the lens offset left out altogether
 * (not added as zero: o is origin itself and d has one subtraction).
 * The hit: the closest hit over [0.001, 1e7] as tmpt_scene_hit answers it, with
 * the scene's tie rule and, where the octree is built, its root test.  A miss
 * writes tri_id = -1, flags = 0 and zeros elsewhere; a hit writes depth = t, u,
 * v, tri_id and flags |= 1.
 * Previous position: (v0', v1', v2') = triangle tri_id of prev_tris (prev_n x 9
 * floats; prev_n must be the scene's n); prev_tris NULL = the geometry did not
 * move: prev_n is ignored and the scene's own vertices are used.
 *   P' = (((1.0f - u) - v) * v0' + u * v1') + v * v2'       (componentwise)
 * A host prev_tris is uploaded into a buffer the scene keeps (grown, never shrunk).
 * Projection through prev_cam (fields o, ll, hz, vt, w), a pinhole: the lens is
 * ignored, so a defocused camera reprojects its plane of focus exactly and
 * everything else to the centre of its blur:
 *   dd  = P' - o            q = ll - o            (componentwise)
 *   den = dot(dd, w)        num = dot(q, w)
 *   valid iff den < 0.0f    (in front of the camera; a NaN is not valid)
 *   k   = num / den         r = k*dd - q          (r.c = k*dd.c - q.c)
 *   px  = (dot(r, hz) / dot(hz, hz)) * (float)width
 *   py  = (dot(r, vt) / dot(vt, vt)) * (float)height
 *   depth_prev = sqrtf(dot(dd, dd))
 * Valid: flags |= 2.  Not valid: px = py = depth_prev = 0.
 *
 * -22 with a message, before any device call and in this order: a null cam,
 * prev_cam, desc or out; a size outside tmpt_render's limits; an invalid shard;
 * TMPT_FLAG_COUNT_VISITS; a misaligned device out; a null scene; prev_n != n where
 * prev_tris is given (the scene is looked at last, so the checks before it need no
 * device).  *ray_count (may be NULL) = the pixels of the tile.  tmpt_get_stats
 * afterwards as after the AOV pass: render_ms, extend_ms, extend_rays,
 * extend_launches = 1, tie_queries, root_misses, crack_queries.  The progressive
 * state is left alone, and option sample_base is not read. */
int tmpt_render_motion(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_camera* prev_cam,
                       const float* prev_tris, int32_t prev_n, const tmpt_render_desc* desc,
                       tmpt_motion_pixel* out, uint64_t* ray_count);

typedef struct {
    int32_t width, height;
    int32_t flags;          /* TMPT_FLAG_OUT_DEVICE (every pointer a device pointer), TMPT_FLAG_WAIT_STREAM */
    float   n_max;          /* cap on the history length, >= 1; 0 = default (3) */
    float   sigma_depth;    /* relative depth tolerance, > 0; 0 = default (0.05) */
    int32_t reserved0;
    uint64_t wait_stream;
    int32_t reserved[4];
} tmpt_temporal_desc;
/* One step of temporal accumulation over whole frames (width x height, contiguous
 * rows, row 0 at the bottom, as tmpt_denoise): the current radiance frame blended
 * with the previous accumulation, fetched where motion says each pixel's surface
 * was and accepted where prev_motion (the previous frame's motion records) shows
 * the same depth there.  A frame's .w is its history length: tmpt_render_radiance
 * writes 1.0f, so a plain radiance frame is a history of length one, and
 * tmpt_denoise passes .w through.  rgba32f_out (may be NULL) may be rgba32f_cur;
 * it must not overlap rgba32f_history, whose neighbours are read.  rgba8_out (may
 * be NULL) takes the packed pixels; at least one output is given.
 *
 * Per pixel p = (x, y), with m = motion[p]:
 *   reset:  out_p = {cur_p.r, cur_p.g, cur_p.b, 1.0f}
 *   if !(m.flags & 2), or m.px / m.py is not finite or lies outside
 *      [-1, width+1) / [-1, height+1): reset
 *   fx = m.px - 0.5f   fy = m.py - 0.5f   x0 = floorf(fx)   y0 = floorf(fy)
 *   ax = fx - x0       ay = fy - y0
 *   csum = {0,0,0}  nsum = 0  wsum = 0
 *   for j = 0, 1 (outer), i = 0, 1 (inner): q = ((int)x0 + i, (int)y0 + j)
 *       wgt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay)
 *       skipped: q outside the frame;  !(prev_motion[q].flags & 1);
 *                fabsf(prev_motion[q].depth - m.depth_prev) > sigma_depth * m.depth_prev
 *                (a NaN compares false: not skipped)
 *       csum.k = csum.k + hist_q.k * wgt  (k = r, g, b)
 *       nsum = nsum + hist_q.w * wgt      wsum = wsum + wgt
 *   if !(wsum > 0.0f): reset
 *   h.k = csum.k / wsum    n = fminf(nsum / wsum + 1.0f, n_max)    a = 1.0f / n
 *   out_p.k = h.k + (cur_p.k - h.k) * a      out_p.w = n
 * rgba8_out packs out as every render packs its pixels (sqrt, saturate, * 255).
 * Nothing is screened (a NaN in an input spreads to the pixels that read it), as in
 * tmpt_denoise.  Sky pixels (misses) restart every frame.
 * Defaults n_max = 3, sigma_depth = 0.05 (tools/temporal_sweep.py,
 * profiles/temporal_sweep.log, DESIGN.md "Temporal accumulation": over twisting
 * and static sequences at 4 spp a frame, 3 is the cap whose worst sequence is best
 * -- the shading of a moving surface changes under the fixed light, and a longer
 * mean lags behind it; a static view gains up to n_max = 16 and beyond, so raise it
 * where little moves.  sigma_depth 0.02 .. 0.2 measured within 0.3 % of one another).
 * The scene lends its device, stream and error channel; no geometry is read and
 * the progressive state is left alone.  -22, in this order, for: a null desc; a
 * size outside tmpt_render's limits; a missing pointer (cur, motion, prev_motion,
 * history, or both outputs); n_max < 1 (after the default) or not finite; a
 * negative or non-finite sigma_depth; other flags; a misaligned device pointer (16
 * bytes; rgba8_out: 4); rgba32f_out overlapping rgba32f_history; a null scene.  tmpt_get_stats
 * afterwards: render_ms is the blend's time on the device; the other fields keep
 * the last render's. */
int tmpt_temporal(tmpt_scene* scene, const tmpt_temporal_desc* desc, const float* rgba32f_cur,
                  const tmpt_motion_pixel* motion, const tmpt_motion_pixel* prev_motion,
                  const float* rgba32f_history, float* rgba32f_out, uint8_t* rgba8_out);

typedef struct {
    int32_t width, height;
    int32_t flags;          /* TMPT_FLAG_OUT_DEVICE (every pointer a device pointer), TMPT_FLAG_WAIT_STREAM */
    float   n_max;          /* cap on the history length, >= 1; 0 = default (3) */
    float   sigma_depth;    /* relative depth tolerance, > 0; 0 = default (0.05, tmpt_temporal's) */
    float   gamma;          /* box half-width in window standard deviations, > 0; 0 = default (0.5) */
    int32_t radius;         /* window radius 1..3; 0 = default (1) */
    int32_t reserved0;
    uint64_t wait_stream;
    int32_t reserved[4];
} tmpt_temporal_clip_desc;
/* tmpt_temporal with history clipping (variance clipping): the reprojected
 * history value is pulled into the box mean +- gamma * sigma of the current
 * frame's neighbourhood before it is blended, and a history that had to be pulled
 * far loses its length.  The window's sigma contains the frame's noise, so the box
 * is wide where the frame is noisy and tight where it is not.  Frames, rows, the
 * motion records and a frame's .w are tmpt_temporal's.
 *   rgba32f_stat  the frame the window statistics are taken from (for instance
 *                 rgba32f_cur through tmpt_denoise); NULL = rgba32f_cur
 *   aux_cur, aux_history, aux_out  all three or none: a second frame (for instance
 *                 the moments frame of tmpt_render_moments) accumulated over the
 *                 same taps with the same blend factor, and not clipped, so that
 *                 it stays consistent with the clipped colour frame and
 *                 tmpt_denoise_moments can follow
 * rgba32f_out (may be NULL) and rgba8_out (may be NULL; at least one of the two is
 * given) as in tmpt_temporal, with one difference: rgba32f_out and aux_out must
 * overlap none of rgba32f_history, aux_history, rgba32f_cur and rgba32f_stat --
 * here the current frame's neighbours are read too, across blocks, so out may NOT
 * be cur.  (aux_out may be aux_cur: that frame is read at the pixel itself only.)
 *
 * The arithmetic is the contract, under the rules stated above tmpt_motion_pixel
 * (tests/temporal_clip_restate.py restates it in numpy).  fmaxf / fminf return the
 * other operand for a NaN; nothing is screened.  Per pixel p = (x, y), with
 * m = motion[p], S = rgba32f_stat or, when NULL, rgba32f_cur, r = radius:
 *   fetch:  the reset rule, the validity of m.px / m.py, fx .. ay, the four taps,
 *           their skip rules, wgt, csum, nsum and wsum are tmpt_temporal's
 *           statements above, word for word; with aux, on the taps that count,
 *           asum.k = asum.k + aux_history_q.k * wgt  (k = x, y, z; asum = {0,0,0})
 *   reset:  out_p = {cur_p.r, cur_p.g, cur_p.b, 1.0f}
 *           aux_out_p = {aux_cur_p.x, aux_cur_p.y, aux_cur_p.z, 1.0f}
 *   h.k = csum.k / wsum     nh = nsum / wsum     ha.k = asum.k / wsum
 *   window: s1 = s2 = {0,0,0}  cnt = 0
 *     for j = -r .. r (outer), i = -r .. r (inner): q = p + (i, j)
 *         skipped: q outside the frame;
 *                  (motion[q].flags & 1) != (m.flags & 1)   (coverage, as tmpt_denoise's cov_q != cov_p)
 *         s1.k = s1.k + S_q.k     s2.k = s2.k + S_q.k * S_q.k     cnt = cnt + 1.0f
 *     (the centre always counts; the sums run over the window in exactly this
 *     order, rows outer, not separably)
 *   box:    mu.k = s1.k / cnt
 *           var.k = fmaxf(0.0f, s2.k / cnt - mu.k * mu.k)     sd.k = sqrtf(var.k)
 *           g.k = gamma * sd.k     lo.k = mu.k - g.k     hi.k = mu.k + g.k
 *   clip:   hc.k = fminf(fmaxf(h.k, lo.k), hi.k)
 *           e    = fmaxf(fmaxf(fabsf(h.r - hc.r), fabsf(h.g - hc.g)), fabsf(h.b - hc.b))
 *           span = fmaxf(fmaxf(g.r, g.g), g.b)
 *   length: nh' = e > 0.0f ? nh * (span / (span + e)) : nh      (a NaN compares false)
 *   blend:  n = fminf(nh' + 1.0f, n_max)     a = 1.0f / n
 *           out_p.k = hc.k + (cur_p.k - hc.k) * a          out_p.w = n
 *           aux_out_p.k = ha.k + (aux_cur_p.k - ha.k) * a   aux_out_p.w = n
 * rgba8_out packs out as every render packs its pixels.  What follows:
 *   - where no history value leaves its box -- with gamma = 3e38f that is every
 *     pixel whose window has sd.k > 0 for all k (3e38f * sd.k is then far beyond
 *     any radiance, or +inf) -- hc = h, e = 0, and out is tmpt_temporal's output
 *     bit for bit at the same n_max and sigma_depth;
 *   - a window that is the centre alone (a 1 x 1 frame, an isolated covered pixel)
 *     has mu = S_p and sd = 0, so hc = S_p whatever gamma is (S_p not a NaN), and
 *     a history that differed from S_p restarts: span = 0, nh' = 0, n = 1.
 * Defaults n_max = 3, gamma = 0.5, radius = 1: the grid point of
 * tools/temporal_clip_sweep.py (profiles/temporal_clip_sweep.log, DESIGN.md
 * "History clipping") whose worst sequence is best; sigma_depth as tmpt_temporal.
 * The scene lends its device, stream and error channel; the progressive state is
 * left alone.  Host pointers are staged through one buffer the scene keeps (grown,
 * never shrunk).  -22, in tmpt_temporal's order, for: a null desc; a size outside
 * tmpt_render's limits; a missing pointer (cur, motion, prev_motion, history, an
 * aux triple given in part, or both outputs); n_max < 1 (after the default) or not
 * finite; a negative or non-finite sigma_depth; a negative or non-finite gamma; a
 * radius outside 0..3; other flags; a misaligned device pointer (16 bytes;
 * rgba8_out: 4); an output overlapping a frame named above; a null scene.
 * tmpt_get_stats afterwards: render_ms is the kernel's time on the device; the
 * other fields keep the last render's.  Additive, the ABI version stays. */
int tmpt_temporal_clip(tmpt_scene* scene, const tmpt_temporal_clip_desc* desc, const float* rgba32f_cur,
                       const float* rgba32f_stat, const tmpt_motion_pixel* motion,
                       const tmpt_motion_pixel* prev_motion, const float* rgba32f_history, const float* aux_cur,
                       const float* aux_history, float* aux_out, float* rgba32f_out, uint8_t* rgba8_out);

/* ---- History-guided sampling: a sample plan and a guided adaptive render.
 *
 * tmpt_sample_plan reprojects the accumulated moments frame (the aux frame of
 * tmpt_temporal_clip, or a moments frame through tmpt_temporal: {mean mu1, mean
 * mu2, mean 1/n, history length}) into a per-pixel prior for this frame;
 * tmpt_render_guided is tmpt_render_moments whose stopping test judges the
 * variance of the frame AS IT WILL BE AFTER THE BLEND, not of the raw frame.  A
 * pixel with a long, quiet history stops at spp_min = 2; a pixel with no history
 * keeps the plain test and runs to the cap.
 *
 * Frames, row order, flags, defaults and the -22 order are tmpt_temporal's, with
 * its colour frames left out; desc supplies n_max and sigma_depth with the same
 * defaults.  prior_out is width * height float4, 16-byte aligned where it is a
 * device pointer; it must not overlap moments_history, whose neighbours are read.
 *
 * The arithmetic is the contract, under the rules stated above tmpt_motion_pixel
 * (tests/guided_restate.py restates it in numpy).  fmaxf / fminf return the other
 * operand for a NaN.  Per pixel p = (x, y), with m = motion[p]:
 *   fetch:  the reset rule, the validity of m.px / m.py, fx .. ay, the four taps,
 *           their skip rules, wgt, nsum and wsum are tmpt_temporal's statements
 *           above, word for word, with hist = moments_history; on the taps that
 *           count,  asum.k = asum.k + hist_q.k * wgt  (k = x, y, z; asum = {0,0,0})
 *   reset:  prior_p = {0.0f, 0.0f, 1.0f, 0.0f}            -- the null prior
 *   history statistics:
 *           hY = asum.x / wsum    h2 = asum.y / wsum    hz = asum.z / wsum
 *           nh = nsum / wsum
 *           ne = nh / hz                     the effective sample count, as
 *                                            tmpt_denoise_moments forms mom.w / mom.z
 *           vh = fmaxf(0.0f, h2 - hY * hY) / fmaxf(ne - 1.0f, 1.0f)
 *   blend weights:
 *           n = fminf(nh + 1.0f, n_max)      a = 1.0f / n      b = 1.0f - a
 *   result: prior_p = {hY, (b * b) * vh, a, nh}
 * Nothing is screened.  In words, the prior holds the luminance the history will
 * contribute, the share of the blended pixel's variance that the history brings,
 * the blend factor tmpt_temporal will use for this frame at the same n_max, and
 * the history length.  (tmpt_temporal_clip may shorten a history after the plan
 * was made; the plan does not anticipate that.)
 * The scene lends its device, stream and error channel; no geometry is read and
 * the progressive state is left alone.  Host pointers are staged through the
 * buffer tmpt_temporal_clip keeps.  -22, in this order, for: a null desc; a size
 * outside tmpt_render's limits; a missing pointer; n_max < 1 (after the default)
 * or not finite; a negative or non-finite sigma_depth; other flags; a misaligned
 * device pointer (16 bytes); prior_out overlapping moments_history; a null scene.
 * tmpt_get_stats afterwards: render_ms is the kernel's time on the device; the
 * other fields keep the last render's.  Additive, the ABI version stays. */
int tmpt_sample_plan(tmpt_scene* scene, const tmpt_temporal_desc* desc, const tmpt_motion_pixel* motion,
                     const tmpt_motion_pixel* prev_motion, const float* moments_history, float* prior_out);

/* tmpt_render_guided is tmpt_render_moments in every rule, with these differences:
 *   moments_out  may be NULL; at least one of the four outputs must be given
 *                (-22 otherwise).  ad NULL means the uniform schedule, as in
 *                tmpt_render_moments.
 *   prior        tmpt_tile_rows(desc) * width float4 in the COMPACT TILE LAYOUT of
 *                the shard (tile row t holds the prior of global row
 *                tmpt_tile_row_to_y(desc, t)).  It follows the outputs' flag: a
 *                device pointer under TMPT_FLAG_OUT_DEVICE, 16-byte aligned (-22
 *                otherwise).  NULL means the null prior everywhere.
 * Only the own test changes.  After a pass ending at n, with mean, se2 and
 * lim4 = 4.0f * (tau * tau) as tmpt_adaptive_desc states them and pr = prior[p]:
 *   se2b  = pr.y + (pr.z * pr.z) * se2
 *   meanb = pr.x + (mean - pr.x) * pr.z
 *   lim   = lim4 * fmaxf(meanb, 1.0f / 256.0f)
 *   own_p = n < S and se2b > lim
 * The schedule, the sums, m1, m2, the radius rule over own, the bands,
 * sample_base, the outputs, info, the ray count and the statistics are unchanged.
 * With the null prior {0, 0, 1, 0}, se2b = se2 and meanb = mean exactly for every
 * finite mean and every non-negative, infinite or NaN se2.  The call is then
 * tmpt_render_moments bit for bit.
 * Per-count identity still holds: a pixel that stopped at n is
 * tmpt_render_radiance's pixel at spp = n.  Shard tiles still assemble, for the
 * same reason as before: the prior is read at the pixel itself.  Additive, the
 * ABI version stays. */
int tmpt_render_guided(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc,
                       const tmpt_adaptive_desc* ad, const float* prior, float* rgba32f_out, float* moments_out,
                       uint8_t* rgba8_out, int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count);

/* main.cpp:312-331 over several devices in ONE process (SURVEY.md §8e's
 * single-process form): a scene per entry of devices[] (created here, freed on
 * return), the frame's rows dealt round-robin to them (1-row bands), one host
 * thread per device rendering into a device tile, then ONE RCCL gather
 * (ncclCommInitAll over devices[], ncclGather of the equal-size tiles to
 * devices[0] over xGMI, ncclReduce of the uint64 ray counts) and the rows
 * de-interleaved on devices[0] into rgba_full (width*height*4, row 0 =
 * bottom, as tmpt_render).  RCCL ranks need distinct devices: with a device
 * listed twice the gather is device-to-device copies instead (or an error
 * with TMPT_FLAG_REQUIRE_RCCL in desc->flags).  desc's band_rows, shard and
 * num_shards are taken over; *seconds = wall time from the renders' start to
 * the assembled frame on devices[0] (scene builds excluded, main.cpp:319-333);
 * *ray_count = all devices' rays.  The one-process-per-GPU form is bench.py
 * (torch.distributed + RCCL).  octree_box: each device's scene also builds the
 * reference's octree over it (tmpt_scene_build_octree), as main.cpp:312 does. */
int tmpt_render_multi(const float* tris, int32_t n, const float* octree_box /* bmin[3], bmax[3] or NULL */,
                      const tmpt_camera* cam, const tmpt_render_desc* desc, const int32_t* devices,
                      int32_t ndevices, uint8_t* rgba_full, uint64_t* ray_count, double* seconds);

/* rows in the tile of desc's shard; global row of tile row r */
int32_t tmpt_tile_rows(const tmpt_render_desc* desc);
int32_t tmpt_tile_row_to_y(const tmpt_render_desc* desc, int32_t r);

int tmpt_get_stats(const tmpt_scene* scene, tmpt_stats* out);

/* PNG writer (stbi_write_png with flip-on-write, main.cpp:341-342):
 * rgba rows bottom-up as rendered. */
int tmpt_write_png(const char* path, const uint8_t* rgba, int32_t width, int32_t height);

/* RandomUnitVector's (cos a, sin a) (maths.cpp:33-36: a = ((k / 2^24) * 2) * kPI,
 * then libm cosf/sinf) for the RNG keys [key0, key0 + n): out = n x {cos, sin}
 * (host memory).  device >= 0: computed by the device code the renderers run;
 * device < 0: the same restatement on the host.  A check hook -- the
 * reference has no counterpart; tests compare it with the host libm. */
int tmpt_unit_sincos(int32_t device, uint32_t key0, uint32_t n, float* out);

/* The multiply-shift divider the path kernel divides by the frame's width and
 * a unit's block counts with (exact for dividends below 2^31): out[i] = x[i] /
 * divisor for the n dividends x (host memory), by the host's statement of the
 * device's expression; mul_shift (may be null) receives the pair.  A check
 * hook like the one above: tests compare it with integer division.  Additive,
 * the ABI version stays. */
int tmpt_fastdiv(uint32_t divisor, const uint32_t* x, uint64_t n, uint32_t* out, uint32_t mul_shift[2]);

/* Check hook: the camera pre-pass of sample seeding (render option cam_pre) run
 * alone, its entries copied to host memory.  Reads desc's width, height, spp,
 * spp_begin / spp_count (the pass, as tmpt_render takes them), band_rows, shard
 * and num_shards; seed_mode, engine and flags are not read.  out holds
 * tmpt_tile_rows(desc) * width * count entries of 8 uint32 words, count the
 * samples of the pass, entry (slot, sample) at slot * count + (sample -
 * spp_begin), slot the pixel's index in the compact tile layout of tmpt_render:
 *   [0..2] the ray's origin, [3..5] its direction (f32 bits): Camera::GetRay of
 *          main.cpp:212-216 for that pixel, from the state sample seeding gives
 *          the sample (the pixel's seed jumped to the sample)
 *   [6]    the RNG state after the camera's draws (two for the jitter, two per
 *          try of the lens disk)
 *   [7]    flags: 1 the ray holds a NaN, else 2 it misses the reference's root
 *          box (set only where the render would make that test: the octree
 *          built, tie_rule visit, the lens not wholly inside the box)
 * The scene's statistics and progressive state are left alone.  -22 for sizes
 * outside tmpt_render's limits, -12 when the entries do not fit on the device.
 * Additive, the ABI version stays. */
int tmpt_camera_rays(tmpt_scene* scene, const tmpt_camera* cam, const tmpt_render_desc* desc, uint32_t* out);

/* Check hook: the BVH a scene holds, as its kernels read it, copied to host
 * memory.  The scene's stream is synchronised first; no kernel is launched and
 * nothing of the scene changes.
 *   nodes  n_nodes4 records of 16 uint32 words (64 B):
 *          [0..2]  origin.xyz, the f32 bits of the node box's minimum
 *          [3]     bytes 0..2 the signed exponents ex, ey, ez (scale = 2^e per axis), byte 3 the
 *                  child-valid mask
 *          [4..9]  qlo.x, qhi.x, qlo.y, qhi.y, qlo.z, qhi.z: child k's 8-bit plane in byte k of each;
 *                  the child box is origin + q * 2^e, in exact arithmetic
 *          [10,11] 0
 *          [12..15] child links: an internal child is its node index; a leaf is
 *                  bit 31 | (count - 1) << count_shift | first record
 *   tris   n + 1 records of 12 words (48 B), in leaf order: v0.xyz, e1 = v1 - v0, e2 = v2 - v0 (f32 bits),
 *          [9] = 2 x the triangle's index | the flat mark (tmpt_scene_build_octree), [10,11] = 0
 *   info   {n, n_nodes4, depth4, leaf_max, count_shift, link_bits, builder_iters, 1 if the scene has
 *          the SoA planes (build option layout=soa) else 0}
 * layout 0 copies the AoS records; layout 1 puts the same two arrays together again from the
 * SoA planes (words [10,11], which no plane holds, are 0) and is an error on a scene built
 * without layout=soa.  nodes = tris = NULL: only info is written (the sizes to allocate).
 * n = 0: no node record (n_nodes4 = depth4 = leaf_max = 0) and the one all-zero triangle record;
 * n = 1: one node whose only child is the leaf of record 0 (depth4 = 1).
 * -22 with a message for a null scene or info, a layout other than 0 / 1, one buffer without the
 * other, layout 1 on an AoS scene, or a buffer shorter than 16 * n_nodes4 / 12 * (n + 1) words:
 * all checked before any device call.
 *
 * What every build keeps (tests/bvh_check.py checks each from this dump, exhaustively and
 * with no tolerance; DESIGN.md section 4 "Invariants of the built tree"):
 *   tree    every node in [0, n_nodes4) is reached from node 0 exactly once; nodes are numbered
 *           level by level -- depth L's nodes fill one contiguous index range straight after depth
 *           L-1's (the path kernels copy nodes [0, kTopNodes) to LDS on that), so a child's index
 *           exceeds its parent's; the depth is depth4 = tmpt_stats.bvh4_depth, 3 * depth4 + 1 <= 128
 *   order   WITHIN a level the indices come from an atomic counter: two builds of one scene have
 *           equal node arrays only after renumbering breadth-first in child-slot order
 *           (bvh_check.canonical); raw they differ (observed: 16,247 of the stand-in's 16,662
 *           node records between two builds), while the triangle records are equal raw
 *   slots   valid children fill slots 0..nc-1, mask = (1 << nc) - 1, nc >= 2 (the one-triangle tree:
 *           1); an empty slot has qlo = 255, qhi = 0 on all three axes and the null-leaf link
 *           bit 31 | n; words [10,11] are 0; bits 30..link_bits of every link are 0 (the
 *           traversal ORs its pop key in there), (count_shift, link_bits) = (bits(n),
 *           max(bits(n) + bits(leaf_max - 1), bits(n - 2))), bits(v) = v's bit length
 *   leaves  the ranges [first, first + count) partition [0, n); 1 <= count <= leaf_max; under
 *           collapse=greedy no internal child heads a subtree of <= leaf_max triangles
 *   records [9] >> 1 over records 0..n-1 is a permutation of 0..n-1; v0, e1, e2 are the f32
 *           differences bit for bit; record n is all zero; bit 0 of [9] is set exactly on the
 *           triangles flat on a plane of the scene's octree (none without one)
 *   boxes   a triangle's box is its f32 min / max widened by kBoxPadRel * (max(|lo|, |hi|) +
 *           (hi - lo)) + 1e-30f, every operation rounded to f32; a child's decoded box contains
 *           the union U of the boxes beneath it on all six faces and each face lies less than one
 *           quantum 2^e outside U; origin = the minimum of the children's U per axis, bit for
 *           bit; e is the least exponent in [-126, 127] with 255 * 2^e >= max(extent, 1e-30)
 *           (either neighbour where the extent is within 2^-40 relative of 255 * 2^k) */
int tmpt_scene_dump_bvh(const tmpt_scene* scene, int32_t layout, uint32_t* nodes, uint64_t node_words,
                        uint32_t* tris, uint64_t tri_words, int32_t info[8]);
/* Scene update: new triangles for a scene that exists, in place of tmpt_scene_destroy +
 * tmpt_scene_create_ex.  tris holds n x 9 floats in host memory, as tmpt_scene_create takes them.
 *
 * TMPT_UPDATE_REFIT needs n equal to the scene's n (else -22).  The tree keeps its shape and is
 * fitted to the new triangles: triangle i of tris takes the slot triangle i had.
 *   unchanged   the topology and the numbering of the nodes (links, masks), the leaf ranges and the
 *               order of the triangle records, count_shift, link_bits, pop_key_bits, and every
 *               other word of info
 *   recomputed  every triangle record (v0, e1, e2 with the build's roundings, [9] = 2 x index with
 *               the flat mark cleared), every TriOrig record with its normal, and every node's
 *               origin, exponents and quantised planes; on a layout=soa scene the planes too
 *   contract    after a refit the dump is the one the rules of "What every build keeps" give for
 *               the OLD links and the NEW triangles, word for word: a child's box is the union U
 *               of the padded boxes beneath it (an exact f32 min / max, so the order of reduction
 *               does not matter), and a node's words are a function of its children's U alone
 *               (tests/bvh_refit_restate.py restates it in numpy).  Rules tree, order, slots,
 *               leaves, records and boxes all still hold; only "leaves: collapse=greedy ..."
 *               speaks of the tree's shape, which the refit does not touch.  A refit with the
 *               scene's own triangles changes no word.
 *   cost        one launch per triangle record and one per BVH4 level, deepest first, on the
 *               scene's stream, no host synchronisation between them; n = 0 does nothing, n = 1
 *               rewrites the one-leaf node.  The tree no longer follows the triangles' new
 *               positions: option bvh_cost says by how much.
 * TMPT_UPDATE_REBUILD takes any n >= 0 and runs the full build with the scene's build options into
 * fresh allocations, swapped in only on success: a failed rebuild (a tree too deep for the
 * traversal stack, out of memory) returns the build's error and leaves the scene exactly as it
 * was.  The handle, the stream, every option, the workspace, the sample, camera pre-pass and
 * shadow-split buffers and the jump tables are kept.
 *
 * Both modes synchronise the scene's stream first, replace the scene's host copy of the
 * triangles, and DROP THE OCTREE exactly as if none had been built: the device octree is freed,
 * tmpt_stats.octree_* read 0, tie_rule in effect is index (1), no record carries the flat mark.
 * Call tmpt_scene_build_octree again with the new bounds (only the caller knows them; under option
 * octree_build=device that build runs on the device too).  The progressive state is invalidated: a render with spp_begin > 0
 * straight after fails with -22, as after a camera change.  Like tmpt_scene_build_octree the call
 * must not run while a call on the scene is in flight on another host thread.
 * -22 with a message, checked in this order before any device call: an unknown mode, n < 0, null
 * tris with n > 0, a null scene, a refit whose n is not the scene's.
 * Read-only options afterwards (tmpt_scene_get_option): update_kind, update_ms, bvh_cost. */
enum { TMPT_UPDATE_REFIT = 0, TMPT_UPDATE_REBUILD = 1 };
int tmpt_scene_update(tmpt_scene* scene, const float* tris, int32_t n, int32_t mode);
/* Check hook: the device radix sort the build (Morton keys) and the pixel-seeded renders (the
 * cost-ordered pixel supply) use, run on caller data: the n pairs (keys[i], vals[i]) (host
 * memory) are uploaded, sorted on the scene's stream and written back in place.  The scene only
 * lends its device and stream.  The sort is stable and works in whole 8-bit passes from bit 0:
 * the pairs come back ordered by keys[i] & mask, mask = the low 8 * ceil(bits / 8) bits (all 32
 * for bits > 24); bits above the mask do not take part.  -22 for bits outside 1..32, n outside
 * 0..2^22, a null array with n > 0, or a null scene -- checked in that order, before any
 * device call; n = 0 does nothing. */
int tmpt_radix_sort(const tmpt_scene* scene, uint32_t* keys, uint32_t* vals, int64_t n, int32_t bits);

const char* tmpt_last_error(void);
int tmpt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TMPT_H */
