// tmpt_render.h -- what the render translation units share (tmpt_render.hip:
// the persistent path engine and the host side of a render call;
// tmpt_rows.hip: the row engines; tmpt_mega.hip: the megakernel;
// tmpt_wavefront.hip: the wavefront engine; tmpt_hitscene.hip: the batched
// queries; tmpt_aov.hip: the AOV pass; tmpt_motion.hip: the motion pass and
// the reprojected history;
// tmpt_denoise.hip: the filter over a finished frame): the kernel argument
// block of one render call, the wave helpers, the host helpers of a render
// call (defined in tmpt_render.hip) and the entry points of the engines that
// have a unit of their own.
#pragma once

#include "tmpt.h"
#include "tmpt_internal.h"
#include "tmpt_traverse.h"

namespace tmpt {

struct RenderArgs {
    Camera cam;
    int32_t W, H, spp, seed_mode, band_rows, shard, nshards, tile_rows;
    float invW, invH, spp_recip;
    int64_t slots;  // tile_rows * W
    // progressive spp: samples [smp_begin, smp_end) this call; prog = per-pixel
    // {colour sum, rng} carried between calls (null: one full pass)
    int32_t smp_begin, smp_end;
    float out_recip;  // 1/spp for the final pass, 1/smp_end for a preview
    float4* prog;
    // sample seeding (TMPT_SEED_SAMPLE): jump tables of sample_seed (null in the
    // other modes); a lane's run of samples ends where smp & bmask == 0 (its
    // block of the persistent engine; 2047 = never inside 1..1024)
    const uint32_t* jt;
    uint32_t bmask;
    // row seeding in the megakernel: rows per wave (lanes 0..row_lanes-1 each
    // run one row's chain; the rest of the wave idles)
    int32_t row_lanes;
    // camera rays take the reference's root box test first (SceneView::oct
    // set and the lens may lie outside the root box: camera_root_check decides)
    int32_t root_check;
    // the dividers of W and band_rows (k_path's shading round divides by
    // neither at run time: tmpt_internal.h FastDiv)
    FastDiv div_w, div_band;
};

__device__ __forceinline__ int tile_row_to_y(const RenderArgs& a, int lr)
{
    int lb = lr / a.band_rows, r = lr - lb * a.band_rows;
    return (lb * a.nshards + a.shard) * a.band_rows + r;
}

// the same for lr >= 0, by the launch's divider of band_rows
__device__ __forceinline__ int tile_row_to_y_fd(const RenderArgs& a, int lr)
{
    int lb = (int)fastdiv((uint32_t)lr, a.div_band), r = lr - lb * a.band_rows;
    return (lb * a.nshards + a.shard) * a.band_rows + r;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// wave64 sum of a 32-bit value (all lanes must call)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

// wave64 ballot straight from the predicate (HIP's __ballot widens the bool to
// an int and compares it again: two extra VALU per call in the hot loops)
__device__ __forceinline__ uint64_t wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool wany(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// s_memtime (shader clock), for the PROF build of k_path only
__device__ __forceinline__ uint64_t stamp()
{
    uint64_t t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// Compacted append: every lane of the wave calls; lanes with pred get
// consecutive slots, one atomic per wave (ballot + mbcnt prefix).
__device__ __forceinline__ uint32_t wave_append(uint32_t* counter, bool pred)
{
    uint64_t m = wballot(pred);
    if (m == 0) return 0;
    int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t base = 0;
    if (lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                               __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    return base + below;
}

template <int BLOCK, bool COUNT>
__device__ __forceinline__ void flush_counts(unsigned long long* counters, uint32_t rays,
                                             const TravCount& cnt)
{
    uint32_t r = wave_sum(rays);
    uint32_t nv = COUNT ? wave_sum(cnt.nodes) : 0u;
    uint32_t nt = COUNT ? wave_sum(cnt.tris) : 0u;
    if (lane_id() == 0) {
        atomicAdd(&counters[0], (unsigned long long)r);
        if (COUNT) {
            atomicAdd(&counters[1], (unsigned long long)nv);
            atomicAdd(&counters[2], (unsigned long long)nt);
        }
    }
}

// Queues are segmented: the P path slots are cut into kSeg contiguous ranges
// of seg_cap slots (seg_cap a multiple of the 256-slot shade block); segment j
// of a queue holds only entries of slots in range j, at [j*seg_cap, +count_j).
// Every counter and fetch head sits on its own 64-B line, so the producers'
// wave appends and the consumers' chunk reservations spread over kSeg words
// instead of serialising on one (MI355X_MICROARCH.md: one word saturates at
// ~88 atomics/us).
constexpr int kSeg = 64;  // == wave width: one lane probes one segment
static_assert(kSeg == 64, "segment probing maps segments to the 64 lanes of a wave");
constexpr int kCtr = 16;  // words between counters (64 B)
constexpr uint32_t kChunk = 64;  // queue entries a wave reserves per atomic

// ---- host helpers of a render call (tmpt_render.hip)
constexpr int kBlk = 256;
constexpr int kSL = 16;  // LDS stack entries per lane

// blocks of `block` threads the device holds at once (occupancy API x CUs)
int occupancy_grid(const void* fn, int block, size_t dyn_lds, int device);
// the scene's render workspace, grown to `bytes`
int ensure_ws(Scene& s, size_t bytes);
SceneView view(const Scene& s);
RenderArgs make_args(const tmpt_camera* c, const tmpt_render_desc* d);
// sample_seed's jump tables on the device for samples [0, spp) of the window that
// option sample_base opens (Scene::jt, grown, never shrunk)
int ensure_sample_tables(Scene& s, int32_t spp, const char* what);
// a jump table uploaded into a new buffer that replaces dst's on success
int upload_tables(DeviceBuffer<uint32_t>& dst, const std::vector<uint32_t>& tab, const char* what);
// TMPT_FLAG_WAIT_STREAM: the scene's stream waits for the work enqueued on d->wait_stream
int wait_caller_stream(Scene& s, const tmpt_render_desc* d, const char* what);
// RenderArgs::root_check of a camera: 1 unless no octree answers (none built,
// or tie_rule = index) or the whole lens lies inside the octree's root box
int32_t camera_root_check(const Scene& s, const Camera& cam);
// the statistics of the last render, zeroed before a new one
void reset_render_stats(Scene& s);
// sample_seed's byte tables for jumps J_i = M^((first + i) * stride), i in [0, count)
void jump_tables(uint64_t stride_steps, int32_t count, std::vector<uint32_t>& tab, uint32_t first = 0);

// ---- the engines outside tmpt_render.hip (its render() picks one)
// tmpt_mega.hip
int render_megakernel(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count,
                      unsigned long long* d_counters);
// tmpt_wavefront.hip
int render_wavefront(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count);
// tmpt_rows.hip
struct PixelChains;  // tmpt_path.h
int render_rowstream(Scene& s, const RenderArgs& a, uint32_t* d_out, unsigned long long* d_counters);
int render_rowspec(Scene& s, const RenderArgs& a, uint32_t* d_out, unsigned long long* d_counters,
                   const PixelChains* ch = nullptr);

// tmpt_aov.hip: the AOV pass of one shard (tmpt_render_aov), d_out on the device
int render_aov(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, tmpt_aov_pixel* d_out,
               uint64_t* ray_count);

// tmpt_render.hip: the persistent path engine, one pass (render() calls it for
// a render, render_adaptive for each of its passes: Scene::adapt_on / adapt_list)
int render_persistent(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count, unsigned long long* d_counters);

// tmpt_adaptive.hip: adaptive sampling (tmpt_render_adaptive) of one shard; ad
// holds the resolved spp_min, spp_step, threshold and radius (checked by the caller),
// the three tiles are device pointers or null; d_mom: the moments tile of
// tmpt_render_moments (`what` then names that call in errors), or null; d_prior:
// the prior tile of tmpt_render_guided (the tile's float4 in slot order), or null
// (the update kernels' no-prior instantiations: the calls as they were)
int render_adaptive(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, const tmpt_adaptive_desc* ad,
                    float4* d_f32, uint32_t* d_u8, int32_t* d_spp, tmpt_adaptive_info* info, uint64_t* ray_count,
                    float4* d_mom = nullptr, const char* what = "tmpt_render_adaptive",
                    const float4* d_prior = nullptr);

// tmpt_denoise.hip: the a-trous filter (tmpt_denoise) over a whole frame, every
// pointer on the device; d (checked by the caller) holds the resolved levels,
// normal_exp and sigmas.  d_out32 or d_out8 may be null; d_out32 may be d_in.
int denoise(Scene& s, const tmpt_denoise_desc* d, const float4* d_in, const tmpt_aov_pixel* d_aov, float4* d_out32,
            uint32_t* d_out8);
// the noise-aware form (tmpt_denoise_moments): d_mom the frame's moments, shrink resolved and > 0
int denoise_moments(Scene& s, const tmpt_denoise_desc* d, float shrink, const float4* d_in, const tmpt_aov_pixel* d_aov,
                    const float4* d_mom, float4* d_out32, uint32_t* d_out8);

// tmpt_motion.hip: the motion pass of one shard (tmpt_render_motion), d_out on
// the device; d_prev the previous pose on the device (9 floats per triangle) or
// null (the scene's own vertices)
int render_motion(Scene& s, const tmpt_camera* cam, const tmpt_camera* prev_cam, const float* d_prev,
                  const tmpt_render_desc* d, tmpt_motion_pixel* d_out, uint64_t* ray_count);
// tmpt_motion.hip: the reprojected history (tmpt_temporal) over a whole frame,
// every pointer on the device; d (checked by the caller) holds the resolved
// n_max and sigma_depth.  d_out32 or d_out8 may be null; d_out32 may be d_cur.
int temporal(Scene& s, const tmpt_temporal_desc* d, const float4* d_cur, const tmpt_motion_pixel* d_motion,
             const tmpt_motion_pixel* d_pmotion, const float4* d_hist, float4* d_out32, uint32_t* d_out8);
// tmpt_motion.hip: the clipped form (tmpt_temporal_clip); d holds the resolved
// n_max, sigma_depth, gamma and radius; d_stat a frame (d_cur where none was
// given); the aux pointers all three or none.  No output overlaps d_cur, d_stat
// or a history.
int temporal_clip(Scene& s, const tmpt_temporal_clip_desc* d, const float4* d_cur, const float4* d_stat,
                  const tmpt_motion_pixel* d_motion, const tmpt_motion_pixel* d_pmotion, const float4* d_hist,
                  const float4* d_aux_cur, const float4* d_aux_hist, float4* d_aux_out, float4* d_out32,
                  uint32_t* d_out8);
// tmpt_motion.hip: the sample plan (tmpt_sample_plan) over a whole frame, every
// pointer on the device; d holds the resolved n_max and sigma_depth; d_out
// overlaps no input
int sample_plan(Scene& s, const tmpt_temporal_desc* d, const tmpt_motion_pixel* d_motion,
                const tmpt_motion_pixel* d_pmotion, const float4* d_hist, float4* d_out);

}  // namespace tmpt
