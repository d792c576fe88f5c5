// tmpt_render.h -- what the render translation units share (tmpt_render.hip:
// the path tracer's engines; tmpt_aov.hip: the AOV pass; tmpt_denoise.hip: the
// filter over a finished frame): the kernel argument
// block of one render call, the wave helpers, and the host helpers of a render
// call (defined in tmpt_render.hip).
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

// ---- host helpers of a render call (tmpt_render.hip)
constexpr int kBlk = 256;
constexpr int kSL = 16;  // LDS stack entries per lane

// blocks of `block` threads the device holds at once (occupancy API x CUs)
int occupancy_grid(const void* fn, int block, size_t dyn_lds, int device);
// the scene's render workspace, grown to `bytes`
int ensure_ws(Scene& s, size_t bytes);
SceneView view(const Scene& s);
RenderArgs make_args(const tmpt_camera* c, const tmpt_render_desc* d);
// sample_seed's jump tables on the device for samples [0, spp) (Scene::jt, grown, never shrunk)
int ensure_sample_tables(Scene& s, int32_t spp, const char* what);
// TMPT_FLAG_WAIT_STREAM: the scene's stream waits for the work enqueued on d->wait_stream
int wait_caller_stream(Scene& s, const tmpt_render_desc* d, const char* what);
// RenderArgs::root_check of a camera: 1 unless no octree answers (none built,
// or tie_rule = index) or the whole lens lies inside the octree's root box
int32_t camera_root_check(const Scene& s, const Camera& cam);
// the statistics of the last render, zeroed before a new one
void reset_render_stats(Scene& s);

// tmpt_aov.hip: the AOV pass of one shard (tmpt_render_aov), d_out on the device
int render_aov(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, tmpt_aov_pixel* d_out,
               uint64_t* ray_count);

// tmpt_denoise.hip: the a-trous filter (tmpt_denoise) over a whole frame, every
// pointer on the device; d (checked by the caller) holds the resolved levels,
// normal_exp and sigmas.  d_out32 or d_out8 may be null; d_out32 may be d_in.
int denoise(Scene& s, const tmpt_denoise_desc* d, const float4* d_in, const tmpt_aov_pixel* d_aov, float4* d_out32,
            uint32_t* d_out8);

}  // namespace tmpt
