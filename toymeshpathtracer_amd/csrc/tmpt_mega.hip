// tmpt_mega.hip -- the megakernel and its host, render_megakernel (render() in
// tmpt_render.hip calls it):
//  * megakernel: one lane per pixel (pixel mode) or per row (row mode: the
//    unmodified reference RNG chain, H-way parallel -- a correctness mode).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tmpt_lane_path.h"

namespace tmpt {

template <bool ROW, bool COUNT, int BLOCK, int SL>
__global__ void __launch_bounds__(BLOCK) k_mega(SceneView sv, RenderArgs a,
                                                uint32_t* __restrict__ out,
                                                uint32_t* __restrict__ ovf,
                                                unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    __shared__ float s_light[kMaxDepth * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    float* lbuf = &s_light[threadIdx.x];
    // ROW (one latency-bound chain per wave): the persistent engine's node step,
    // with the top BVH4 levels copied to LDS
    constexpr bool TOPC = ROW;
    if (TOPC) {
        __shared__ uint4 s_top[TOPC ? kTopNodes * 4 : 1];
        const uint32_t ntop = (uint32_t)min(kTopNodes, sv.n_nodes4);
        const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
        for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
        __syncthreads();
        st.top = (const lds_u4*)s_top;
        st.ntop = ntop;
    }
    uint32_t rays = 0;
    TravCount cnt;
    const int64_t items = ROW ? (int64_t)a.tile_rows : a.slots;
    // ROW: lane l < row_lanes of wave v takes rows v*row_lanes + l, strided
    // over the grid's waves (one chain per lane, spread over the SIMDs)
    const int64_t first = ROW ? (lane_id() < a.row_lanes ? (gtid >> 6) * a.row_lanes + lane_id() : items) : gtid;
    const int64_t stride = ROW ? (int64_t)gridDim.x * (BLOCK / 64) * a.row_lanes : (int64_t)gridDim.x * BLOCK;
    for (int64_t w = first; w < items; w += stride) {
        if (ROW) {
            int lr = (int)w;
            int y = tile_row_to_y(a, lr);
            uint32_t rng = row_seed((uint32_t)y);  // main.cpp:204, unmodified
            for (int x = 0; x < a.W; ++x)
                out[(int64_t)lr * a.W + x] = render_pixel<COUNT, BLOCK, SL, TOPC>(sv, a, x, y, rng, rays, st, lbuf, cnt);
        } else {
            int lr = (int)(w / a.W), x = (int)(w - (int64_t)lr * a.W);
            int y = tile_row_to_y(a, lr);
            uint32_t rng = pixel_seed((uint32_t)x, (uint32_t)y, (uint32_t)a.W);
            out[w] = render_pixel<COUNT, BLOCK, SL, TOPC>(sv, a, x, y, rng, rays, st, lbuf, cnt);
        }
    }
    flush_counts<BLOCK, COUNT>(counters, rays, cnt);
}

namespace {

template <bool ROW, bool COUNT>
int launch_mega(Scene& s, const RenderArgs& a, uint32_t* out, unsigned long long* counters)
{
    auto fn = k_mega<ROW, COUNT, kBlk, kSL>;
    int grid = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    // ROW: one wave per row_lanes rows (up to the resident grid)
    int64_t items = ROW ? ((int64_t)a.tile_rows + a.row_lanes - 1) / a.row_lanes * 64 : a.slots;
    grid = (int)std::min<int64_t>(grid, (items + kBlk - 1) / kBlk);
    grid = std::max(grid, 1);
    size_t ovf_bytes = (size_t)grid * kBlk * (kStackTotal - kSL) * sizeof(uint32_t);
    if (ensure_ws(s, ovf_bytes)) return -1;
    fn<<<grid, kBlk, 0, s.stream>>>(view(s), a, out, s.ws.as<uint32_t>(), counters);
    TMPT_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int render_megakernel(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count,
                      unsigned long long* d_counters)
{
    const bool row = a.seed_mode == TMPT_SEED_ROW;
    if (row) return count ? launch_mega<true, true>(s, a, d_out, d_counters) : launch_mega<true, false>(s, a, d_out, d_counters);
    return count ? launch_mega<false, true>(s, a, d_out, d_counters) : launch_mega<false, false>(s, a, d_out, d_counters);
}

}  // namespace tmpt
