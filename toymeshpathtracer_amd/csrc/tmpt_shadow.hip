// tmpt_shadow.hip -- the shadow split of sample seeding (option shadow_split;
// DESIGN.md section 4): the two kernels that follow k_path SPLIT
// (tmpt_render.hip).  k_shadow answers the shadow queries that kernel queued,
// k_split_resolve turns the sample records into pixels.
#include "tmpt_path.h"

namespace tmpt {

// ============================================================ k_shadow
// A persistent any-hit kernel over the queue.  Every lane holds one query at a
// time and steps trav_step4q2_mixed with `any` true in voted rounds, as the
// shadow lanes of k_path do (the top levels from the block's LDS copy, the
// scene's shadow_order weight), so a query visits the nodes it visited there in
// the same order.  Idle lanes refill from the queue inside the loop: a wave
// reserves kShadowFetch entries per atomic and hands them to its idle lanes
// once kShadowFillMin of them wait (or none is left traversing), checked every
// kShadowSteps rounds -- after every round: a finished lane has nothing else
// to do, and the check is two scalar compares.
// Every shadow ray has the light's direction, so the direction, its inverse
// and the octant are compile-time constants of the step here: the octant
// selects of the node decode fold away and the slab scales are scalar
// operands; a lane keeps the origin and origin / direction only.
// A hit stores 0 into the record's cosine of that bounce: one writer per word
// (a bounce has one shadow query), ordered after k_path by the kernel boundary.
// (each with its A/B macro: tools/ab_build.sh, tools/ab_kpath.py)
#ifndef TMPT_SHADOW_SL
#define TMPT_SHADOW_SL 12
#endif
#ifndef TMPT_SHADOW_OCC
#define TMPT_SHADOW_OCC 8
#endif
#ifndef TMPT_SHADOW_STEPS
#define TMPT_SHADOW_STEPS 1
#endif
#ifndef TMPT_SHADOW_FILL
#define TMPT_SHADOW_FILL 16
#endif
constexpr int kShadowSL = TMPT_SHADOW_SL;         // LDS stack entries per lane (any-hit stacks stay shallow; the rest spills)
constexpr int kShadowOcc = TMPT_SHADOW_OCC;       // blocks per CU: 8 waves per SIMD, <= 64 VGPRs
constexpr int kShadowSteps = TMPT_SHADOW_STEPS;   // traversal rounds between refill checks
constexpr int kShadowFillMin = TMPT_SHADOW_FILL;  // idle lanes that trigger a refill
constexpr uint32_t kShadowFetch = 512u;  // queue entries a wave reserves per atomic

template <int BLOCK, int SL>
__global__ void __launch_bounds__(BLOCK, kShadowOcc) k_shadow(SceneView sv, const uint4* __restrict__ sq,
                                                              const uint32_t* __restrict__ count, uint32_t cap,
                                                              uint32_t* __restrict__ head, float* __restrict__ srec,
                                                              uint32_t n_rec, uint32_t* __restrict__ ovf)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    __shared__ uint4 s_top[kTopNodes5 * 4];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    {
        const uint32_t ntop = (uint32_t)min(kTopNodes5, sv.n_nodes4);
        const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
        for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
        __syncthreads();
        st.top = (const lds_u4*)s_top;
        st.ntop = ntop;
    }
    const uint32_t n = min(*count, cap);
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    const f3 ldir = light_dir();
    uint32_t res = 0, res_end = 0;
    bool exhausted = n == 0u || sv.n <= 0;  // no triangles: every query is a miss
    bool in_query = false;
    uint32_t dst = 0;  // record << 4 | bounce of the lane's query
    TravRay r = make_trav_ray(mk(0.0f, 0.0f, 0.0f), ldir);
    TravState ts;
    TravCount cnt;
    trav_init(ts, kMaxT);
    for (;;) {
        const uint64_t idle = wballot(!in_query);
        if (!exhausted && (__popcll(idle) >= kShadowFillMin || idle == ~0ull)) {
            if (res >= res_end) {
                uint32_t b = 0;
                if (lane_id() == 0) b = atomicAdd(head, kShadowFetch);
                b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
                if (b >= n) {
                    exhausted = true;
                } else {
                    res = b;
                    res_end = min(b + kShadowFetch, n);
                }
            }
            if (!exhausted) {
                const uint32_t take = min((uint32_t)__popcll(idle), res_end - res);
                const uint32_t k = (uint32_t)__popcll(idle & lt);
                if (!in_query && k < take) {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 e = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(sq) + (res + k));
                    // (an entry that names no record of this pass is none of k_path's: skipped)
                    if (e.w != kSplitEmpty && (e.w >> 4) < n_rec && (e.w & 15u) < (uint32_t)kMaxDepth) {
                        const f3 o = mk(__uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z));
                        r = make_trav_ray(o, ldir);
                        trav_init(ts, kMaxT);
                        dst = e.w;
                        in_query = !ray_has_nan(o, ldir);  // a NaN ray: a miss (k_path's query set-up)
                    }
                }
                res += take;
            }
        }
        if (!wany(in_query)) {
            if (exhausted) break;
            continue;
        }
        for (int k = 0; k < kShadowSteps; ++k) {  // voted rounds, as k_path's
            const uint64_t q = wballot(in_query);
            const uint64_t at_leaf = q & wballot(ts.node < 0);
            const uint64_t at_node = q & ~at_leaf;
            if (q == 0) break;
            const uint32_t n_leaf = (uint32_t)__builtin_popcount((uint32_t)at_leaf) +
                                    (uint32_t)__builtin_popcount((uint32_t)(at_leaf >> 32));
            const uint32_t n_node = (uint32_t)__builtin_popcount((uint32_t)at_node) +
                                    (uint32_t)__builtin_popcount((uint32_t)(at_node >> 32));
            const bool leaf_round = n_leaf > n_node;
            const bool stepping = in_query && ((ts.node < 0) == leaf_round);
            bool done = false;
            if (leaf_round) {
                if (stepping) done = trav_step4q2_mixed<false, BLOCK, SL, true, 2>(sv, r, true, ts, st, cnt);
            } else {
                if (stepping) done = trav_step4q2_mixed<false, BLOCK, SL, true, 1>(sv, r, true, ts, st, cnt);
            }
            if (done) {
                in_query = false;
                if (ts.best >= 0) srec[(size_t)(dst >> 4) * 16u + 4u + (dst & 15u)] = 0.0f;  // occluded
            }
        }
    }
}

static int shadow_grid(int device)
{
    return occupancy_grid((const void*)k_shadow<kBlk, kShadowSL>, kBlk, 0, device);
}

size_t shadow_ovf_words(int device) { return (size_t)shadow_grid(device) * kBlk * (kStackTotal - kShadowSL); }

int launch_shadow(hipStream_t stream, int device, const SceneView& sv, const uint4* sq, const uint32_t* count,
                  uint32_t cap, uint32_t* head, float4* srec, uint32_t n_rec, uint32_t* ovf)
{
    k_shadow<kBlk, kShadowSL><<<shadow_grid(device), kBlk, 0, stream>>>(sv, sq, count, cap, head,
                                                                        reinterpret_cast<float*>(srec), n_rec, ovf);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ============================================================ k_split_resolve
// One wave per 64 pixels, as k_resolve_px: 16 samples of each pixel at a time,
// a lane per (pixel, sample) reads the sample's record (16 consecutive
// records of a pixel are 1 KB), runs the backward recurrence -- backward_step
// from the end colour over the cosines, last bounce first, the operations
// k_path's finish runs -- and leaves the colour in LDS; then every lane sums
// its own pixel's samples in sample order (main.cpp:218) and packs the pixel
// (main.cpp:221-233).
// carry_in / carry_out (a render in several passes): the sums so far, as
// k_resolve_px's prog; they may be the same array (a lane reads its pixel's
// before it writes it).
__global__ void __launch_bounds__(64) k_split_resolve(const float4* __restrict__ srec, int64_t P, int32_t cnt,
                                                       float spp_recip, uint32_t* __restrict__ out,
                                                       const float4* carry_in, float4* carry_out)
{
    constexpr int kC = 16;
    __shared__ float4 tile[64][kC + 1];
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int t = threadIdx.x;
    const int np = (int)min<int64_t>(64, P - p0);
    f3 col = mk(0.0f, 0.0f, 0.0f);
    if (carry_in && t < np) {
        const float4 c = carry_in[p0 + t];
        col = mk(c.x, c.y, c.z);
    }
    for (int32_t s0 = 0; s0 < cnt; s0 += kC) {
        const int nc = min(kC, cnt - s0);
        for (int e = t; e < 64 * kC; e += 64) {
            const int i = e / kC, j = e - i * kC;
            if (i < np && j < nc) {
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                const f32x4* rec =
                    reinterpret_cast<const f32x4*>(srec) + 4 * ((size_t)(p0 + i) * (size_t)cnt + (size_t)(s0 + j));
                const f32x4 h = __builtin_nontemporal_load(rec);
                const uint32_t depth = __float_as_uint(h.w);
                f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = c0, c2 = c0;
                if (depth > 0u) c0 = __builtin_nontemporal_load(rec + 1);
                if (depth > 4u) c1 = __builtin_nontemporal_load(rec + 2);
                if (depth > 8u) c2 = __builtin_nontemporal_load(rec + 3);
                const float cs[kMaxDepth] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y};
                f3 color = mk(h.x, h.y, h.z);
#pragma unroll
                for (int k = kMaxDepth - 1; k >= 0; --k)
                    if ((uint32_t)k < depth) color = backward_step(color, cs[k]);
                tile[i][j] = make_float4(color.x, color.y, color.z, 0.0f);
            }
        }
        __syncthreads();
        if (t < np)
            for (int j = 0; j < nc; ++j) col = col + mk(tile[t][j].x, tile[t][j].y, tile[t][j].z);
        __syncthreads();
    }
    if (t < np) {
        if (carry_out) carry_out[p0 + t] = make_float4(col.x, col.y, col.z, 0.0f);
        out[p0 + t] = pack_pixel(col, spp_recip);
    }
}

void launch_split_resolve(hipStream_t stream, const float4* srec, int64_t P, int32_t cnt, float spp_recip,
                          uint32_t* out, const float4* carry_in, float4* carry_out)
{
    k_split_resolve<<<(unsigned)((P + 63) / 64), 64, 0, stream>>>(srec, P, cnt, spp_recip, out, carry_in, carry_out);
}

}  // namespace tmpt
