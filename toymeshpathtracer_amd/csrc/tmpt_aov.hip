// tmpt_aov.hip -- the AOV pass (tmpt_render_aov, include/tmpt.h tmpt_aov_pixel):
// per pixel the guide buffers of a sample-seeded frame -- hit normal, depth,
// the first bounce's light scalar, triangle id, coverage -- from exactly the
// camera rays the beauty render traces (main.cpp:209-221: sample_seed, then
// camera_sample; main.cpp:53-72: the bounce-0 shadow query and light term).
//
// One closest-hit query and at most one any-hit query per sample, through the
// traversal every engine steps (tmpt_traverse.h), with the scene's tie, crack
// and flat handling and the octree root test, so a camera ray gets the very
// answer the beauty's camera ray gets.
//
// Work: G lanes (1, 2, 4, 8 or 16; aligned groups of a wave) share a pixel,
// lane g of the group tracing samples g, g + G, ...; a wave takes 64 / G
// consecutive pixels per ticket.  After each round of G samples every lane
// reads the round's values from their owners by shuffle, in sample order, so
// the float32 sums are taken in the order s = 0 .. spp-1 whatever G is and
// the record is bit-identical for every G.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "tmpt_render.h"

namespace tmpt {

static_assert(sizeof(tmpt_aov_pixel) == 32, "AOV record: two 16-byte stores");

constexpr int kAovTicket = 8;  // counters[]: the next pixel no wave has taken

// What one lane keeps of one sample: bit 0 of flags = the camera ray hit,
// bit 1 = its light scalar counts (cosine > 0 and the shadow query missed).
struct AovSample {
    f3 n;
    float t, lc;
    uint32_t flags;
    int32_t tri;
};

template <int BLOCK, int SL>
__device__ __forceinline__ AovSample aov_sample(const SceneView& sv, const RenderArgs& a, uint32_t x, uint32_t y,
                                                uint32_t smp, uint32_t& rays, uint32_t& srays,
                                                TravStack<BLOCK, SL>& st, TravCount& cnt)
{
    AovSample r{mk(0.0f, 0.0f, 0.0f), 0.0f, 0.0f, 0u, -1};
    uint32_t rng = sample_seed(a.jt, smp, pixel_seed(x, y, (uint32_t)a.W));
    f3 o, d;
    camera_sample(a.cam, x, y, a.invW, a.invH, rng, o, d);
    ++rays;
    float t, u, v;
    int id = -1;
    if (a.root_check && !octree_root_hit(sv, o, d, kMinT, kMaxT)) {
        atomicAdd(&sv.oct->ties[1], 1ull);  // the camera ray misses the reference's root box
    } else {
        id = traverse<false, false, BLOCK, SL>(sv, make_trav_ray(o, d), kMinT, kMaxT, t, u, v, st, cnt);
    }
    if (id < 0) return r;
    f3 pos;
    hit_record(sv, id, u, v, pos, r.n);
    r.t = t;
    r.tri = id;
    r.flags = 1u;
    ++srays;  // the shadow ray, main.cpp:57-59 (counted whether or not it is traced)
    const float lc = light_cosine(r.n, d);
    if (lc > 0.0f) {  // a zero light term does not depend on the answer
        float ts, us, vs;
        const int sid = traverse<true, false, BLOCK, SL>(sv, make_trav_ray(pos, light_dir()), kMinT, kMaxT, ts, us,
                                                         vs, st, cnt);
        if (sid < 0) {
            r.lc = lc;
            r.flags |= 2u;
        }
    }
    return r;
}

template <int G, int BLOCK, int SL>
__global__ void __launch_bounds__(BLOCK) k_aov(SceneView sv, RenderArgs a, float4* __restrict__ out,
                                               uint32_t* __restrict__ ovf,
                                               unsigned long long* __restrict__ counters)
{
    static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "lane groups: aligned powers of two");
    constexpr int kPix = 64 / G;  // pixels of one wave ticket
    __shared__ uint32_t s_stack[SL * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    TravCount cnt;
    const int lane = lane_id();
    const int g = lane & (G - 1), lead = lane & ~(G - 1);
    const int rounds = (a.spp + G - 1) / G;
    uint32_t rays = 0, srays = 0;
    for (;;) {
        // one ticket per wave: 64 / G consecutive pixels of the tile
        // (a tile has at most 10^8 pixels and the tickets overshoot by one per wave: 32 bits hold them)
        uint32_t base = 0;
        if (lane == 0) base = (uint32_t)atomicAdd(&counters[kAovTicket], (unsigned long long)kPix);
        const int64_t first = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (first >= a.slots) break;
        const int64_t pix = first + lane / G;
        const bool live = pix < a.slots;
        const int lr = live ? (int)(pix / a.W) : 0;
        const uint32_t x = live ? (uint32_t)(pix - (int64_t)lr * a.W) : 0u;
        const uint32_t y = (uint32_t)tile_row_to_y(a, lr);
        f3 nsum = mk(0.0f, 0.0f, 0.0f);
        float dsum = 0.0f, lsum = 0.0f;
        uint32_t hits = 0, lit = 0;
        int32_t tri0 = -1;
        for (int k = 0; k < rounds; ++k) {  // the same count in every lane: the shuffles below meet
            const int smp = k * G + g;
            AovSample r{mk(0.0f, 0.0f, 0.0f), 0.0f, 0.0f, 0u, -1};
            if (live && smp < a.spp) r = aov_sample<BLOCK, SL>(sv, a, x, y, (uint32_t)smp, rays, srays, st, cnt);
            if (k == 0) tri0 = r.tri;  // sample 0 is the group's first lane's first
#pragma unroll
            for (int j = 0; j < G; ++j) {  // samples k G + j in order, each from its owner
                const int src = lead + j;
                const uint32_t f = G == 1 ? r.flags : (uint32_t)__shfl((int)r.flags, src);
                const float nx = G == 1 ? r.n.x : __shfl(r.n.x, src), ny = G == 1 ? r.n.y : __shfl(r.n.y, src),
                            nz = G == 1 ? r.n.z : __shfl(r.n.z, src);
                const float t = G == 1 ? r.t : __shfl(r.t, src), lc = G == 1 ? r.lc : __shfl(r.lc, src);
                if (f & 1u) {  // a miss adds nothing
                    nsum = nsum + mk(nx, ny, nz);
                    dsum = dsum + t;
                    ++hits;
                }
                if (f & 2u) {
                    lsum = lsum + lc;
                    ++lit;
                }
            }
        }
        if (live && g == 0) {  // the record, scaled as pack_pixel scales colour; two 16-byte stores
            const f3 n = nsum * a.spp_recip;
            float4* p = out + 2 * pix;
            p[0] = make_float4(n.x, n.y, n.z, dsum * a.spp_recip);
            p[1] = make_float4(lsum * a.spp_recip, __int_as_float(tri0), __uint_as_float(hits), __uint_as_float(lit));
        }
    }
    // [0] every query, [3] the closest-hit ones (as the path kernels count)
    const uint32_t r0 = wave_sum(rays), r1 = wave_sum(srays);
    if (lane == 0) {
        atomicAdd(&counters[0], (unsigned long long)r0 + r1);
        atomicAdd(&counters[3], (unsigned long long)r0);
    }
}

// aov_group = 0: the lanes per pixel.  Measured on the bench frame at 64 spp
// (profiles/aov_pass.log, DESIGN.md "AOV pass"): 16 is the fastest both for the
// whole frame (2.07 M pixels, 12.5 ms against 19.4 ms at one lane per pixel)
// and for a 1/8 shard (259 k pixels, 1.9 ms against 5.6 ms) -- a group's rays
// differ only by jitter and lens position, so a wave walks 4 pixels' worth of
// nodes instead of 64 -- and each step down is slower by more than the
// run-to-run spread.  So: the largest group the pixel's samples fill (a
// larger one only idles lanes), up to 16, whatever the tile's size.
static int aov_auto_group(int32_t spp)
{
    int g = 1;
    while (g < 16 && 2 * g <= spp) g *= 2;
    return g;
}

template <int G>
static int launch_aov(Scene& s, const RenderArgs& a, tmpt_aov_pixel* d_out)
{
    auto fn = k_aov<G, kBlk, kSL>;
    const int resident = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    int grid = (int)std::max<int64_t>(1, std::min<int64_t>(resident, (a.slots * G + kBlk - 1) / kBlk));
    const size_t ovf_bytes = (size_t)grid * kBlk * (kStackTotal - kSL) * sizeof(uint32_t);
    if (ensure_ws(s, ovf_bytes)) return -1;
    fn<<<grid, kBlk, 0, s.stream>>>(view(s), a, reinterpret_cast<float4*>(d_out), s.ws.as<uint32_t>(), s.counters);
    TMPT_HIP(hipGetLastError());
    return 0;
}

// The call leaves the progressive state (Scene::prog, prog_key), the colour
// buffer and the redo list alone; it shares the workspace, the counters and
// the jump tables with render().
int render_aov(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, tmpt_aov_pixel* d_out,
               uint64_t* ray_count)
{
    RenderArgs a = make_args(cam, d);
    s.row_render = s.pixel_render = false;  // the AOV pass traces the sample-seeded frame's camera rays
    if (int rc = ensure_sample_tables(s, a.spp, "tmpt_render_aov")) return rc;
    a.jt = s.jt;
    if (int rc = wait_caller_stream(s, d, "tmpt_render_aov")) return rc;
    if (ensure_counters(s)) return -1;
    a.root_check = camera_root_check(s, a.cam);
    TMPT_HIP(hipMemsetAsync(s.counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    reset_render_stats(s);
    int rc = 0;
    if (a.slots > 0) {
        switch (s.opt.aov_group ? s.opt.aov_group : aov_auto_group(a.spp)) {
        case 1: rc = launch_aov<1>(s, a, d_out); break;
        case 2: rc = launch_aov<2>(s, a, d_out); break;
        case 4: rc = launch_aov<4>(s, a, d_out); break;
        case 8: rc = launch_aov<8>(s, a, d_out); break;
        default: rc = launch_aov<16>(s, a, d_out); break;
        }
    }
    (void)hipEventRecord(e1, s.stream);
    hipError_t se = rc == 0 ? hipMemcpyAsync(s.counters_host, s.counters, kRenderCounters * sizeof(unsigned long long),
                                             hipMemcpyDeviceToHost, s.stream)
                            : hipSuccess;
    const hipError_t se2 = hipStreamSynchronize(s.stream);
    if (se == hipSuccess) se = se2;
    if (rc) return rc;
    if (se != hipSuccess) {
        set_error(std::string("tmpt_render_aov: ") + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const unsigned long long* c = s.counters_host;
    s.render_ms = ms;
    s.extend_ms = ms;
    s.extend_rays = c[3];
    s.shadow_rays = c[0] - c[3];
    s.extend_launches = a.slots > 0 ? 1 : 0;
    s.iterations = s.extend_launches;
    s.tie_queries = c[kTieCounter];
    s.root_misses = c[kTieCounter + 1];
    s.crack_queries = c[kCrackCounter];
    if (ray_count) *ray_count = c[0];
    return 0;
}

}  // namespace tmpt
