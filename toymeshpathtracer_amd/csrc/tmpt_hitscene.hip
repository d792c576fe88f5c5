// tmpt_hitscene.hip -- the batched HitScene: k_intersect and its host,
// intersect_batch (tmpt_scene_hit in tmpt_api.cpp calls it).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tmpt_render.h"

namespace tmpt {

// ============================================================ batched HitScene
// Scene::HitScene (scene.cpp:86-97) over a batch: rays n x {o.xyz, d.xyz}
// with one [tmin, tmax] for all (RANGED = 0), or n x {o.xyz, d.xyz, tmin, tmax}
// (RANGED = 1, the per-call range of scene.h:36-37).  hits n x {pos, normal, t}
// where ids >= 0.
// NEG: the range can start behind the origin (every per-ray range, and a
// single range with tmin < 0): the traversal's far-distance slack by magnitude.
template <bool ANY, bool RANGED, int BLOCK, int SL, bool SOA = false, bool NEG = RANGED>
__global__ void __launch_bounds__(BLOCK) k_intersect(SceneView sv, const float* __restrict__ rays,
                                                     int64_t n, float tmin, float tmax,
                                                     float* __restrict__ hits,
                                                     int32_t* __restrict__ ids,
                                                     uint32_t* __restrict__ ovf)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    TravCount cnt;
    constexpr int kStride = RANGED ? 8 : 6;
    for (int64_t i = gtid; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const float* r = rays + kStride * i;
        f3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
        const float t0 = RANGED ? r[6] : tmin, t1 = RANGED ? r[7] : tmax;
        float t, u, v;
        int id = -1;
        // with the reference's octree: its root box test first (scene.cpp:25)
        if (sv.oct && !octree_root_hit(sv, o, d, t0, t1)) {
            atomicAdd(&sv.oct->ties[1], 1ull);
        } else {
            // a range that may start behind the origin: sign-aware slack (NEG)
            id = traverse<ANY, false, BLOCK, SL, false, SOA, NEG>(sv, make_trav_ray(o, d), t0, t1, t, u, v, st, cnt);
        }
        ids[i] = id;
        if (id >= 0) {
            f3 pos, nrm;
            hit_record(sv, id, u, v, pos, nrm);
            float* h = hits + 7 * i;
            h[0] = pos.x; h[1] = pos.y; h[2] = pos.z;
            h[3] = nrm.x; h[4] = nrm.y; h[5] = nrm.z;
            h[6] = t;
        }
    }
}

// rays: n x 6 floats (one [tmin, tmax] for all) or, ranged, n x 8 (per ray)
int intersect_batch(Scene& s, const float* d_rays, int64_t n, float tmin, float tmax, bool any, bool ranged,
                    float* d_hits, int32_t* d_ids)
{
    s.row_render = s.pixel_render = false;
    if (ensure_counters(s)) return -1;
    TMPT_HIP(hipMemsetAsync(s.ties, 0, 2 * sizeof(unsigned long long), s.stream));
    TMPT_HIP(hipMemsetAsync(s.counters + kCrackCounter, 0, sizeof(unsigned long long), s.stream));
    const bool soa = s.bvh.soa.na != nullptr;
    // one range starting behind the origin takes the NEG slack too
    const bool neg1 = !ranged && tmin < 0.0f;
    auto fn = soa ? (ranged ? (any ? k_intersect<true, true, kBlk, kSL, true> : k_intersect<false, true, kBlk, kSL, true>)
                    : neg1  ? (any ? k_intersect<true, false, kBlk, kSL, true, true>
                                   : k_intersect<false, false, kBlk, kSL, true, true>)
                            : (any ? k_intersect<true, false, kBlk, kSL, true> : k_intersect<false, false, kBlk, kSL, true>))
                  : (ranged ? (any ? k_intersect<true, true, kBlk, kSL> : k_intersect<false, true, kBlk, kSL>)
                    : neg1  ? (any ? k_intersect<true, false, kBlk, kSL, false, true>
                                   : k_intersect<false, false, kBlk, kSL, false, true>)
                            : (any ? k_intersect<true, false, kBlk, kSL> : k_intersect<false, false, kBlk, kSL>));
    int grid = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    grid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (n + kBlk - 1) / kBlk));
    size_t ovf_bytes = (size_t)grid * kBlk * (kStackTotal - kSL) * sizeof(uint32_t);
    if (ensure_ws(s, ovf_bytes)) return -1;
    fn<<<grid, kBlk, 0, s.stream>>>(view(s), d_rays, n, tmin, tmax, d_hits, d_ids, s.ws.as<uint32_t>());
    TMPT_HIP(hipGetLastError());
    TMPT_HIP(hipMemcpyAsync(s.counters_host + kTieCounter, s.ties, 2 * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, s.stream));
    TMPT_HIP(hipMemcpyAsync(s.counters_host + kCrackCounter, s.counters + kCrackCounter, sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, s.stream));
    return 0;
}

}  // namespace tmpt
