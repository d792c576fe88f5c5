// tmpt_lane_path.h -- one lane tracing one whole path: a whole query
// (mega_query), a path from any of its closest-hit queries on (trace_path) and
// a pixel's samples (render_pixel).  Used by the megakernel (tmpt_mega.hip
// k_mega) and by the deferred ties' re-trace (tmpt_render.hip redo_sample, k_redo).
#pragma once

#include "tmpt_render.h"

namespace tmpt {

// Whole query; TOPC: the top BVH4 levels from the block's LDS copy (the
// latency-bound row chains).
template <bool ANY, bool COUNT, bool TOPC, int BLOCK, int SL, bool CHECK_ANY = true>
__device__ __forceinline__ int mega_query(const SceneView& sv, f3 o, f3 d, float& t, float& u, float& v,
                                          TravStack<BLOCK, SL>& st, TravCount& cnt)
{
    return traverse<ANY, COUNT, BLOCK, SL, TOPC, false, false, CHECK_ANY>(sv, make_trav_ray(o, d), kMinT, kMaxT, t, u,
                                                                          v, st, cnt);
}

// rays: closest-hit queries, srays: shadow queries (the same counter where the
// caller does not split them)
// CHECK_ANY: the shadow answers are checked against the octree (settle_any);
// the deferred-tie redo passes false (tie_defer is off wherever a shadow
// answer can need the octree, PathCtl::oct_shadow)
template <bool COUNT, int BLOCK, int SL, bool TOPC = false, bool CHECK_ANY = true>
__device__ __forceinline__ f3 trace_path(const SceneView& sv, f3 o, f3 d, uint32_t& rng,
                                         uint32_t& rays, uint32_t& srays, TravStack<BLOCK, SL>& st, float* lbuf,
                                         TravCount& cnt, bool root_check, int depth0 = 0, int* end_depth = nullptr)
{
    // end_depth (the shadow split's re-trace): the path's depth goes there and
    // its end colour is returned as it stands, lbuf[0, depth) holding the terms
    // of the backward recurrence, which the caller's record leaves to k_split_resolve
    int depth = depth0;  // > 0: a path resumed at its depth0-th closest-hit query, lbuf[0, depth0) set
    f3 color = mk(0.0f, 0.0f, 0.0f);
    while (depth < kMaxDepth) {  // Trace, main.cpp:89-110
        ++rays;
        float t, u, v;
        int id = -1;
        if (depth == 0 && root_check && !octree_root_hit(sv, o, d, kMinT, kMaxT)) {
            atomicAdd(&sv.oct->ties[1], 1ull);  // the camera ray misses the reference's root box
        } else {
            id = mega_query<false, COUNT, TOPC>(sv, o, d, t, u, v, st, cnt);
        }
        if (id >= 0) {
            f3 pos, nrm;
            hit_record(sv, id, u, v, pos, nrm);
            ++srays;  // shadow ray, main.cpp:57-59 (always counted)
            float lc = light_cosine(nrm, d);
            if (lc > 0.0f) {  // a zero light term does not depend on the answer
                float ts, us, vs;
                int sid = mega_query<true, COUNT, TOPC, BLOCK, SL, CHECK_ANY>(sv, pos, light_dir(), ts, us, vs, st, cnt);
                if (sid >= 0) lc = 0.0f;
            }
            lbuf[depth * BLOCK] = lc;
            f3 rnd = random_unit_vector(rng);  // main.cpp:71-72
            f3 target = pos + nrm + rnd;
            d = normalize(target - pos);
            o = pos;
            ++depth;
        } else {
            color = sky(d);
            break;
        }
    }
    if (end_depth) {
        *end_depth = depth;
        return color;
    }
    for (int i = depth - 1; i >= 0; --i) color = backward_step(color, lbuf[i * BLOCK]);
    return color;
}

template <bool COUNT, int BLOCK, int SL, bool TOPC = false>
__device__ __forceinline__ uint32_t render_pixel(const SceneView& sv, const RenderArgs& a, int x,
                                                 int y, uint32_t& rng, uint32_t& rays,
                                                 TravStack<BLOCK, SL>& st, float* lbuf,
                                                 TravCount& cnt)
{
    f3 col = mk(0.0f, 0.0f, 0.0f);
    const uint32_t pseed = rng;
    for (int s = 0; s < a.spp; ++s) {  // main.cpp:209-219
        f3 o, d;
        if (a.jt) rng = sample_seed(a.jt, (uint32_t)s, pseed);  // sample seeding
        camera_sample(a.cam, (uint32_t)x, (uint32_t)y, a.invW, a.invH, rng, o, d);
        col = col + trace_path<COUNT, BLOCK, SL, TOPC>(sv, o, d, rng, rays, rays, st, lbuf, cnt, a.root_check != 0);
    }
    return pack_pixel(col, a.spp_recip);
}

}  // namespace tmpt
