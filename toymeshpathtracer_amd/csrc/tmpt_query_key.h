// tmpt_query_key.h -- the sort key of a batched query's ray (option
// query_sort, tmpt_scene_hit_device) and the sizes of the call's chunk loop,
// one body for the host and for gfx950: k_query_keys (tmpt_query.hip) and the
// check hooks tmpt_query_keys / tmpt_query_plan (tmpt_api.cpp) compile the same
// functions, as tmpt_octree_build.h's are, so the key is checked without a
// device (tests/test_query_keys.py against tests/query_key_restate.py).
//
// The key, 24 bits (three 8-bit passes of radix_sort_pairs).  box = the root
// box of the scene's BVH (Bvh::node_box[0..5]: min.xyz, max.xyz); every
// operation is float32 and rounds once (-ffp-contract=off on both sides):
//   inv[a] = 32.0f / fmaxf(box.max[a] - box.min[a], 1e-30f)
//   c[a]   = (int)fminf(fmaxf((o[a] - box.min[a]) * inv[a], 0.0f), 31.0f)     the origin's cell of a 32^3 grid
//   q[a]   = (int)fminf(fmaxf((d[a] + 1.0f) * 4.0f, 0.0f), 7.0f)              the direction, 8 steps per axis
//   key    = morton3(c.x, c.y, c.z) << 9 | q.x << 6 | q.y << 3 | q.z          x in the lowest bit of each triple
// A ray with a NaN anywhere in o or d (ray_has_nan) gets 0xFFFFFF and sorts last.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tmpt_traverse.h"

namespace tmpt {

constexpr uint32_t kQueryKeyNan = 0xFFFFFFu;
constexpr int kQueryKeyBits = 24;

// the low 5 bits of v spread to every third bit
TMPT_HD uint32_t query_spread5(uint32_t v)
{
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}

TMPT_HD uint32_t query_morton3(uint32_t x, uint32_t y, uint32_t z)
{
    return query_spread5(x) | (query_spread5(y) << 1) | (query_spread5(z) << 2);
}

TMPT_HD uint32_t query_key(f3 o, f3 d, const float* box)
{
    if (ray_has_nan(o, d)) return kQueryKeyNan;
    const float oc[3] = {o.x, o.y, o.z}, dc[3] = {d.x, d.y, d.z};
    uint32_t c[3], q[3];
    for (int a = 0; a < 3; ++a) {
        const float inv = 32.0f / fmaxf(box[3 + a] - box[a], 1e-30f);
        c[a] = (uint32_t)(int)fminf(fmaxf((oc[a] - box[a]) * inv, 0.0f), 31.0f);
        q[a] = (uint32_t)(int)fminf(fmaxf((dc[a] + 1.0f) * 4.0f, 0.0f), 7.0f);
    }
    return query_morton3(c[0], c[1], c[2]) << 9 | q[0] << 6 | q[1] << 3 | q[2];
}

// ---------------------------------------------------------------- the chunk loop's sizes
// What one tmpt_scene_hit_device call launches and holds, from its arguments
// alone (no device call): a sorted batch runs in chunks of at most `chunk`
// rays (key -> sort -> k_query each, the last chunk partial), an unsorted one
// in a single launch over all n.  `resident`: blocks the device holds at once
// (the occupancy grid); `grid_cap`: option query_grid (0: none).  The overflow
// stacks are sized by the launched grid, the sort buffers by the largest chunk.
struct QueryPlan {
    int64_t chunks;      // launches of k_query
    int64_t chunk_n;     // rays of every chunk but the last
    int64_t last_n;      // rays of the last chunk
    int32_t grid;        // blocks of the largest launch
    uint64_t ovf_bytes, sort_bytes, hist_words;
};

constexpr int kQueryBlock = 256;         // == kBlk (tmpt_render.h)
constexpr int64_t kQueryChunkMax = 1 << 22;

inline QueryPlan query_plan(int64_t n, bool sorted, int64_t chunk, int64_t grid_cap, int64_t resident,
                            int64_t ovf_words_per_lane, size_t (*hist_words)(int32_t) = nullptr)
{
    QueryPlan p{};
    if (n <= 0) return p;
    chunk = chunk < 64 ? 64 : (chunk > kQueryChunkMax ? kQueryChunkMax : chunk);
    p.chunk_n = sorted ? (n < chunk ? n : chunk) : n;
    p.chunks = sorted ? (n + chunk - 1) / chunk : 1;
    p.last_n = n - (p.chunks - 1) * p.chunk_n;
    int64_t grid = (p.chunk_n + kQueryBlock - 1) / kQueryBlock;
    if (resident < 1) resident = 1;
    if (grid > resident) grid = resident;
    if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
    p.grid = (int32_t)(grid < 1 ? 1 : grid);
    p.ovf_bytes = (uint64_t)p.grid * kQueryBlock * (uint64_t)ovf_words_per_lane * sizeof(uint32_t);
    if (sorted) {
        p.hist_words = hist_words ? (uint64_t)hist_words((int32_t)p.chunk_n) : 0;  // radix_sort_hist_words
        p.sort_bytes = 4 * (uint64_t)p.chunk_n * sizeof(uint32_t) + p.hist_words * sizeof(uint32_t);
    }
    return p;
}

}  // namespace tmpt
