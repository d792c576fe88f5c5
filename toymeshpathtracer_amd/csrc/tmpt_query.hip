// tmpt_query.hip -- device-resident batched queries (tmpt_scene_hit_device):
// k_query, the key kernel of option query_sort, and their host, query_batch.
// k_intersect (tmpt_hitscene.hip) stays the kernel of tmpt_scene_hit; the
// answers of the two are the same ray for ray (DESIGN.md section 4,
// "Device-resident queries").
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tmpt_query_key.h"
#include "tmpt_render.h"

namespace tmpt {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x2 lds_f2;
typedef __attribute__((address_space(3))) f32x4 lds_f4;

// A wave's 64 rays (S = 6 or 8 dwords each, 64 S contiguous dwords from ray
// `first`) through LDS: the wave loads them as whole dwordx4 lines (vec: the
// rays' base is 16-byte aligned; otherwise as consecutive dwords, still one
// line per instruction) and every lane reads its own ray back as S / 2
// ds_read_b64.  The staging area is the wave's own columns of the block's
// traversal stack, which is empty between two queries: dword m of the wave's
// rays lies in stack row m / 64, column 64 w + m % 64, so a 16-byte group never
// leaves its row (64 is a multiple of 4) and an even dword pair neither (S is
// even).  Banks: the b128 writes are consecutive within a row and the rows
// are 256 dwords apart, so a 16-lane group covers the 64 banks once; lane j's
// b64 read starts at dword S j + 2 p: no two lanes of a 32-lane half share a
// bank at S = 6, four do at S = 8 (j, j + 8, j + 16, j + 24), on four reads
// per query.
// Every lane of the wave must call; `valid` = the dwords of the batch from
// the wave's first ray on, at most 64 S count.  r[] takes lane j's S dwords.
template <int S, int BLOCK>
__device__ __forceinline__ void wave_load_rays(const float* __restrict__ src, int64_t valid, bool vec,
                                               uint32_t* s_stack, float (&r)[8])
{
    const int lane = lane_id();
    uint32_t* col = s_stack + (threadIdx.x & ~63u);  // the wave's columns of row 0
    const int count = valid < 64 * S ? (int)valid : 64 * S;
    if (vec) {
#pragma unroll
        for (int k = 0; k < (64 * S / 4 + 63) / 64; ++k) {
            const int i = lane + 64 * k;  // the wave's dwordx4 number i
            if (4 * i < count) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (4 * i + 4 <= count) {
                    v = reinterpret_cast<const float4*>(src)[i];
                } else {  // the batch's last, partial line (S = 6: two dwords)
                    v.x = src[4 * i];
                    if (4 * i + 1 < count) v.y = src[4 * i + 1];
                    if (4 * i + 2 < count) v.z = src[4 * i + 2];
                }
                const int m = 4 * i;
                *(lds_f4*)(col + (m >> 6) * BLOCK + (m & 63)) = (f32x4){v.x, v.y, v.z, v.w};
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int m = lane + 64 * k;
            if (m < count) ((lds_u32*)col)[(m >> 6) * BLOCK + (m & 63)] = __float_as_uint(src[m]);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int p = 0; p < S / 2; ++p) {
        const int m = S * lane + 2 * p;
        const f32x2 v = *(const lds_f2*)(col + (m >> 6) * BLOCK + (m & 63));
        r[2 * p] = v.x;
        r[2 * p + 1] = v.y;
    }
    // the reads are done before this wave's next stack push lands in the same words
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One ray gathered by its lane (a permuted batch): dwordx4 / dwordx2 loads
// where the base's alignment allows them (vec), single dwords otherwise.
template <int S>
__device__ __forceinline__ void lane_load_ray(const float* __restrict__ p, bool vec, float (&r)[8])
{
    if (vec && S == 8) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w;
    } else if (vec) {
#pragma unroll
        for (int k = 0; k < S / 2; ++k) {
            const float2 a = reinterpret_cast<const float2*>(p)[k];
            r[2 * k] = a.x, r[2 * k + 1] = a.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) r[k] = p[k];
    }
}

// What a launch of k_query or k_query_keys works on: rays [first, first +
// count) of the batch; lane slot j of it takes ray first + (perm ? perm[j] : j).
struct QueryArgs {
    const float* rays;
    const uint32_t* perm;  // the chunk's sorted order (indices within the chunk), or null: the identity
    int64_t first, count;
    float tmin, tmax;
    int32_t vec;           // rays is 16-byte aligned: the wide loads
    int32_t* ids;
    float* hits;
    float* uv;
};

// ============================================================ k_query
// Scene::HitScene over a batch, as k_intersect answers it (the root box test
// first with the octree, then traverse<>: a per-lane traversal that is a
// function of the ray alone, so the answers do not depend on the order, the
// grid or the chunking), with
//  * the wave's rays loaded as whole lines and transposed through LDS
//    (wave_load_rays), or gathered per lane under a permutation;
//  * TOPC: the top BVH4 levels in LDS, staged as k_wf_trace stages them;
//  * HITS / UV: the hit record / Moller-Trumbore's (u, v) written where the
//    ray hit, nothing where it missed.
// The any-hit form steps the traversal itself instead of calling
// traverse<true>: settle_any keeps only the octree walk's bit, and here the
// record and (u, v) of a reported hit are those of the reported triangle.
template <bool ANY, bool RANGED, bool SOA, bool NEG, bool HITS, bool UV, bool TOPC>
__global__ void __launch_bounds__(kBlk, 6) k_query(SceneView sv, QueryArgs a, uint32_t* __restrict__ ovf)
{
    constexpr int BLOCK = kBlk, SL = kSL, S = RANGED ? 8 : 6;
    __shared__ uint32_t s_stack[SL * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    if (TOPC) {  // the top BVH4 levels in LDS (as k_path, k_wf_trace)
        __shared__ uint4 s_top[TOPC ? kTopNodes * 4 : 1];
        const uint32_t ntop = (uint32_t)min(kTopNodes, sv.n_nodes4);
        const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
        for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
        __syncthreads();
        st.top = (const lds_u4*)s_top;
        st.ntop = ntop;
    }
    TravCount cnt;
    const float* rays = a.rays + (int64_t)S * a.first;
    // wave-uniform trip count: every lane of a wave takes part in the wave's load
    for (int64_t w0 = gtid - lane_id(); w0 < a.count; w0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t slot = w0 + lane_id();
        const bool live = slot < a.count;
        float r[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int64_t i = slot;
        if (a.perm == nullptr) {
            wave_load_rays<S, BLOCK>(rays + S * w0, (a.count - w0) * S, a.vec != 0, s_stack, r);
        } else if (live) {
            i = (int64_t)a.perm[slot];
            lane_load_ray<S>(rays + S * i, a.vec != 0, r);
        }
        if (!live) continue;
        i += a.first;
        const f3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
        const float t0 = RANGED ? r[6] : a.tmin, t1 = RANGED ? r[7] : a.tmax;
        float t = t1, u = 0.0f, v = 0.0f;
        int id = -1;
        // with the reference's octree: its root box test first (scene.cpp:25)
        if (sv.oct && !octree_root_hit(sv, o, d, t0, t1)) {
            atomicAdd(&sv.oct->ties[1], 1ull);
        } else if (!ANY) {
            id = traverse<false, false, BLOCK, SL, TOPC, SOA, NEG>(sv, make_trav_ray(o, d), t0, t1, t, u, v, st, cnt);
        } else if (sv.n > 0 && !ray_has_nan(o, d)) {
            const TravRay tr = make_trav_ray(o, d);
            TravState ts;
            trav_init(ts, t1);
            const float tlo = fminf(t0, 0.0f);
            while (!trav_step4q2_mixed<false, BLOCK, SL, TOPC, 0, SOA, NEG>(sv, tr, true, ts, st, cnt, tlo, t0, t1)) {
            }
            if (octree_flag(sv, tr, ts)) {  // settle_any, keeping the walk's (t, u, v) with its triangle
                octree_count(sv.oct, ts.best);
                ts.best = octree_closest(sv, o, d, t0, t1, -INFINITY, ts.bt, ts.bu, ts.bv);
            } else {
                ts.best >>= 1;
            }
            id = ts.best, t = ts.bt, u = ts.bu, v = ts.bv;
        }
        a.ids[i] = id;
        if (id >= 0) {
            if (HITS) {
                f3 pos, nrm;
                hit_record(sv, id, u, v, pos, nrm);
                float* h = a.hits + 7 * i;
                h[0] = pos.x; h[1] = pos.y; h[2] = pos.z;
                h[3] = nrm.x; h[4] = nrm.y; h[5] = nrm.z;
                h[6] = t;
            }
            if (UV) {
                a.uv[2 * i] = u;
                a.uv[2 * i + 1] = v;
            }
        }
    }
}

// ============================================================ the key kernel
// keys[j] = query_key of ray first + j, vals[j] = j, for the chunk's count rays;
// the rays loaded as k_query loads them.  box: the BVH's root box on the device.
template <bool RANGED>
__global__ void __launch_bounds__(kBlk) k_query_keys(QueryArgs a, const float* __restrict__ box,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    constexpr int BLOCK = kBlk, S = RANGED ? 8 : 6;
    __shared__ uint32_t s_stage[8 * BLOCK];  // rows 0..7 of wave_load_rays' layout (64 S <= 512 dwords per wave)
    const int64_t w0 = (int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63u);
    if (w0 >= a.count) return;  // wave-uniform
    float bx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) bx[k] = box[k];
    float r[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    wave_load_rays<S, BLOCK>(a.rays + S * (a.first + w0), (a.count - w0) * S, a.vec != 0, s_stage, r);
    const int64_t j = w0 + lane_id();
    if (j < a.count) {
        keys[j] = query_key(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), bx);
        vals[j] = (uint32_t)j;
    }
}

// ============================================================ host
namespace {

typedef void (*QueryFn)(SceneView, QueryArgs, uint32_t*);

template <bool ANY, bool RANGED, bool SOA, bool NEG, bool TOPC>
QueryFn pick_out(bool hits, bool uv)
{
    return hits ? (uv ? k_query<ANY, RANGED, SOA, NEG, true, true, TOPC> : k_query<ANY, RANGED, SOA, NEG, true, false, TOPC>)
                : (uv ? k_query<ANY, RANGED, SOA, NEG, false, true, TOPC> : k_query<ANY, RANGED, SOA, NEG, false, false, TOPC>);
}

template <bool ANY, bool SOA, bool TOPC>
QueryFn pick_range(bool ranged, bool neg1, bool hits, bool uv)
{
    // every per-ray range takes the NEG slack, a single range only when it starts behind the origin
    return ranged ? pick_out<ANY, true, SOA, true, TOPC>(hits, uv)
                  : neg1 ? pick_out<ANY, false, SOA, true, TOPC>(hits, uv) : pick_out<ANY, false, SOA, false, TOPC>(hits, uv);
}

template <bool ANY>
QueryFn pick_scene(bool soa, bool top, bool ranged, bool neg1, bool hits, bool uv)
{
    return soa ? (top ? pick_range<ANY, true, true>(ranged, neg1, hits, uv) : pick_range<ANY, true, false>(ranged, neg1, hits, uv))
               : (top ? pick_range<ANY, false, true>(ranged, neg1, hits, uv)
                      : pick_range<ANY, false, false>(ranged, neg1, hits, uv));
}

}  // namespace

// TMPT_FLAG_WAIT_STREAM: the scene's stream waits for the work enqueued on the caller's (wait_caller_stream)
int query_wait(Scene& s, uint64_t wait_stream)
{
    TMPT_HIP(s.wait_ev.ensure(hipEventDisableTiming));
    hipError_t e = hipEventRecord(s.wait_ev, reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(wait_stream)));
    if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, s.wait_ev, 0);
    if (e != hipSuccess) {
        set_error(std::string("tmpt_scene_hit_device: wait_stream: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// rays [n x 6 | n x 8], ids, hits (or null), uv (or null): device pointers;
// wait: the work starts after the caller's wait_stream.
// 0; -12: the scratch does not fit under option query_max (nothing changed,
// nothing created); -1: a HIP error.  Returns with the work complete on the device.
int query_batch(Scene& s, const float* d_rays, int64_t n, float tmin, float tmax, bool any, bool ranged,
                int32_t* d_ids, float* d_hits, float* d_uv, bool wait, uint64_t wait_stream)
{
    const Options& o = s.opt;
    const bool sorted = o.query_sort >= 0 ? o.query_sort != 0 : (kQuerySortMinN > 0 && n >= kQuerySortMinN);
    const bool top = o.query_top >= 0 ? o.query_top != 0 : kQueryTopDefault != 0;
    const bool soa = s.bvh.soa.na != nullptr;
    const bool neg1 = !ranged && tmin < 0.0f;
    const QueryFn fn = any ? pick_scene<true>(soa, top, ranged, neg1, d_hits != nullptr, d_uv != nullptr)
                           : pick_scene<false>(soa, top, ranged, neg1, d_hits != nullptr, d_uv != nullptr);
    const int resident = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    const QueryPlan p = query_plan(n, sorted, o.query_chunk, o.query_grid, resident, kStackTotal - kSL,
                                   radix_sort_hist_words);
    // the scene's query scratch: overflow stacks, then keys, vals and their ping-pong pair, then the histogram
    const size_t need = (size_t)p.ovf_bytes + (size_t)p.sort_bytes;
    if (s.query_buf.bytes() < need) {
        const size_t cap = o.query_max > 0.0 ? (size_t)std::min(o.query_max, 1e18) : free_budget(1, 2, s.query_buf.bytes());
        if (need > cap) {
            set_error("tmpt_scene_hit_device: the query scratch (" + std::to_string(need) + " bytes) does not fit under "
                      "query_max (" + std::to_string(cap) + " bytes)");
            return -12;
        }
        if (!s.query_buf.reserve(need)) {
            set_error("tmpt_scene_hit_device: out of device memory (query scratch)");
            return -12;
        }
    }
    if (wait && query_wait(s, wait_stream)) return -1;
    s.row_render = s.pixel_render = false;
    if (ensure_counters(s)) return -1;
    for (auto& e : s.query_ev) TMPT_HIP(e.ensure());
    const size_t timed = sorted ? (size_t)std::min<int64_t>(p.chunks, kQuerySortTimed) : 0;
    if (s.query_sort_ev.size() < 2 * timed) s.query_sort_ev.resize(2 * timed);
    for (size_t k = 0; k < 2 * timed; ++k) TMPT_HIP(s.query_sort_ev[k].ensure());
    TMPT_HIP(hipEventRecord(s.query_ev[0], s.stream));
    TMPT_HIP(hipMemsetAsync(s.ties, 0, 2 * sizeof(unsigned long long), s.stream));
    TMPT_HIP(hipMemsetAsync(s.counters + kCrackCounter, 0, sizeof(unsigned long long), s.stream));
    uint32_t* ovf = s.query_buf.as<uint32_t>();
    uint32_t* sortb = ovf + p.ovf_bytes / sizeof(uint32_t);
    QueryArgs a{d_rays, nullptr, 0, n, tmin, tmax, (reinterpret_cast<uintptr_t>(d_rays) & 15u) == 0 ? 1 : 0,
                d_ids, d_hits, d_uv};
    const int64_t stride = ranged ? 8 : 6;
    const SceneView sv = view(s);
    if (!sorted) {
        fn<<<p.grid, kBlk, 0, s.stream>>>(sv, a, ovf);
        TMPT_HIP(hipGetLastError());
    } else {
        for (int64_t c = 0; c < p.chunks; ++c) {  // back to back on the stream, no host wait between them
            a.first = c * p.chunk_n;
            a.count = c + 1 == p.chunks ? p.last_n : p.chunk_n;
            a.perm = nullptr;
            a.vec = (reinterpret_cast<uintptr_t>(d_rays + stride * a.first) & 15u) == 0 ? 1 : 0;  // this chunk's base
            const size_t cn = (size_t)p.chunk_n;
            uint32_t *keys = sortb, *vals = sortb + cn, *tkeys = sortb + 2 * cn, *tvals = sortb + 3 * cn;
            if ((size_t)c < timed) TMPT_HIP(hipEventRecord(s.query_sort_ev[2 * c], s.stream));
            const int kb = (int)((a.count + kBlk - 1) / kBlk);
            if (ranged) k_query_keys<true><<<kb, kBlk, 0, s.stream>>>(a, s.bvh.node_box, keys, vals);
            else k_query_keys<false><<<kb, kBlk, 0, s.stream>>>(a, s.bvh.node_box, keys, vals);
            TMPT_HIP(hipGetLastError());
            const int which = radix_sort_pairs(keys, vals, tkeys, tvals, (int32_t)a.count, kQueryKeyBits, sortb + 4 * cn,
                                               s.stream);
            TMPT_HIP(hipGetLastError());
            if ((size_t)c < timed) TMPT_HIP(hipEventRecord(s.query_sort_ev[2 * c + 1], s.stream));
            a.perm = which ? tvals : vals;
            const int grid = (int)std::min<int64_t>(p.grid, (a.count + kBlk - 1) / kBlk);
            fn<<<grid, kBlk, 0, s.stream>>>(sv, a, ovf);
            TMPT_HIP(hipGetLastError());
        }
    }
    TMPT_HIP(hipMemcpyAsync(s.counters_host + kTieCounter, s.ties, 2 * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, s.stream));
    TMPT_HIP(hipMemcpyAsync(s.counters_host + kCrackCounter, s.counters + kCrackCounter, sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, s.stream));
    TMPT_HIP(hipEventRecord(s.query_ev[1], s.stream));
    TMPT_HIP(hipStreamSynchronize(s.stream));
    s.tie_queries = s.counters_host[kTieCounter];
    s.root_misses = s.counters_host[kTieCounter + 1];
    s.crack_queries = s.counters_host[kCrackCounter];
    float ms = 0.0f;
    TMPT_HIP(hipEventElapsedTime(&ms, s.query_ev[0], s.query_ev[1]));
    s.query_ms = ms;
    double sort_ms = 0.0;
    for (size_t k = 0; k < timed; ++k) {
        TMPT_HIP(hipEventElapsedTime(&ms, s.query_sort_ev[2 * k], s.query_sort_ev[2 * k + 1]));
        sort_ms += ms;
    }
    // beyond kQuerySortTimed chunks: the timed chunks' mean for the rest
    s.query_sort_ms = timed ? sort_ms * (double)p.chunks / (double)timed : 0.0;
    s.query_chunks = p.chunks;
    s.query_sorted = sorted ? 1 : 0;
    return 0;
}

}  // namespace tmpt
