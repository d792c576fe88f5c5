// tmpt_render.hip -- the path tracer of main.cpp:44-119 / 172-246 on gfx950:
// the persistent path engine (k_path and its variants, render_persistent) and
// the host side of a render call (render(), which tmpt_api.cpp calls).  The
// row engines launch k_path's row variants from tmpt_rows.hip, through the
// contract in tmpt_path.h.  The megakernel, the wavefront engine and the
// batched HitScene have units of their own too (tmpt_mega.hip,
// tmpt_wavefront.hip, tmpt_hitscene.hip; tmpt_render.h).
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "tmpt_lane_path.h"
#include "tmpt_path.h"

namespace tmpt {

#ifdef TMPT_EXP_WAVETIME  // the timeline experiment's arrays (kWaveTimeMax: tmpt_path.h)
__device__ unsigned long long g_wavetime[3 * kWaveTimeMax];
__device__ unsigned long long g_rowtime[kWaveTimeMax];  // streaming row engine: when each row's chain ended
__device__ unsigned long long g_claimtime[kWaveTimeMax];  // streaming row engine: each worker wave's last claim
// their copies to and from the host (tmpt_path.h)
bool wavetime_get(unsigned long long* w)
{
    return hipMemcpyFromSymbol(w, HIP_SYMBOL(g_wavetime), 3 * kWaveTimeMax * 8) == hipSuccess;
}
bool rowtime_get(unsigned long long* r, unsigned long long* cl)
{
    return hipMemcpyFromSymbol(r, HIP_SYMBOL(g_rowtime), kWaveTimeMax * 8) == hipSuccess &&
           hipMemcpyFromSymbol(cl, HIP_SYMBOL(g_claimtime), kWaveTimeMax * 8) == hipSuccess;
}
void wavetime_put(const unsigned long long* w)
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wavetime), w, 3 * kWaveTimeMax * 8);
}
void rowtime_put(const unsigned long long* r)
{
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rowtime), r, kWaveTimeMax * 8);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_claimtime), r, kWaveTimeMax * 8);
}
#endif

// ============================================================ octree walk, one wave
__device__ __forceinline__ float rlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int rlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// octree_walk (tmpt_traverse.h) for ONE query, run by the whole wave (every
// lane active, every argument wave-uniform): the lanes test the slab of 64
// consecutive preorder nodes at once and the DFS then steps through that
// window on scalar masks (a failed node jumps to its skip link, a passed one
// to the next node), so a window costs one memory round trip instead of one
// per node; a visited leaf's triangles are tested one per lane, and the leaf
// keeps what the serial scan would: the first triangle at the leaf's least t
// when that t beats the best so far (strict <, scene.cpp:34).  The walk
// stops at the first triangle at `target` (nothing is nearer).  The
// reference visits ~100 nodes per tied query on the bench frame (up to ~950:
// profiles/r04_ties/walkstat_n1.log).
__device__ __forceinline__ OctHit octree_walk_wave(const OctNode* __restrict__ nodes, const int32_t* __restrict__ refs,
                                                   int n_oct, const TriOrig* __restrict__ tris, f3 o, f3 d,
                                                   float tmin, float tmax, float target TMPT_CHK_PARAMS)
{
    const f3 inv = ref_inverse(d);
    const int lane = lane_id();
    OctHit h{-1, tmax, 0.0f, 0.0f};
    int i = 0;
    while (i < n_oct) {
        const int j = i + lane;
        bool pass = false;
        int skip = 0, ref = -1;
        if (j < n_oct) {
            const float4 lo = nodes[j].lo, hi = nodes[j].hi;
            pass = ref_slab(o, inv, lo, hi, tmin, tmax);
            skip = __float_as_int(lo.w);
            ref = __float_as_int(hi.w);
        }
        const uint64_t P = wballot(pass), L = wballot(pass && ref >= 0);
        int cur = i;
        const int end = min(i + 64, n_oct);
        while (cur < end) {
            const int k = cur - i;
            if (((P >> k) & 1ull) == 0) {
                const int sk = rlane(skip, k);
                if (TMPT_CHK(chk, sk > cur && sk <= n_oct, kChkOctSkip, sk)) return h;
                cur = sk;
                continue;
            }
            if ((L >> k) & 1ull) {
                const int r = rlane(ref, k);
                if (TMPT_CHK(chk, (int64_t)r < n_refs && (int64_t)r + refs[r] < n_refs, kChkOctRef, r)) return h;
                const int cnt = refs[r];
                for (int b = 0; b < cnt; b += 64) {
                    float t = INFINITY, u = 0.0f, v = 0.0f;
                    int id = -1;
                    bool ok = false;
                    if (b + lane < cnt) {
                        id = refs[r + 1 + b + lane];
                        if (TMPT_CHK(chk, (uint32_t)id < (uint32_t)n_tri, kChkTri, id)) id = 0;
                        const float4* p = reinterpret_cast<const float4*>(tris + id);
                        const float4 a = p[0], bb = p[1], c = p[2];
                        const f3 v0 = mk(a.x, a.y, a.z), v1 = mk(a.w, bb.x, bb.y), v2 = mk(bb.z, bb.w, c.x);
                        ok = mt_test(o, d, v0, v1 - v0, v2 - v0, tmin, tmax, t, u, v);
                    }
                    float m = ok ? t : INFINITY;
                    for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off));
                    const float mt = rlane(m, 0);
                    if (mt < h.t) {
                        const int f = (int)__builtin_ctzll(wballot(ok && t == mt));
                        h = OctHit{rlane(id, f), mt, rlane(u, f), rlane(v, f)};
                        if (mt == target) return h;
                    }
                }
            }
            ++cur;  // a leaf's skip link is the next node; an inner node descends to child 0
        }
        i = cur;
    }
    return h;
}

// ============================================================ deferred ties
// A sample the deferring sample kernel (k_path DEFER) dropped on a flagged
// closest hit is traced again from that query on by one lane, ties settled
// (trace_path's queries end in settle_closest).  The drop records where the
// path stopped -- the query's ray, the RNG state, its depth and the light
// terms of the bounces before it (redo_state_put) -- so the re-trace resumes
// there instead of restarting the sample; its colour goes
// to the colour buffer, where k_resolve_px sums it in sample order.  The list
// entry is (pixel, sample | depth << 16).
constexpr uint32_t kRedoEmpty = 0xFFFFFFFFu;  // a list entry not yet written
constexpr uint32_t kRedoDone = 0xFFFFFFFEu;   // an entry already traced
constexpr int kRedoTaken = 27, kRedoWaves = 28, kRedoTraced = 29;  // counters[]: tickets, waves past the main loop, traced
constexpr int kRedoState4 = 5;  // float4 per slot: o.xyz rng, d.xyz -, light[0..9], -, -
static_assert(2 * 4 + kMaxDepth <= 4 * kRedoState4, "redo state slot too small");

// the state words go out write-through (agent scope: another XCD's lane reads
// them), before the entry that publishes them (release fence in the caller)
__device__ __forceinline__ void redo_state_put(float4* ps, f3 o, f3 d, uint32_t rng, const float* light, uint32_t depth,
                                               uint32_t ls)
{
    float* w = reinterpret_cast<float*>(ps);
    const float h[8] = {o.x, o.y, o.z, __uint_as_float(rng), d.x, d.y, d.z, 0.0f};
#pragma unroll
    for (int i = 0; i < 7; ++i) __hip_atomic_store(&w[i], h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t i = 0; i < depth; ++i)
        __hip_atomic_store(&w[8 + i], light[i * ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The shadow split's sample record (tmpt_path.h SplitRec) of a finished path:
// its end colour and depth, and the light cosines of its bounces from the
// lane's LDS slots (stride ls), a 16-byte quarter only where the depth reaches
// it.  Nontemporal: the records stream through once.
__device__ __forceinline__ void split_rec_put(float4* rec, f3 end, uint32_t depth, const float* light, uint32_t ls)
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4* q = reinterpret_cast<f32x4*>(rec);
    __builtin_nontemporal_store((f32x4){end.x, end.y, end.z, __uint_as_float(depth)}, q);
    if (depth > 0u)
        __builtin_nontemporal_store((f32x4){light[0], light[ls], light[2 * ls], light[3 * ls]}, q + 1);
    if (depth > 4u)
        __builtin_nontemporal_store((f32x4){light[4 * ls], light[5 * ls], light[6 * ls], light[7 * ls]}, q + 2);
    if (depth > 8u) __builtin_nontemporal_store((f32x4){light[8 * ls], light[9 * ls], 0.0f, 0.0f}, q + 3);
}

// srec (the shadow split): the re-trace leaves the sample's record there, not
// a colour in sbuf.  The bounces before the dropped query keep the cosines the
// drop recorded (their shadow queries are in the queue); the re-trace answers
// the later bounces' shadow queries itself, so k_shadow and it together leave
// the cosines the fused kernel would have used.
template <int BLOCK, int SL>
__device__ __forceinline__ void redo_sample(const SceneView& sv, const RenderArgs& a, uint32_t pix, uint32_t smp_depth,
                                            const float4* __restrict__ ps, float4* __restrict__ sbuf, uint32_t sb_ss,
                                            uint32_t sb_sp, uint32_t& rays_e, uint32_t& rays_s,
                                            TravStack<BLOCK, SL>& st, float* lbuf, float4* __restrict__ srec = nullptr)
{
    const uint32_t smp = smp_depth & 0xFFFFu, depth = smp_depth >> 16;
    const float* w = reinterpret_cast<const float*>(ps);
    float h[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) h[i] = __hip_atomic_load(&w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t i = 0; i < depth; ++i)
        lbuf[i * BLOCK] = __hip_atomic_load(&w[8 + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t rng = __float_as_uint(h[3]);
    TravCount cnt;
    if (srec) {
        int end_depth = 0;
        const f3 e = trace_path<false, BLOCK, SL, true, false>(sv, mk(h[0], h[1], h[2]), mk(h[4], h[5], h[6]), rng,
                                                               rays_e, rays_s, st, lbuf, cnt, false, (int)depth,
                                                               &end_depth);
        const uint32_t cnt_smp = (uint32_t)(a.smp_end - a.smp_begin);
        split_rec_put(srec + 4 * ((size_t)pix * cnt_smp + (smp - (uint32_t)a.smp_begin)), e, (uint32_t)end_depth, lbuf,
                      BLOCK);
        return;
    }
    const f3 c = trace_path<false, BLOCK, SL, true, false>(sv, mk(h[0], h[1], h[2]), mk(h[4], h[5], h[6]), rng, rays_e,
                                                           rays_s, st, lbuf, cnt, false, (int)depth);
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store((f32x4){c.x, c.y, c.z, 0.0f},
                                reinterpret_cast<f32x4*>(sbuf + ((size_t)smp * sb_ss + (size_t)pix * sb_sp)));
}

__device__ __forceinline__ uint2 redo_load(const uint2* p)
{
    const unsigned long long w =
        __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_uint2((uint32_t)w, (uint32_t)(w >> 32));
}

__device__ __forceinline__ void redo_put(uint2* p, uint32_t pix, uint32_t smp_depth)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), ((unsigned long long)smp_depth << 32) | pix,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void redo_mark(uint2* p)
{
    __hip_atomic_store(reinterpret_cast<unsigned int*>(p), kRedoDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The entries the deferring launch left untraced (its waves gave up waiting,
// see k_path's redo phase): one lane per entry, grid-stride.
// SPLIT (the shadow split): sbuf is the sample records (PathCtl::srec).
template <int BLOCK, int SL, bool SPLIT = false>
__global__ void __launch_bounds__(BLOCK) k_redo(SceneView sv, RenderArgs a, uint2* __restrict__ list, uint32_t cap,
                                                const float4* __restrict__ state, float4* __restrict__ sbuf,
                                                uint32_t sb_ss, uint32_t sb_sp,
                                                uint32_t* __restrict__ ovf, unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    __shared__ float s_light[kMaxDepth * BLOCK];
    __shared__ uint4 s_top[kTopNodes * 4];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    const uint32_t ntop = (uint32_t)min(kTopNodes, sv.n_nodes4);
    const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
    for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
    __syncthreads();
    st.top = (const lds_u4*)s_top;
    st.ntop = ntop;
    const uint32_t n = (uint32_t)min(counters[kRedoCounter], (unsigned long long)cap);
    uint32_t rays_e = 0, rays_s = 0;
    for (uint32_t i = (uint32_t)gtid; i < n; i += gridDim.x * BLOCK) {
        const uint2 e = list[i];
        if (e.x >= kRedoDone) continue;
        redo_sample<BLOCK, SL>(sv, a, e.x, e.y, state + (size_t)i * kRedoState4, sbuf, sb_ss, sb_sp, rays_e, rays_s,
                               st, &s_light[threadIdx.x], SPLIT ? sbuf : nullptr);
    }
    const uint32_t re = wave_sum(rays_e), rs = wave_sum(rays_s);
    if (lane_id() == 0 && re + rs) {
        atomicAdd(&counters[0], (unsigned long long)(re + rs));
        atomicAdd(&counters[3], (unsigned long long)re);
        atomicAdd(&counters[kRedoRaysCounter], (unsigned long long)(re + rs));
    }
}

// the deferred-tie list and its per-slot state (freed together)
static void free_redo(Scene& s)
{
    s.redo.reset();
    s.redo_state.reset();
    s.redo_cap = 0;
}
static bool alloc_redo(Scene& s, int64_t cap)
{
    free_redo(s);
    if (!s.redo.alloc(sizeof(uint2) * (size_t)cap) ||
        !s.redo_state.alloc(sizeof(float4) * kRedoState4 * (size_t)cap)) {
        free_redo(s);
        return false;
    }
    s.redo_cap = (uint32_t)cap;
    return true;
}

// ============================================================ persistent path engine
// One persistent kernel per frame.  Every lane owns one pixel at a time and
// runs its whole sample sequence (the RNG stream threads through the samples,
// main.cpp:204-218); the extend / shadow / shade stages of the wavefront
// engine become per-lane states scheduled inside the wave:
//   * traversal rounds: lanes with a query in flight (closest hit or shadow,
//     mixed) take STEPS steps; each step runs only the kind (inner node or
//     leaf) that more lanes are waiting for;
//   * shading rounds: once >= SHADE_MIN lanes have a finished query (or none is
//     traversing), those lanes shade (Scatter / sky / backward recurrence /
//     next camera sample / pixel write) and idle lanes take new pixels, a
//     64-pixel reservation per atomic on segmented heads.
// No per-bounce grid-wide synchronisation and no path state in HBM: light
// scalars and the pending bounce ray live in LDS.
// Pixel supply: the tile's pixel ranks are cut into chunks of kChunk;
// segment s owns chunks s, s+kSeg, s+2kSeg, ... and its head counts the
// chunks taken, so all segments together hand out ranks in increasing order
// (the waves walk segments from their own one, one atomic per chunk).  Rank r
// is pixel order[r] (a cost-descending order from a pilot pass) or r itself.

constexpr uint32_t kSimdKeys = 8u * 8u * 2u * 16u * 4u;  // XCC x SE x SH x CU x SIMD (HW_ID fields)

// Rank of this wave among the waves resident on its SIMD -- its hardware wave
// slot, which the dispatcher fills oldest first, so rank 0 is the wave the
// SIMD's arbiter favours (oldest first) -- and the SIMD's dense registration
// index (PathCtl::simd_reg).  Lane 0 registers; the first wave of a SIMD to
// arrive draws the dense index and publishes it, later ones wait for it (it
// is already running: it won the claim before them).
__device__ __forceinline__ uint2 simd_rank(uint32_t* reg)
{
    uint32_t r = 0, d = 0;
    if (lane_id() == 0) {
        const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_ID
        const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 7u;  // XCC_ID
        const uint32_t key = ((((xcc * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u +
                               ((hw >> 8) & 15u)) * 4u) + ((hw >> 4) & 3u);
        r = hw & 15u;  // wave slot
        if (atomicAdd(&reg[2 * key], 1u) == 0) {
            d = atomicAdd(&reg[2 * kSimdKeys], 1u);
            __hip_atomic_store(&reg[2 * key + 1], d + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            uint32_t v;
            while ((v = __hip_atomic_load(&reg[2 * key + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
                __builtin_amdgcn_s_sleep(2);
            d = v - 1u;
        }
    }
    return make_uint2((uint32_t)__shfl((int)r, 0), (uint32_t)__shfl((int)d, 0));
}

__device__ __forceinline__ unsigned long long rss_ld(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t rss_ld32(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long rss_win(uint32_t p, uint32_t q, uint32_t hi)
{
    return ((unsigned long long)(p + 1u) << 48) | ((unsigned long long)q << 24) | hi;
}

// The chaser of render_rowstream: lane = row.  Walks the row's chain through
// the finished units (k_rs_chase's walk, main.cpp:209-219), records each chain
// sample's offset, plans pixel windows ahead (k_rs_plan's placement: pixel x + i
// expected i - 1 pixels after the current pixel's expected end, +- spread *
// sqrt(i) pixels) and, when the chain needs an offset no window covers, opens
// it (the demand window for a start before the current window, an extension
// past its end).  Exits when its rows are done or the launch aborts.
template <int BLOCK>
__device__ void rss_chaser(const RenderArgs& a, const RsStream& S, int wave)
{
    const int row = wave * 64 + lane_id();
    const bool mine = row < S.nrows;
    const uint32_t W = (uint32_t)a.W, spp = (uint32_t)a.spp, T = (uint32_t)kRssT;
    uint32_t c = 0, x = 0, k = 0, pdraws = 0, rays = 0, erays = 0, planned = 0;
    uint32_t n_wait = 0, n_ext = 0, n_pre = 0, n_sweep = 0;  // statistics (ctl[8..11])
    uint32_t stuck = 0;  // sweeps the chain has waited at the same (x, c)
    float mean = 17.0f;  // draws per sample before any is seen (k_rs_init)
    float spread = S.spread;
    uint32_t nw = (uint32_t)S.nw;
    bool done = !mine, err = false;
    unsigned long long* slot = S.slots + (size_t)(mine ? row : 0) * (T + 1u);
    uint32_t* lo = S.lo + (size_t)(mine ? row : 0) * T;
    const unsigned long long* res = S.res + (size_t)(mine ? row : 0) * T * S.R;
    const uint32_t cap_span = S.R - 64u;  // live offsets ahead of the chain: under one ring
    // plan pixel q (> x) from the chain's position
    auto plan = [&](uint32_t q) {
        const float E = (float)spp * mean * 0.5f, rest = (float)(spp - k) * mean * 0.5f;
        const float i = (float)(q - x);
        const float P = (float)c + rest + (i - 1.0f) * E;
        const float lo_f = fmaxf((float)c, P - spread * sqrtf(i) * E);
        const float hi_f = P + E + spread * sqrtf(i + 1.0f) * E + 2.0f;
        const uint32_t l = (uint32_t)lo_f, h = min((uint32_t)hi_f, c + cap_span);
        lo[q % T] = l;
        __hip_atomic_exchange(&slot[q % T], rss_win(q, min(l, h), h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (mine) {  // the first pixel from offset 0, then the lookahead windows
        const float E = (float)spp * mean * 0.5f;
        const uint32_t h = min((uint32_t)(E + S.spread * E) + 2u, cap_span);
        lo[0] = 0;
        __hip_atomic_exchange(&slot[0], rss_win(0, 0, h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        planned = 0;
        while (planned + 1u < min(W, (uint32_t)S.nw)) plan(++planned);
    }
    for (;;) {
        bool moved = false;
        if (!done) {
            for (int it = 0; it < 64; ++it) {
                const unsigned long long w = rss_ld(res + (size_t)(x % T) * S.R + (c & S.rmask));
                if ((w >> 28) != (((unsigned long long)(x + 1u) << 24) | c)) {
                    // not finished, or no window holds (x, c): looked at once
                    // the chain has waited two sweeps (usually the unit is in flight)
                    if (++stuck < 3u) break;
                    stuck = 0;
                    const unsigned long long sw = rss_ld(&slot[x % T]);
                    const uint32_t q = (uint32_t)(sw >> 24) & kRssM24, hi = (uint32_t)sw & kRssM24;
                    const uint32_t l = lo[x % T];
                    const uint32_t rest = (uint32_t)((float)(spp - k) * mean * 0.65f) + 16u;
                    ++n_wait;
                    if (c < l) {  // the pixel starts before its window: demand [c, l)
                        ++n_pre;
                        __hip_atomic_exchange(&slot[T], rss_win(x, c, min(l, c + cap_span)), __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
                        lo[x % T] = c;
                    } else if (c >= hi) {  // past the window's end: a new window from c
                        // (everything below hi was handed out; the workers' adds
                        // past hi handed out nothing, so q restarts at c)
                        ++n_ext;
                        __hip_atomic_exchange(&slot[x % T], rss_win(x, c, c + min(rest, cap_span)),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    (void)q;
                    break;
                }
                stuck = 0;
                const uint32_t draws = (uint32_t)w & 0x3FFFu;
                rays += (uint32_t)(w >> 14) & 31u;
                erays += (uint32_t)(w >> 19) & 15u;
                pdraws += draws;
                S.list[((size_t)row * W + x) * spp + k] = c;  // sample k of pixel x: offset c
                c += draws >> 1;
                moved = true;
                if (c + cap_span >= S.jlimit) {  // offsets past the anchors (or 24-bit words): abort, fall back
                    err = true;
                    done = true;
                    break;
                }
                if (++k == spp) {  // pixel done (main.cpp:221-233 packs it in the final pass)
                    mean = (float)pdraws / (float)k;
                    k = 0;
                    pdraws = 0;
                    if (++x == W) {
                        done = true;
                        break;
                    }
                    if (S.dyn) {  // the rows still chasing set the room per row
                        const uint32_t live = (uint32_t)S.nrows - min((uint32_t)S.nrows, rss_ld32(&S.ctl[0]));
                        const float room = S.room_lanes / (float)max(live, 1u);
                        if (S.dyn & 1u)
                            nw = (uint32_t)min((int)kRssT - 1, max(2, (int)rintf(2.6f + 1.5f * __logf(fmaxf(room, 1e-3f)))));
                        if (S.dyn & 2u) spread = fminf(0.25f, fmaxf(0.0f, 0.055f * room - 0.015f));
                    }
                    while (planned + 1u < W && planned < x + nw - 1u) plan(++planned);
                }
            }
            if (moved) __hip_atomic_store(&S.chainpos[row], ((unsigned long long)x << 32) | c, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
            if (done) {
#ifdef TMPT_EXP_WAVETIME
                if (row < kWaveTimeMax) g_rowtime[row] = __builtin_amdgcn_s_memrealtime();
#endif
                S.rowrays[2 * row] = rays;
                S.rowrays[2 * row + 1] = erays;
                if (err) {
                    atomicExch(&S.ctl[3], 1u);
                    atomicExch(&S.ctl[1], 1u);
                }
                __threadfence();
                atomicAdd(&S.ctl[0], 1u);
            }
        }
        const uint64_t mv = wballot(moved);
        if (lane_id() == 0 && mv) atomicAdd(&S.ctl[2], 1u);
        ++n_sweep;
        if (!wany(!done)) break;
        if (rss_ld32(&S.ctl[1]) != 0u) break;  // aborted
        if (!mv) __builtin_amdgcn_s_sleep(8);
    }
    if (mine) {
        atomicAdd(&S.ctl[8], n_wait);
        atomicAdd(&S.ctl[9], n_ext);
        atomicAdd(&S.ctl[10], n_pre);
    }
    if (lane_id() == 0) atomicAdd(&S.ctl[11], n_sweep);
}


template <bool COUNT, int BLOCK, int SL, int STEPS, int SHADE_MIN, int OCC = 1, int TAIL = 0, int PROF = 0,
          int HELP = 0, int SAMP = 0, bool SOA = false, int TIES = 0, bool SUMS = false, int CAM = 0,
          bool LIST = false, int SPLIT = 0>
__global__ void __launch_bounds__(BLOCK, OCC) k_path(SceneView sv, RenderArgs a, PathCtl pc,
                                                uint32_t* __restrict__ out,
                                                uint32_t* __restrict__ ovf,
                                                unsigned long long* __restrict__ counters)
{
    // TIES: how closest hits tied on t are answered.  0: the leaf keeps the
    // lowest index beside the tie flag and a flagged query is re-answered over
    // the octree when there is one (else the lowest index stands); 2: the
    // octree is there (the caller guarantees it), so the leaf keeps the first
    // triangle met and only flags the tie, and the octree answers; 1 (DEFER,
    // sample seeding): as 2, but a flagged sample is dropped and traced again
    // in the redo phase -- the main loop carries no octree walk.
    constexpr bool DEFER = TIES == 1, FLAG = TIES != 0;
    // SUMS (tmpt_render_radiance, sample seeding with a pixel as one unit, no
    // colour buffer): the pixel's colour sum goes to a.prog beside the packed
    // pixel, as pixel mode's does; the instantiations tmpt_render launches have
    // SUMS false and no such store.
    static_assert(!SUMS || SAMP == 1, "SUMS: the sample kernel's float sums");
    // CAM (sample seeding, 5 waves): a sample's camera ray and the RNG state
    // after the camera's draws are the pre-pass's entry (k_cam_rays,
    // PathCtl::cam_rays) instead of the camera block's work on the few lanes
    // that start a sample in a round: no pixel decode, seed jump, disk
    // rejection loop, sqrt or divide here, no jump-table prefetch state, and
    // the Camera of RenderArgs is not read.
    static_assert(!CAM || (SAMP == 1 && OCC >= 5 && !COUNT && !SOA && !HELP), "CAM: the 5-wave sample kernels");
    // LIST (sample seeding, a pass of tmpt_render_adaptive over the pixels still
    // active): the unit decode's pixel is a position in PathCtl::order, and one
    // load turns it into the tile pixel slot (as pixel seeding's rank and the
    // row engines' pc.upix do); the colour buffer, the seed and the redo entries then
    // go by the pixel as everywhere else -- the pre-pass's entries too (CAM:
    // k_cam_rays_list leaves a listed pixel's where its slot's always are).
    static_assert(!LIST || (SAMP == 1 && !SUMS && !COUNT && !SOA && !HELP), "LIST: the plain sample kernels");
    // SPLIT (the shadow split, CAM twins): a bounce whose light cosine is > 0
    // counts its shadow ray, appends the query to PathCtl::sq for k_shadow and
    // starts the scattered ray in the same shading round; the lane never
    // traces an any-hit query, so qany is false throughout and the pending
    // ray (s_next) and the shadow branch of the shading round are not there.
    // A finished sample leaves its record (SplitRec) instead of a colour.
    static_assert(!SPLIT || (CAM && !SUMS && !LIST && PROF == 0), "SPLIT: the plain CAM sample kernels");
    // OCC 6 (6 waves per SIMD: <= 80 VGPRs, kTopNodes6 top nodes): the SPLIT
    // twins only -- without the shadow branch and the pending ray they fit
    static_assert(OCC < 6 || (SPLIT && SL == kPathSL6), "OCC 6: the shadow split's twins");
    // a SPLIT lane's queries are closest-hit queries at compile time
    constexpr int QK = SPLIT ? kQueryClosest : kQueryRuntime;
    __shared__ uint32_t s_stack[SL * BLOCK];
    // SAMP 3, 4 (shadow-free speculation): no light terms, no pending next ray
    __shared__ float s_light[SAMP >= 3 ? 1 : kMaxDepth * BLOCK];
    // OCC 5 (5 waves per SIMD, <= 32 KB of LDS per block): only the scattered
    // ray's direction is kept while its bounce's shadow query runs -- its
    // origin is the shadow ray's (r.o)
    constexpr bool NEXT3 = OCC >= 5;
    __shared__ float s_next[SAMP >= 3 || SPLIT ? 1 : (NEXT3 ? 3 : 6) * BLOCK];
    if (SAMP == 4) {
        // The chaser role goes by arrival, not by blockIdx: the first nchase
        // blocks to START take it, so every chaser is resident by construction
        // and the workers' spin on chain progress cannot wait on a block that
        // the dispatcher holds back behind them.
        __shared__ uint32_t s_ticket;
        if (threadIdx.x == 0) s_ticket = atomicAdd(&pc.rss.ctl[12], 1u);
        __syncthreads();
        const uint32_t ticket = s_ticket;
        if ((int)ticket < pc.rss.nchase) {
            if (!pc.rss.test_abort) rss_chaser<BLOCK>(a, pc.rss, (int)(ticket * (BLOCK / 64) + threadIdx.x / 64));
            return;
        }
    }
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    constexpr uint32_t LS = BLOCK;  // stride between a lane's LDS entries
    float* light = &s_light[threadIdx.x];
    float* nxt = &s_next[threadIdx.x];
    // HELP: lane ids of this round's offloading lanes, by rank (per wave)
    __shared__ uint8_t s_pair[HELP ? BLOCK : 1];
    {  // the top BVH4 levels (nodes are numbered level by level) in LDS
        // HELP: 4 nodes fewer, so s_pair keeps the block at 4 per CU
        constexpr int kTop = OCC >= 6 ? kTopNodes6 : OCC >= 5 ? kTopNodes5 : (HELP ? kTopNodes - 4 : kTopNodes);
        __shared__ uint4 s_top[kTop * 4];
        // six co-resident blocks: the block's LDS in the CU's allocation units
        // (16 B of slack for the one-word arrays' alignment)
        static_assert(OCC < 6 || (sizeof(s_stack) + sizeof(s_light) + sizeof(s_next) + sizeof(s_pair) + sizeof(s_top) + 16 +
                                  kLdsGranule - 1) / kLdsGranule * OCC <= kLdsBytes / kLdsGranule,
                      "OCC 6: six blocks' LDS must fit the CU");
        const uint32_t ntop = (uint32_t)min(kTop, sv.n_nodes4);
        const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
        for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
        __syncthreads();
        st.top = (const lds_u4*)s_top;
        st.ntop = ntop;
    }
    // SAMP: the sample kernel has none of pixel mode's pilot order, balanced
    // first chunks, priorities or progressive state; compiling them out frees
    // the scalar registers they held
    constexpr bool kFull = !SAMP;
    float dp0 = kFull ? pc.dprio[0] : 0.0f, dp1 = kFull ? pc.dprio[1] : 0.0f, dp2 = kFull ? pc.dprio[2] : 0.0f;
    if (kFull && pc.dprio_cost && pc.order && a.smp_begin > 0) {  // relative thresholds (wave-uniform)
        const float sc = (float)pc.dprio_cost[pc.order[0]] * (float)(a.smp_end - a.smp_begin) / (float)a.smp_begin;
        dp0 *= sc;
        dp1 *= sc;
        dp2 *= sc;
    }
    TravCount cnt, cnt_s;  // COUNT: closest-hit and shadow queries apart
    uint32_t rays_e = 0, rays_s = 0;
    const f3 ldir = light_dir();
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    uint32_t seg = (uint32_t)(gtid >> 6) % kSeg, walked = 0;
    uint32_t res = 0, res_end = 0;
    uint32_t q_res = 0, q_end = 0;  // SPLIT: the wave's reservation in the shadow queue
    if (SAMP == 2 || SAMP == 3) {  // the speculative row engine plans its units on the device
        pc.P = *pc.p_dev;
        pc.nchunks = (uint32_t)((pc.P + pc.chunk - 1) / pc.chunk);
    }
    bool exhausted = SAMP == 4 ? false : pc.P == 0;
    // SAMP 4: the row the wave takes units from (it moves on when that row has
    // none), the row and pixel of its reservation, the watchdog's last seen
    // chain progress and when it changed
    uint32_t crow = SAMP == 4 ? (uint32_t)((gtid >> 6) % (int64_t)max(1, pc.rss.nrows)) : 0u;
    uint32_t srow = 0, spx = 0, wd_tick = 0, n_claim = 0, n_miss = 0, n_cas = 0;  // (ctl[5..7])
    uint32_t crow_rng = (uint32_t)(gtid >> 6) * 2654435761u + 1u;
    uint64_t wd_time = 0;
    if (kFull && pc.simd_reg && !exhausted) {  // SIMD-balanced first chunk
        const uint2 rd = simd_rank(pc.simd_reg);
        if (rd.x < pc.wps && rd.y < pc.nsimd) {
            const uint32_t c = rd.x * pc.nsimd + ((rd.x & 1u) ? pc.nsimd - 1u - rd.y : rd.y);
            uint32_t got = 0;
            if (c < pc.nchunks && lane_id() == 0) got = atomicExch(&pc.claim[c], 1u) == 0u;
            if (__shfl((int)got, 0)) {
                res = c * pc.chunk;
                res_end = (uint32_t)min<int64_t>((int64_t)res + pc.chunk, pc.P);
            } else if (c < pc.nchunks && lane_id() == 0) {
                atomicAdd(&counters[21], 1ull);  // balance diagnostics: lost the claim
            }
        } else if (lane_id() == 0) {
            atomicAdd(&counters[20 + (rd.x >= pc.wps ? 2 : 3)], 1ull);  // slot beyond wps / no dense index
        }
        // a wave left without a first chunk waits ~20 us before the segment
        // supply, so it does not take a chunk another wave is about to claim
        if (res >= res_end)
            for (int k = 0; k < 6; ++k) __builtin_amdgcn_s_sleep(127);
    }
#ifdef TMPT_EXP_WAVETIME
    const int wt_id = (int)(gtid >> 6);
    if (lane_id() == 0 && wt_id < kWaveTimeMax) g_wavetime[3 * wt_id] = __builtin_amdgcn_s_memrealtime();
#endif
    bool has_pix = false, in_query = false, qany = false;
    // HELP (shadow offload to idle lanes): once the pixel supply is exhausted, a
    // lane without a pixel becomes a helper that traces another lane's shadow
    // query (Scatter's HitScene toward the light only gates that bounce's light
    // term, main.cpp:57-67: it feeds neither the RNG stream nor the path), so
    // the owner's chain goes on with the scattered ray at once.  The owner's
    // light slot holds -cosine while the answer is pending (the cosine is > 0
    // whenever a shadow query is traced); the helper writes 0 (occluded) or
    // the cosine.  A path whose slots are still pending waits (`waiting`)
    // before its backward recurrence.
    bool helper = false, waiting = false;
    uint32_t hown = 0;  // helper: owner lane << 4 | light slot
    uint32_t pix = 0, rng = 0, smp = 0, depth = 0;
    // SAMP: the four jump-table words of the next sample's seed, loaded one
    // camera phase ahead (pf_smp = the sample they belong to), so a new sample
    // does not wait for their memory round trip
    uint32_t pf0 = 0, pf1 = 0, pf2 = 0, pf3 = 0, pf_smp = 0xFFFFFFFFu, pf_pix = 0;
    // SAMP 2: the unit held, the ray counts at its start, the camera's RNG draws
    uint32_t cur_unit = 0, re0 = 0, rs0 = 0, ndraw = 0;
    bool single = false;  // SAMP 1: the unit is one sample of the frame's tail (PathCtl::ua)
    uint32_t psteps = 0;  // traversal steps of this pixel in this call (pc.cost_out)
    // COUNT: wave-uniform round statistics (node/leaf rounds and their stepping
    // lanes, shading rounds, lanes wanting shading, lanes traversing meanwhile)
    uint64_t rs_nr = 0, rs_nl = 0, rs_lr = 0, rs_ll = 0, rs_sr = 0, rs_sl = 0, rs_st = 0;
    // PROF: wave-uniform s_memtime cycles in shading rounds, node rounds, leaf rounds
    uint64_t pt_shade = 0, pt_node = 0, pt_leaf = 0, pt_t = PROF ? stamp() : 0;
    // PROF >= 2: the shading round split (pixel fetch, hit/finish shading, camera, query set-up)
    uint64_t ps_fetch = 0, ps_shade = 0, ps_cam = 0, ps_start = 0;
    // PROF >= 2: shading rounds, those whose camera block runs, the lanes in it
    uint64_t pc_sr = 0, pc_cr = 0, pc_cl = 0;
    // Top-walk rounds (pc.top_walk) and the top levels' share of the node
    // rounds, wave-uniform.  COUNT: node lane-steps on an LDS-resident node
    // (tv_n), those of them before the query's first other step (tv_lead,
    // `lead` per lane), voted node rounds with lanes on both sides of ntop /
    // on the LDS side only (tv_mix, tv_only).  COUNT or PROF: top-walk rounds
    // and their lanes (tw_r, tw_l).  PROF: cycles in top-walk rounds (pt_top),
    // voted node rounds and their cycles with a global-side lane (pn_g, pt_node_g)
    uint64_t tv_n = 0, tv_lead = 0, tv_mix = 0, tv_only = 0, tw_r = 0, tw_l = 0;
    uint64_t pt_top = 0, pt_node_g = 0, pn_g = 0, pn_all = 0;
    bool lead = false;
    f3 col = mk(0.0f, 0.0f, 0.0f);
    TravRay r;
    TravState ts;
    trav_init(ts, kMaxT);

    for (;;) {
        const bool wants = has_pix ? !in_query : (HELP && helper ? !in_query : !exhausted);
        const uint64_t need = wballot(wants);
        const uint64_t trav = wballot(in_query);
        // Sparse waves (TAIL = D > 0): a wave shades once SHADE_MIN lanes wait, or
        // -- when fewer than D*SHADE_MIN lanes still hold a pixel -- once 1/D of
        // them wait, so the last pixels of a wave (the frame's critical path at
        // low load) do not idle until every other lane's query has finished.
        int shade_min = SHADE_MIN;
        if (TAIL > 0) {
            const int act = __popcll(wballot(has_pix));
            shade_min = max(1, min(SHADE_MIN, act / TAIL));
        }
        if (need != 0 && (__popcll(need) >= shade_min || trav == 0)) {
            if (COUNT || PROF >= 3) {
                ++rs_sr;
                rs_sl += (uint64_t)__popcll(need);
                rs_st += (uint64_t)__popcll(trav);
            }
            // Each lane decides at most one next query this round; camera
            // sampling and the query set-up are emitted once, after the
            // branches, so the wave runs each at most once per round.
            bool cam = false, start = false, sany = false;
            f3 so = mk(0.0f, 0.0f, 0.0f), sd = so;
            // ---- new pixels for idle lanes (wave-uniform reservation)
            const uint64_t nopix = wballot(!has_pix && !(HELP && helper) && !exhausted);
            if (SAMP == 4 && nopix != 0 && res >= res_end && !exhausted) {
                // offsets of one pixel window, as many as the wave has idle
                // lanes (a held reservation would delay units the chain may be
                // waiting for): the row's demand window first, then its live
                // windows in pixel order.  Lane i < T reads slot i, lane T the
                // demand slot; the pick takes its offsets with one fetch-add,
                // and the word it returns says which window they belong to
                // (the chaser may have re-planned the slot meanwhile), so no
                // offset handed out is ever lost; adds past a window's end
                // hand out nothing.
                const RsStream& S = pc.rss;
                const uint32_t T = (uint32_t)kRssT;
                // a wave with lanes still tracing looks at 1 row per round, an idle one at 4
                const int natt = wany(has_pix) ? 1 : 4;
                for (int att = 0; att < natt && res >= res_end; ++att) {
                    const uint32_t x = (uint32_t)(rss_ld(&S.chainpos[crow]) >> 32);
                    bool moved_on = true;
                    if (x < (uint32_t)a.W) {
                        unsigned long long* sl = S.slots + (size_t)crow * (T + 1u);
                        const uint32_t ln = (uint32_t)lane_id();
                        unsigned long long w = 0;
                        if (ln <= T) w = rss_ld(&sl[ln]);
                        const uint32_t p1 = (uint32_t)(w >> 48), q = (uint32_t)(w >> 24) & kRssM24;
                        const uint32_t hi = (uint32_t)w & kRssM24;
                        const bool valid = ln <= T && p1 > x && p1 <= (uint32_t)a.W && q < hi;
                        // priority: demand, then the lowest pixel; key unique per lane
                        uint32_t key = valid ? (((ln == T ? 0u : p1 - x) << 5) | ln) : 0xFFFFFFFFu;
                        // (over all 64 lanes: the pick must be wave-uniform)
                        for (int off = 1; off < 64; off <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, off));
                        if (key != 0xFFFFFFFFu) {
                            moved_on = false;
                            const int pick = (int)(key & 31u);
                            uint32_t got = 0, gq = 0, gp = 0;
                            if (ln == (uint32_t)pick) {
                                const uint32_t n = min((uint32_t)__popcll(nopix), hi - q);
                                const unsigned long long old = atomicAdd(&sl[ln], (unsigned long long)n << 24);
                                const uint32_t op = (uint32_t)(old >> 48), oq = (uint32_t)(old >> 24) & kRssM24;
                                const uint32_t ohi = (uint32_t)old & kRssM24;
                                if (op != 0u && oq < ohi) {
                                    got = min(n, ohi - oq);
                                    gq = oq;
                                    gp = op - 1u;
                                }
                            }
                            got = (uint32_t)__shfl((int)got, pick);
                            if (!got) ++n_cas;
                            if (got) {
                                ++n_claim;
#ifdef TMPT_EXP_WAVETIME  // the row workers: when each wave last found speculation work
                                if (lane_id() == 0 && wt_id < kWaveTimeMax)
                                    g_claimtime[wt_id] = __builtin_amdgcn_s_memrealtime();
#endif
                                res = (uint32_t)__shfl((int)gq, pick);
                                res_end = res + got;
                                srow = crow;
                                spx = (uint32_t)__shfl((int)gp, pick);
                            }
                        }
                    }
                    if (moved_on) {  // no work there: a pseudo-random next row spreads the waves
                        ++n_miss;
                        crow_rng ^= crow_rng << 13;
                        crow_rng ^= crow_rng >> 17;
                        crow_rng ^= crow_rng << 5;
                        crow = crow_rng % (uint32_t)S.nrows;
                        // (taking the laggier of two random rows instead measured within
                        // noise: profiles/r05_experiments/row_pick2.log)
                    }
                }
                if (res >= res_end && (rss_ld32(&S.ctl[0]) >= (uint32_t)S.nrows || rss_ld32(&S.ctl[1]) != 0u))
                    exhausted = true;  // every row's chain is done (or the launch aborted)
            }
            if (nopix != 0) {
                while (SAMP != 4 && res >= res_end && !exhausted) {
                    // chunks of segment seg: seg, seg + kSeg, ...
                    const uint32_t c = seg < pc.nchunks ? (pc.nchunks - 1u - seg) / (uint32_t)kSeg + 1u : 0u;
                    uint32_t b = c;
                    if (c != 0) {
                        if (lane_id() == 0) b = atomicAdd(&pc.heads[seg * kCtr], 1u);
                        b = (uint32_t)__shfl((int)b, 0);
                    }
                    if (b < c && kFull && pc.claim) {  // taken as some wave's balanced first chunk?
                        uint32_t got = 0;
                        if (lane_id() == 0) got = atomicExch(&pc.claim[seg + b * (uint32_t)kSeg], 1u) == 0u;
                        if (!__shfl((int)got, 0)) continue;
                    }
                    if (b < c) {
                        res = (seg + b * (uint32_t)kSeg) * pc.chunk;
                        res_end = (uint32_t)min<int64_t>((int64_t)res + pc.chunk, pc.P);
                    } else {
                        seg = (seg + 1) & 63u;
                        if (++walked == kSeg) exhausted = true;
                    }
                }
                uint32_t take = min((uint32_t)__popcll(nopix), res_end - res);
                if (pc.lane_cap < 64u)  // low load: pixels spread over all resident waves
                    take = min(take, pc.lane_cap - min(pc.lane_cap, (uint32_t)__popcll(wballot(has_pix))));
                const uint32_t k = (uint32_t)__popcll(nopix & lt);
                if (!has_pix && ((nopix >> lane_id()) & 1ull) && k < take) {
                    uint32_t smp0 = (uint32_t)a.smp_begin;
                    if (SAMP == 4) {  // streaming row engine: offset res + k of pixel spx of row srow
                        cur_unit = res + k;
                        pix = srow * (uint32_t)a.W + spx;
                        re0 = rays_e;
                        rs0 = rays_s;
                    } else if (SAMP >= 2) {  // speculative row seeding: one sample from a given state
                        cur_unit = res + k;
                        // no unit arrays: the chain list's unit u is sample u % spp of tile pixel u / spp
                        pix = pc.upix ? pc.upix[cur_unit] : cur_unit / (uint32_t)a.spp;
                        if (pc.uslot) smp0 = pc.uslot[cur_unit];
                        else if (!pc.upix) smp0 = cur_unit - pix * (uint32_t)a.spp;
                        re0 = rays_e;
                        rs0 = rays_s;
                    } else if (SAMP && pc.nblk > 1) {  // sample seeding: (pixel, block) units
                        const uint32_t unit = res + k;
                        uint32_t q = unit, sub = 0u;  // block, sample within it (tail units)
                        single = unit >= pc.ua;
                        if (single) {
                            const uint32_t v = unit - pc.ua, qv = fastdiv(v, pc.div_blk);
                            q = pc.ua + qv;
                            sub = v - qv * pc.blk;
                        }
                        pix = fastdiv(q, pc.div_nblk);
                        smp0 = (q - pix * pc.nblk + pc.blk0) * pc.blk + sub;  // blk0: a progressive pass's first block
                    } else {
                        pix = (kFull && pc.order) ? pc.order[res + k] : res + k;
                    }
                    if (LIST) pix = pc.order[pix];  // list position -> tile pixel slot
                    psteps = 0;
                    has_pix = true;
                    const int lr = (int)fastdiv(pix, a.div_w);
                    const int x = (int)(pix - (uint32_t)lr * (uint32_t)a.W);
                    if (SAMP == 4) {
                        rng = rss_state(pc.rss, (int)srow, cur_unit);
                    } else if (SAMP >= 2) {
                        rng = pc.ustate[cur_unit];
                    } else if (!kFull || a.smp_begin == 0) {
                        // (CAM: every sample's state comes with its entry)
                        if (!CAM) rng = pixel_seed((uint32_t)x, (uint32_t)tile_row_to_y_fd(a, lr), (uint32_t)a.W);
                        col = mk(0.0f, 0.0f, 0.0f);
                    } else {  // progressive: continue the previous pass's stream and sum
                        const float4 pv = a.prog[pix];
                        col = mk(pv.x, pv.y, pv.z);
                        rng = __float_as_uint(pv.w);
                    }
                    smp = smp0;
                    depth = 0;
                    cam = true;
                }
                res += take;
            }
            if (HELP && helper && !in_query) {  // deliver a finished offloaded shadow query
                float* ol = &s_light[(threadIdx.x & ~63u) + (hown >> 4) + (hown & 15u) * BLOCK];
                const float v = *ol;
                *ol = ts.best >= 0 ? 0.0f : -v;
                helper = false;
            }
            if (HELP) __atomic_signal_fence(__ATOMIC_SEQ_CST);
            uint64_t ps_t = 0;
            if (PROF >= 2) {
                ps_t = stamp();
                ps_fetch += ps_t - pt_t;
            }
            // Finished closest hits flagged as ties (not DEFER): each answered
            // over the octree by the whole wave (octree_walk_wave), one after
            // another -- here, where every lane is active.  A HELP lane
            // waiting on shadow answers holds no fresh query.
            // (the row engines, SAMP >= 2, answer in the closest-hit branch
            // with the serial walk: the wave walk's registers spill there --
            // row seeding 927 -> 888 MRays/s)
            // Also the crack queries (octree_flag), and -- where the host says a
            // shadow answer can need it (PathCtl::oct_shadow: a flat triangle in
            // the scene, or a light direction that can run along a crack) --
            // finished shadow queries whose hit the reference may not see: the
            // walk's closest answer gives their hit / miss bit.
            bool settled = false;
            if (!DEFER && SAMP < 2) {
                const bool fin = has_pix && !in_query && !cam && !(HELP && waiting) && (!qany || pc.oct_shadow);
                uint64_t T = wballot(fin && octree_flag(sv, r, ts));
                if (T != 0) {
                    const OctView* ov = sv.oct;
                    do {
                        const int l = (int)__builtin_ctzll(T);
                        T &= T - 1;
                        const f3 qo = mk(rlane(r.o.x, l), rlane(r.o.y, l), rlane(r.o.z, l));
                        const f3 qd = mk(rlane(r.d.x, l), rlane(r.d.y, l), rlane(r.d.z, l));
                        const OctHit h = octree_walk_wave(ov->nodes, ov->refs, ov->n, sv.tri_orig, qo, qd, kMinT, kMaxT,
                                                          rlane(qany ? -INFINITY : ts.bt, l) TMPT_CHK_ARGS(sv));
                        if (lane_id() == l) {
                            octree_count(ov, ts.best);
                            ts.best = h.best;
                            ts.bt = h.t;
                            ts.bu = h.u;
                            ts.bv = h.v;
                            settled = true;
                        }
                    } while (T != 0);
                }
            }
            // ---- finished queries: shade
            bool finish = false, want_off = false, emit = false;
            f3 color = mk(0.0f, 0.0f, 0.0f);
            if (has_pix && !in_query && !cam) {
                if (HELP && waiting) {  // path ended, shadow answers were pending
                    finish = true;
                    if (depth < (uint32_t)kMaxDepth) color = sky(r.d);
                } else if (!qany) {  // closest hit (Trace, main.cpp:91-109)
                    // the triangle index (2 x index | tie flag in the leaves'
                    // records); a tie was answered over the octree at the top of
                    // the round, or (DEFER) drops the sample here
                    bool drop = false;
                    if (DEFER) {
                        // the deferring kernel: a tied sample is dropped here
                        // (its rays so far uncounted: depth + 1 closest-hit
                        // queries and one shadow query per earlier hit) and
                        // traced again whole by redo_sample.  It finishes at
                        // once with colour x = -1 (no path colour is negative),
                        // which the colour-buffer stores below skip.
                        drop = octree_flag(sv, r, ts);
                        if (wany(drop)) {
                            if (drop) {
                                const unsigned long long slot = atomicAdd(&counters[kRedoCounter], 1ull);
                                // write-through (sc1): a plain store would sit in this
                                // XCD's L2, unseen by a waiting lane on another XCD
                                // until evicted, and its write-back at the kernel's end
                                // could land after that lane's done-mark and undo it
                                // (k_redo then traced the sample again: rays counted
                                // twice -- MI355X_MICROARCH.md, per-XCD L2s)
                                if (slot < (unsigned long long)pc.redo_cap) {
                                    redo_state_put(pc.redo_state + (size_t)slot * kRedoState4, r.o, r.d, rng, light,
                                                   depth, LS);
                                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // state before entry
                                    redo_put(pc.redo + slot, pix, smp | (depth << 16));
                                }
                                // the re-trace counts this query again and the rest of the
                                // path; the bounces before it stay counted here
                                rays_e -= 1u;
                                depth = 0;
                                ts.best = -1;
                            }
                        }
                        ts.best >>= 1;  // -1 stays -1
                    } else if (SAMP >= 2) {
                        const bool tie = octree_flag(sv, r, ts);
                        if (wany(tie)) {
                            if (tie) settle_closest<BLOCK, SL, true, SOA, false>(sv, r, 0.0f, kMinT, kMaxT, ts, st);
                        }
                        if (!tie) ts.best >>= 1;
                    } else if (!settled) {
                        ts.best >>= 1;  // the index (a tie was answered above)
                    }
                    if (ts.best >= 0) {  // Scatter, main.cpp:44-73
                        // the hit record's loads go out first; RandomUnitVector
                        // (RNG + sincos, independent of them) runs while they are
                        // in flight -- the same draws, the same values
                        const float4* hp = reinterpret_cast<const float4*>(sv.tri_orig + ts.best);
                        float4 ha = hp[0], hb = hp[1], hc = hp[2];
                        f3 rnd = random_unit_vector(rng);
                        materialize(ha, hb, hc);
                        const f3 nrm = mk(hc.y, hc.z, hc.w);
                        const f3 pos = hit_pos(mk(ha.x, ha.y, ha.z), mk(ha.w, hb.x, hb.y), mk(hb.z, hb.w, hc.x),
                                               ts.bu, ts.bv);
                        const float lc = light_cosine(nrm, r.d);
                        if (SAMP < 3) light[depth * LS] = lc;  // zeroed if occluded
                        f3 target = pos + nrm + rnd;
                        f3 nd = normalize(target - pos);
                        ++depth;
                        if (SPLIT && lc > 0.0f) {  // queued for k_shadow from `so`; counted below
                            emit = true;
                            so = pos;  // (the kMaxDepth-th bounce starts no ray that would set it)
                        }
                        if (!SPLIT && SAMP < 3 && lc > 0.0f && !(SAMP == 2 && pc.rs_noshadow)) {
                            if (NEXT3) {
                                nxt[0] = nd.x; nxt[LS] = nd.y; nxt[2 * LS] = nd.z;
                            } else {
                                nxt[0] = pos.x; nxt[LS] = pos.y; nxt[2 * LS] = pos.z;
                                nxt[3 * LS] = nd.x; nxt[4 * LS] = nd.y; nxt[5 * LS] = nd.z;
                            }
                            start = true;  // shadow query toward the light
                            sany = true;
                            so = pos;
                            sd = ldir;
                            want_off = HELP != 0;
                        } else {  // nothing to trace (no light term)
                            // The reference still calls HitScene for the shadow ray
                            // (main.cpp:57, counted), but a surface turned away from
                            // the light adds max(0, cos) = 0 whatever it answers
                            // (main.cpp:59-67): count the query, skip the traversal.
                            ++rays_s;
                            if (depth < (uint32_t)kMaxDepth) {
                                start = true;  // the scattered ray of this bounce
                                so = pos;
                                sd = nd;
                            } else {
                                finish = true;  // kMaxDepth hits, colour stays 0 (main.cpp:88-89)
                            }
                        }
                    } else {
                        color = sky(r.d);  // main.cpp:106-107
                        if (DEFER && drop) color.x = -1.0f;
                        finish = true;
                    }
                } else if (SAMP < 3 && !SPLIT) {  // shadow query of bounce depth-1
                    if (SAMP == 2 && pc.oct_shadow && octree_flag(sv, r, ts))
                        settle_any(sv, r, kMinT, kMaxT, ts);  // the row engines' serial walk (pixel, sample: above)
                    if (ts.best >= 0) light[(depth - 1) * LS] = 0.0f;
                    if (depth < (uint32_t)kMaxDepth) {
                        start = true;  // the scattered ray of that bounce
                        if (NEXT3) {  // the shadow ray started at the hit point
                            so = r.o;
                            sd = mk(nxt[0], nxt[LS], nxt[2 * LS]);
                        } else {
                            so = mk(nxt[0], nxt[LS], nxt[2 * LS]);
                            sd = mk(nxt[3 * LS], nxt[4 * LS], nxt[5 * LS]);
                        }
                    } else {
                        finish = true;  // kMaxDepth hits, colour stays 0 (main.cpp:88-89)
                    }
                }
            }
            if (SPLIT) {  // append this round's shadow queries (the hit point is `so`)
                const uint64_t em = wballot(emit);
                if (em != 0) {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    u32x4* q = reinterpret_cast<u32x4*>(pc.sq);
                    const uint32_t ne = (uint32_t)__popcll(em);
                    if (q_end - q_res < ne) {  // a new reservation; the old one's rest stays empty
                        for (uint32_t i = q_res + (uint32_t)lane_id(); i < min(q_end, pc.sq_cap); i += 64u)
                            __builtin_nontemporal_store((u32x4){0u, 0u, 0u, kSplitEmpty}, q + i);
                        uint32_t b = 0;
                        if (lane_id() == 0) b = atomicAdd(&pc.sq_ctl[0], kSplitChunk);
                        q_res = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
                        q_end = q_res + kSplitChunk;
                    }
                    const uint32_t idx = q_res + (uint32_t)__popcll(em & lt);
                    if (emit) {
                        // the record of (pix, smp) and the bounce (depth was advanced past it)
                        const uint32_t rec = pix * pc.cam_count + (smp - (uint32_t)a.smp_begin);
                        if (idx < pc.sq_cap)
                            __builtin_nontemporal_store((u32x4){__float_as_uint(so.x), __float_as_uint(so.y),
                                                                __float_as_uint(so.z), (rec << 4) | (depth - 1u)},
                                                        q + idx);
                        else  // cannot happen (the queue holds the worst case): the render call's error
                            atomicAdd(&counters[kSplitOverflowCounter], 1ull);
                    }
                    q_res += ne;
                }
            }
            if (HELP) {  // pair lanes starting a shadow query with idle lanes
                const uint64_t S = wballot(want_off);
                // lanes left without a pixel after this round's fetch (supply
                // exhausted, or the wave's pixel cap reached) are free to help
                const uint64_t I = S ? wballot(!has_pix && !helper && !in_query) : 0ull;
                if (I != 0) {
                    const uint32_t n = min(__popcll(S), __popcll(I));
                    const uint32_t ks = (uint32_t)__popcll(S & lt), ki = (uint32_t)__popcll(I & lt);
                    const uint32_t wb = threadIdx.x & ~63u;
                    if (want_off && ks < n) s_pair[wb + ks] = (uint8_t)lane_id();
                    __atomic_signal_fence(__ATOMIC_SEQ_CST);
                    const bool idle = ((I >> lane_id()) & 1ull) != 0 && ki < n;
                    const int src = idle ? (int)s_pair[wb + ki] : (int)lane_id();
                    const float hx = __shfl(so.x, src), hy = __shfl(so.y, src), hz = __shfl(so.z, src);
                    const uint32_t hs = (uint32_t)__shfl((int)depth, src) - 1u;
                    if (want_off && ks < n) {  // offloaded: go on with the scattered ray
                        light[(depth - 1) * LS] = -light[(depth - 1) * LS];
                        sany = false;
                        if (depth < (uint32_t)kMaxDepth) {
                            sd = NEXT3 ? mk(nxt[0], nxt[LS], nxt[2 * LS]) : mk(nxt[3 * LS], nxt[4 * LS], nxt[5 * LS]);
                        } else {
                            start = false;
                            finish = true;  // kMaxDepth hits, colour stays 0 (main.cpp:88-89)
                        }
                    }
                    if (idle) {
                        helper = true;
                        hown = ((uint32_t)src << 4) | hs;
                        start = true;
                        sany = true;
                        so = mk(hx, hy, hz);
                        sd = ldir;
                    }
                }
            }
            if (finish) {
                bool pend = false;
                if (HELP)
                    for (int kk = 0; kk < (int)depth; ++kk) pend |= light[kk * LS] < 0.0f;
                waiting = pend;
                if (!pend) {
                    if (SAMP < 3 && !SPLIT)
                        for (int kk = (int)depth - 1; kk >= 0; --kk)
                            color = backward_step(color, light[kk * LS]);
                    if (SAMP == 2 && pc.sbuf) {  // a chain sample traced in full: k_resolve sums in order
                        typedef float f32x4 __attribute__((ext_vector_type(4)));
                        __builtin_nontemporal_store((f32x4){color.x, color.y, color.z, 0.0f},
                                                    reinterpret_cast<f32x4*>(pc.sbuf + ((size_t)smp * pc.sb_ss +
                                                                                        (size_t)pix * pc.sb_sp)));
                    } else if (SAMP == 4) {  // streaming row engine: the unit's word for the chaser
                        const uint32_t draws = ndraw + 2u * depth;
                        const uint32_t ne = rays_e - re0, nr = ne + rays_s - rs0;  // <= 10, <= 20
                        const uint32_t row = pix / (uint32_t)a.W, p = pix - row * (uint32_t)a.W;
                        if (draws > 0x3FFFu) atomicExch(&pc.rss.ctl[3], 2u);  // cannot happen: 8k disk tries
                        const unsigned long long word =
                            ((((unsigned long long)(p + 1u) << 24) | cur_unit) << 28) |
                            (unsigned long long)(min(draws, 0x3FFFu) | (nr << 14) | (ne << 19));
                        atomicMax(pc.rss.res + ((size_t)row * kRssT + p % kRssT) * pc.rss.R + (cur_unit & pc.rss.rmask),
                                  word);
                    } else if (SAMP >= 2) {  // speculative row seeding: render_rowspec's chase consumes it
                        // draws: the camera's, and RandomUnitVector's 2 at each of the
                        // `depth` hits (main.cpp:71, drawn at the 10th hit too)
                        const uint32_t draws = ndraw + 2u * depth;
                        const uint32_t ne = rays_e - re0, nr = ne + rays_s - rs0;  // <= 10, <= 20
                        // SAMP 3 (the shadow-free pass): no colour, the chain is traced again
                        pc.rs_out[cur_unit] =
                            make_float4(SAMP == 3 ? 0.0f : color.x, SAMP == 3 ? 0.0f : color.y, SAMP == 3 ? 0.0f : color.z,
                                        __uint_as_float(draws | (nr << 23) | (ne << 28)));
                        pc.rs_end[cur_unit] = rng;
                    } else if (SPLIT) {  // the sample's record: k_split_resolve runs the recurrence
                        // DEFER: a dropped sample's record (x = -1) is redo_sample's
                        if (!DEFER || !(color.x < 0.0f))
                            split_rec_put(pc.srec + 4 * ((size_t)pix * pc.cam_count + (smp - (uint32_t)a.smp_begin)),
                                          color, depth, light, LS);
                    } else if (SAMP && pc.sbuf) {  // sample seeding, blocks: k_resolve_px sums in sample order
                        typedef float f32x4 __attribute__((ext_vector_type(4)));
                        f32x4* dst = reinterpret_cast<f32x4*>(pc.sbuf + ((size_t)smp * pc.sb_ss + (size_t)pix * pc.sb_sp));
                        // paired stores (pc.pair): an even sample with a successor in
                        // the unit is held in `col` (unused with a colour buffer) and
                        // written with it, back to back into one 32-B sector
                        const bool odd = (smp & 1u) != 0u;
                        if (pc.pair && !odd && !single && smp + 1u < (uint32_t)a.smp_end && ((smp + 1u) & a.bmask) != 0u) {
                            col = color;
                        } else {
                            // DEFER: a dropped sample's slot (x = -1) is redo_sample's
                            if (pc.pair && odd && !single && (!DEFER || !(col.x < 0.0f)))
                                __builtin_nontemporal_store((f32x4){col.x, col.y, col.z, 0.0f}, dst - 1);
                            if (!DEFER || !(color.x < 0.0f))
                                __builtin_nontemporal_store((f32x4){color.x, color.y, color.z, 0.0f}, dst);
                        }
                    } else
                        col = col + color;
                    ++smp;
                    depth = 0;
                    if (smp < (uint32_t)a.smp_end && (!SAMP || ((smp & a.bmask) != 0u && !single))) {
                        cam = true;
                    } else {
                        if ((kFull || (SUMS && !pc.sbuf)) && a.prog)
                            a.prog[pix] = make_float4(col.x, col.y, col.z, __uint_as_float(rng));
                        if (kFull && pc.cost_out) pc.cost_out[pix] = psteps;
                        if (SAMP < 2 && (!SAMP || !pc.sbuf)) out[pix] = pack_pixel(col, a.out_recip);
                        has_pix = false;
                    }
                }
            }
            if (PROF >= 2) {
                const uint64_t t = stamp();
                ps_shade += t - ps_t;
                ps_t = t;
            }
            if (PROF >= 2) {
                const uint64_t cm = wballot(cam);
                ++pc_sr;
                if (cm != 0) {
                    ++pc_cr;
                    pc_cl += (uint64_t)__popcll(cm);
                }
            }
            uint32_t cflags = 0;  // CAM: the entry's flag word
            if (CAM && cam) {  // the pre-pass's entry for (pix, smp): ray, RNG state, flags
                // nontemporal: 4 GB per bench frame stream through once and
                // must not evict BVH nodes from L2
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4* e = reinterpret_cast<const u32x4*>(
                    pc.cam_rays + ((size_t)pix * pc.cam_count + (size_t)(smp - (uint32_t)a.smp_begin)));
                const u32x4 e0 = __builtin_nontemporal_load(e), e1 = __builtin_nontemporal_load(e + 1);
                so = mk(__uint_as_float(e0.x), __uint_as_float(e0.y), __uint_as_float(e0.z));
                sd = mk(__uint_as_float(e0.w), __uint_as_float(e1.x), __uint_as_float(e1.y));
                rng = e1.z;
                cflags = e1.w;
                start = true;
            }
            if (!CAM && cam) {  // next camera sample of this lane's pixel (main.cpp:212-216)
                const int lr = (int)fastdiv(pix, a.div_w);
                const int x = (int)(pix - (uint32_t)lr * (uint32_t)a.W);
                const uint32_t y = (uint32_t)tile_row_to_y_fd(a, lr);
                if (SAMP == 1) {
                    const uint32_t ps = pixel_seed((uint32_t)x, y, (uint32_t)a.W);
                    rng = (pf_smp == smp && pf_pix == pix) ? (pf0 ^ pf1 ^ pf2 ^ pf3) : sample_seed(a.jt, smp, ps);
                    // the block's next sample: its table words now, XORed at its start
                    const uint32_t* t = a.jt + (size_t)(smp + 1u) * 1024u;
                    const bool more = smp + 1u < (uint32_t)a.smp_end && ((smp + 1u) & a.bmask) != 0u && !single;
                    const uint32_t* tt = more ? t : a.jt;
                    pf0 = tt[ps & 255u];
                    pf1 = tt[256u + ((ps >> 8) & 255u)];
                    pf2 = tt[512u + ((ps >> 16) & 255u)];
                    pf3 = tt[768u + (ps >> 24)];
                    pf_smp = more ? smp + 1u : 0xFFFFFFFFu;
                    pf_pix = pix;
                }
                if (SAMP >= 2) {
                    ndraw = 0;
                    camera_sample(a.cam, (uint32_t)x, y, a.invW, a.invH, rng, so, sd, ndraw);
                } else {
                    camera_sample(a.cam, (uint32_t)x, y, a.invW, a.invH, rng, so, sd);
                }
                start = true;
            }
            if (PROF >= 2) {
                const uint64_t t = stamp();
                ps_cam += t - ps_t;
                ps_t = t;
            }
            if (start) {
                r = make_trav_ray(so, sd);
                trav_init(ts, kMaxT);
                qany = SPLIT ? false : sany;
                if (sany) ++rays_s; else ++rays_e;
                in_query = sv.n > 0 && !ray_has_nan(so, sd);  // NaN ray / no triangles: a counted miss
                // (CAM: the pre-pass made the root box test; its answer is the entry's flag)
                if (!DEFER && a.root_check && cam && in_query &&
                    (CAM ? (cflags & kCamRootMiss) != 0u : !octree_root_hit(sv, so, sd, kMinT, kMaxT))) {
                    in_query = false;  // a camera ray outside the reference's root box: a counted miss
                    atomicAdd(&sv.oct->ties[1], 1ull);
                }
            }
            if (PROF >= 2) ps_start += stamp() - ps_t;
            if (COUNT && start) lead = true;
            // Top-walk rounds (pc.top_walk): every query starts at node 0 and
            // its first visits are nodes of the LDS copy, but in a voted node
            // round some other lane nearly always stands on a global node, so
            // those visits wait out the global loads' latency with it.  Here
            // the lanes on an LDS-resident node -- the queries just started
            // and any lane already traversing that stands on one -- take up to
            // top_walk node rounds that hold no global load at all.  The same
            // step on the same state in the same order per lane: every answer,
            // tie flag and count is what the voted rounds alone give.  No
            // vote: every stepping lane is at a node.
            if (pc.top_walk) {
                uint64_t tw_t = 0;
                if (PROF) {
                    tw_t = stamp();
                    pt_shade += tw_t - pt_t;
                }
                for (uint32_t k = 0; k < pc.top_walk; ++k) {
                    const bool top = in_query && ts.node >= 0 && (uint32_t)ts.node < st.ntop;
                    const uint64_t tm = wballot(top);
                    if (tm == 0) break;
                    if (COUNT || PROF) {
                        ++tw_r;
                        tw_l += (uint64_t)__popcll(tm);
                    }
                    if (COUNT) {
                        tv_n += (uint64_t)__popcll(tm);
                        tv_lead += (uint64_t)__popcll(wballot(top && lead));
                    }
                    if (top) {
                        bool done;
                        if (!COUNT) {
                            done = trav_step4q2_mixed<false, BLOCK, SL, true, 1, SOA, false, FLAG, true, QK>(sv, r, qany, ts,
                                                                                                            st, cnt);
                        } else {
                            TravCount c1;
                            done = trav_step4q2_mixed<COUNT, BLOCK, SL, true, 1, SOA, false, FLAG, true>(sv, r, qany, ts, st,
                                                                                                        c1);
                            (qany ? cnt_s : cnt).nodes += c1.nodes;
                            cnt.stale += c1.stale;  // (closest-hit lanes only: an any-hit lane discards nothing)
                            cnt.stale2 += c1.stale2;
                        }
                        if (done) in_query = false;
                        if ((kFull && pc.cost_out) || dp0 > 0.0f) ++psteps;
                    }
                }
                if (PROF) {
                    pt_t = stamp();
                    pt_top += pt_t - tw_t;
                }
            }
        }
        if (dp0 > 0.0f) {  // longest remaining traversal work first (wave-uniform)
            float rem = 0.0f;
            if (has_pix)
                rem = smp > (uint32_t)a.smp_begin
                          ? (float)psteps * (float)((uint32_t)a.smp_end - smp) *
                                __builtin_amdgcn_rcpf((float)(smp - (uint32_t)a.smp_begin))
                          : 3.0e38f;
            for (int o = 32; o > 0; o >>= 1) rem = fmaxf(rem, __shfl_xor(rem, o));
            if (rem >= dp0) __builtin_amdgcn_s_setprio(3);
            else if (rem >= dp1) __builtin_amdgcn_s_setprio(2);
            else if (rem >= dp2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        if (PROF) {
            const uint64_t t = stamp();
            pt_shade += t - pt_t;
            pt_t = t;
        }
        if (!wany(in_query)) {
            if (exhausted && !wany(has_pix)) break;
            if (SAMP == 4 && !wany(has_pix)) {  // nothing to take yet: wait for the chasers
                // watchdog: no chain progress anywhere for ~1 s means the
                // chasers cannot run; abort (the host re-renders the frame
                // with render_rowspec) rather than spin forever
                const uint32_t tick = rss_ld32(&pc.rss.ctl[2]);
                const uint64_t now = __builtin_amdgcn_s_memrealtime();  // 100 MHz
                if (tick != wd_tick || wd_time == 0) {
                    wd_tick = tick;
                    wd_time = now;
                } else if (now - wd_time > (uint64_t)pc.rss.watchdog) {
                    if (lane_id() == 0) atomicExch(&pc.rss.ctl[1], 1u);
                    exhausted = true;
                }
                __builtin_amdgcn_s_sleep(32);
            }
            continue;
        }
        for (int k = 0; k < STEPS; ++k) {  // traversal rounds
            // two compares straight to lane masks (a ballot of a combined bool
            // made the compiler materialise it in a VGPR and compare again)
            const uint64_t q = wballot(in_query);
            const uint64_t at_leaf = q & wballot(ts.node < 0);
            const uint64_t at_node = q & ~at_leaf;
            if (q == 0) break;
            // 32-bit counts, so the vote stays a scalar compare (the 64-bit
            // popcount compare was widened onto the VALU)
            const uint32_t n_leaf = (uint32_t)__builtin_popcount((uint32_t)at_leaf) +
                                    (uint32_t)__builtin_popcount((uint32_t)(at_leaf >> 32));
            const uint32_t n_node = (uint32_t)__builtin_popcount((uint32_t)at_node) +
                                    (uint32_t)__builtin_popcount((uint32_t)(at_node >> 32));
            const bool leaf_round = n_leaf > n_node;
            if (COUNT || PROF >= 3) {
                if (!leaf_round) { ++rs_nr; rs_nl += (uint64_t)__popcll(at_node); }
                if (leaf_round) { ++rs_lr; rs_ll += (uint64_t)__popcll(at_leaf); }
            }
            uint64_t top_m = 0;  // COUNT / PROF: this node round's lanes on an LDS-resident node
            if ((COUNT || PROF) && !leaf_round) top_m = at_node & wballot(ts.node >= 0 && (uint32_t)ts.node < st.ntop);
            if (COUNT) {
                tv_n += (uint64_t)__popcll(top_m);
                tv_lead += (uint64_t)__popcll(top_m & wballot(lead));
                if (top_m != 0) ++((at_node & ~top_m) != 0 ? tv_mix : tv_only);
                // the lane's first step that is not on an LDS-resident node ends its leading run
                if (in_query && (ts.node < 0) == leaf_round && !((top_m >> lane_id()) & 1ull)) lead = false;
            }
            if (!COUNT) {
                // voted round: the kind is wave-uniform, so only its code runs
                // (a scalar branch instead of exec-mask splits around both)
                const bool stepping = in_query && ((ts.node < 0) == leaf_round);
                bool done = false;
                if (leaf_round) {
                    if (stepping)
                        done = trav_step4q2_mixed<false, BLOCK, SL, true, 2, SOA, false, FLAG, false, QK>(sv, r, qany, ts, st, cnt);
                } else {
                    if (stepping)
                        done = trav_step4q2_mixed<false, BLOCK, SL, true, 1, SOA, false, FLAG, false, QK>(sv, r, qany, ts, st, cnt);
                }
                if (done) in_query = false;
                if (stepping && ((kFull && pc.cost_out) || dp0 > 0.0f)) ++psteps;
            } else if (in_query && (ts.node < 0) == leaf_round) {
                TravCount c1;
                if (trav_step4q2_mixed<COUNT, BLOCK, SL, true, 0, SOA, false, FLAG>(sv, r, qany, ts, st, c1)) in_query = false;
                TravCount& dst = qany ? cnt_s : cnt;
                dst.nodes += c1.nodes;
                dst.tris += c1.tris;
                dst.stale += c1.stale;
                dst.stale2 += c1.stale2;
                if ((kFull && pc.cost_out) || dp0 > 0.0f) ++psteps;
            }
            if (PROF) {
                const uint64_t t = stamp();
                (leaf_round ? pt_leaf : pt_node) += t - pt_t;
                if (!leaf_round) {
                    ++pn_all;
                    if ((at_node & ~top_m) != 0) {
                        ++pn_g;
                        pt_node_g += t - pt_t;
                    }
                }
                pt_t = t;
            }
        }
    }
#ifdef TMPT_EXP_WAVETIME
    if (lane_id() == 0 && wt_id < kWaveTimeMax) g_wavetime[3 * wt_id + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    if (DEFER && pc.redo_inline) {
        // Redo phase: the wave's main loop is over; it traces the samples the
        // main loops dropped on ties (one per lane, by ticket), while the other
        // waves finish theirs, so the re-traces fill the frame's tail.  The
        // list is final by a completion count: a lane waits on an entry while
        // some wave of the grid is still in its main loop (kRedoWaves < waves)
        // and leaves once every wave is past it and no ticket below the list
        // length is left.  The grid is the co-resident block count
        // (occupancy_grid), so every wave reaches its redo phase and no entry
        // is left to k_redo (stats redo_late = 0, asserted by the GPU suite).
        // kRedoGuard is only a deadlock guard for a dispatcher that holds
        // blocks back behind resident ones (the GPU shared with another
        // process): after 20 ms in which neither the list nor the count of
        // waves past their main loop changed, the wave leaves its tickets to
        // k_redo.  A wave waits through the frame's tail only, and the count
        // changes every time a wave leaves its main loop (the main loops end
        // within ~2 ms of each other), so a working launch never sees 20 ms
        // without a change; round 5's 250 ms cost each frame of 4 processes
        // sharing one GPU (the gloo rehearsal) a quarter second once the
        // deferral ran at their shard size.  (Counting started waves instead
        // of the grid cost 2 % in register allocation, measured.)
        constexpr uint64_t kRedoGuard = 2000000;  // s_memrealtime ticks (100 MHz): 20 ms
        const unsigned long long waves = (unsigned long long)gridDim.x * (BLOCK / 64);
        // pc.redo_lanes lanes of the wave take tickets: a re-trace is one
        // lane's whole path, so fewer per wave spread them over more waves
        // (the wave waits for its slowest lane).  Bench frame, k_path ms with
        // 64 / 16 / 4 / 1 lanes: 1/8 shard 27.3 / 26.4 / 26.1 / 25.8, N=1
        // 184.8 / 184.9 / 184.5 (profiles/r04_ties/redo_lanes_*.log): 4
        uint32_t t = 0;
        if (lane_id() == 0) {
            atomicAdd(&counters[kRedoWaves], 1ull);
            t = (uint32_t)atomicAdd(&counters[kRedoTaken], (unsigned long long)pc.redo_lanes);
        }
        t = lane_id() < pc.redo_lanes ? (uint32_t)__shfl((int)t, 0) + lane_id() : 0xFFFFFFFFu;
        unsigned long long seen = ~0ull;
        uint64_t since = 0;
        for (;;) {
            const unsigned long long listed =
                __hip_atomic_load(&counters[kRedoCounter], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t lim = (uint32_t)min(listed, (unsigned long long)pc.redo_cap);
            uint2 e = make_uint2(kRedoEmpty, 0u);
            if (t < lim) e = redo_load(pc.redo + t);
            const bool have = e.x < kRedoDone;
            if (wany(have)) {
                if (have) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the entry before its state
                    redo_sample<BLOCK, SL>(sv, a, e.x, e.y, pc.redo_state + (size_t)t * kRedoState4, pc.sbuf, pc.sb_ss,
                                           pc.sb_sp, rays_e, rays_s, st, light, SPLIT ? pc.srec : nullptr);
                    redo_mark(pc.redo + t);
                    atomicAdd(&counters[kRedoTraced], 1ull);
                    t = (uint32_t)atomicAdd(&counters[kRedoTaken], 1ull);
                }
                since = 0;
                continue;
            }
            const unsigned long long past =
                __hip_atomic_load(&counters[kRedoWaves], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (past >= waves && !wany(t < lim)) break;
            const uint64_t now = __builtin_amdgcn_s_memrealtime();
            const unsigned long long sig = (past << 40) ^ listed;
            if (sig != seen || since == 0) {
                seen = sig;
                since = now;
            } else if (now - since > kRedoGuard) {
                break;
            }
            __builtin_amdgcn_s_sleep(16);
        }
    }
#ifdef TMPT_EXP_WAVETIME
    if (lane_id() == 0 && wt_id < kWaveTimeMax) g_wavetime[3 * wt_id + 2] = __builtin_amdgcn_s_memrealtime();
#endif
    if (SPLIT) {  // the rest of the wave's last reservation stays empty
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        for (uint32_t i = q_res + (uint32_t)lane_id(); i < min(q_end, pc.sq_cap); i += 64u)
            __builtin_nontemporal_store((u32x4){0u, 0u, 0u, kSplitEmpty}, reinterpret_cast<u32x4*>(pc.sq) + i);
    }
    if (SAMP == 4 && lane_id() == 0) {
        atomicAdd(&pc.rss.ctl[5], n_claim);
        atomicAdd(&pc.rss.ctl[6], n_miss);
        atomicAdd(&pc.rss.ctl[7], n_cas);
    }
    uint32_t re = wave_sum(rays_e), rs = wave_sum(rays_s);
    uint32_t nv = COUNT ? wave_sum(cnt.nodes) : 0u;
    uint32_t nt = COUNT ? wave_sum(cnt.tris) : 0u;
    uint32_t nvs = COUNT ? wave_sum(cnt_s.nodes) : 0u;
    uint32_t nts = COUNT ? wave_sum(cnt_s.tris) : 0u;
    uint32_t nst = COUNT ? wave_sum(cnt.stale) : 0u;
    uint32_t nst2 = COUNT ? wave_sum(cnt.stale2) : 0u;
    if (lane_id() == 0) {
        atomicAdd(&counters[0], (unsigned long long)(re + rs));
        atomicAdd(&counters[3], (unsigned long long)re);
        if (COUNT) {
            atomicAdd(&counters[kWalkCounter], (unsigned long long)nst);
            atomicAdd(&counters[kWalkCounter + 1], (unsigned long long)nst2);
            atomicAdd(&counters[1], (unsigned long long)nv);
            atomicAdd(&counters[2], (unsigned long long)nt);
            atomicAdd(&counters[4], (unsigned long long)nvs);
            atomicAdd(&counters[5], (unsigned long long)nts);
        }
        if (COUNT || PROF >= 3) {
            atomicAdd(&counters[6], (unsigned long long)rs_nr);
            atomicAdd(&counters[7], (unsigned long long)rs_nl);
            atomicAdd(&counters[8], (unsigned long long)rs_lr);
            atomicAdd(&counters[9], (unsigned long long)rs_ll);
            atomicAdd(&counters[10], (unsigned long long)rs_sr);
            atomicAdd(&counters[11], (unsigned long long)rs_sl);
            atomicAdd(&counters[12], (unsigned long long)rs_st);
        }
        if (PROF) {
            atomicAdd(&counters[13], (unsigned long long)pt_shade);
            atomicAdd(&counters[14], (unsigned long long)pt_node);
            atomicAdd(&counters[15], (unsigned long long)pt_leaf);
        }
        if (PROF >= 2) {
            atomicAdd(&counters[16], (unsigned long long)ps_fetch);
            atomicAdd(&counters[17], (unsigned long long)ps_shade);
            atomicAdd(&counters[18], (unsigned long long)ps_cam);
            atomicAdd(&counters[19], (unsigned long long)ps_start);
            atomicAdd(&counters[kCamCounter], (unsigned long long)pc_sr);
            atomicAdd(&counters[kCamCounter + 1], (unsigned long long)pc_cr);
            atomicAdd(&counters[kCamCounter + 2], (unsigned long long)pc_cl);
        }
        if (COUNT) {
            atomicAdd(&counters[kTopCounter], (unsigned long long)tv_n);
            atomicAdd(&counters[kTopCounter + 1], (unsigned long long)tv_lead);
            atomicAdd(&counters[kTopCounter + 2], (unsigned long long)tv_mix);
            atomicAdd(&counters[kTopCounter + 3], (unsigned long long)tv_only);
        }
        if (COUNT || PROF) {
            atomicAdd(&counters[kTopCounter + 4], (unsigned long long)tw_r);
            atomicAdd(&counters[kTopCounter + 5], (unsigned long long)tw_l);
        }
        if (PROF) {
            atomicAdd(&counters[kTopCounter + 6], (unsigned long long)pt_top);
            atomicAdd(&counters[kTopCounter + 7], (unsigned long long)pt_node_g);
            atomicAdd(&counters[kTopCounter + 8], (unsigned long long)pn_g);
            atomicAdd(&counters[kTopCounter + 9], (unsigned long long)pn_all);
        }
    }
}

// ============================================================ the camera pre-pass
// Sample seeding's camera samples of one pass, before k_path (CAM) starts: in
// that seeding a sample's camera ray and the RNG state after the camera's
// draws depend on (pixel, sample) alone, so they need not be made inside
// k_path, where the camera block ran for ~4.5 of a wave's 64 lanes at a time
// (DESIGN.md section 5).  One lane per (tile pixel slot, sample of [smp_begin,
// smp_end)), entry slot * count + (sample - smp_begin), in 64 bits; the
// statements are the camera block's own -- the same source functions under the
// same flags, so every bit is what k_path would have made.
// A block is 64 slots (blockIdx.x) by kCamBlockSamples samples (blockIdx.y),
// each wave one sample of the 64 slots: the wave's four jump-table gathers
// then fall into one sample's 4-KB table (8 lines per gather instead of 64,
// with a wave that held one pixel's 64 samples), and the blocks in flight, x
// fastest, share a few tables.  The entries go through LDS, so that a slot's
// samples leave as one contiguous 128-B piece, nontemporal.
constexpr int kCamBlockSamples = 4;
__global__ void __launch_bounds__(64 * kCamBlockSamples) k_cam_rays(SceneView sv, RenderArgs a,
                                                                    CamRay* __restrict__ out, uint32_t count)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t S = kCamBlockSamples;
    __shared__ u32x4 s_e[64 * S * 2];  // [slot][sample][half]
    const uint32_t l = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t pix0 = blockIdx.x * 64u, rel0 = blockIdx.y * S;
    // (past the end: the last slot or sample again, not stored)
    const uint32_t pix = min(pix0 + l, (uint32_t)a.slots - 1u);
    const uint32_t smp = (uint32_t)a.smp_begin + min(rel0 + w, count - 1u);
    const int lr = (int)fastdiv(pix, a.div_w);
    const int x = (int)(pix - (uint32_t)lr * (uint32_t)a.W);
    const uint32_t y = (uint32_t)tile_row_to_y_fd(a, lr);
    const uint32_t ps = pixel_seed((uint32_t)x, y, (uint32_t)a.W);
    uint32_t rng = sample_seed(a.jt, smp, ps);
    f3 so, sd;
    camera_sample(a.cam, (uint32_t)x, y, a.invW, a.invH, rng, so, sd);
    uint32_t flags = 0;
    if (ray_has_nan(so, sd)) flags = kCamNan;
    else if (a.root_check && !octree_root_hit(sv, so, sd, kMinT, kMaxT)) flags = kCamRootMiss;
    s_e[(l * S + w) * 2u] = (u32x4){__float_as_uint(so.x), __float_as_uint(so.y), __float_as_uint(so.z),
                                    __float_as_uint(sd.x)};
    s_e[(l * S + w) * 2u + 1u] = (u32x4){__float_as_uint(sd.y), __float_as_uint(sd.z), rng, flags};
    __syncthreads();
#pragma unroll
    for (uint32_t h = threadIdx.x; h < 64u * S * 2u; h += 64u * S) {
        const uint32_t sl = h / (2u * S), r = h % (2u * S);  // the slot of the block; sample and half within it
        const uint32_t p = pix0 + sl, rel = rel0 + (r >> 1);
        if (p < (uint32_t)a.slots && rel < count)
            __builtin_nontemporal_store(s_e[h], reinterpret_cast<u32x4*>(out + ((size_t)p * count + rel)) + (r & 1u));
    }
}

// The same over a list of pixels (a pass of tmpt_render_adaptive over the
// pixels still active), k_cam_rays's statements one for one: the block's 64
// "slots" are 64 positions of the list, and position i's samples are the
// entries of the tile pixel slot list[i] -- the buffer stays indexed by slot,
// so k_path (CAM, LIST) reads a pixel's entries where every CAM kernel does;
// the slots not listed are neither written nor read.  A kernel of its own, so
// that k_cam_rays stays the code it was.
__global__ void __launch_bounds__(64 * kCamBlockSamples) k_cam_rays_list(SceneView sv, RenderArgs a,
                                                                         CamRay* __restrict__ out, uint32_t count,
                                                                         const uint32_t* __restrict__ list,
                                                                         uint32_t n_list)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t S = kCamBlockSamples;
    __shared__ u32x4 s_e[64 * S * 2];  // [slot][sample][half]
    const uint32_t l = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t pix0 = blockIdx.x * 64u, rel0 = blockIdx.y * S;
    // (past the end: the last position or sample again, not stored)
    const uint32_t pix = list[min(pix0 + l, n_list - 1u)];
    const uint32_t smp = (uint32_t)a.smp_begin + min(rel0 + w, count - 1u);
    const int lr = (int)fastdiv(pix, a.div_w);
    const int x = (int)(pix - (uint32_t)lr * (uint32_t)a.W);
    const uint32_t y = (uint32_t)tile_row_to_y_fd(a, lr);
    const uint32_t ps = pixel_seed((uint32_t)x, y, (uint32_t)a.W);
    uint32_t rng = sample_seed(a.jt, smp, ps);
    f3 so, sd;
    camera_sample(a.cam, (uint32_t)x, y, a.invW, a.invH, rng, so, sd);
    uint32_t flags = 0;
    if (ray_has_nan(so, sd)) flags = kCamNan;
    else if (a.root_check && !octree_root_hit(sv, so, sd, kMinT, kMaxT)) flags = kCamRootMiss;
    s_e[(l * S + w) * 2u] = (u32x4){__float_as_uint(so.x), __float_as_uint(so.y), __float_as_uint(so.z),
                                    __float_as_uint(sd.x)};
    s_e[(l * S + w) * 2u + 1u] = (u32x4){__float_as_uint(sd.y), __float_as_uint(sd.z), rng, flags};
    __syncthreads();
#pragma unroll
    for (uint32_t h = threadIdx.x; h < 64u * S * 2u; h += 64u * S) {
        const uint32_t sl = h / (2u * S), r = h % (2u * S);  // the position of the block; sample and half within it
        const uint32_t p = pix0 + sl, rel = rel0 + (r >> 1);
        if (p < n_list && rel < count)
            __builtin_nontemporal_store(s_e[h],
                                        reinterpret_cast<u32x4*>(out + ((size_t)list[p] * count + rel)) + (r & 1u));
    }
}

// the pre-pass of a pass (a.smp_begin .. a.smp_end) over the tile's slots, or
// over the n_list slots of `list`, on the scene's stream
static void launch_cam_rays(Scene& s, const RenderArgs& a, CamRay* out, const uint32_t* list = nullptr,
                            int64_t n_list = 0)
{
    const uint32_t count = (uint32_t)(a.smp_end - a.smp_begin);
    const int64_t n = list ? n_list : a.slots;
    const dim3 grid((unsigned)((n + 63) / 64), (count + kCamBlockSamples - 1) / kCamBlockSamples);
    if (list)
        k_cam_rays_list<<<grid, 64 * kCamBlockSamples, 0, s.stream>>>(view(s), a, out, count, list, (uint32_t)n_list);
    else
        k_cam_rays<<<grid, 64 * kCamBlockSamples, 0, s.stream>>>(view(s), a, out, count);
}

// ============================================================ k_path's variants
// Every k_path the library instantiates, one line per kernel, by who launches
// it ("The path kernel's variants").  A caller describes
// the kernel it needs (PathVariant, above k_path) and path_kernel() finds it
// here; a variant without a line has no kernel, and asking for it is the
// render call's error.  A new kernel is a new line.
namespace {
constexpr bool F = false, T = true;
constexpr PathVariant kPathVariants[] = {
    // count sl        steps         shade_min  occ prof help samp soa ties sums cam list split
    // ---- sample seeding (render_persistent, SAMP 1): 4 waves per SIMD ...
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 0, F, 0},   // no octree (or tie_rule index)
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 2, F, 0},   // the octree answers flagged ties in the main loop
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 1, F, 0},   // ... or the redo phase does (deferred ties)
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 0, T, 0},   // tmpt_render_radiance without the colour buffer
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 2, T, 0},
    {T, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 0, F, 0},   // the visit counters (TIES 0 with the octree too)
    // ... layout=soa: 4 waves, never flagging or deferring
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, T, 0, F, 0},
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, T, 0, T, 0},
    {T, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, T, 0, F, 0},
    // ... 5 waves per SIMD (the default; option path_waves)
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, F, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, F, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 1, F, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, T, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, T, 0},
    // ... and their twins that read the camera pre-pass's entries (CAM; option cam_pre)
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, F, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, F, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 1, F, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, T, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, T, 1},
    // ... and the CAM twins of the shadow split (SPLIT; option shadow_split),
    // the three tie modes
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, F, 1, F, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, F, 1, F, 1},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 1, F, 1, F, 1},
    // ... and those at 6 waves per SIMD (option path_waves 6; kPathSL6, kTopNodes6)
    {F, kPathSL6, kSampleSteps, kShadeMin, 6, 0, 0, 1, F, 0, F, 1, F, 1},
    {F, kPathSL6, kSampleSteps, kShadeMin, 6, 0, 0, 1, F, 2, F, 1, F, 1},
    {F, kPathSL6, kSampleSteps, kShadeMin, 6, 0, 0, 1, F, 1, F, 1, F, 1},
    // ... and the passes over a list of pixels (LIST; tmpt_render_adaptive's
    // passes after the first): 4 or 5 waves, the three tie modes, at 5 waves
    // with the CAM twins; they read the AoS records (layout=soa too)
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 0, F, 0, T},
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 2, F, 0, T},
    {F, kPathSL, kSampleSteps, kShadeMin, 4, 0, 0, 1, F, 1, F, 0, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, F, 0, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, F, 0, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 1, F, 0, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 0, F, 1, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 2, F, 1, T},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 0, 0, 1, F, 1, F, 1, T},
    // ---- pixel seeding (render_persistent, SAMP 0): 4 or 5 waves, with or
    // without the shadow helpers (HELP), lowest-index ties or flagged for the octree
    {F, kPathSL, kPixSteps, kShadeMin, 4, 0, 0, 0, F, 0, F, 0},
    {F, kPathSL, kPixSteps, kShadeMin, 4, 0, 0, 0, F, 2, F, 0},
    {F, kPathSL, kPixSteps, kShadeMin, 4, 0, 1, 0, F, 0, F, 0},
    {F, kPathSL, kPixSteps, kShadeMin, 4, 0, 1, 0, F, 2, F, 0},
    {T, kPathSL, kPixSteps, kShadeMin, 4, 0, 0, 0, F, 0, F, 0},      // the visit counters
    {F, kPathSL5, kPixSteps, kShadeMin, 5, 0, 0, 0, F, 0, F, 0},
    {F, kPathSL5, kPixSteps, kShadeMin, 5, 0, 0, 0, F, 2, F, 0},
    {F, kPathSL5, kPixSteps, kShadeMin, 5, 0, 1, 0, F, 0, F, 0},
    {F, kPathSL5, kPixSteps, kShadeMin, 5, 0, 1, 0, F, 2, F, 0},
    // ---- the row engines.  Iterated (render_rowspec, and
    // render_persistent's pixel chains): units in full (SAMP 2), shadow-free (SAMP 3)
    {F, kPathSL, kRowIterSteps, kRowIterShadeMin, 4, 0, 0, 2, F, 0, F, 0},
    {F, kPathSL, kRowIterSteps, kRowIterShadeMin, kRsOcc3, 0, 0, 3, F, 0, F, 0},
    // streaming (render_rowstream): the chain's full re-trace (SAMP 2) at 4 or
    // 5 waves, the workers (SAMP 4) at 4 waves or kRsOcc3 blocks per CU; ties
    // flagged for the octree (option row_flag_leaves) or lowest index
    {F, kPathSL, kRowSteps, kRowShadeMin, 4, 0, 0, 2, F, 0, F, 0},
    {F, kPathSL, kRowSteps, kRowShadeMin, 4, 0, 0, 2, F, 2, F, 0},
    {F, kPathSL5, kRowSteps, kRowShadeMin, 5, 0, 0, 2, F, 0, F, 0},
    {F, kPathSL5, kRowSteps, kRowShadeMin, 5, 0, 0, 2, F, 2, F, 0},
    {F, kPathSL, kRowSteps, kRowShadeMin, 4, 0, 0, 4, F, 0, F, 0},
    {F, kPathSL, kRowSteps, kRowShadeMin, 4, 0, 0, 4, F, 2, F, 0},
    {F, kPathSL, kRowSteps, kRowShadeMin, kRsOcc3, 0, 0, 4, F, 0, F, 0},
    {F, kPathSL, kRowSteps, kRowShadeMin, kRsOcc3, 0, 0, 4, F, 2, F, 0},
#ifdef TMPT_DIAG
    // ---- the diagnostic build's wave-time profiles (TMPT_PROF = prof), one
    // block per CU: pixel seeding 1 / 2 / 3, sample seeding 1 / 2, and the
    // shading split (2) of the 5-wave sample kernel the product runs
    {F, kPathSL, kPixSteps, kShadeMin, 1, 1, 0, 0, F, 0, F, 0},
    {F, kPathSL, kPixSteps, kShadeMin, 1, 2, 0, 0, F, 0, F, 0},
    {F, kPathSL, kPixSteps, kShadeMin, 1, 3, 0, 0, F, 0, F, 0},
    {F, kPathSL, kSampleSteps, kShadeMin, 1, 1, 0, 1, F, 0, F, 0},
    {F, kPathSL, kSampleSteps, kShadeMin, 1, 2, 0, 1, F, 0, F, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 2, 0, 1, F, 0, F, 0},
    {F, kPathSL5, kSampleSteps, kShadeMin, 5, 2, 0, 1, F, 0, F, 1},   // ... and its CAM twin
#endif
};
constexpr size_t kNumPathVariants = sizeof(kPathVariants) / sizeof(kPathVariants[0]);

constexpr bool same_variant(const PathVariant& a, const PathVariant& b)
{
    return a.count == b.count && a.sl == b.sl && a.steps == b.steps && a.shade_min == b.shade_min && a.occ == b.occ &&
           a.prof == b.prof && a.help == b.help && a.samp == b.samp && a.soa == b.soa && a.ties == b.ties &&
           a.sums == b.sums && a.cam == b.cam && a.list == b.list && a.split == b.split;
}

// line I's kernel: the table's fields in k_path's parameter order
template <size_t I>
constexpr PathFn variant_kernel()
{
    constexpr PathVariant v = kPathVariants[I];
    return k_path<v.count, kBlk, v.sl, v.steps, v.shade_min, v.occ, path_tail(v.samp), v.prof, v.help, v.samp, v.soa,
                  v.ties, v.sums, v.cam, v.list, v.split>;
}

template <size_t... I>
PathFn kernel_at(size_t i, std::index_sequence<I...>)
{
    static const PathFn fns[] = {variant_kernel<I>()...};
    return fns[i];
}
}  // namespace

PathFn path_kernel(const PathVariant& v)
{
    for (size_t i = 0; i < kNumPathVariants; ++i)
        if (same_variant(v, kPathVariants[i])) return kernel_at(i, std::make_index_sequence<kNumPathVariants>{});
    return nullptr;
}

int find_path_kernel(const PathVariant& v, const char* who, PathFn& fn)
{
    fn = path_kernel(v);
    if (fn) return 0;
    set_error(std::string(who) + ": no k_path kernel for count " + std::to_string(v.count) + ", sl " +
              std::to_string(v.sl) + ", steps " + std::to_string(v.steps) + ", shade_min " +
              std::to_string(v.shade_min) + ", occ " + std::to_string(v.occ) + ", prof " + std::to_string(v.prof) +
              ", help " + std::to_string(v.help) + ", samp " + std::to_string(v.samp) + ", soa " +
              std::to_string(v.soa) + ", ties " + std::to_string(v.ties) + ", sums " + std::to_string(v.sums) +
              ", cam " + std::to_string(v.cam) + ", list " + std::to_string(v.list) + ", split " +
              std::to_string(v.split));
    return -22;
}

// TMPT_PAIR=<h>: every 64-rank chunk takes h ranks from the expensive end of the
// order and 64-h from the cheap end, so a wave's cheap pixels finish early and
// its lanes then help (HELP) with the expensive ones' shadow queries.
__global__ void __launch_bounds__(256) k_pair_order(const uint32_t* __restrict__ order, int64_t P, int32_t h,
                                                     uint32_t* __restrict__ paired)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= P) return;
    const int64_t full = P / 64, c = r / 64, i = r - c * 64;
    const int64_t m = c < full ? 64 : P - full * 64;  // ranks in this chunk
    const int64_t hc = c < full ? h : (m * h + 63) / 64;  // expensive ranks in this chunk
    const int64_t src = i < hc ? c * h + i : P - 1 - (c * (64 - h) + (i - hc));
    paired[r] = order[src];
}

// Pilot ordering: 3x3 box sum of each pixel's pilot-pass traversal steps,
// as a 16-bit key that sorts ascending = most expensive first.
__global__ void __launch_bounds__(256) k_order_keys(const uint32_t* __restrict__ cost, int32_t W,
                                                     int32_t rows, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)W * rows) return;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    uint32_t sum = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= rows) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx >= 0 && xx < W) sum += cost[(int64_t)yy * W + xx];
        }
    }
    keys[i] = 65535u - min(sum, 65535u);
    vals[i] = (uint32_t)i;
}

// Sample seeding with several blocks per pixel: the pixel's colour is the sum
// of its samples' colours in sample order (main.cpp:209-219, col += Trace),
// then main.cpp:221-233.  The buffer is [pixel][sample]: one wave per 64
// pixels stages 16 samples of each in LDS with coalesced 256-B reads (16
// lanes per pixel run), then every lane sums its own pixel's samples in order.
// A progressive pass (prog != null) sums its samples [s_begin, s_end) onto the
// sum the previous pass left in prog (none when s_begin = 0), keeps the new sum
// there, and writes the preview with out_recip = 1/s_end (the full render's
// 1/spp on the last pass).  tmpt_render_radiance hands in its float tile as
// prog with s_begin = 0: the whole render's sums, kept beside the pixels.
__global__ void __launch_bounds__(64) k_resolve_px(const float4* __restrict__ sbuf, int64_t P, int32_t spp,
                                                    float spp_recip, uint32_t* __restrict__ out,
                                                    int32_t s_begin = 0, int32_t s_end = -1,
                                                    float4* __restrict__ prog = nullptr)
{
    constexpr int kC = 16;                  // samples per staged chunk
    __shared__ float4 tile[64][kC + 1];     // +1: a lane's row starts on another bank
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int t = threadIdx.x;
    const int np = (int)min<int64_t>(64, P - p0);
    if (s_end < 0) s_end = spp;
    f3 col = mk(0.0f, 0.0f, 0.0f);
    if (prog && s_begin > 0 && t < np) {
        const float4 c = prog[p0 + t];
        col = mk(c.x, c.y, c.z);
    }
    for (int32_t s0 = s_begin; s0 < s_end; s0 += kC) {
        const int nc = min(kC, s_end - s0);
        for (int e = t; e < 64 * kC; e += 64) {
            const int i = e / kC, j = e - i * kC;
            if (i < np && j < nc) tile[i][j] = sbuf[(size_t)(p0 + i) * (size_t)spp + (size_t)(s0 + j)];
        }
        __syncthreads();
        if (t < np)
            for (int j = 0; j < nc; ++j) col = col + mk(tile[t][j].x, tile[t][j].y, tile[t][j].z);
        __syncthreads();
    }
    if (t < np) {
        if (prog) prog[p0 + t] = make_float4(col.x, col.y, col.z, 0.0f);
        out[p0 + t] = pack_pixel(col, spp_recip);
    }
}

void launch_resolve_px(hipStream_t stream, const float4* sbuf, int64_t P, int32_t spp, float spp_recip,
                       uint32_t* out)
{
    k_resolve_px<<<(unsigned)((P + 63) / 64), 64, 0, stream>>>(sbuf, P, spp, spp_recip, out);
}

// ============================================================ host side
// (kBlk, kSL and the helpers up to make_args: shared with tmpt_aov.hip, tmpt_render.h)
// co-resident blocks per CU of a kernel (at least 1)
static int occupancy_blocks(const void* fn, int block, size_t dyn_lds)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, dyn_lds) != hipSuccess || per_cu < 1) per_cu = 1;
    return per_cu;
}

int occupancy_grid(const void* fn, int block, size_t dyn_lds, int device)
{
    int per_cu = occupancy_blocks(fn, block, dyn_lds), cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        cus < 1)
        cus = 256;
    return per_cu * cus;
}

int ensure_ws(Scene& s, size_t bytes)
{
    if (s.ws.reserve(bytes)) return 0;
    set_error("render: out of device memory (workspace)");
    return -1;
}

// SceneView::any_w from option shadow_order: the weight of a child's exit
// distance tf in an any-hit lane's sort key tn + w * tf.  0: nearest first;
// -1: tn - tf, the longest overlap first; -1024: the exit distance decides and
// the entry distance only breaks near-ties.
// Default (-1), from the same-box A/B per seeding mode:
// largest exit first in sample and pixel seeding and the batched queries; in
// row seeding, where no order moves the whole render by more than its noise,
// the old walk.
static float shadow_order_weight(const Options& o, bool row)
{
    const int order = o.shadow_order >= 0 ? o.shadow_order : row ? 0 : kShadowOrderDefault;
    return order == 0 ? 0.0f : order == 1 ? -1.0f : -1024.0f;
}

// Option pop_cull; its default (-1) from the same-box A/B per seeding mode
// ("A key in the entry's spare bits").
static bool pop_cull_on(const Scene& s)
{
    if (s.opt.pop_cull >= 0) return s.opt.pop_cull != 0;
    return (s.row_render ? kPopCullRow : s.pixel_render ? kPopCullPixel : kPopCullSample) != 0;
}

SceneView view(const Scene& s)
{
    SceneView v{s.bvh.nodes4, s.bvh.tri_pre, s.bvh.tri_orig, s.bvh.n, s.bvh.n_nodes4};
    v.soa = s.bvh.soa;
    v.any_w = shadow_order_weight(s.opt, s.row_render);
    v.count_shift = (uint32_t)s.bvh.count_shift;
    v.key_mask = pop_cull_on(s) ? pop_key_mask(pop_key_bits(s.bvh.link_bits, s.opt.pop_key_cap)) : 0u;
#ifdef TMPT_CHECK
    v.chk = s.chk;
    // TMPT_CHECK_SELFTEST=1 (the report's own test, tests/test_gpu_check.py):
    // the view claims a single BVH node, so every query that descends past
    // the root fails the node test
    if (const char* e = getenv("TMPT_CHECK_SELFTEST"))
        if (atoi(e) == 1) v.n_nodes4 = std::min(v.n_nodes4, 1);
#endif
    if (s.octree.oct && s.opt.tie_rule == 0) {  // the reference's visit order for ties
        v.oct = s.octree.oct_view;
        const OctGrid& g = s.octree.oct_grid;
        v.crack = make_float4(g.reach, g.drift[0], g.drift[1], g.drift[2]);
    }
    return v;
}

namespace {

// Columns of M^n, M the xorshift32 step as a GF(2) 32x32 matrix (maths.cpp:5-13):
// column j = image of bit j.
void gf2_mul(const uint32_t* x, const uint32_t* y, uint32_t* out)  // out = x * y
{
    uint32_t t[32];
    for (int j = 0; j < 32; ++j) {
        uint32_t r = 0;
        for (int i = 0; i < 32; ++i)
            if ((y[j] >> i) & 1u) r ^= x[i];
        t[j] = r;
    }
    memcpy(out, t, sizeof t);
}

void xorshift_power(uint64_t n, uint32_t* acc)
{
    uint32_t m[32];
    for (int j = 0; j < 32; ++j) {
        uint32_t v = 1u << j;
        m[j] = xorshift32(v);
        acc[j] = 1u << j;
    }
    for (; n; n >>= 1) {
        if (n & 1u) gf2_mul(m, acc, acc);
        gf2_mul(m, m, m);
    }
}

}  // namespace

// sample_seed's byte tables for jumps J_i = M^((first + i) * stride), i in [0, count)
void jump_tables(uint64_t stride_steps, int32_t count, std::vector<uint32_t>& tab, uint32_t first)
{
    uint32_t stride[32], J[32];
    xorshift_power(stride_steps, stride);
    xorshift_power(stride_steps * first, J);  // the identity for first = 0
    tab.assign((size_t)count * 1024u, 0u);
    for (int32_t i = 0; i < count; ++i) {
        uint32_t* t = tab.data() + (size_t)i * 1024u;
        for (int k = 0; k < 4; ++k)
            for (uint32_t b = 1; b < 256; ++b)  // table[b] = table[b without its lowest bit] ^ column
                t[256 * k + b] = t[256 * k + (b & (b - 1u))] ^ J[8 * k + __builtin_ctz(b)];
        gf2_mul(stride, J, J);
    }
}

// sample_seed's byte tables for samples [0, spp): J_s = M^(s * kSampleStride)
void sample_jump_tables(int32_t spp, std::vector<uint32_t>& tab) { jump_tables(kSampleStride, spp, tab); }

RenderArgs make_args(const tmpt_camera* c, const tmpt_render_desc* d)
{
    RenderArgs a;
    a.cam.origin = mk(c->origin[0], c->origin[1], c->origin[2]);
    a.cam.lower_left = mk(c->lower_left[0], c->lower_left[1], c->lower_left[2]);
    a.cam.horizontal = mk(c->horizontal[0], c->horizontal[1], c->horizontal[2]);
    a.cam.vertical = mk(c->vertical[0], c->vertical[1], c->vertical[2]);
    a.cam.u = mk(c->u[0], c->u[1], c->u[2]);
    a.cam.v = mk(c->v[0], c->v[1], c->v[2]);
    a.cam.w = mk(c->w[0], c->w[1], c->w[2]);
    a.cam.lens_radius = c->lens_radius;
    a.W = d->width;
    a.H = d->height;
    a.spp = d->spp;
    a.seed_mode = d->seed_mode;
    a.band_rows = d->band_rows > 0 ? d->band_rows : d->height;
    a.shard = d->num_shards > 1 ? d->shard : 0;
    a.nshards = d->num_shards > 1 ? d->num_shards : 1;
    a.tile_rows = tmpt_tile_rows(d);
    a.invW = 1.0f / (float)d->width;             // main.cpp:186
    a.invH = 1.0f / (float)d->height;            // main.cpp:187
    a.spp_recip = 1.0f / (float)d->spp;          // main.cpp:188
    a.slots = (int64_t)a.tile_rows * a.W;
    a.smp_begin = d->spp_begin;
    a.smp_end = d->spp_count > 0 ? d->spp_begin + d->spp_count : d->spp;
    a.out_recip = a.smp_end == d->spp ? a.spp_recip : 1.0f / (float)a.smp_end;
    a.prog = nullptr;
    a.jt = nullptr;
    a.bmask = 2047u;
    a.row_lanes = 1;  // one row per wave: measured fastest
    a.root_check = 0;
    a.div_w = fastdiv_make((uint32_t)a.W);
    a.div_band = fastdiv_make((uint32_t)a.band_rows);
    return a;
}

// PathCtl::top_walk from option top_walk: the round cap, or (-1, auto) the
// seeding's measured default.  seeding: 0 sample, 1 pixel, 2 row (both row
// engines and the pixel chains).  Bench frame, same box, parent / cap 0 / 2 /
// 3 / 4 / 5 / 6 / 8 (profiles/r07_top_walk/): sample
// seeding, k_path ms, N=1 171.9 / 172.3 / 170.5 / 169.3 / 168.7 / 171.3 /
// 174.3 / 178.3, 1/8 shard 24.2 / 24.0 / 23.9 / 23.7 / 23.6 / 24.0 / 24.4 /
// 24.8 -- the queries of a shading round leave the LDS copy after 3.7 visits,
// and past the fourth round a few lanes hold the whole wave; row seeding,
// whole render, 1814 / 1830 / 1815 / - / 1803 / - / - / 1886 ms; pixel
// seeding, k_path ms, cap 0 / 2 / 4 / 8: N=1 192.6 / 193.9 / 194.8 / 204.8,
// 1/8 35.3 / 35.6 / 35.0 / 36.7 -- no cap gains there, so off.
constexpr int kTopWalkSample = 4, kTopWalkPixel = 0, kTopWalkRow = 4;
uint32_t top_walk_cap(const Options& o, int seeding)
{
    if (o.top_walk >= 0) return (uint32_t)o.top_walk;
    return (uint32_t)(seeding == 0 ? kTopWalkSample : seeding == 1 ? kTopWalkPixel : kTopWalkRow);
}

// PathCtl::oct_shadow: whether a shadow query's answer can need the octree --
// a triangle lying flat on one of its planes, or a light direction that can
// drift along a crack (octree_crack's test at the smallest t a hit can have,
// kMinT): the constant light of main.cpp:36 never can in these scenes, but
// the test is the device's own.
uint32_t oct_shadow_check(const Scene& s)
{
    if (!s.octree.oct_view || s.opt.tie_rule != 0) return 0u;
    if (s.octree.oct_flat > 0) return 1u;
    const f3 ld = light_dir();
    const float l[3] = {fabsf(ld.x), fabsf(ld.y), fabsf(ld.z)};
    for (int k = 0; k < 3; ++k)
        if (l[k] * fminf(kMinT, s.octree.oct_grid.reach) <= s.octree.oct_grid.drift[k]) return 1u;
    return 0u;
}

// Option cam_pre's default (-1), from the same-box A/B (DESIGN.md section 5,
// "The camera pre-pass").
constexpr int kCamPreDefault = 1;

// The scene's buffer of camera entries (k_cam_rays), grown to `need` bytes and
// kept, as sbuf is.  False -- the caller then renders with the kernels that
// make their own camera samples -- where the buffer is over option
// cam_pre_max, or has to grow and does not fit in half of the device memory
// still free (the colour buffer of the same call is allocated by then; the
// buffer held counts as free), or cannot be allocated.
// The shadow split's buffer for a pass of n samples: the control words (the
// queue's counter and k_shadow's fetch head, a line each), a queue for the
// worst case and the records.  Worst case: every bounce of
// every sample queues a query (kMaxDepth each); a wave's reservation of
// kSplitChunk entries leaves fewer than 64 unused when it takes the next one,
// and its last one up to all of it.  False when that does not fit under option
// shadow_split_max (or, where the buffer has to grow, in half of the device
// memory still free), or a queue entry could not name the records.
constexpr size_t kSplitCtlWords = 2 * kCtr;
// the buffer's bytes for n samples (0: the entries cannot be counted or named), and the queue's entries
static size_t split_need(int64_t n, int64_t waves, uint32_t& sq_cap)
{
    if (n <= 0 || n >= kSplitMaxRecs) return 0;
    const int64_t worst = n * kMaxDepth;
    // (a wave that queues holds a sample: no more of them than samples)
    const int64_t cap = worst + worst / (kSplitChunk / 64 - 1) + (std::min(waves, n) + 1) * (int64_t)kSplitChunk;
    if (cap >= (1ll << 32) - (int64_t)kSplitChunk * (waves + 1)) return 0;  // the counter is 32 bits
    sq_cap = (uint32_t)cap;
    return kSplitCtlWords * 4 + sizeof(uint4) * (size_t)cap + sizeof(SplitRec) * (size_t)n;
}
// what the buffer may take: option shadow_split_max, else half of the device
// memory that is free or already the buffer's
static size_t split_budget(const Scene& s)
{
    const size_t half = free_budget(1, 1, s.split_buf.bytes()) / 2;
    return s.opt.shadow_split_max > 0.0 ? (size_t)std::min((double)half, s.opt.shadow_split_max) : half;
}
static bool ensure_split(Scene& s, int64_t n, int64_t waves, uint32_t& sq_cap)
{
    const size_t need = split_need(n, waves, sq_cap);
    if (need == 0) return false;
    if (s.opt.shadow_split_max > 0.0 && (double)need > s.opt.shadow_split_max) return false;
    if (s.split_buf.bytes() >= need) return true;
    if (need > split_budget(s)) return false;
    return s.split_buf.alloc(need);
}

static bool ensure_cam_rays(Scene& s, size_t need)
{
    if (s.opt.cam_pre_max > 0.0 && (double)need > s.opt.cam_pre_max) return false;
    if (s.cam_rays.bytes() >= need) return true;
    if (need > free_budget(1, 1, s.cam_rays.bytes()) / 2) return false;
    return s.cam_rays.alloc(need);
}

// Persistent path engine: one launch per frame (shard).
int render_persistent(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count,
                      unsigned long long* d_counters)
{
    const Options& o = s.opt;
    // HIP events around each k_path launch (pilot: 0-1, final: 2-3) on the
    // stream it runs on: the dominant kernel's own time for the roofline
    for (auto& e : s.path_ev) TMPT_HIP(e.ensure());
    // Which k_path: the facts first, then one variant (PathVariant) from them.
    // Pixel seeding, and sample seeding (its own instantiations: the pixel-mode
    // kernel keeps its register allocation).
    const bool jt = a.jt != nullptr;
    // the reference's octree answers ties (tie_rule visit)
    const bool oct = s.octree.oct_view && o.tie_rule == 0;
    int prof = 0;
#ifdef TMPT_DIAG
    // diagnostic build only: TMPT_PROF=1 s_memtime split of wave time (shading /
    // node / leaf rounds); 2: + shading-round split; 3: + per-round cycle counts
    // (more registers: compare its times only among PROF=3 runs)
    if (const char* pe = getenv("TMPT_PROF")) prof = count ? 0 : atoi(pe);
#endif
    // k_path's PROF of that: sample seeding has no level 3
    const int prof_level = !prof ? 0 : prof >= 3 && !jt ? 3 : prof >= 2 ? 2 : 1;
    // layout=soa: the sample kernel reads the SoA planes (the A/B of DESIGN.md
    // section 3; the other engines keep the AoS records, and so do the
    // profiling kernels)
    // A pass of tmpt_render_adaptive (Scene::adapt_on) over the pixels still
    // active (Scene::adapt_list; its first pass has none and is planned as a
    // progressive pass over every slot): the units, the block size, the tail
    // and the deferral rule go by the list's length, not by a.slots; the LIST
    // kernels read the AoS records.
    const bool list = s.adapt_list != nullptr;
    const int64_t npix = list ? s.adapt_n : a.slots;  // pixels the supply hands out
    const bool soa = s.bvh.soa.na != nullptr && !list;
    const bool soa_kernel = jt && soa && !prof;
    // TMPT_PROF=2 in sample seeding: the shading split of the 5-wave kernel the
    // product runs (its LDS layout and 96 VGPRs), unless path_waves = 4
    const bool prof5 = prof == 2 && jt && !soa && o.path_waves != 4;
    // Sample seeding's path kernels run 5 waves per SIMD (OCC 5: the 30-KB LDS
    // layout, 96 VGPRs; option path_waves): the lanes below are theirs.  No
    // instrumented, profiling (but prof5) or SoA kernel has a 5-wave variant.
    const bool waves5 = jt && !count && (!prof || prof5) && !soa && o.path_waves != 4;
    // Ties: the leaves flag them for the octree (TIES 2; 1 when the flagged
    // samples are deferred, below).  An instrumented or profiling render keeps
    // the lowest-index leaf (TIES 0) even with the octree, and SoA has no
    // flagging or deferring variant.
    const bool flag = oct && !count && !prof && !soa_kernel;
    // Every field once, from the facts above and those that depend on the
    // load: 5 waves per SIMD, the shadow helpers, the tie rule (0, or with
    // `flag` 2 or 1) and the float sums.  prof forces one block per CU (OCC 1)
    // except the prof5 case, which is a 5-wave kernel.
    auto variant = [&](bool w5, int help, int ties, bool sums, int cam = 0) {
        PathVariant v{};
        v.count = count;
        v.sl = w5 ? kPathSL5 : kPathSL;
        v.steps = jt ? kSampleSteps : kPixSteps;
        v.shade_min = kShadeMin;
        v.occ = w5 ? 5 : prof ? 1 : 4;
        v.prof = prof_level;
        v.help = help;
        v.samp = jt ? 1 : 0;
        v.soa = soa_kernel;
        v.ties = ties;
        v.sums = sums;
        v.cam = cam;
        v.list = list;
        return v;
    };
    // Pixel seeding's instantiations too, but only with several pixels per
    // lane: at low load a pixel's sample chain is the frame's critical path
    // and a fifth wave on the SIMD slows every chain (whole renders, 4 / 5
    // waves: N=1 207.2 / 197.6 ms, 1/2 116.9 / 113.9, 1/4 63.6 / 65.7, 1/8
    // 36.2 / 39.1; profiles/r06_experiments/occ5/ab_pixel_waves.log), so from
    // 3 pixels per 4-wave lane (option path_waves 5 forces it, 4 keeps 4).
    // The 4-wave grid is that of the render's kernel before the load-dependent
    // choices (no helpers, no flagged ties); the 5-wave grid that of the
    // 5-wave deferring sample kernel, in pixel seeding too (every OCC 5
    // instantiation has the same LDS and VGPR footprint).
    PathVariant probe5{};
    probe5.sl = kPathSL5;
    probe5.steps = kSampleSteps;
    probe5.shade_min = kShadeMin;
    probe5.occ = 5;
    probe5.samp = 1;
    probe5.ties = 1;
    PathFn fn_base, fn_probe5;
    if (int rc = find_path_kernel(variant(prof5, 0, 0, false), "tmpt_render", fn_base)) return rc;
    if (int rc = find_path_kernel(probe5, "tmpt_render", fn_probe5)) return rc;
    const int grid4 = occupancy_grid((const void*)fn_base, kBlk, 0, s.device);
    const int grid5 = occupancy_grid((const void*)fn_probe5, kBlk, 0, s.device);
    const bool waves5p = !jt && !count && !prof &&
                         (o.path_waves >= 5 || (o.path_waves == 0 && a.slots >= 3 * (int64_t)grid4 * kBlk));
    const int grid = waves5 || waves5p ? grid5 : grid4;
    // Six waves per SIMD (option path_waves 6): only the shadow split's twins
    // have 6-wave kernels (kPathVariants), so the render wants them only where
    // the split can run, and runs the 5-wave kernels wherever it then does not
    // (split_on below).  The load rules above and below (sample blocks, tail
    // units, the deferral) keep going by the 5-wave grid; what is sized by the
    // launch -- the stack spill area, the shadow queue's reservations -- goes
    // by the larger of the two grids.
    // Auto (path_waves 0): the deferring twin (TIES 1, pick_main below) from
    // kPathWaves6MinLoad samples per 5-wave lane -- the loads it was measured
    // at are in tmpt_path.h.
    const bool want6 = waves5 && !prof && !list && o.shadow_split != 0 &&
                       (o.path_waves == 6 ||
                        (o.path_waves == 0 && kPathWaves6Auto != 0 &&
                         a.slots * (int64_t)(a.smp_end - a.smp_begin) >= kPathWaves6MinLoad * (int64_t)grid5 * kBlk));
    int grid6 = 0;
    if (want6) {
        PathVariant probe6 = probe5;
        probe6.sl = kPathSL6;
        probe6.occ = 6;
        probe6.cam = 1;
        probe6.split = 1;
        PathFn fn_probe6;
        if (int rc = find_path_kernel(probe6, "tmpt_render", fn_probe6)) return rc;
        grid6 = occupancy_grid((const void*)fn_probe6, kBlk, 0, s.device);
    }
    // Sample seeding: the work units are (pixel, block of blk samples).  The
    // block is the largest power of two up to 8 that still leaves >=
    // kUnitsPerLane units per resident lane.  Bench frame (1-row bands,
    // k_path ms): N=1 blk 2/4/8 = 220.7/217.8/217.3; 1/2 shard blk 1/2/4/8 =
    // 113.3/110.9/110.2/111.7; 1/4 blk 1/2/4 = 57.1/56.2/56.6; 1/8 blk 1/2/4/8
    // = 29.4/29.4/30.2/32.7 -- best at ~63 units per lane while the frame
    // ended on a lane's last block (rounds 2-4: 60 picked 8, 4, 2, 1 at N = 1,
    // 2, 4, 8).  With the single-sample tail units below the end no longer
    // depends on the block, and fewer, longer blocks win (round 5, k_path ms,
    // profiles/r05_experiments/blk_tail_*.log): 1/8 blk 1 / 2 / 4 / 8 with a
    // 4-block tail 25.55 / 24.93 / 24.54 / 24.73, 1/4 blk 2 / 4 / 8 49.24 /
    // 48.22 / 48.31, N=1 blk 8 / 16 / 32 186.27 / 186.25 / 188.92, 1/2 blk
    // 8 / 16 94.47 / 95.09 -- so 15 units per lane and at most 8 samples: 8,
    // 8, 8, 4 at N = 1, 2, 4, 8.  Option sample_block fixes it.
    uint32_t blk = 1u, nblk = 1u, blk0 = 0u;
    // Progressive passes in sample seeding (samples [s0, s1) of every pixel):
    // the units are the blocks of the pass -- a block size that divides s0, so
    // the blocks keep their alignment -- and every sample's colour goes to the
    // colour buffer; k_resolve_px adds the pass's samples, in order, to the sum
    // the previous pass left (main.cpp:218 summed across the passes).
    // (every pass of tmpt_render_adaptive is one, its last too: the update
    // kernel reads the samples from the colour buffer)
    const bool pass = a.jt && (a.smp_begin > 0 || a.smp_end < a.spp || s.adapt_on);
    const int64_t s0 = a.smp_begin, s1 = a.smp_end;
    if (a.jt) {
        // (15 units per 4-wave lane; with 5 waves per SIMD a quarter more lanes
        // share the work, and 12 per lane picks the same blocks as 15 did:
        // 8, 8, 8, 4 at N = 1, 2, 4, 8 -- round 6, profiles/r06_experiments/occ5/)
        const int64_t kUnitsPerLane = waves5 ? 12 : 15;
        const int64_t lanes0 = (int64_t)grid * kBlk;
        blk = 1u;
        while ((int64_t)blk * 2 <= 8 && blk * 2u <= (uint32_t)(s1 - s0) &&
               npix * ((s1 - s0 + blk * 2 - 1) / (blk * 2)) >= kUnitsPerLane * lanes0)
            blk *= 2u;
        if (o.sample_block > 0) blk = (uint32_t)o.sample_block;
        while (npix * ((s1 - s0 + blk - 1) / blk) >= (1ll << 31)) blk *= 2u;  // 32-bit unit ids
        while (s0 % blk) blk /= 2u;  // a pass's first sample starts a block
        // the alignment can undo the 32-bit guard above (e.g. 4K x 1024 spp
        // from spp_begin 2: blocks of 2, ~4.2 G units): the unit ids, res and
        // nchunks are uint32, so such a pass is refused, not wrapped
        if (npix * ((s1 - s0 + blk - 1) / blk) >= (1ll << 31)) {
            set_error("tmpt_render: this progressive pass (samples " + std::to_string(s0) + ".." +
                      std::to_string(s1) + " of " + std::to_string(a.slots) +
                      " pixels) needs more than 2^31 sample units at the block size its first sample allows (" +
                      std::to_string(blk) + "): start passes at a multiple of a larger power of two, or render "
                      "the frame in one call");
            return -22;
        }
        blk0 = (uint32_t)(s0 / blk);
        nblk = (uint32_t)((s1 + blk - 1) / blk - blk0);
        // Several blocks per pixel need the per-sample colour buffer (16 B per
        // sample of the tile: 2.1 GB at 1080p x 64).  If it does not fit in 3/4
        // of the free device memory (or the sbuf_max option), the pixel is one
        // unit: same image, only the tail of a small shard is longer.  A
        // progressive pass needs the buffer whatever its block count.
        if (nblk > 1 || pass) {
            const size_t need = sizeof(float4) * (size_t)a.spp * (size_t)a.slots;
            size_t budget = free_budget(3, 4, s.sbuf.bytes());  // the buffer already held is free for this call
            if (o.sbuf_max > 0.0) budget = std::min(budget, (size_t)o.sbuf_max);
            if (need > budget) {
                if (pass) {
                    set_error(s.adapt_on
                                  ? "tmpt_render_adaptive: the per-sample colour buffer (" + std::to_string(need >> 20) +
                                        " MiB) does not fit (render option sbuf_max, or 3/4 of the free device memory)"
                                  : "tmpt_render: progressive passes in sample seeding need the per-sample colour buffer (" +
                                        std::to_string(need >> 20) + " MiB), which does not fit: render the frame in one call");
                    return -12;
                }
                while (blk < (uint32_t)a.spp) blk *= 2u;
                nblk = 1u;
            }
        }
    }
    int64_t P = npix * (int64_t)nblk;  // units the supply hands out
    // Sample seeding's tail (option sample_tail): the last sample_tail blocks
    // per resident lane are handed out as single samples, so a lane's last
    // unit is one sample, not a block of blk, and the waves leave their main
    // loops closer together: bench frame, N=1, blocks of 8, the main loops
    // ended over 8.6 ms without it and over 1.7 ms with 8 blocks per lane
    // (profiles/r05_wavetime/; the deferred re-traces are then the last
    // ~2 ms).  k_path, tail 0 / 8 blocks per lane: N=1 188.0 / 186.0 ms, 1/2
    // 96.1 / 94.7 ms (16: slower again, the single units' own seed jumps;
    // profiles/r05_experiments/sample_tail*.log).  With the longer blocks
    // above: a quarter of a lane's samples, at most 64 (N=1 and 1/2: 8 blocks
    // of 8; 1/4: 4 of 8; 1/8: 4 of 4).
    uint32_t ua = 0xFFFFFFFFu;
    // (only when every block is full: a partial last block would map tail
    // units to samples past the pass's end)
    // Auto (-1): a quarter of a lane's samples, at most 64, in blocks.
    int64_t tail_blocks = o.sample_tail;
    if (tail_blocks < 0) {
        const int64_t spl = npix * (s1 - s0) / std::max<int64_t>(1, (int64_t)grid * kBlk);  // samples per lane
        const int64_t b = std::max<uint32_t>(1u, blk);
        tail_blocks = std::max<int64_t>(1, (std::min<int64_t>(64, spl / 4) + b - 1) / b);
    }
    if (a.jt && nblk > 1 && blk >= 2u && tail_blocks > 0 && (s1 - s0) % blk == 0) {
        int64_t nb = std::min<int64_t>(P, tail_blocks * grid * kBlk);
        while (nb > 0 && (P - nb) + nb * (int64_t)blk >= (1ll << 31)) nb /= 2;
        if (nb > 0) {
            ua = (uint32_t)(P - nb);
            P = (P - nb) + nb * (int64_t)blk;
        }
    }
    // Pilot ordering (SURVEY §8e "pull tiles dynamically", at pixel grain): when
    // a shard has several pixels per resident lane, the frame ends with the
    // chains of the pixels started last.  A first pass runs `pilot` samples of
    // every pixel and records its traversal steps; the remaining samples run
    // with pixels handed out most expensive first (3x3-smoothed pilot cost).
    // The passes continue each pixel's RNG stream and colour sum exactly as
    // progressive spp does, so the image is the single-pass image bit for bit.
    // 4 pilot samples; 2 at low load (at most ~2.5 pixels per resident lane,
    // where the pilot pass is a tail of its own: 1/8 shard 42.2 -> 41.3 ms,
    // 1/4 74.6 -> 73.5 ms).  Option pilot (0 = off).
    int pilot = 2 * P <= 5 * (int64_t)grid * kBlk ? 2 : 4;
    if (o.pilot >= 0) pilot = o.pilot;
    const bool ordered = pilot > 0 && !count && !a.jt && a.smp_begin == 0 && a.smp_end == a.spp &&
                         a.spp >= 2 * pilot && P < (1ll << 31);
    // Shadow offload at low load (k_path HELP): with at most ~2.5 pixels per
    // resident lane the frame is bound by the most expensive pixels' chains, and
    // 27-28 % of their traversal work is shadow queries, which feed neither the
    // RNG stream nor the path (main.cpp:57-67).  Lanes without a pixel then trace
    // other lanes' shadow queries, and (ordered passes) each 64-rank chunk pairs
    // `pair` expensive ranks with 64-pair cheap ones, whose lanes free up early.
    // Bench frame: 1/4 shard 86.4 -> 77.2 ms (pair 56), 1/8 shard 45.7 -> 43.9 ms
    // (pair 52).  Re-measured in round 5 as whole renders (help on / off,
    // profiles/r05_experiments/*_help.log): 1080p N=1 214.4 / 210.6 ms, 1/2
    // 116.6 / 120.6, 1/4 63.9 / 75.5, 1/8 36.4 / 38.8; 4K x 256 1/2 1599.6 /
    // 1531.5, 1/4 838.6 / 814.5, 1/8 450.3 / 467.9 -- it wins up to ~4 pixels
    // per resident lane and loses from ~8 (the extra shading code), so it is
    // on at <= 4.5.  Options help and pair override the choice.
    const int64_t lanes = (int64_t)grid * kBlk;
    int help = ordered && !prof && 2 * P <= 9 * lanes ? 1 : 0;  // (ordered: pixel seeding, not instrumented)
    if (o.help >= 0) help = o.help != 0 && !count && !prof && !jt;
    const uint32_t oct_shadow = oct_shadow_check(s);
    if (oct_shadow) help = 0;  // the helpers' shadow answers are not checked
    int pair = help && ordered ? (2 * P <= 3 * lanes ? 52 : 56) : 0;
    if (o.pair >= 0) pair = o.pair;
    const bool w5 = jt ? waves5 : waves5p;
    // stack spill areas for either kind of kernel's lanes (4 waves, 16 LDS
    // entries; 5 waves, 12)
    size_t ovf_words = std::max({(size_t)grid4 * (kStackTotal - kPathSL),
                                 (size_t)std::max(grid4, grid5) * (kStackTotal - kPathSL5),
                                 (size_t)grid6 * (kStackTotal - kPathSL6)}) * kBlk;
    // (k_shadow's lanes spill there after k_path's: more lanes, shorter LDS stacks)
    if (jt && o.shadow_split != 0) ovf_words = std::max(ovf_words, shadow_ovf_words(s.device));
    const size_t head_words = (size_t)kSeg * kCtr;
    const size_t hist_words = ordered ? radix_sort_hist_words((int32_t)P) : 0;
    const size_t reg_words = ordered ? 2 * (size_t)kSimdKeys + 64 + (size_t)P : 0;  // + claim words
    const size_t extra_words = ordered ? (size_t)P * (4 + 5) + hist_words + reg_words : 0;
    if (ensure_ws(s, (ovf_words + head_words + extra_words) * 4)) return -1;
    uint32_t* heads = s.ws.as<uint32_t>() + ovf_words;
    TMPT_HIP(hipMemsetAsync(heads, 0, head_words * 4, s.stream));
    PathCtl pc;
    memset(&pc, 0, sizeof(pc));
    pc.heads = heads;
    pc.oct_shadow = oct_shadow;
    pc.top_walk = top_walk_cap(o, a.jt ? 0 : 1);
    pc.P = P;
    pc.nblk = nblk;
    pc.blk = blk;
    pc.div_nblk = fastdiv_make(nblk);
    pc.div_blk = fastdiv_make(blk);
    pc.blk0 = blk0;
    pc.ua = ua;
    if (list) pc.order = s.adapt_list;  // (k_path LIST; sample seeding has no cost order)
    RenderArgs as = a;  // sample seeding: a lane's run of samples is its block
    if (a.jt) {
        as.bmask = nblk > 1 ? blk - 1u : 2047u;
        if (nblk > 1 || pass) {
            const size_t need = sizeof(float4) * (size_t)a.spp * (size_t)a.slots;
            TMPT_ALLOC(s.sbuf.reserve(need), "tmpt_render: the per-sample colour buffer");
            pc.sbuf = s.sbuf;
        }
    }
    // sbuf is [pixel][sample] with nontemporal stores (a 16-B store into a
    // [sample][pixel] line pulled the whole line into L2 -- 27 GB of extra
    // fetches per 1080p frame); k_resolve_px reads it through LDS
    pc.sb_ss = 1u;
    pc.sb_sp = (uint32_t)a.spp;
    // A unit of >= 2 samples holds each even sample's colour until the next one
    // and writes both into the same 32-B sector (spp even: sectors align), so
    // the two 16-B halves can leave L2 as one write instead of two (option sbuf_pair)
    pc.pair = pc.sbuf && blk >= 2u && a.spp % 2 == 0 && o.sbuf_pair ? 1u : 0u;
    // Small shards (at most a quarter as many pixels as resident lanes): a wave
    // holds at most 32 pixels at once, so the pixels spread over more SIMD
    // slots and each wave's chain -- the frame's critical path at that load --
    // has fewer lanes to interleave (bench frame, 1/32 shard: 44.1 -> 40.9 ms;
    // at 1/16 (half the lanes) it measured 44.4 -> 45.5 ms, so not there; 16
    // lanes per wave was slower still).  Option wave_cap fixes the cap.
    {
        const int64_t waves = std::max<int64_t>(1, (int64_t)grid * (kBlk / 64));
        int64_t c = P <= waves * 16 ? 32 : 64;
        if (o.wave_cap > 0) c = o.wave_cap;
        pc.lane_cap = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(64, c));
    }
    pc.chunk = std::min<uint32_t>(kChunk, pc.lane_cap);
    pc.nchunks = (uint32_t)((P + pc.chunk - 1) / pc.chunk);
    if (!ordered) {
        // Deferred ties (PathCtl::redo, k_path DEFER): with per-sample colours
        // (sbuf) a tied sample can be traced again on its own, so the main loop
        // runs without the octree walk and root-box test (and takes the first
        // triangle met on a tie, flagged) and the launch's waves trace the
        // dropped samples in their tail (k_redo the rest).  Only when no camera
        // ray needs the root-box test (root_check = 0).  Auto: at >= 192 samples
        // per resident lane (4 waves per SIMD), where the tail hides the
        // re-traces -- bench frame, k_path ms, base (no octree) / ties settled
        // inline / deferred: N=1 184.8 / 190.2 / 185.3, 1/2 93.1 / 96.3 / 94.9,
        // 1/4 47.7 / 49.4 / 49.8, 1/8 24.6 / 25.5 / 27.1;
        // with 5 waves per SIMD the deferring kernel wins down to the 1/8
        // shard (51 samples per lane; inline / deferred with its block rule:
        // 1/4 47.3 / 45.9, 1/8 24.3 / 24.2 ms), so from 48 per lane
        // (profiles/r06_experiments/occ5/ab_low_rules.log)
        const bool defer = jt && !count && !prof && !soa && pc.sbuf && a.root_check == 0 && o.tie_defer != 0 &&
                           !oct_shadow &&
                           (o.tie_defer > 0 ||
                            (list ? npix * (s1 - s0) : a.slots * (int64_t)a.spp) >= (waves5 ? 48 : 192) * lanes);
        bool redo = defer && oct;
        if (redo && o.redo_cap > 0 && s.redo_cap != (uint32_t)o.redo_cap) free_redo(s);  // the test hook's size
        if (redo && s.redo_cap == 0) {
            int64_t cap = std::min<int64_t>(1ll << 31, std::max<int64_t>(1 << 16, a.slots * (int64_t)a.spp / 128));
            if (o.redo_cap > 0) cap = o.redo_cap;
            (void)alloc_redo(s, cap);
        }
        const bool redo_nomem = redo && s.redo_cap == 0;
        if (redo_nomem) redo = false;
        // (the deferring kernel keeps the first triangle met on a tie and flags
        // it: only the redo pass gives those samples their answer)
        // (with the octree but no deferral: the leaf only flags ties, TIES 2)
        // five waves per SIMD (waves5, option path_waves; the 30-KB LDS layout
        // of OCC 5, 96 VGPRs): bench frame, k_path ms, 4 / 5 waves, same box:
        // N=1 185.6 / 171.0, 1/2 94.3 / 87.7
        // tmpt_render_radiance in sample seeding without the colour buffer (a
        // pixel is one unit): the launch's kernel with SUMS, which stores
        // the pixel's float sum in a.prog beside the packed pixel.  With the
        // buffer k_resolve_px stores it, in pixel seeding k_path<SAMP 0> does.
        const bool sums = jt && a.prog && !pc.sbuf;
        if (sums && (count || prof)) {
            set_error("tmpt_render_radiance: no instrumented kernel stores the float sums");
            return -22;
        }
        // The camera pre-pass (option cam_pre; k_cam_rays, k_path CAM): the
        // 5-wave sample kernels have twins that read the pass's camera samples
        // from the scene's buffer.  Taken when the buffer fits
        // (ensure_cam_rays); otherwise today's kernels, with the same image.
        // Nothing is kept across calls: the camera moves every frame in real
        // use, so the pre-pass runs in every such render, inside render_ms.
        const int cam_pre = o.cam_pre >= 0 ? o.cam_pre : kCamPreDefault;
        const int64_t cam_n = a.slots * (s1 - s0);
        // (a list pass: the entries of the listed pixels only, at their slots' places)
        const bool cam_on = waves5 && !help && cam_pre != 0 && ensure_cam_rays(s, sizeof(CamRay) * (size_t)cam_n);
        if (cam_on) {
            const uint32_t cnt = (uint32_t)(s1 - s0);
            pc.cam_rays = s.cam_rays.as<CamRay>();
            pc.cam_count = cnt;
            launch_cam_rays(s, as, s.cam_rays.as<CamRay>(), s.adapt_list, s.adapt_n);
            TMPT_HIP(hipGetLastError());
            s.cam_rays_used = 1;
        }
        // The shadow split (option shadow_split; k_path SPLIT, tmpt_shadow.hip):
        // the CAM kernels' twins queue their shadow queries for k_shadow and
        // leave sample records for k_split_resolve.  With the colour buffer's
        // units only (several blocks per pixel), for a whole plain render
        // (no progressive or adaptive pass, no float sums), and not where a
        // shadow answer can need the octree (oct_shadow: k_shadow does not
        // carry that check).  Taken when the records and a queue for the
        // worst case -- every bounce of every sample queues -- fit
        // (ensure_split); otherwise the fused kernels, with the same image.
        uint32_t sq_cap = 0;
        // (split_sub: a pass of render_split_passes, whose carried sums are a.prog)
        const bool split_on = o.shadow_split != 0 && cam_on && !sums && pc.sbuf && !s.adapt_on &&
                              (s.split_sub || (!pass && !a.prog)) && !oct_shadow &&
                              ensure_split(s, cam_n, (int64_t)std::max(grid5, grid6) * (kBlk / 64), sq_cap);
        if (split_on) {
            uint32_t* ctl = s.split_buf.as<uint32_t>();
            pc.sq_ctl = ctl;
            pc.sq = reinterpret_cast<uint4*>(ctl + kSplitCtlWords);
            pc.sq_cap = sq_cap;
            pc.srec = reinterpret_cast<float4*>(pc.sq + sq_cap);
            TMPT_HIP(hipMemsetAsync(ctl, 0, kSplitCtlWords * 4, s.stream));
            for (auto& e : s.split_ev) TMPT_HIP(e.ensure());
            s.split_used = 1;
        }
        // the launch's kernel: flagged ties deferred (TIES 1) with the redo list,
        // answered in the main loop (TIES 2) without
        PathVariant v_main = variant(w5, help, flag ? (redo ? 1 : 2) : 0, sums, cam_on ? 1 : 0);
        v_main.split = split_on ? 1 : 0;
        PathFn fn_main;
        int grid_main = 0;
        // The kernel of v_main and its grid.  The split's twin at 6 waves per
        // SIMD where the render wants it (want6) and six of its blocks are
        // co-resident on a CU by the occupancy query; otherwise the 5-wave
        // kernel: a kernel built for 80 VGPRs never runs at 5 waves.  The
        // launch's grid is the launched kernel's co-resident block count (the
        // deferred re-traces' completion count relies on it).
        auto pick_main = [&]() -> int {
            if (want6 && v_main.split && (o.path_waves == 6 || v_main.ties == 1)) {
                PathVariant v6 = v_main;
                v6.sl = kPathSL6;
                v6.occ = 6;
                PathFn fn6;
                if (int rc = find_path_kernel(v6, "tmpt_render", fn6)) return rc;
                if (occupancy_blocks((const void*)fn6, kBlk, 0) >= 6) {
                    v_main = v6;
                    fn_main = fn6;
                    grid_main = occupancy_grid((const void*)fn6, kBlk, 0, s.device);
                    return 0;
                }
            }
            v_main.sl = w5 ? kPathSL5 : kPathSL;
            v_main.occ = w5 ? 5 : prof ? 1 : 4;
            if (int rc = find_path_kernel(v_main, "tmpt_render", fn_main)) return rc;
            grid_main = occupancy_grid((const void*)fn_main, kBlk, 0, s.device);
            return 0;
        };
        if (int rc = pick_main()) return rc;
        // (the spill area of the launched grid at the launched kernel's LDS stack depth)
        if ((size_t)grid_main * kBlk * (kStackTotal - v_main.sl) > ovf_words) {
            set_error("tmpt_render: internal: stack spill area sized for fewer lanes");
            return -1;
        }
        s.path_waves_used = v_main.occ;
        s.tie_path = !oct ? 0 : redo ? 2 : redo_nomem ? 3 : 1;
        s.path_launches = 1;
        for (int attempt = 0;; ++attempt) {
            pc.redo = redo ? s.redo : nullptr;
            pc.redo_state = redo ? s.redo_state : nullptr;
            pc.redo_cap = redo ? s.redo_cap : 0u;
            pc.redo_inline = o.redo_inline ? 1u : 0u;
            pc.redo_lanes = (uint32_t)std::max(1, std::min(64, o.redo_lanes));
            if (redo) TMPT_HIP(hipMemsetAsync(s.redo, 0xFF, sizeof(uint2) * (size_t)s.redo_cap, s.stream));
            TMPT_HIP(hipEventRecord(s.path_ev[2], s.stream));
            fn_main<<<grid_main, kBlk, 0, s.stream>>>(view(s), as, pc, d_out, s.ws.as<uint32_t>(), d_counters);
            TMPT_HIP(hipGetLastError());
            TMPT_HIP(hipEventRecord(s.path_ev[3], s.stream));
            if (!redo) break;
            // the list's count and the entries the launch traced itself
            TMPT_HIP(hipMemcpyAsync(s.counters_host + kRedoCounter, d_counters + kRedoCounter,
                                    4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s.stream));
            TMPT_HIP(hipStreamSynchronize(s.stream));
            const unsigned long long n = s.counters_host[kRedoCounter];
            const unsigned long long traced = s.counters_host[kRedoTraced];
            s.redo_samples = (int64_t)n;
            if (n > s.redo_cap && attempt == 0) {
                // the list overflowed: grow it to the count (the same frame lists
                // the same samples) or, failing that, render with the exact kernel
                if (!(n < (1ull << 31) && alloc_redo(s, (int64_t)n))) {
                    redo = false;
                    v_main.ties = 2;  // the same kernel but for the ties: answered in the main loop
                    if (int rc = pick_main()) return rc;
                    if ((size_t)grid_main * kBlk * (kStackTotal - v_main.sl) > ovf_words) {
                        set_error("tmpt_render: internal: stack spill area sized for fewer lanes");
                        return -1;
                    }
                    s.path_waves_used = v_main.occ;
                    s.redo_samples = 0;
                    s.tie_path = 3;
                }
                TMPT_HIP(hipMemsetAsync(d_counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
                TMPT_HIP(hipMemsetAsync(heads, 0, head_words * 4, s.stream));
                if (split_on) TMPT_HIP(hipMemsetAsync(pc.sq_ctl, 0, kSplitCtlWords * 4, s.stream));
                continue;
            }
            s.redo_late = (int64_t)(std::min<unsigned long long>(n, s.redo_cap) - std::min(traced, n));
            if (traced < std::min<unsigned long long>(n, s.redo_cap)) {  // entries the launch left
                TMPT_HIP(hipEventRecord(s.path_ev[0], s.stream));
                if (split_on)
                    k_redo<kBlk, kPathSL, true><<<grid, kBlk, 0, s.stream>>>(view(s), as, s.redo, s.redo_cap,
                                                                            s.redo_state, pc.srec, pc.sb_ss, pc.sb_sp,
                                                                            s.ws.as<uint32_t>(), d_counters);
                else
                    k_redo<kBlk, kPathSL><<<grid, kBlk, 0, s.stream>>>(view(s), as, s.redo, s.redo_cap, s.redo_state,
                                                                      pc.sbuf, pc.sb_ss, pc.sb_sp, s.ws.as<uint32_t>(),
                                                                      d_counters);
                TMPT_HIP(hipGetLastError());
                TMPT_HIP(hipEventRecord(s.path_ev[1], s.stream));
                s.redo_launches = 1;  // timed apart from k_path (tmpt_stats.redo_ms)
            }
            break;
        }
        if (split_on) {
            // after k_path (and k_redo): the queued shadow queries, then the records
            TMPT_HIP(hipEventRecord(s.split_ev[0], s.stream));
            if (launch_shadow(s.stream, s.device, view(s), pc.sq, pc.sq_ctl, pc.sq_cap, pc.sq_ctl + kCtr, pc.srec,
                              (uint32_t)cam_n, s.ws.as<uint32_t>())) {
                set_error("tmpt_render: k_shadow launch failed");
                return -1;
            }
            TMPT_HIP(hipEventRecord(s.split_ev[1], s.stream));
            launch_split_resolve(s.stream, pc.srec, a.slots, (int32_t)(s1 - s0), a.out_recip, d_out,
                                 a.smp_begin > 0 ? a.prog : nullptr, a.prog);
            TMPT_HIP(hipGetLastError());
            TMPT_HIP(hipEventRecord(s.split_ev[2], s.stream));
            return 0;
        }
        // (tmpt_render_adaptive sums the pass's samples itself, k_adapt_update)
        if (pc.sbuf && !s.adapt_on) {
            // (a.prog: a progressive pass's carried sums, or tmpt_render_radiance's
            // float sums of a whole render; null for a plain tmpt_render)
            k_resolve_px<<<(unsigned)((a.slots + 63) / 64), 64, 0, s.stream>>>(
                pc.sbuf, a.slots, a.spp, a.out_recip, d_out, a.smp_begin, a.smp_end, a.prog);
            TMPT_HIP(hipGetLastError());
        }
        return 0;
    }
    s.tie_path = oct ? 1 : 0;  // pixel seeding answers in the main loop
    // both pixel launches run one kernel -- 4 or 5 waves, with or without the
    // helpers, ties flagged for the octree when it answers: their grid is its
    // own co-resident block count (`grid` above came from the two probes)
    PathFn fn;
    if (int rc = find_path_kernel(variant(w5, help, flag ? 2 : 0, false), "tmpt_render", fn)) return rc;
    const int grid_px = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    s.path_waves_used = w5 ? 5 : prof ? 1 : 4;
    if ((size_t)grid_px * kBlk * (kStackTotal - (waves5p ? kPathSL5 : kPathSL)) > ovf_words) {
        set_error("tmpt_render: internal: stack spill area sized for fewer lanes");
        return -1;
    }
    uint32_t* base = heads + head_words;
    float4* state = reinterpret_cast<float4*>(base);  // P x {colour sum, rng}
    uint32_t* cost = base + 4 * (size_t)P;
    uint32_t* keys = cost + P;
    uint32_t* vals = keys + P;
    uint32_t* tkeys = vals + P;
    uint32_t* tvals = tkeys + P;
    uint32_t* hist = tvals + P;
    uint32_t* simd_reg = hist + hist_words;
    RenderArgs a1 = a;  // pass 1: samples [0, pilot), per-pixel steps
    a1.smp_end = pilot;
    a1.out_recip = 1.0f / (float)pilot;
    a1.prog = state;
    pc.cost_out = cost;
    TMPT_HIP(hipEventRecord(s.path_ev[0], s.stream));
    fn<<<grid_px, kBlk, 0, s.stream>>>(view(s), a1, pc, d_out, s.ws.as<uint32_t>(), d_counters);
    TMPT_HIP(hipGetLastError());
    TMPT_HIP(hipEventRecord(s.path_ev[1], s.stream));
    k_order_keys<<<(unsigned)((P + 255) / 256), 256, 0, s.stream>>>(cost, a.W, a.tile_rows, keys, vals);
    const int which = radix_sort_pairs(keys, vals, tkeys, tvals, (int32_t)P, 16, hist, s.stream);
    TMPT_HIP(hipMemsetAsync(heads, 0, head_words * 4, s.stream));
    RenderArgs a2 = a;  // pass 2: samples [pilot, spp), most expensive pixels first
    a2.smp_begin = pilot;
    a2.prog = state;
    pc.cost_out = nullptr;
    pc.order = which ? tvals : vals;
    // Pixel chains (low load): at about one pixel per resident lane the frame
    // ends on the sample chains of its heaviest pixels.
    // The `chains` heaviest per 1024 (the head of the cost order) leave pass 2
    // and run as speculative chains instead -- render_rowspec's engine with one
    // pixel per chain: every even RNG offset of a window past the pilot's state
    // traced shadow-free, the chain walked through it, its samples traced again
    // in full -- so their samples run side by side, not in sequence.  Same
    // image: each sample is a pure function of (pixel, start state), summed in
    // sample order after the pilot's sum (k_resolve_chains).  Option pixel_chains.
    int64_t nch = 0;
    {
        int per1024 = 0;  // measured: no gain at the 1/8 shard, so off by default
        if (o.pixel_chains >= 0) per1024 = o.pixel_chains;
        nch = std::min<int64_t>(P, (P * per1024 + 1023) / 1024);
    }
    if (nch > 0) {
        const PixelChains ch{pc.order, state, (int)nch, pilot, a.spp - pilot};
        const int rc = render_rowspec(s, a, d_out, d_counters, &ch);
        if (rc < 0) return rc;
        if (rc == 0) {  // pass 2 takes the rest of the order
            pc.order += nch;
            pc.P = P - nch;
            pc.nchunks = (uint32_t)((pc.P + pc.chunk - 1) / pc.chunk);
        }
        s.chain_pixels = rc == 0 ? nch : 0;
    }
    if (pair > 0 && pair < 64 && pc.chunk == 64u) {
        uint32_t* paired = which ? vals : tvals;
        k_pair_order<<<(unsigned)((pc.P + 255) / 256), 256, 0, s.stream>>>(pc.order, pc.P, pair, paired);
        pc.order = paired;
    }
    // SIMD-balanced first chunks (PathCtl::simd_reg): with the chunks in
    // descending cost, the resident waves of every SIMD take one chunk from
    // each quarter, alternating ends, instead of the launch order's heaviest or
    // lightest of every quarter.  Option balance.
    if (o.balance) {
        int dev_cus = 0;
        if (hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, s.device) != hipSuccess ||
            dev_cus < 1)
            dev_cus = 256;
        const uint32_t per_cu = (uint32_t)std::max(1, grid_px / dev_cus);  // blocks per CU
        pc.simd_reg = simd_reg;
        pc.nsimd = (uint32_t)dev_cus * 4u;
        pc.wps = per_cu * (uint32_t)(kBlk / 64) / 4u;
        pc.claim = simd_reg + 2 * (size_t)kSimdKeys + 64;
        TMPT_HIP(hipMemsetAsync(simd_reg, 0, reg_words * 4, s.stream));
    }
    // Dynamic priority (PathCtl::dprio) in cost-ordered passes of up to ~12
    // pixels per resident lane: the heaviest waves start at the top level and
    // step down as their projected remaining work falls below 32 / 21 / 10.5 %
    // of the heaviest pixel's, so the issue slots go to the waves with the
    // most work left instead of to the oldest.  Bench frame, 1/8 shard 44.9 ->
    // 42.4 ms, 1/4 78.9 -> 75.3 ms (with the balanced first chunks; rounds
    // 1-2).  It was on only with the helpers until round 5, which measured it
    // without them (whole renders, on / off, profiles/r05_experiments/dprio_*):
    // 1080p N=1 207.1 / 209.8 ms (7.9 pixels per lane: the pass ends over
    // ~24 ms as the last pixels' 64-sample chains run out,
    // profiles/r05_wavetime/), 4K x 256 1/4 807.5 / 820.9 (7.9 per lane), but
    // 1/2 1550.4 / 1528.5 and N=1 3023.4 / 2969.0 (15.8 and 31.6 per lane: the
    // tail is short against the pass and the priority's own cost shows).
    // Option dprio.
    if (ordered && o.dprio && P <= 12 * lanes) {
        pc.dprio[0] = 0.32f;
        pc.dprio[1] = 0.21f;
        pc.dprio[2] = 0.105f;
        pc.dprio_cost = cost;
    }
    TMPT_HIP(hipEventRecord(s.path_ev[2], s.stream));
    fn<<<grid_px, kBlk, 0, s.stream>>>(view(s), a2, pc, d_out, s.ws.as<uint32_t>(), d_counters);
    TMPT_HIP(hipGetLastError());
    TMPT_HIP(hipEventRecord(s.path_ev[3], s.stream));
    s.path_launches = 2;
    // tmpt_render_radiance: pass 2 (and k_resolve_chains) left every pixel's
    // float sum in the pilot's state array
    if (a.prog)
        TMPT_HIP(hipMemcpyAsync(a.prog, state, sizeof(float4) * (size_t)P, hipMemcpyDeviceToDevice, s.stream));
    return 0;
}

// the render counters (device), their pinned host copy and the render's two
// timing events: created once per scene, so a render call costs no allocation
// (it matters for the small shards of a multi-GPU frame); the octree's
// counters live in the same array (Scene::ties)
int ensure_counters(Scene& s)
{
    if (s.counters) return 0;
    TMPT_ALLOC(s.counters.alloc(kRenderCounters * sizeof(unsigned long long)), "render counters");
    TMPT_HIP(hipMemset(s.counters, 0, kRenderCounters * sizeof(unsigned long long)));
    TMPT_HIP(s.counters_host.ensure(kRenderCounters * sizeof(unsigned long long)));
    for (auto& e : s.render_ev) TMPT_HIP(e.ensure());
    s.ties = s.counters + kTieCounter;
#ifdef TMPT_CHECK
    TMPT_ALLOC(s.chk.alloc(4 * sizeof(uint32_t)), "check words");
    TMPT_HIP(hipMemset(s.chk, 0, 4 * sizeof(uint32_t)));
#endif
    return 0;
}

// The checked build's report (tmpt_internal.h kChk*): after a call's kernels
// are done, kCheckError with the codes, the count and the last offending
// value when any index test failed (the word triple is cleared for the next
// call); 0 otherwise, and always 0 in the product build.
int check_report(Scene& s, const char* what)
{
#ifdef TMPT_CHECK
    if (!s.chk) return 0;
    uint32_t h[3] = {0, 0, 0};
    TMPT_HIP(hipDeviceSynchronize());
    TMPT_HIP(hipMemcpy(h, s.chk, sizeof(h), hipMemcpyDeviceToHost));
    if (h[0] == 0) return 0;
    TMPT_HIP(hipMemset(s.chk, 0, 4 * sizeof(uint32_t)));
    char msg[256];
    snprintf(msg, sizeof(msg),
             "%s: device index check failed: codes 0x%x (1 node, 2 leaf, 4 stack, 8 octree skip, 16 octree refs, "
             "32 triangle id), %u times, last value %d",
             what, h[0], h[1], (int)h[2]);
    fprintf(stderr, "tmpt: %s\n", msg);
    set_error(msg);
    return kCheckError;
#else
    (void)s;
    (void)what;
    return 0;
#endif
}

int upload_tables(DeviceBuffer<uint32_t>& dst, const std::vector<uint32_t>& tab, const char* what)
{
    DeviceBuffer<uint32_t> nt;
    TMPT_ALLOC(nt.alloc(tab.size() * sizeof(uint32_t)), what);
    if (hipMemcpy(nt, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        set_error(std::string(what) + ": jump table upload failed");
        return -1;
    }
    dst = std::move(nt);
    return 0;
}

// Option sample_base = B: table s holds J_(s + B), so every kernel's
// sample_seed(jt, s, ...) starts 2^16 (s + B) steps into the pixel's stream
// (setting the option drops the tables: jt_spp = 0)
int ensure_sample_tables(Scene& s, int32_t spp, const char* what)
{
    if (s.jt_spp >= spp) return 0;
    std::vector<uint32_t> tab;
    jump_tables(kSampleStride, spp, tab, (uint32_t)s.opt.sample_base);
    if (int rc = upload_tables(s.jt, tab, what)) return rc;
    s.jt_spp = spp;
    return 0;
}

int wait_caller_stream(Scene& s, const tmpt_render_desc* d, const char* what)
{
    if (!(d->flags & TMPT_FLAG_WAIT_STREAM)) return 0;  // order after the caller's stream (tmpt.h)
    TMPT_HIP(s.wait_ev.ensure(hipEventDisableTiming));
    hipError_t e = hipEventRecord(s.wait_ev, reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(d->wait_stream)));
    if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, s.wait_ev, 0);
    if (e != hipSuccess) {
        set_error(std::string(what) + ": wait_stream: " + hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// camera rays take the reference's root box test unless the whole lens
// (origin +- lens_radius along u and v) lies inside the root box by more
// than tMin and a rounding margin: a ray from inside always passes it
int32_t camera_root_check(const Scene& s, const Camera& cam)
{
    if (!(s.octree.oct && s.opt.tie_rule == 0)) return 0;
    const float o[3] = {cam.origin.x, cam.origin.y, cam.origin.z};
    const float uu[3] = {cam.u.x, cam.u.y, cam.u.z}, vv[3] = {cam.v.x, cam.v.y, cam.v.z};
    bool inside = true;
    for (int c = 0; c < 3; ++c) {
        const double r = (double)cam.lens_radius * (std::fabs((double)uu[c]) + std::fabs((double)vv[c]));
        const double m = 2.0 * kMinT + 1e-4 * ((double)s.octree.oct_hi[c] - (double)s.octree.oct_lo[c]);
        inside = inside && (double)o[c] - r > (double)s.octree.oct_lo[c] + m && (double)o[c] + r < (double)s.octree.oct_hi[c] - m;
    }
    return inside ? 0 : 1;
}

void reset_render_stats(Scene& s)
{
    s.extend_ms = s.shadow_ms = 0;
    s.extend_rays = s.shadow_rays = s.node_visits = s.tri_tests = 0;
    s.shadow_node_visits = s.shadow_tri_tests = 0;
    s.extend_launches = s.shadow_launches = s.iterations = 0;
    s.row_engine = 0;
    s.stream_fallbacks = 0;
    s.chain_pixels = 0;
    s.redo_samples = 0;
    s.redo_late = 0;
    s.redo_launches = 0;
    s.redo_ms = 0.0;
    s.redo_rays = 0;
    s.tie_path = 0;
    s.cam_rays_used = 0;
    s.split_used = 0;
    s.split_passes = 0;
    s.path_waves_used = 0;
    s.split_resolve_ms = 0.0;
}

// tmpt_camera_rays: the camera pre-pass of desc's pass alone, with the
// arguments a sample-seeded render of that desc gives it, into a buffer of its
// own; the entries copied to `out` (host memory).  The scene's progressive
// state, statistics and buffers are left alone.
int camera_rays(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* out)
{
    RenderArgs a = make_args(cam, d);
    if (int rc = ensure_sample_tables(s, a.spp, "tmpt_camera_rays")) return rc;
    a.jt = s.jt;
    a.root_check = camera_root_check(s, a.cam);
    const uint32_t cnt = (uint32_t)(a.smp_end - a.smp_begin);
    const int64_t n = a.slots * (int64_t)cnt;
    if (n <= 0) return 0;
    DeviceBuffer<CamRay> buf;
    if (!buf.alloc(sizeof(CamRay) * (size_t)n)) {
        set_error("tmpt_camera_rays: out of device memory");
        return -12;
    }
    launch_cam_rays(s, a, buf);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e == hipSuccess) e = hipMemcpy(out, buf, sizeof(CamRay) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("tmpt_camera_rays: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// The shadow split where the whole render's records and queue do not fit
// (option shadow_split_max, the device's free memory, or the 2^28 records a
// queue entry can name): the samples per pass that do, a multiple of the
// largest sample block (8) where it can be, else a power of two, so every
// pass starts on a block; 0: no split render (the option is off, or not even
// one sample of every pixel fits), >= spp: one pass, render_persistent's own.
static int32_t split_pass_samples(Scene& s, const RenderArgs& a)
{
    const Options& o = s.opt;
    if (o.shadow_split == 0 || !a.jt || a.slots <= 0 || o.path_waves == 4 || o.cam_pre == 0 || s.bvh.soa.na != nullptr ||
        oct_shadow_check(s))
        return 0;
    PathVariant probe5{};
    probe5.sl = kPathSL5;
    probe5.steps = kSampleSteps;
    probe5.shade_min = kShadeMin;
    probe5.occ = 5;
    probe5.samp = 1;
    probe5.ties = 1;
    PathFn fn;
    if (find_path_kernel(probe5, "tmpt_render", fn)) return 0;
    int64_t waves = (int64_t)occupancy_grid((const void*)fn, kBlk, 0, s.device) * (kBlk / 64);
    if (o.path_waves == 6 || (o.path_waves == 0 && kPathWaves6Auto != 0)) {  // the 6-wave twins' larger grid
        PathVariant probe6 = probe5;
        probe6.sl = kPathSL6;
        probe6.occ = 6;
        probe6.cam = 1;
        probe6.split = 1;
        if (find_path_kernel(probe6, "tmpt_render", fn)) return 0;
        waves = std::max(waves, (int64_t)occupancy_grid((const void*)fn, kBlk, 0, s.device) * (kBlk / 64));
    }
    const size_t budget = split_budget(s);
    uint32_t cap = 0;
    auto fits = [&](int64_t c) {
        if (o.shadow_split_pass > 0 && c > o.shadow_split_pass) return false;
        const size_t need = split_need(a.slots * c, waves, cap);
        return need != 0 && need <= budget;
    };
    if (fits(a.spp)) return a.spp;
    {  // several passes: each is a pass of render_persistent, which needs the colour buffer (its rule)
        const size_t need = sizeof(float4) * (size_t)a.spp * (size_t)a.slots;
        size_t sbuf_budget = free_budget(3, 4, s.sbuf.bytes());
        if (o.sbuf_max > 0.0) sbuf_budget = std::min(sbuf_budget, (size_t)o.sbuf_max);
        if (need > sbuf_budget) return 0;
    }
    int64_t c = 0;
    for (int64_t step = 1ll << 20; step >= 8; step >>= 1)  // the largest multiple of 8 that fits
        if (c + step < a.spp && fits(c + step)) c += step;
    if (c == 0)
        for (int64_t p = 4; p >= 1 && c == 0; p >>= 1)
            if (fits(p)) c = p;
    return (int32_t)c;
}

// ... and that render: passes of cs samples, each a pass of render_persistent
// (its shadow split between k_path and the resolve) that adds its samples, in
// order, to the pixels' float sums carried in Scene::split_carry, as a
// progressive pass adds to Scene::prog -- the same additions in the same order
// as one pass makes.  The counters add up on the device; the deferred ties'
// (a list per launch) start at zero in every pass.  The host waits once per
// pass, for its kernels' times.
static int render_split_passes(Scene& s, const RenderArgs& a, int32_t cs, uint32_t* d_out,
                               unsigned long long* d_counters)
{
    TMPT_ALLOC(s.split_carry.reserve(sizeof(float4) * (size_t)a.slots), "tmpt_render: the shadow split's carried sums");
    Scene::SplitAcc acc;
    int rc = 0;
    int32_t tie_path = 0, passes = 0;
    for (int32_t b = 0; b < a.spp && rc == 0; b += cs, ++passes) {
        RenderArgs ap = a;
        ap.smp_begin = b;
        ap.smp_end = std::min(b + cs, a.spp);
        ap.prog = s.split_carry;
        if (b > 0) {
            TMPT_HIP(hipMemsetAsync(d_counters + kRedoCounter, 0, 4 * sizeof(unsigned long long), s.stream));
            reset_render_stats(s);
        }
        s.split_sub = true;
        rc = render_persistent(s, ap, d_out, false, d_counters);
        s.split_sub = false;
        if (rc) break;
        TMPT_HIP(hipStreamSynchronize(s.stream));
        float k = 0.0f;
        (void)hipEventElapsedTime(&k, s.path_ev[2], s.path_ev[3]);
        acc.extend_ms += k;
        if (s.redo_launches) {
            (void)hipEventElapsedTime(&k, s.path_ev[0], s.path_ev[1]);
            acc.redo_ms += k;
        }
        if (s.split_used) {
            (void)hipEventElapsedTime(&k, s.split_ev[0], s.split_ev[1]);
            acc.shadow_ms += k;
            (void)hipEventElapsedTime(&k, s.split_ev[1], s.split_ev[2]);
            acc.resolve_ms += k;
        }
        acc.redo_samples += s.redo_samples;
        acc.redo_late += s.redo_late;
        acc.redo_launches += s.redo_launches;
        acc.launches += s.path_launches;
        acc.used += s.split_used;
        if (b == 0) tie_path = s.tie_path;
    }
    if (rc) return rc;
    s.split_acc = acc;
    s.split_passes = passes;
    s.tie_path = tie_path;
    return 0;
}

// tmpt_render_radiance's last step: the float sums {r, g, b, -} the render left
// per pixel become the float frame {sum * spp_recip, 1.0f}, in place
// (main.cpp:221: col *= spp_recip, before the sqrtf of :224)
__global__ void __launch_bounds__(256) k_radiance_scale(float4* __restrict__ px, int64_t n, float spp_recip)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = px[i];
    const f3 col = mk(c.x, c.y, c.z) * spp_recip;
    px[i] = make_float4(col.x, col.y, col.z, 1.0f);
}

// d_sums (tmpt_render_radiance: a whole render on the persistent engine in
// pixel or sample seeding, checked by the caller; null for tmpt_render): one
// float4 per pixel of the tile, which the render's own stores of the float
// colour sum fill (RenderArgs::prog: k_path in pixel seeding, k_resolve_px or
// k_path<SUMS> in sample seeding) and k_radiance_scale then scales.  The
// launch plan (units, blocks, grids, passes) does not depend on it, and the
// scene's progressive state is not touched: the sums are this buffer's, not
// Scene::prog's.
int render(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* d_out,
           uint64_t* ray_count, float4* d_sums)
{
    RenderArgs a = make_args(cam, d);
    bool count = (d->flags & TMPT_FLAG_COUNT_VISITS) != 0;
    s.row_render = d->seed_mode == TMPT_SEED_ROW;  // view(): shadow_order's default
    s.pixel_render = d->seed_mode == TMPT_SEED_PIXEL;  // view(): pop_cull's default
    // progressive spp: keep per-pixel state for the shard between calls
    const bool progressive = a.smp_begin > 0 || a.smp_end < a.spp;
    if (progressive) {
        const int32_t key[6] = {d->width, d->height, d->spp, a.band_rows, a.shard, a.nshards};
        // the carried colour sums and RNG states belong to one camera: a pass
        // with another camera (or seeding) must not blend into them
        uint64_t cam_key = 1469598103934665603ull;
        const unsigned char* cb = reinterpret_cast<const unsigned char*>(cam);
        for (size_t i = 0; i < sizeof(tmpt_camera); ++i) cam_key = (cam_key ^ cb[i]) * 1099511628211ull;
        cam_key = (cam_key ^ (uint32_t)d->seed_mode) * 1099511628211ull;
        if (a.smp_begin > 0 &&
            (memcmp(key, s.prog_key, sizeof(key)) != 0 || s.prog_key[6] != a.smp_begin || s.prog_cam != cam_key)) {
            set_error("tmpt_render: spp_begin does not continue the previous pass of this shard "
                      "(same camera, size, spp and shard)");
            return -22;
        }
        s.prog_cam = cam_key;
        TMPT_ALLOC(s.prog.reserve(sizeof(float4) * (size_t)a.slots), "tmpt_render: the progressive sums");
        a.prog = s.prog;
        memcpy(s.prog_key, key, sizeof(key));
        s.prog_key[6] = -1;  // valid again only once this pass completes
    } else if (d_sums) {
        a.prog = d_sums;
    }
    if (a.seed_mode == TMPT_SEED_SAMPLE) {  // jump tables of sample_seed, grown to spp
        if (int rc = ensure_sample_tables(s, a.spp, "tmpt_render")) return rc;
        a.jt = s.jt;
    }
    if (int rc = wait_caller_stream(s, d, "tmpt_render")) return rc;
    if (ensure_counters(s)) return -1;
    a.root_check = camera_root_check(s, a.cam);
    unsigned long long* d_counters = s.counters;
    TMPT_HIP(hipMemsetAsync(d_counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    int rc = 0;
    const bool wave = d->engine == TMPT_ENGINE_WAVEFRONT && a.seed_mode != TMPT_SEED_ROW;
    const bool persistent = d->engine == TMPT_ENGINE_PERSISTENT && a.seed_mode != TMPT_SEED_ROW;
    // row seeding on the persistent engine: the speculative row chains
    // (render_rowspec); instrumented renders and option rowspec=0 run the
    // megakernel's one lane per row
    const bool rowspec = d->engine == TMPT_ENGINE_PERSISTENT && a.seed_mode == TMPT_SEED_ROW && !count &&
                         !progressive && s.opt.rowspec != 0;
    if (progressive && !persistent) {
        set_error("tmpt_render: progressive spp needs the persistent engine");
        return -22;
    }
    reset_render_stats(s);
    if (a.slots > 0) {
        if (wave) rc = render_wavefront(s, a, d_out, count);
        else if (persistent) {
            // (the shadow split in several passes where one pass's buffers do not fit)
            const int32_t cs = !count && !progressive && !d_sums ? split_pass_samples(s, a) : 0;
            rc = cs > 0 && cs < a.spp ? render_split_passes(s, a, cs, d_out, d_counters)
                                      : render_persistent(s, a, d_out, count, d_counters);
        } else if (rowspec) {
            // the streaming engine, or the iterated one where it does not apply
            rc = s.opt.rowspec_stream != 0 && s.opt.rowspec_noshadow != 0 ? render_rowstream(s, a, d_out, d_counters)
                                                                          : 1;
            s.row_engine = rc == 0 ? 3 : 2;
            if (rc == 2) {  // the streaming launch aborted: its counters are partial, start over
                s.stream_fallbacks = 1;
                TMPT_HIP(hipMemsetAsync(d_counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
            }
            if (rc == 1 || rc == 2) rc = render_rowspec(s, a, d_out, d_counters);
        } else {
            rc = render_megakernel(s, a, d_out, count, d_counters);
            if (a.seed_mode == TMPT_SEED_ROW) s.row_engine = 1;
        }
        if (rc == 0 && d_sums) {
            k_radiance_scale<<<(unsigned)((a.slots + 255) / 256), 256, 0, s.stream>>>(d_sums, a.slots, a.spp_recip);
            if (hipGetLastError() != hipSuccess) rc = (set_error("tmpt_render_radiance: scale launch failed"), -1);
        }
    }
    (void)hipEventRecord(e1, s.stream);
    hipError_t se = rc == 0 ? hipMemcpyAsync(s.counters_host, d_counters, kRenderCounters * sizeof(unsigned long long),
                                             hipMemcpyDeviceToHost, s.stream)
                            : hipSuccess;
    const hipError_t se2 = hipStreamSynchronize(s.stream);
    if (se == hipSuccess) se = se2;
    unsigned long long c[kRenderCounters] = {};
    if (rc == 0 && se == hipSuccess) memcpy(c, s.counters_host, sizeof(c));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (rc) return rc;
    if (se != hipSuccess) {
        set_error(std::string("render: ") + hipGetErrorString(se));
        return -1;
    }
    if (c[kSplitOverflowCounter]) {
        set_error("tmpt_render: internal: the shadow split's queue overflowed");
        return -1;
    }
    s.render_ms = ms;
    s.tie_queries = c[kTieCounter];
    s.root_misses = c[kTieCounter + 1];
    s.crack_queries = c[kCrackCounter];
#ifdef TMPT_EXP_WAVETIME
    {
        std::vector<unsigned long long> w(3 * kWaveTimeMax, 0ull);
        if (wavetime_get(w.data())) {
            std::vector<double> st, ml, ex;
            unsigned long long t0 = ~0ull;
            for (int i = 0; i < kWaveTimeMax; ++i)
                if (w[3 * i] && w[3 * i + 2]) t0 = std::min(t0, w[3 * i]);
            for (int i = 0; i < kWaveTimeMax; ++i)
                if (w[3 * i] && w[3 * i + 2]) {
                    st.push_back((w[3 * i] - t0) * 0.01);  // 100 MHz ticks -> us
                    ml.push_back((w[3 * i + 1] - t0) * 0.01);
                    ex.push_back((w[3 * i + 2] - t0) * 0.01);
                }
            auto pct = [](std::vector<double> v, double q) {
                if (v.empty()) return 0.0;
                std::sort(v.begin(), v.end());
                return v[std::min(v.size() - 1, (size_t)(q * (v.size() - 1)))];
            };
            fprintf(stderr, "waves %zu; start us p0/p50/p100 %.0f/%.0f/%.0f; main loop end p0/p10/p50/p90/p100 "
                            "%.0f/%.0f/%.0f/%.0f/%.0f; exit p0/p50/p99/p100 %.0f/%.0f/%.0f/%.0f\n",
                    st.size(), pct(st, 0), pct(st, 0.5), pct(st, 1), pct(ml, 0), pct(ml, 0.1), pct(ml, 0.5),
                    pct(ml, 0.9), pct(ml, 1), pct(ex, 0), pct(ex, 0.5), pct(ex, 0.99), pct(ex, 1));
            std::fill(w.begin(), w.end(), 0ull);
            wavetime_put(w.data());
        }
    }
#endif
    if (progressive) s.prog_key[6] = a.smp_end < a.spp ? a.smp_end : -1;
    if (persistent) {  // one kernel for both query kinds
        // k_path launches only (the render's other kernels: order keys, sort,
        // resolve, memsets excluded)
        float k1 = 0.0f, k0 = 0.0f;
        (void)hipEventElapsedTime(&k1, s.path_ev[2], s.path_ev[3]);
        if (s.path_launches == 2) (void)hipEventElapsedTime(&k0, s.path_ev[0], s.path_ev[1]);
        s.extend_ms = (double)k0 + (double)k1;
        if (s.redo_launches) {  // the k_redo launch after the main one: its own figure
            float kr = 0.0f;
            (void)hipEventElapsedTime(&kr, s.path_ev[0], s.path_ev[1]);
            s.redo_ms = kr;
            s.redo_rays = c[kRedoRaysCounter];
        }
        if (s.split_passes > 1) {  // render_split_passes: its passes' sums
            const Scene::SplitAcc& acc = s.split_acc;
            s.extend_ms = acc.extend_ms;
            s.shadow_ms = acc.shadow_ms;
            s.split_resolve_ms = acc.resolve_ms;
            s.redo_ms = acc.redo_ms;
            s.redo_samples = acc.redo_samples;
            s.redo_late = acc.redo_late;
            s.redo_launches = acc.redo_launches;
            s.redo_rays = c[kRedoRaysCounter];
            s.path_launches = acc.launches;
            s.shadow_launches = s.split_used = acc.used;
        } else if (s.split_used) {  // the shadow split: k_shadow's time apart from the twin's
            float ks = 0.0f, kr = 0.0f;
            (void)hipEventElapsedTime(&ks, s.split_ev[0], s.split_ev[1]);
            (void)hipEventElapsedTime(&kr, s.split_ev[1], s.split_ev[2]);
            s.shadow_ms = ks;
            s.split_resolve_ms = kr;
            s.shadow_launches = 1;
        }
        s.extend_rays = c[3];
        s.shadow_rays = c[0] - c[3];
        s.node_visits = c[1];
        s.tri_tests = c[2];
        s.shadow_node_visits = c[4];
        s.shadow_tri_tests = c[5];
        s.extend_launches = s.path_launches;  // same k_path instantiation per launch
        s.iterations = 1;
#ifdef TMPT_DIAG
        if (c[13] + c[14] + c[15]) {
            const double tot = (double)(c[13] + c[14] + c[15]);
            fprintf(stderr, "k_path wave time: shading %.1f%%, node rounds %.1f%%, leaf rounds %.1f%% "
                            "(%.3g wave-cycles)\n",
                    100.0 * c[13] / tot, 100.0 * c[14] / tot, 100.0 * c[15] / tot, tot);
            if (c[6] && c[8] && c[10])
                fprintf(stderr, "  cycles per round: node %.0f (%.1f lanes), leaf %.0f (%.1f lanes), shading %.0f "
                                "(%.1f lanes shading, %.1f traversing); rounds node %llu leaf %llu shading %llu\n",
                        (double)c[14] / c[6], (double)c[7] / c[6], (double)c[15] / c[8], (double)c[9] / c[8],
                        (double)c[13] / c[10], (double)c[11] / c[10], (double)c[12] / c[10], c[6], c[8], c[10]);
            if (c[16] + c[17] + c[18] + c[19])
                fprintf(stderr, "  shading split: ballots+pixel fetch %.1f%%, shade/finish %.1f%%, camera %.1f%%, "
                                "query set-up %.1f%% (of all wave time)\n",
                        100.0 * c[16] / tot, 100.0 * c[17] / tot, 100.0 * c[18] / tot, 100.0 * c[19] / tot);
            if (c[kCamCounter])
                fprintf(stderr, "  camera block: runs in %llu of %llu shading rounds (%.3f), %.2f lanes per run\n",
                        c[kCamCounter + 1], c[kCamCounter], (double)c[kCamCounter + 1] / c[kCamCounter],
                        c[kCamCounter + 1] ? (double)c[kCamCounter + 2] / c[kCamCounter + 1] : 0.0);
        }
        if (count && getenv("TMPT_ROUND_LOG"))  // wave-round efficiency
            fprintf(stderr,
                    "k_path rounds: node %llu (%.1f lanes), leaf %llu (%.1f lanes), shade %llu "
                    "(%.1f wanting, %.1f traversing)\n",
                    c[6], c[6] ? (double)c[7] / c[6] : 0.0, c[8], c[8] ? (double)c[9] / c[8] : 0.0,
                    c[10], c[10] ? (double)c[11] / c[10] : 0.0, c[10] ? (double)c[12] / c[10] : 0.0);
        if (count && getenv("TMPT_ROUND_LOG")) {  // pop culling (kWalkCounter) and the work per closest-hit query
            const unsigned long long* w = c + kWalkCounter;
            const SceneView sv = view(s);
            fprintf(stderr,
                    "k_path walk: %d key bits, culling %s; per closest-hit query %.3f node visits, %.3f triangle "
                    "tests; stale pops discarded %llu (%.4f of closest-hit node visits and discards), followed by another "
                    "stale entry %.4f\n",
                    pop_key_bits(s.bvh.link_bits, s.opt.pop_key_cap), sv.key_mask ? "on" : "off",
                    c[3] ? (double)c[1] / c[3] : 0.0, c[3] ? (double)c[2] / c[3] : 0.0, w[0],
                    c[1] + w[0] ? (double)w[0] / (double)(c[1] + w[0]) : 0.0,
                    w[0] ? (double)w[1] / w[0] : 0.0);
        }
        {  // the top levels' share (k_path tv_*, tw_*, pt_top, pt_node_g)
            const unsigned long long* t = c + kTopCounter;
            const unsigned long long nv = c[1] + c[4];
            if (count && getenv("TMPT_ROUND_LOG") && nv)
                fprintf(stderr,
                        "k_path top levels: %.4f of node lane-steps on an LDS node, %.4f of those before the query's "
                        "first other step (%.2f per query); voted node rounds with LDS lanes %.4f, of them mixed "
                        "with global lanes %.4f; top-walk rounds %llu (%.1f lanes)\n",
                        (double)t[0] / nv, t[0] ? (double)t[1] / t[0] : 0.0, (double)t[1] / (double)c[0],
                        c[6] ? (double)(t[2] + t[3]) / c[6] : 0.0, t[2] + t[3] ? (double)t[2] / (t[2] + t[3]) : 0.0,
                        t[4], t[4] ? (double)t[5] / t[4] : 0.0);
            if (t[9])
                fprintf(stderr,
                        "  node rounds with a global-side lane: %llu of %llu, %.0f cycles each; without: %.0f cycles "
                        "each; top-walk rounds %llu (%.1f lanes), %.0f cycles each, %.2f%% of wave time\n",
                        t[8], t[9], t[8] ? (double)t[7] / t[8] : 0.0,
                        t[9] > t[8] ? (double)(c[14] - t[7]) / (t[9] - t[8]) : 0.0, t[4],
                        t[4] ? (double)t[5] / t[4] : 0.0, t[4] ? (double)t[6] / t[4] : 0.0,
                        100.0 * t[6] / (double)(c[13] + c[14] + c[15] + t[6]));
        }
#endif
    } else if (rowspec) {
        s.extend_ms = ms;
        s.extend_rays = c[3];
        s.shadow_rays = c[0] - c[3];
        s.extend_launches = s.path_launches;
        s.iterations = s.path_launches;
    } else if (!wave) {
        s.extend_ms = ms;
        s.extend_rays = c[0];
        s.node_visits = c[1];
        s.tri_tests = c[2];
        s.extend_launches = 1;
    }
    if (ray_count) *ray_count = wave ? (s.extend_rays + s.shadow_rays) : c[0];
    return 0;
}

}  // namespace tmpt
