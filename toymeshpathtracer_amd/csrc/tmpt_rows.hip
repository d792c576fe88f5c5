// tmpt_rows.hip -- the two row engines (row seeding on the persistent engine):
// the iterated speculative chains (render_rowspec, k_rs_*; also
// render_persistent's pixel chains) and the streaming engine
// (render_rowstream, k_rss_*).  Both launch k_path's row variants, which they
// get as pointers from find_path_kernel (tmpt_path.h).  render() in
// tmpt_render.hip calls both, render_persistent (there too) render_rowspec.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "tmpt_path.h"

namespace tmpt {

// ============================================================ speculative row seeding
// Row seeding (main.cpp:204) threads ONE xorshift stream through a row's
// pixels and samples, and a sample's draws depend on its path, so a row is a
// sequential chain (the megakernel runs one lane per row).  But a sample is
// a pure function of (pixel, start state), and every draw site takes two
// draws (maths.cpp:25, 32-33, main.cpp:214-215), so the next sample starts
// an even number of draws after this one's start.  render_rowspec traces,
// for each row, one sample at EVERY even offset 2j of a window past the
// row's current state (units of k_path<SAMP 2>), then a chase walks the
// chain through the window: take the sample at offset 0, add its colour in
// sample order, jump to offset + its draws, ...  Each window costs ~draws/2
// traces per chain sample (speculation), but all of them run in parallel.
constexpr int kRsMaxWin = 32;  // windows per row and iteration: this pixel + up to 31 lookaheads

struct RowSpec {
    int row0, nrows;  // this group's tile rows [row0, row0 + nrows)
    // per row of the group: chain state, current pixel and samples done in it,
    // its draws so far and the previous pixel's mean draws per sample (window
    // sizing), chain rays (all, closest-hit), unit offsets (nrows + 1)
    uint32_t *rng, *x, *k, *pdraws, *prev_mean, *rays, *erays, *offs;
    // window i (pixel x + i) of row r: offsets [ws[i*nrows + r], + win[i*nrows + r]);
    // window 0 starts at 0; win = 0: none
    uint32_t *win, *ws;
    uint32_t* short_win;  // iterations whose window ended before the pixel did (diagnostic)
    float4* col;
    uint32_t* total;  // units of this iteration
    unsigned long long* planned;  // units over all iterations (diagnostic)
    uint32_t wmax;
    float spread;   // windows from expected positions +- spread * sqrt(i) pixels
    int nwin;       // windows per row (1 = no lookahead)
    // no-shadow speculation: the chase lists the chain's samples (tile pixel,
    // start state, sample index) for the full re-trace; scratch holds a row's
    // (unit, sample index) pairs of one iteration (scap per row)
    uint32_t *lpix, *lstate, *lslot, *lcount;
    uint2* scratch;
    uint32_t scap;
    // Chains: a row is a chain of cw = W pixels x cspp = spp samples from the
    // row seed.  Pixel chains (pixel seeding, render_pixel_chains): chain r is
    // tile pixel cpix[r] alone (cw = 1), its samples smp0 .. smp0 + cspp - 1,
    // from the RNG state the pilot pass left in cinit[pixel].w.
    const uint32_t* cpix;
    const float4* cinit;
    int cw, cspp, smp0;
};

// Decode of a unit's rs_out.w: draws | rays << 23 | extend rays << 28.
constexpr uint32_t kRsDrawBits = 23;

__global__ void __launch_bounds__(256) k_rs_init(RenderArgs a, RowSpec rs)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rs.nrows) return;
    rs.rng[r] = rs.cpix ? __float_as_uint(rs.cinit[rs.cpix[r]].w)           // pixel chain: after its pilot
                        : row_seed((uint32_t)tile_row_to_y(a, rs.row0 + r));  // main.cpp:204, unmodified
    rs.x[r] = rs.k[r] = rs.pdraws[r] = rs.rays[r] = rs.erays[r] = rs.short_win[r] = 0u;
    rs.prev_mean[r] = __float_as_uint(17.0f);  // draws per sample before any is seen
    rs.col[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Windows per row.  E = a pixel's expected units (spp x mean draws per
// sample / 2: even offsets only), the mean the larger of this pixel's so far
// and the previous pixel's.  Pixel x + i is expected to start c_i = e0 +
// (i - 1) E units ahead (e0 = this pixel's expected rest) and end c_i + E,
// each give or take spread * sqrt(i) * E; window i spans its start's and its
// end's ranges (window 0 starts at 0).  Exclusive scan into offs; total units.
// One block.
__global__ void __launch_bounds__(1024) k_rs_plan(RenderArgs a, RowSpec rs)
{
    __shared__ uint32_t part[1024];
    const int rows = rs.nrows;
    const int per = (rows + 1023) / 1024;
    const int r0 = min(rows, (int)threadIdx.x * per), r1 = min(rows, r0 + per);
    uint32_t sum = 0;
    for (int r = r0; r < r1; ++r) {
        const uint32_t x = rs.x[r];
        uint32_t t = 0;  // end of the previous window
        float mean = 0.0f, e0 = 0.0f, E = 0.0f;
        if (x < (uint32_t)rs.cw) {
            const uint32_t k = rs.k[r];
            mean = __uint_as_float(rs.prev_mean[r]);
            if (k > 0) mean = fmaxf(mean, (float)rs.pdraws[r] / (float)k);
            e0 = (float)((uint32_t)rs.cspp - k) * mean * 0.5f;  // expected units to this pixel's end
            E = (float)rs.cspp * mean * 0.5f;                   // ... of one whole pixel
        }
        for (int i = 0; i < rs.nwin; ++i) {
            uint32_t w = 0, s = 0;
            if (x + (uint32_t)i < (uint32_t)rs.cw) {
                const float ci = i == 0 ? 0.0f : e0 + (float)(i - 1) * E;
                const float ui = i == 0 ? 0.0f : rs.spread * sqrtf((float)i) * E;
                const float ce = e0 + (float)i * E, ue = rs.spread * sqrtf((float)(i + 1)) * E;
                s = i == 0 ? 0u : min(t, (uint32_t)fmaxf(0.0f, ci - ui));
                w = min(rs.wmax, (uint32_t)(ce + ue) + 2u - min(s, (uint32_t)(ce + ue)));
                t = s + w;
            }
            rs.win[i * rows + r] = w;
            rs.ws[i * rows + r] = s;
            sum += w;
        }
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // inclusive scan of the thread sums
        const uint32_t v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t o = part[threadIdx.x] - sum;
    for (int r = r0; r < r1; ++r) {
        rs.offs[r] = o;
        for (int i = 0; i < rs.nwin; ++i) o += rs.win[i * rows + r];
    }
    if (threadIdx.x == 1023) {
        rs.offs[rows] = part[1023];
        *rs.total = part[1023];
        atomicAdd(rs.planned, (unsigned long long)part[1023]);
    }
}

// Unit u -> (row, window i, offset index j): pixel x + i and start state
// M^(2j) rng[row].  Launched over the largest possible count; the plan's
// total bounds it.
__global__ void __launch_bounds__(256) k_rs_fill(RenderArgs a, RowSpec rs, const uint32_t* __restrict__ jt2,
                                                 uint32_t* __restrict__ upix, uint32_t* __restrict__ ustate)
{
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= *rs.total) return;
    int lo = 0, hi = rs.nrows - 1;  // last row with offs <= u
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rs.offs[mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    uint32_t l = u - rs.offs[lo];
    int i = 0;
    for (; i + 1 < rs.nwin && l >= rs.win[i * rs.nrows + lo]; ++i) l -= rs.win[i * rs.nrows + lo];
    const uint32_t j = rs.ws[i * rs.nrows + lo] + l;
    upix[u] = rs.cpix ? rs.cpix[lo] : (uint32_t)(rs.row0 + lo) * (uint32_t)a.W + rs.x[lo] + (uint32_t)i;
    ustate[u] = sample_seed(jt2, j, rs.rng[lo]);
}

// The chase, one thread per row: the chain's samples in order through the
// windows (main.cpp:209-219), each pixel packed after its spp-th (:221-233);
// on into window i + 1 when the next pixel's first sample falls in it.
__global__ void __launch_bounds__(64) k_rs_chase(RenderArgs a, RowSpec rs, const float4* __restrict__ rs_out,
                                                 const uint32_t* __restrict__ rs_end, uint32_t* __restrict__ out,
                                                 const uint32_t* __restrict__ upix, const uint32_t* __restrict__ ustate)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    const int rows = rs.nrows;
    const bool listing = rs.lpix != nullptr;  // no-shadow speculation: list the chain, no colours
    uint32_t n = r < rows ? rs.win[r] : 0u, nl = 0;
    if (n > 0) {
        uint32_t k = rs.k[r], x = rs.x[r], pdraws = rs.pdraws[r], rays = rs.rays[r], erays = rs.erays[r];
        const float4 c0 = rs.col[r];
        f3 col = mk(c0.x, c0.y, c0.z);
        // window i: offsets [lo, lo + n) at wb
        uint32_t j = 0, last = 0xFFFFFFFFu, lo = 0, wb = rs.offs[r];
        int i = 0;
        while (j >= lo && j - lo < n) {
            const uint32_t idx = wb + (j - lo);
            const float4 t = rs_out[idx];
            const uint32_t w = __float_as_uint(t.w);
            const uint32_t draws = w & ((1u << kRsDrawBits) - 1u);
            rays += (w >> kRsDrawBits) & 31u;
            erays += w >> 28;
            pdraws += draws;
            if (listing) rs.scratch[(size_t)r * rs.scap + nl++] = make_uint2(idx, (uint32_t)rs.smp0 + k);
            else col = col + mk(t.x, t.y, t.z);  // col += Trace(...), main.cpp:218
            last = idx;
            j += draws >> 1;
            if (++k == (uint32_t)rs.cspp) {  // the rest of this window belongs to this pixel: dropped
                if (!listing) out[(size_t)(rs.row0 + r) * a.W + x] = pack_pixel(col, a.spp_recip);
                rs.prev_mean[r] = __float_as_uint((float)pdraws / (float)k);
                ++x;
                k = 0;
                pdraws = 0;
                col = mk(0.0f, 0.0f, 0.0f);
                if (++i >= rs.nwin) break;
                wb += n;
                n = rs.win[i * rows + r];
                lo = rs.ws[i * rows + r];
                if (n == 0) break;
            }
        }
        if (last != 0xFFFFFFFFu) rs.rng[r] = rs_end[last];  // the next sample's start state
        if (k != 0) ++rs.short_win[r];
        rs.k[r] = k;
        rs.x[r] = x;
        rs.pdraws[r] = pdraws;
        rs.rays[r] = rays;
        rs.erays[r] = erays;
        rs.col[r] = make_float4(col.x, col.y, col.z, 0.0f);
    }
    if (!listing) return;
    // the row's chain samples into the frame's list: one atomic per wave
    uint32_t incl = nl;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
        if ((threadIdx.x & 63) >= (unsigned)off) incl += v;
    }
    uint32_t base = 0;
    if ((threadIdx.x & 63) == 63) base = atomicAdd(rs.lcount, incl);
    base = (uint32_t)__shfl((int)base, 63) + incl - nl;
    for (uint32_t t = 0; t < nl; ++t) {
        const uint2 e = rs.scratch[(size_t)r * rs.scap + t];
        rs.lpix[base + t] = upix[e.x];
        rs.lstate[base + t] = ustate[e.x];
        rs.lslot[base + t] = e.y;
    }
}

// The same chase for the listing (shadow-free) pass, one wave per row: the
// row's unit words are staged in LDS with coalesced loads first, so the
// chain's walk -- one dependent read per chain sample -- runs on LDS latency
// instead of a global round trip each (the one-thread-per-row kernel spent
// ~3.6 us per chain sample there).  The chain's (unit, sample) pairs collect
// in LDS and the wave copies them into the frame's list.  Rows with more
// units than kChaseUnits walk from global memory; the host only picks this
// kernel when a row's chain samples per iteration fit kChaseList.
constexpr uint32_t kChaseUnits = 8192, kChaseList = 2048;
__global__ void __launch_bounds__(64) k_rs_chase_lds(RenderArgs a, RowSpec rs, const float4* __restrict__ rs_out,
                                                     const uint32_t* __restrict__ rs_end,
                                                     const uint32_t* __restrict__ upix,
                                                     const uint32_t* __restrict__ ustate)
{
    __shared__ uint32_t s_w[kChaseUnits];
    __shared__ uint2 s_l[kChaseList];
    __shared__ uint32_t s_n, s_base;
    const int r = blockIdx.x;
    const int rows = rs.nrows;
    const uint32_t lane = threadIdx.x;
    if (rs.win[r] == 0) return;  // row finished (block-uniform)
    const uint32_t u0 = rs.offs[r], nu = rs.offs[r + 1] - u0;
    const bool staged = nu <= kChaseUnits;
    if (staged)
        for (uint32_t i = lane; i < nu; i += 64) s_w[i] = __float_as_uint(rs_out[u0 + i].w);
    __syncthreads();
    if (lane == 0) {
        uint32_t k = rs.k[r], x = rs.x[r], pdraws = rs.pdraws[r], rays = rs.rays[r], erays = rs.erays[r];
        uint32_t n = rs.win[r], nl = 0;
        uint32_t j = 0, last = 0xFFFFFFFFu, lo = 0, wb = u0;
        int i = 0;
        while (j >= lo && j - lo < n) {
            const uint32_t idx = wb + (j - lo);
            const uint32_t w = staged ? s_w[idx - u0] : __float_as_uint(rs_out[idx].w);
            const uint32_t draws = w & ((1u << kRsDrawBits) - 1u);
            rays += (w >> kRsDrawBits) & 31u;
            erays += w >> 28;
            pdraws += draws;
            s_l[nl++] = make_uint2(idx, (uint32_t)rs.smp0 + k);
            last = idx;
            j += draws >> 1;
            if (++k == (uint32_t)rs.cspp) {  // the rest of this window belongs to this pixel: dropped
                rs.prev_mean[r] = __float_as_uint((float)pdraws / (float)k);
                ++x;
                k = 0;
                pdraws = 0;
                if (++i >= rs.nwin) break;
                wb += n;
                n = rs.win[i * rows + r];
                lo = rs.ws[i * rows + r];
                if (n == 0) break;
            }
        }
        if (last != 0xFFFFFFFFu) rs.rng[r] = rs_end[last];  // the next sample's start state
        if (k != 0) ++rs.short_win[r];
        rs.k[r] = k;
        rs.x[r] = x;
        rs.pdraws[r] = pdraws;
        rs.rays[r] = rays;
        rs.erays[r] = erays;
        s_n = nl;
        s_base = nl ? atomicAdd(rs.lcount, nl) : 0u;
    }
    __syncthreads();
    const uint32_t nl = s_n, base = s_base;
    for (uint32_t t = lane; t < nl; t += 64) {
        const uint2 e = s_l[t];
        rs.lpix[base + t] = upix[e.x];
        rs.lstate[base + t] = ustate[e.x];
        rs.lslot[base + t] = e.y;
    }
}

// render_rowstream: each row's anchor states M^(2^15 a) row_seed, a < na, from
// the byte tables of M^(2^15 a0) (j1) and M^(2^20 a1) (j2), a = 32 a1 + a0;
// thread 0 also publishes the final pass's unit count.
__global__ void __launch_bounds__(256) k_rss_anchors(RenderArgs a, RsStream S, const uint32_t* __restrict__ j1,
                                                     const uint32_t* __restrict__ j2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) S.ctl[4] = (uint32_t)((size_t)a.slots * (size_t)a.spp);
    if (i >= (size_t)S.nrows * S.na) return;
    const int row = (int)(i / S.na);
    const uint32_t an = (uint32_t)(i - (size_t)row * S.na);
    const uint32_t seed = row_seed((uint32_t)tile_row_to_y(a, row));  // main.cpp:204, unmodified
    const_cast<uint32_t*>(S.anchors)[i] = sample_seed(j2, an >> 5, sample_seed(j1, an & 31u, seed));
}

// The chain list's offsets -> start states, in place (unit u: row u / spp / W).
__global__ void __launch_bounds__(256) k_rss_states(RenderArgs a, RsStream S)
{
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (size_t)a.slots * (size_t)a.spp) return;
    const int row = (int)(u / ((size_t)a.spp * (size_t)a.W));
    S.list[u] = rss_state(S, row, S.list[u]);
}

// The chain rays of render_rowstream's rows: counters[0] all, [3] closest-hit.
__global__ void __launch_bounds__(256) k_rss_count(RsStream S, unsigned long long* counters)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    unsigned long long sv = r < S.nrows ? S.rowrays[2 * r] : 0u, se = r < S.nrows ? S.rowrays[2 * r + 1] : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        sv += __shfl_xor(sv, off);
        se += __shfl_xor(se, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counters[0], sv);
        atomicAdd(&counters[3], se);
    }
}

// The chain's rays (the reference's count): counters[0] all, [3] closest-hit.
__global__ void __launch_bounds__(256) k_rs_count(RowSpec rs, unsigned long long* counters)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = r < rs.nrows ? rs.rays[r] : 0u, e = r < rs.nrows ? rs.erays[r] : 0u;
    unsigned long long sv = v, se = e;
    for (int off = 32; off > 0; off >>= 1) {
        sv += __shfl_xor(sv, off);
        se += __shfl_xor(se, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&counters[0], sv);
        atomicAdd(&counters[3], se);
    }
}

// The chains' pixels: the pilot's colour sum, then samples smp0 .. spp-1 from
// the colour buffer, in sample order (main.cpp:218), packed (main.cpp:221-233).
// sums (tmpt_render_radiance; null otherwise): the pixel's float sum is kept
// there too, as pass 2 keeps the other pixels' (it may be cinit itself: each
// thread reads its own pixel's entry before it writes it).
__global__ void __launch_bounds__(256) k_resolve_chains(PixelChains ch, const float4* __restrict__ sbuf, int32_t spp,
                                                        float spp_recip, uint32_t* __restrict__ out,
                                                        float4* sums = nullptr)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= ch.n) return;
    const uint32_t p = ch.cpix[r];
    const float4 c0 = ch.cinit[p];
    f3 col = mk(c0.x, c0.y, c0.z);
    for (int32_t k = ch.smp0; k < spp; ++k) {
        const float4 c = sbuf[(size_t)p * (size_t)spp + (size_t)k];
        col = col + mk(c.x, c.y, c.z);
    }
    if (sums) sums[p] = make_float4(col.x, col.y, col.z, c0.w);
    out[p] = pack_pixel(col, spp_recip);
}

// A row engine's k_path variant (PathVariant; the table's rows group): its
// unit kind, LDS stack, blocks per CU, cadence and tie rule.  The row engines
// never count, profile, offload shadows, read the SoA planes or store sums.
static PathVariant row_variant(int samp, int sl, int occ, int steps, int shade_min, int ties)
{
    PathVariant v{};
    v.sl = sl;
    v.steps = steps;
    v.shade_min = shade_min;
    v.occ = occ;
    v.samp = samp;
    v.ties = ties;
    return v;
}

// Streaming row engine (RsStream above): one k_path<SAMP 4> launch whose first
// blocks chase the rows' chains while the rest trace the windows' units, then
// the chain's samples in full (k_path<SAMP 2> over the chain list) and the
// in-order sums (k_resolve_px).  Returns 1 when it does not apply (limits,
// memory) and 2 when the launch aborted (its watchdog: no chain progress for
// ~1 s); the caller runs render_rowspec instead.
int render_rowstream(Scene& s, const RenderArgs& a, uint32_t* d_out, unsigned long long* d_counters)
{
    const Options& o = s.opt;
    // with the reference's octree answering (tie_rule visit) the leaves only
    // flag a tie and keep the first triangle met (TIES 2): the flagged query's
    // answer comes from the octree either way, so the lowest-index bookkeeping
    // is not needed (option row_flag_leaves 0 keeps it, for A/B)
    const bool flag = s.octree.oct_view && o.tie_rule == 0 && o.row_flag_leaves;
    const int ties = flag ? 2 : 0;
    // the chain's full re-trace at 5 waves per SIMD (option path_waves, as the
    // sample kernels: the 30-KB LDS layout of OCC 5)
    const bool w5 = o.path_waves != 4;
    // the workers at kRsOcc3 blocks per CU, or at 4 waves per SIMD (no spills)
    // for light loads (option row_occ)
    PathFn fn2, fn4, fn4_occ4;
    if (int rc = find_path_kernel(row_variant(2, w5 ? kPathSL5 : kPathSL, w5 ? 5 : 4, kRowSteps, kRowShadeMin, ties),
                                  "render_rowstream", fn2))
        return rc;
    if (int rc = find_path_kernel(row_variant(4, kPathSL, kRsOcc3, kRowSteps, kRowShadeMin, ties), "render_rowstream", fn4))
        return rc;
    if (int rc = find_path_kernel(row_variant(4, kPathSL, 4, kRowSteps, kRowShadeMin, ties), "render_rowstream", fn4_occ4))
        return rc;
    const int rows = a.tile_rows;
    const uint32_t W = (uint32_t)a.W, spp = (uint32_t)a.spp, T = (uint32_t)kRssT;
    const size_t lcap = (size_t)a.slots * spp;  // chain samples of the tile
    // a pixel's offsets per window ~ spp x 8.5 (draws / 2); the ring holds the
    // live windows with room to spare (pow2 >= 16 x spp x 8)
    uint32_t R = 1024;
    while (R < 128u * spp) R <<= 1;
    // offsets live in 24-bit fields: ~8.5 per sample on average, 14 allowed,
    // plus 2^20 of room for the workers' fetch-adds past a window's end
    if (rows < 1 || W > 4094u || (uint64_t)W * spp * 14u + R + (1u << 20) >= (1ull << 24) || lcap >= (1ull << 31))
        return 1;
    int grid = occupancy_grid((const void*)fn4, kBlk, 0, s.device);
    const int grid2 = occupancy_grid((const void*)fn2, kBlk, 0, s.device);
    const int nchase = (rows + kBlk - 1) / kBlk;  // blocks of 4 waves x 64 rows
    if (grid <= 2 * nchase) return 1;
    {
        // 5 waves per SIMD (96 VGPRs, 10 spilled dwords) win at full load, 4
        // (no spills) once the GPU has room per row: bench frame, row seeding,
        // 4 / 5 / 6 waves, N=1 1944.7 / 1854.6 / 1889.9 ms, 1/8 436.0 / 450.5 /
        // 477.1 ms; 4 / 5 waves at 1/2 1048.8 / 1043.6, 1/4 639.7 / 658.9, 1/8
        // 434.4 / 450.4 ms (room 1.1, 2.2, 4.4; profiles/r05_experiments/
        // row_worker_occupancy*.log): 4 waves from room 1.6
        const double room5 = (double)(grid - nchase) * kBlk / ((double)rows * (double)spp * 8.5);
        const bool occ4 = o.row_occ == 4 || (o.row_occ == 0 && room5 >= 1.6);
        const int g4 = occ4 ? occupancy_grid((const void*)fn4_occ4, kBlk, 0, s.device) : 0;
        if (occ4 && g4 > 2 * nchase) {
            fn4 = fn4_occ4;
            grid = g4;
        }
    }
    // live windows per row: 2.6 + 1.5 ln(room), room = resident lanes per
    // pixel window of all rows, within 2..kRssT-1.  Bench frame, 64 spp
    // (profiles/r03_rowspec/stream_windows_*, with the spread rule below):
    // best 2 windows at N = 1 (1.82 s), 3 at 1/2 (1.05 s), 4 at 1/4 (0.65 s),
    // 4-5 at 1/8 (0.44 s); this rule picks 2, 3, 4, 5
    const int64_t lanes = (int64_t)(grid - nchase) * kBlk;
    const double E_est = (double)spp * 8.5;
    const double room = (double)lanes / ((double)rows * E_est);  // resident lanes per pixel window of all rows
    // Round 5: the chasers re-apply both rules as rows finish (RsStream::dyn,
    // room per live row): the rows end over ~500 ms of the 1.7 s launch
    // (profiles/r05_wavetime/row_*.log) and the ones left get more windows;
    // N=1 1909 -> 1875 ms, 1/2 1085 -> 1054, 1/8 462.5 -> 459.6 (option
    // rowstream_dynamic; profiles/r05_experiments/row_dynamic_windows.log).
    // More slots per row (TMPT_RSS_T=16) changed nothing (row_rss16.log).
    int nw = (int)std::lround(2.6 + 1.5 * std::log(std::max(room, 1e-3)));
    nw = std::max(2, std::min(kRssT - 1, nw));
    if (o.rowspec_windows > 0) nw = std::min(kRssT - 1, o.rowspec_windows);
    const uint32_t na = (uint32_t)(((uint64_t)W * spp * 14u + R) >> 14) + 1u;
    const size_t ovf_words = std::max((size_t)grid * (kStackTotal - kPathSL), (size_t)grid2 * (kStackTotal - kPathSL5)) * kBlk;
    const size_t head_words = (size_t)kSeg * kCtr;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_res = al((size_t)rows * T * R * 8), b_slots = al((size_t)rows * (T + 1) * 8),
                 b_pos = al((size_t)rows * 8), b_rays = al((size_t)rows * 2 * 4), b_lo = al((size_t)rows * T * 4),
                 b_ctl = al(64), b_ctr = al(24 * 8), b_anch = al((size_t)rows * na * 4),
                 b_ovf = al((ovf_words + head_words) * 4);
    const size_t zero_bytes = b_res + b_slots + b_pos + b_rays + b_lo + b_ctl + b_ctr;
    const size_t need = zero_bytes + b_anch + b_ovf;
    const size_t lneed = lcap * sizeof(uint32_t), sneed = lcap * sizeof(float4);
    if (need + lneed + sneed > free_budget(3, 4, s.rss_buf.bytes() + s.rs_list.bytes() + s.sbuf.bytes())) return 1;
    // HBM short after the budget check (another allocation raced it): the
    // iterated engine may still fit, so fall back rather than fail the frame
    // (reserve() has freed the old buffer and cleared the failed allocation's error)
    if (!s.rss_buf.reserve(need) || !s.rs_list.reserve(lneed) || !s.sbuf.reserve(sneed)) return 1;
    if (!s.rss_tab) {  // M^(2c) and M^(256b) for c, b < 128; M^(2^15 a0), M^(2^20 a1) for a0, a1 < 32
        std::vector<uint32_t> tab, t;
        jump_tables(2, 128, t);
        tab.insert(tab.end(), t.begin(), t.end());
        jump_tables(256, 128, t);
        tab.insert(tab.end(), t.begin(), t.end());
        jump_tables(1ull << 15, 32, t);
        tab.insert(tab.end(), t.begin(), t.end());
        jump_tables(1ull << 20, 32, t);
        tab.insert(tab.end(), t.begin(), t.end());
        if (int rc = upload_tables(s.rss_tab, tab, "render_rowstream")) return rc;
    }
    TMPT_HIP(s.rss_host.ensure(16 * sizeof(uint32_t)));
    char* p = s.rss_buf.as<char>();
    RsStream S;
    memset(&S, 0, sizeof(S));
    S.res = reinterpret_cast<unsigned long long*>(p);
    p += b_res;
    S.slots = reinterpret_cast<unsigned long long*>(p);
    p += b_slots;
    S.chainpos = reinterpret_cast<unsigned long long*>(p);
    p += b_pos;
    S.rowrays = reinterpret_cast<uint32_t*>(p);
    p += b_rays;
    S.lo = reinterpret_cast<uint32_t*>(p);
    p += b_lo;
    S.ctl = reinterpret_cast<uint32_t*>(p);
    p += b_ctl;
    unsigned long long* spec_ctr = reinterpret_cast<unsigned long long*>(p);  // traced (not chain) rays
    p += b_ctr;
    S.anchors = reinterpret_cast<uint32_t*>(p);
    p += b_anch;
    uint32_t* ovf = reinterpret_cast<uint32_t*>(p);
    uint32_t* heads = ovf + ovf_words;
    S.list = s.rs_list.as<uint32_t>();
    S.t1 = s.rss_tab;
    S.t2 = s.rss_tab + 128 * 1024;
    S.na = na;
    S.jlimit = na << 14;
    S.R = R;
    S.rmask = R - 1u;
    S.nrows = rows;
    S.nchase = nchase;
    S.nw = nw;
    S.watchdog = o.rowstream_test_abort ? 200000u : 100000000u;  // ~1 s (2 ms when testing the abort)
    S.test_abort = o.rowstream_test_abort;
    // window spread in pixels: 0.055 x room - 0.015, within 0..0.25.  Bench
    // frame, 64 spp (profiles/r03_rowspec/stream_spread_*): best at 0 - 0.02
    // for N = 1 (1.82 s; 2.03 s at the earlier 0.10), 0.06 - 0.08 at 1/2, 0.12 -
    // 0.15 at 1/4, 0.18 - 0.22 at 1/8 (0.44 s); at full load the chaser's demand
    // and extension windows are cheaper than a wide spread
    S.spread = o.rowspec_spread >= 0.0f ? o.rowspec_spread
                                        : (float)std::min(0.25, std::max(0.0, 0.055 * room - 0.015));
    S.room_lanes = (float)((double)lanes / E_est);
    S.dyn = o.rowstream_dynamic ? ((o.rowspec_windows > 0 ? 0u : 1u) | (o.rowspec_spread >= 0.0f ? 0u : 2u)) : 0u;
    TMPT_HIP(hipMemsetAsync(s.rss_buf, 0, zero_bytes, s.stream));
    {
        const size_t n = (size_t)rows * na;
        k_rss_anchors<<<(unsigned)((n + 255) / 256), 256, 0, s.stream>>>(a, S, s.rss_tab + 256 * 1024,
                                                                        s.rss_tab + 288 * 1024);
        TMPT_HIP(hipGetLastError());
    }
    RenderArgs as = a;
    as.jt = nullptr;
    as.bmask = 0u;  // every unit is one sample
    as.smp_begin = 0;
    as.smp_end = a.spp;
    PathCtl pc;
    memset(&pc, 0, sizeof(pc));
    pc.heads = heads;
    pc.nblk = pc.blk = 1u;
    pc.lane_cap = 64u;
    pc.chunk = kChunk;
    pc.rs_noshadow = 1;
    pc.oct_shadow = oct_shadow_check(s);
    pc.top_walk = top_walk_cap(o, 2);
    pc.rss = S;
    fn4<<<grid, kBlk, 0, s.stream>>>(view(s), as, pc, d_out, ovf, spec_ctr);
    TMPT_HIP(hipGetLastError());
    TMPT_HIP(hipMemcpyAsync(s.rss_host, S.ctl, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    TMPT_HIP(hipStreamSynchronize(s.stream));
#ifdef TMPT_EXP_WAVETIME
    {
        std::vector<unsigned long long> w(3 * kWaveTimeMax, 0ull), r(kWaveTimeMax, 0ull), cl(kWaveTimeMax, 0ull);
        if (wavetime_get(w.data()) && rowtime_get(r.data(), cl.data())) {
            unsigned long long t0 = ~0ull, tend = 0;
            for (int i = 0; i < kWaveTimeMax; ++i)
                if (w[3 * i] && w[3 * i + 2]) {
                    t0 = std::min(t0, w[3 * i]);
                    tend = std::max(tend, w[3 * i + 2]);
                }
            std::vector<double> rt;
            for (int i = 0; i < std::min(rows, kWaveTimeMax); ++i)
                if (r[i]) rt.push_back((r[i] - t0) * 0.01);
            std::sort(rt.begin(), rt.end());
            auto q = [&](double f) { return rt.empty() ? 0.0 : rt[std::min(rt.size() - 1, (size_t)(f * (rt.size() - 1)))]; };
            fprintf(stderr, "rowstream rows %zu done at us p0/p10/p50/p90/p99/p100 %.0f/%.0f/%.0f/%.0f/%.0f/%.0f; "
                            "last worker exit %.0f\n",
                    rt.size(), q(0), q(0.1), q(0.5), q(0.9), q(0.99), q(1), (tend - t0) * 0.01);
            std::vector<double> lc;  // each worker wave's last claim of speculation work
            for (int i = 0; i < kWaveTimeMax; ++i)
                if (w[3 * i] && w[3 * i + 2] && cl[i]) lc.push_back((cl[i] - t0) * 0.01);
            std::sort(lc.begin(), lc.end());
            auto ql = [&](double f) { return lc.empty() ? 0.0 : lc[std::min(lc.size() - 1, (size_t)(f * (lc.size() - 1)))]; };
            fprintf(stderr, "rowstream workers %zu: last claim at us p0/p10/p25/p50/p75/p90/p100 "
                            "%.0f/%.0f/%.0f/%.0f/%.0f/%.0f/%.0f\n",
                    lc.size(), ql(0), ql(0.1), ql(0.25), ql(0.5), ql(0.75), ql(0.9), ql(1));
            std::fill(w.begin(), w.end(), 0ull);
            std::fill(r.begin(), r.end(), 0ull);
            wavetime_put(w.data());
            rowtime_put(r.data());
        }
    }
#endif
    if (s.rss_host[1] != 0u || s.rss_host[3] != 0u || s.rss_host[0] != (uint32_t)rows) {
#ifdef TMPT_DIAG
        fprintf(stderr, "rowstream: aborted (rows done %u of %d, abort %u, error %u); iterated engine instead\n",
                s.rss_host[0], rows, s.rss_host[1], s.rss_host[3]);
#endif
        return 2;  // launched and aborted: the caller falls back and records it (tmpt_stats.stream_fallbacks)
    }
    // the chain's samples in full (shadows included), then the in-order sums
    k_rss_states<<<(unsigned)((lcap + 255) / 256), 256, 0, s.stream>>>(a, S);
    PathCtl pc2 = pc;
    pc2.upix = nullptr;  // unit u = sample u % spp of tile pixel u / spp
    pc2.uslot = nullptr;
    pc2.ustate = S.list;
    pc2.p_dev = S.ctl + 4;
    pc2.rs_noshadow = 0;
    pc2.sbuf = s.sbuf;
    pc2.sb_ss = 1u;
    pc2.sb_sp = spp;
    TMPT_HIP(hipMemsetAsync(heads, 0, head_words * 4, s.stream));
    fn2<<<grid2, kBlk, 0, s.stream>>>(view(s), as, pc2, d_out, ovf, spec_ctr + 16);
    launch_resolve_px(s.stream, s.sbuf, a.slots, a.spp, a.spp_recip, d_out);
    k_rss_count<<<(unsigned)((rows + 255) / 256), 256, 0, s.stream>>>(S, d_counters);
    TMPT_HIP(hipGetLastError());
    s.path_launches = 1;
#ifdef TMPT_DIAG
    if (getenv("TMPT_ROWSPEC_LOG")) {
        unsigned long long c[2] = {0, 0}, t = 0;
        TMPT_HIP(hipMemcpyAsync(c, d_counters, sizeof(c), hipMemcpyDeviceToHost, s.stream));
        TMPT_HIP(hipMemcpyAsync(&t, spec_ctr, sizeof(t), hipMemcpyDeviceToHost, s.stream));
        TMPT_HIP(hipStreamSynchronize(s.stream));
        fprintf(stderr,
                "rowstream: %d rows, %d worker blocks + %d chaser blocks, ring %u, %d windows, traced rays %llu for "
                "%llu chain rays (x%.2f), chain ticks %u\n"
                "rowstream: claims %u, row misses %u, lost CAS %u; chaser waits %u, extensions %u, prefixes %u, "
                "sweeps %u\n",
                rows, grid - nchase, nchase, R, nw, t, c[0], c[0] ? (double)t / (double)c[0] : 0.0, s.rss_host[2],
                s.rss_host[5], s.rss_host[6], s.rss_host[7], s.rss_host[8], s.rss_host[9], s.rss_host[10],
                s.rss_host[11]);
    }
#endif
    return 0;
}

// Speculative row seeding (k_rs_* above): iterations of plan -> fill ->
// k_path<SAMP 2> -> chase until every row of the tile has its W pixels.  Each
// iteration moves every unfinished row through (usually) one pixel.  The rows
// are split into G groups, each iterating on its own stream, so one group's
// k_path tail overlaps another's work; the unit counts stay on the device and
// the host only checks for completion every kCheck iterations.
int render_rowspec(Scene& s, const RenderArgs& a, uint32_t* d_out, unsigned long long* d_counters,
                   const PixelChains* ch)
{
    const Options& o = s.opt;
    // rows: a.tile_rows chains of W pixels x spp samples; pixel chains (ch):
    // ch->n chains of one pixel x ch->cspp samples
    const int cspp = ch ? ch->cspp : a.spp;
    constexpr int kCheck = 64;
    // the units in full (SAMP 2; lowest-index ties whatever the octree: this
    // engine has no flagging variant), and
    // the shadow-free pass: its own instantiation (no shadow, light or colour
    // code, no light / next-ray LDS): 96 VGPRs, 5 waves per SIMD (6 waves: 80
    // VGPRs and 21 spilled dwords, neutral)
    PathFn fn, fn3;
    if (int rc = find_path_kernel(row_variant(2, kPathSL, 4, kRowIterSteps, kRowIterShadeMin, 0), "render_rowspec", fn))
        return rc;
    if (int rc = find_path_kernel(row_variant(3, kPathSL, kRsOcc3, kRowIterSteps, kRowIterShadeMin, 0), "render_rowspec", fn3))
        return rc;
    const int grid = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    const int grid3 = occupancy_grid((const void*)fn3, kBlk, 0, s.device);
    const int rows = ch ? ch->n : a.tile_rows;
    // window cap: one iteration covers a pixel's samples at up to 2 * wmax / spp
    // = 48 draws per sample (the stand-in sponza averages ~17, its deepest rows
    // ~25; a cap of 24 draws left those rows one short window per pixel, and
    // the slowest row sets the iteration count)
    uint32_t wmax = (uint32_t)std::min<int64_t>(8192, std::max<int64_t>(64, (int64_t)cspp * 24));
    if (o.rowspec_wmax > 0) wmax = (uint32_t)o.rowspec_wmax;
    // row groups, each on its own stream (one group: 3 % slower)
    const int G = std::max(1, std::min(std::min(o.rowspec_groups, kRowSpecMaxGroups), rows));
    // every group's k_path gets the whole resident grid (splitting the GPU
    // between the groups, or reserving fewer than 64 units per wave, did not help)
    const int pgrid = grid, pgrid3 = grid3;
    const uint32_t chunk = kChunk;
    // lookahead windows (pixels x+1, x+2, ...; each around its expected
    // start and end): one iteration covers up to nwin pixels of a row.  The
    // extra speculation is cheap while the GPU has room: nwin ~ 5 units per
    // resident lane over the rows' expected pixel windows (~17 draws per
    // sample), 2..kRsMaxWin -- 2 on the whole bench frame, 8 from 1/4 of it.
    // The far windows' spread grows with a pixel's units E = spp x ~8.5, so
    // the windows of one iteration are also capped at ~4400 units per row
    // (8 windows at 64 spp).  Measured (profiles/r02_rowspec/rs16): 640x360x4
    // suzanne 88 -> 51 ms with 8 -> 32 windows; the 1/8 shard of the bench
    // frame 708 ms with 8 windows, 746 with 18.
    const int64_t lanes = (int64_t)pgrid * kBlk;
    const double E_est = (double)cspp * 8.5;
    int nwin = (int)std::lround(std::min((double)lanes * 5.0 / ((double)rows * E_est), 4400.0 / E_est));
    nwin = std::max(2, std::min(kRsMaxWin, nwin));
    if (o.rowspec_windows > 0) nwin = std::min(kRsMaxWin, o.rowspec_windows);
    if (ch) nwin = 1;  // a pixel chain has one pixel: no lookahead windows
    const uint32_t jmax = (uint32_t)nwin * wmax;  // window i ends by (i + 1) * wmax
    // Speculate without shadow traversals and re-trace the chain in full at the
    // end (the frame's chain list and colour buffer must fit; else the colours
    // come from the speculative pass).  Bench frame 3.03 -> 2.49 s, 1/8 shard
    // 0.71 -> 0.61 s (profiles/r02_rowspec/rs19).  Option rowspec_noshadow.
    bool noshadow = o.rowspec_noshadow != 0 || ch;
    // chain samples of the tile (pixel chains: theirs); the colour buffer is
    // the tile's [pixel][sample] in either case
    const size_t lcap = ch ? (size_t)ch->n * (size_t)cspp : (size_t)a.slots * (size_t)a.spp;
    const uint32_t scap = (uint32_t)nwin * (uint32_t)cspp;  // a row's chain samples per iteration
    if (noshadow) {
        const size_t lneed = lcap * 3 * sizeof(uint32_t) + (size_t)rows * scap * sizeof(uint2) + 256;
        const size_t sneed = (size_t)a.slots * (size_t)a.spp * sizeof(float4);
        const size_t budget = free_budget(3, 4, s.rs_list.bytes() + s.sbuf.bytes());
        if (lcap >= (1ull << 32) || lneed + sneed > budget) {
            if (ch) return 1;  // pixel chains need the re-trace: the caller renders them in pass 2
            noshadow = false;  // does not fit: the colours come from the speculative pass
        } else {
            TMPT_ALLOC(s.rs_list.reserve(lneed), "tmpt_render: the chain list");
            TMPT_ALLOC(s.sbuf.reserve(sneed), "tmpt_render: the colour buffer");
        }
    }
    uint32_t* lpix = nullptr;
    uint32_t* lstate = nullptr;
    uint32_t* lslot = nullptr;
    uint32_t* lcount = nullptr;
    uint2* scratch = nullptr;
    if (noshadow) {
        lcount = s.rs_list.as<uint32_t>();
        scratch = reinterpret_cast<uint2*>(s.rs_list.as<char>() + 256);
        lpix = reinterpret_cast<uint32_t*>(scratch + (size_t)rows * scap);
        lstate = lpix + lcap;
        lslot = lstate + lcap;
    }
    if (s.jt2_n < (int32_t)jmax) {  // J_j = M^(2j): the state 2j draws on
        std::vector<uint32_t> tab;
        jump_tables(2, (int32_t)jmax, tab);
        if (int rc = upload_tables(s.jt2, tab, "tmpt_render")) return rc;
        s.jt2_n = (int32_t)jmax;
    }
    const size_t ovf_words = (size_t)std::max(pgrid, pgrid3) * kBlk * (kStackTotal - kPathSL);
    const size_t head_words = (size_t)kSeg * kCtr;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    auto group_rows = [&](int g) { return rows / G + (g < rows % G ? 1 : 0); };
    auto group_bytes = [&](int g) {
        const size_t R = (size_t)group_rows(g), U = R * jmax;
        return al(U * (sizeof(float4) + 3 * sizeof(uint32_t)) + R * sizeof(float4) +
                  ((9 + 2 * (size_t)kRsMaxWin) * R + 2) * sizeof(uint32_t) +
                  (ovf_words + head_words) * sizeof(uint32_t));
    };
    size_t need = al(24 * sizeof(unsigned long long));
    for (int g = 0; g < G; ++g) need += group_bytes(g);
    TMPT_ALLOC(s.rs_buf.reserve(need), "tmpt_render: the row engine's buffers");
    TMPT_HIP(s.rs_host.ensure(kRowSpecMaxGroups * sizeof(uint32_t)));
    for (int g = 0; g < G; ++g) {
        TMPT_HIP(s.rs_stream[g].ensure(hipStreamNonBlocking));
        TMPT_HIP(s.rs_event[g].ensure(hipEventDisableTiming));
    }
    TMPT_HIP(s.rs_event[kRowSpecMaxGroups].ensure(hipEventDisableTiming));
    char* p = s.rs_buf.as<char>();
    unsigned long long* spec_ctr = reinterpret_cast<unsigned long long*>(p);  // every traced unit's rays
    p += al(24 * sizeof(unsigned long long));
    struct Group {
        RowSpec rs;
        PathCtl pc;
        float4* rs_out;
        uint32_t *upix, *ustate, *rs_end, *heads, *ovf;
        size_t U;
        hipStream_t st;
    };
    std::vector<Group> gs(G);
    RenderArgs as = a;
    as.jt = nullptr;
    as.bmask = 0u;  // every unit is one sample
    as.smp_begin = 0;
    as.smp_end = a.spp;
    int row0 = 0;
    for (int g = 0; g < G; ++g) {
        Group& q = gs[g];
        char* gp = p;
        p += group_bytes(g);
        const size_t R = (size_t)group_rows(g);
        q.U = R * jmax;
        q.st = s.rs_stream[g];
        q.rs.row0 = row0;
        q.rs.nrows = (int)R;
        q.rs.wmax = wmax;
        q.rs.nwin = nwin;
        // window placement: expected positions +- spread * sqrt(i) pixels;
        // bench frame, 64 spp (profiles/r02_rowspec/rs15): spread 0.08 / 0.1 /
        // 0.12 / 0.15 = 3.06 / 3.03 / 3.04 / 3.10 s whole, 0.85 / 0.74 / 0.69 /
        // 0.67 s at 1/8 -- wider at low load, where speculation is cheap
        // (with shadow-free speculation: 1/8 shard spread 0.154 / 0.2 = 640 / 576 ms,
        // whole frame 0.106 / 0.14 / 0.2 = 2.51 / 2.52 / 2.62 s, rs20)
        q.rs.spread = o.rowspec_spread >= 0.0f ? o.rowspec_spread : 0.07f + 0.016f * (float)nwin;
        row0 += (int)R;
        q.rs_out = reinterpret_cast<float4*>(gp);
        gp += q.U * sizeof(float4);
        q.rs.col = reinterpret_cast<float4*>(gp);
        gp += R * sizeof(float4);
        uint32_t* w = reinterpret_cast<uint32_t*>(gp);
        q.upix = w;
        q.ustate = q.upix + q.U;
        q.rs_end = q.ustate + q.U;
        w = q.rs_end + q.U;
        uint32_t** fields[] = {&q.rs.rng, &q.rs.x, &q.rs.k, &q.rs.pdraws, &q.rs.prev_mean,
                               &q.rs.rays, &q.rs.erays, &q.rs.short_win};
        for (uint32_t** f : fields) {
            *f = w;
            w += R;
        }
        q.rs.win = w;  // kRsMaxWin x R each
        w += kRsMaxWin * R;
        q.rs.ws = w;
        w += kRsMaxWin * R;
        q.rs.offs = w;  // rows + 1
        w += R + 1;
        q.rs.total = w;
        w += 1;
        q.ovf = w;
        q.heads = w + ovf_words;
        memset(&q.pc, 0, sizeof(q.pc));
        q.pc.heads = q.heads;
        q.pc.nblk = q.pc.blk = 1u;
        q.pc.lane_cap = 64u;
        q.pc.chunk = chunk;
        q.pc.upix = q.upix;
        q.pc.ustate = q.ustate;
        q.pc.rs_out = q.rs_out;
        q.pc.rs_end = q.rs_end;
        q.pc.p_dev = q.rs.total;
        q.pc.rs_noshadow = noshadow ? 1 : 0;
        q.pc.oct_shadow = oct_shadow_check(s);
        q.pc.top_walk = top_walk_cap(o, 2);
        q.rs.lpix = lpix;
        q.rs.lstate = lstate;
        q.rs.lslot = lslot;
        q.rs.lcount = lcount;
        q.rs.scratch = scratch ? scratch + (size_t)q.rs.row0 * scap : nullptr;
        q.rs.scap = scap;
        q.rs.planned = spec_ctr + 8;
        q.rs.cpix = ch ? ch->cpix + q.rs.row0 : nullptr;
        q.rs.cinit = ch ? ch->cinit : nullptr;
        q.rs.cw = ch ? 1 : a.W;
        q.rs.cspp = cspp;
        q.rs.smp0 = ch ? ch->smp0 : 0;
    }
    // the groups start after the work already on the scene's stream (the
    // caller's wait), and that stream resumes after all of them
    TMPT_HIP(hipMemsetAsync(spec_ctr, 0, 24 * sizeof(unsigned long long), s.stream));
    if (noshadow) TMPT_HIP(hipMemsetAsync(lcount, 0, 4, s.stream));
    TMPT_HIP(hipEventRecord(s.rs_event[kRowSpecMaxGroups], s.stream));
    for (Group& q : gs) {
        TMPT_HIP(hipStreamWaitEvent(q.st, s.rs_event[kRowSpecMaxGroups], 0));
        k_rs_init<<<(unsigned)((q.rs.nrows + 255) / 256), 256, 0, q.st>>>(a, q.rs);
    }
    TMPT_HIP(hipGetLastError());
    // the listing pass's chase walks in LDS (one wave per row) when a row's
    // chain samples of one iteration fit its list; option rowspec_chase 0 = the
    // one-thread-per-row kernel
    const bool chase_lds = noshadow && o.rowspec_chase != 0 && (uint64_t)nwin * (uint64_t)cspp <= kChaseList;
    int it = 0;
    // every iteration moves each unfinished row by >= 1 sample, so W * spp bounds them
    const int64_t max_it = (int64_t)(ch ? 1 : a.W) * cspp + kCheck;
    bool done = false;
    // pixel chains finish in a few iterations: the host looks after each one
    // (an empty iteration still launches the persistent grid, ~0.3 ms)
    const int check = ch ? 1 : kCheck;
    while (!done && it < max_it) {
        for (int c = 0; c < check; ++c, ++it)
            for (Group& q : gs) {
                k_rs_plan<<<1, 1024, 0, q.st>>>(a, q.rs);
                k_rs_fill<<<(unsigned)((q.U + 255) / 256), 256, 0, q.st>>>(a, q.rs, s.jt2, q.upix, q.ustate);
                TMPT_HIP(hipMemsetAsync(q.heads, 0, head_words * 4, q.st));
                if (noshadow) fn3<<<pgrid3, kBlk, 0, q.st>>>(view(s), as, q.pc, d_out, q.ovf, spec_ctr);
                else fn<<<pgrid, kBlk, 0, q.st>>>(view(s), as, q.pc, d_out, q.ovf, spec_ctr);
                if (chase_lds)
                    k_rs_chase_lds<<<(unsigned)q.rs.nrows, 64, 0, q.st>>>(a, q.rs, q.rs_out, q.rs_end, q.upix,
                                                                         q.ustate);
                else
                    k_rs_chase<<<(unsigned)((q.rs.nrows + 63) / 64), 64, 0, q.st>>>(a, q.rs, q.rs_out, q.rs_end,
                                                                                    d_out, q.upix, q.ustate);
            }
        TMPT_HIP(hipGetLastError());
        // the last plan of each group: 0 units = the group was already done
        for (int g = 0; g < G; ++g)
            TMPT_HIP(hipMemcpyAsync(&s.rs_host[g], gs[g].rs.total, 4, hipMemcpyDeviceToHost, gs[g].st));
        done = true;
        for (int g = 0; g < G; ++g) {
            TMPT_HIP(hipStreamSynchronize(gs[g].st));
            done = done && s.rs_host[g] == 0;
        }
    }
    if (!done) {  // cannot happen: every iteration moves each unfinished row on
        set_error("render_rowspec: rows unfinished after " + std::to_string(it) + " iterations");
        for (Group& q : gs) (void)hipStreamSynchronize(q.st);
        return -1;
    }
    for (int g = 0; g < G; ++g) {
        k_rs_count<<<(unsigned)((gs[g].rs.nrows + 255) / 256), 256, 0, gs[g].st>>>(gs[g].rs, d_counters);
        TMPT_HIP(hipEventRecord(s.rs_event[g], gs[g].st));
        TMPT_HIP(hipStreamWaitEvent(s.stream, s.rs_event[g], 0));
    }
    TMPT_HIP(hipGetLastError());
    if (noshadow) {  // the chain's samples in full (shadows included), then the in-order sums
        PathCtl pc2 = gs[0].pc;
        pc2.upix = lpix;
        pc2.ustate = lstate;
        pc2.uslot = lslot;
        pc2.p_dev = lcount;
        pc2.rs_noshadow = 0;
        pc2.sbuf = s.sbuf;
        pc2.sb_ss = 1u;
        pc2.sb_sp = (uint32_t)a.spp;
        TMPT_HIP(hipMemsetAsync(gs[0].heads, 0, head_words * 4, s.stream));
        fn<<<pgrid, kBlk, 0, s.stream>>>(view(s), as, pc2, d_out, gs[0].ovf, spec_ctr + 16);
        if (ch)
            // (a radiance render, a.prog set: the chains' sums go back into the pilot's
            // state array, from which render_persistent copies every pixel's)
            k_resolve_chains<<<(unsigned)((ch->n + 255) / 256), 256, 0, s.stream>>>(
                *ch, s.sbuf, a.spp, a.spp_recip, d_out, a.prog ? const_cast<float4*>(ch->cinit) : nullptr);
        else
            launch_resolve_px(s.stream, s.sbuf, a.slots, a.spp, a.spp_recip, d_out);
        TMPT_HIP(hipGetLastError());
    }
    s.path_launches = it;
#ifdef TMPT_DIAG
    if (getenv("TMPT_ROWSPEC_LOG")) {
        unsigned long long c[2] = {0, 0};
        TMPT_HIP(hipMemcpyAsync(c, d_counters, sizeof(c), hipMemcpyDeviceToHost, s.stream));
        unsigned long long t = 0;
        TMPT_HIP(hipMemcpyAsync(&t, spec_ctr, sizeof(t), hipMemcpyDeviceToHost, s.stream));
        std::vector<uint32_t> sw(rows), pm(rows);
        for (Group& q : gs) {
            TMPT_HIP(hipMemcpyAsync(sw.data() + q.rs.row0, q.rs.short_win, q.rs.nrows * 4, hipMemcpyDeviceToHost, s.stream));
            TMPT_HIP(hipMemcpyAsync(pm.data() + q.rs.row0, q.rs.prev_mean, q.rs.nrows * 4, hipMemcpyDeviceToHost, s.stream));
        }
        TMPT_HIP(hipStreamSynchronize(s.stream));
        double pmsum = 0.0;
        for (uint32_t v : pm) {
            float f;
            memcpy(&f, &v, 4);
            pmsum += f;
        }
        unsigned long long planned = 0;
        TMPT_HIP(hipMemcpy(&planned, spec_ctr + 8, sizeof(planned), hipMemcpyDeviceToHost));
        fprintf(stderr, "rowspec: last pixel's draws per sample, mean over rows %.2f; units planned %llu (%.1f rays each)\n",
                rows ? pmsum / rows : 0.0, planned, planned ? (double)t / (double)planned : 0.0);
        uint64_t swsum = 0;
        uint32_t swmax = 0;
        for (uint32_t v : sw) {
            swsum += v;
            swmax = std::max(swmax, v);
        }
        fprintf(stderr,
                "rowspec: %d iterations enqueued, %d groups of %d blocks, window cap %u, %d windows, traced rays "
                "%llu for %llu chain rays (x%.2f); short windows per row: mean %.1f max %u\n",
                it, G, pgrid, wmax, nwin, t, c[0], c[0] ? (double)t / (double)c[0] : 0.0,
                rows ? (double)swsum / rows : 0.0, swmax);
    }
#endif
    return 0;
}

}  // namespace tmpt
