// tmpt_adaptive.hip -- adaptive sampling (tmpt_render_adaptive): per-pixel
// sample counts by a variance test, on sample seeding's persistent engine.
// In that seeding sample s of a pixel is a function of the pixel and s alone,
// so a pixel may stop at any count n and then holds exactly the pixel of an
// n-spp frame.  The call runs passes: pass 0 traces samples [0, spp_min) of
// every pixel of the tile (render_persistent's progressive-style pass), pass
// k+1 samples [n_k, n_k+1) of the pixels still active (k_path LIST over the
// device list).  After each pass k_adapt_update continues every listed
// pixel's sums over the pass's samples, in sample order, from the colour
// buffer, applies the test of include/tmpt.h and marks the pixels that go on;
// k_adapt_scan and k_adapt_scatter compact them, in ascending slot order,
// into the next pass's list.  With a radius (the neighbourhood rule) the marks
// come from the own tests dilated over the tile instead: k_adapt_update_own,
// k_adapt_pack, k_adapt_dilate and k_adapt_gather below; radius 0 launches none
// of them.  k_adapt_final scales, packs and writes the three
// outputs; tmpt_render_moments is the same call with k_adapt_final_mom in its
// place, which also writes each pixel's luminance moments; tmpt_render_guided
// is that call with a per-pixel prior in the test (the update kernels' PRIOR
// form).  The host reads the next list's length (one word, with the pass's
// counters) after every pass but the last: that length sizes the next launch.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <string>

#include "tmpt_path.h"

namespace tmpt {

// What a pixel carries through the call, 32 B (two 16-byte halves): the colour
// sum, the luminance moments and the count it stopped at (the count so far
// while it is active).
struct alignas(16) AdaptState {
    float r, g, b, m1;
    float m2;
    int32_t n;
    uint32_t pad[2];
};
static_assert(sizeof(AdaptState) == 32, "adaptive state: two dwordx4 accesses");

constexpr int kScanBlock = 1024;

// One lane per pixel of the pass's list (list null: position i is slot i, the
// first pass), 64 per block.  The pass's samples [s0, s1) of the block's
// pixels are staged through LDS as k_resolve_px stages them -- 16 lanes read
// one pixel's run of 16 samples, 256 contiguous bytes of the [pixel][sample]
// buffer -- and every lane then continues its own pixel's sums in sample
// order.  The statements of the sums and of the test are include/tmpt.h's, one
// rounding each (the unit is built with contraction off and correctly rounded
// division).  Bit t of mask[block] and cnt[block] say which of the block's
// pixels stay active; none does when the pass is the last (s1 == cap).
// PRIOR (tmpt_render_guided): the test judges the pixel as the temporal blend
// will leave it -- one more 16-byte load per listed pixel, prior[slot]; nothing
// else changes, and PRIOR = false reads no prior at all.
template <bool PRIOR>
__global__ void __launch_bounds__(64) k_adapt_update(const float4* __restrict__ sbuf, const uint32_t* __restrict__ list,
                                                     uint32_t n, int32_t spp, int32_t s0, int32_t s1, float lim4,
                                                     AdaptState* __restrict__ state, uint64_t* __restrict__ mask,
                                                     uint32_t* __restrict__ cnt, const float4* __restrict__ prior)
{
    constexpr int kC = 16;               // samples per staged chunk
    __shared__ float4 tile[64][kC + 1];  // +1: a lane's row starts on another bank
    __shared__ uint32_t s_pix[64];
    const uint32_t p0 = blockIdx.x * 64u;
    const int t = (int)threadIdx.x;
    const int np = (int)min(64u, n - p0);
    const uint32_t pix = t < np ? (list ? list[p0 + t] : p0 + (uint32_t)t) : 0u;
    s_pix[t] = pix;
    AdaptState st{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, {0u, 0u}};
    if (s0 > 0 && t < np) st = state[pix];
    __syncthreads();
    for (int32_t c0 = s0; c0 < s1; c0 += kC) {
        const int nc = min(kC, s1 - c0);
        for (int e = t; e < 64 * kC; e += 64) {
            const int i = e / kC, j = e - i * kC;
            if (i < np && j < nc) tile[i][j] = sbuf[(size_t)s_pix[i] * (size_t)spp + (size_t)(c0 + j)];
        }
        __syncthreads();
        if (t < np)
            for (int j = 0; j < nc; ++j) {
                const float4 c = tile[t][j];
                st.r = st.r + c.x;
                st.g = st.g + c.y;
                st.b = st.b + c.z;
                const float y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
                st.m1 = st.m1 + y;
                st.m2 = st.m2 + y * y;
            }
        __syncthreads();
    }
    bool active = false;
    if (t < np) {
        const float fn = (float)s1;
        const float mean = st.m1 / fn;
        const float var = fmaxf(0.0f, st.m2 / fn - mean * mean);
        float se2 = var / (fn - 1.0f);
        float meanb = mean;
        if (PRIOR) {  // the frame as it will be after the blend (tmpt_render_guided)
            const float4 pr = prior[pix];
            se2 = pr.y + (pr.z * pr.z) * se2;
            meanb = pr.x + (mean - pr.x) * pr.z;
        }
        const float lim = lim4 * fmaxf(meanb, 1.0f / 256.0f);
        active = s1 < spp && se2 > lim;  // a NaN compares false: the pixel stops
        st.n = s1;
        state[pix] = st;
    }
    const uint64_t m = wballot(active);
    if (t == 0) {
        mask[blockIdx.x] = m;
        cnt[blockIdx.x] = (uint32_t)__popcll(m);
    }
}

// k_adapt_update for the neighbourhood rule (radius > 0): the same staging, sums
// and test, statement for statement -- a kernel of its own, so that the radius-0
// call keeps k_adapt_update's code as it is.  The pixel's own test goes to
// own[slot], one byte per tile slot; mask / cnt are left to k_adapt_gather.  A
// pixel leaves the list only at a pass where its own test failed, so the plane
// holds false for every dropped pixel with no clearing; pass 0 lists every slot
// and so initialises it.
template <bool PRIOR>
__global__ void __launch_bounds__(64) k_adapt_update_own(const float4* __restrict__ sbuf,
                                                         const uint32_t* __restrict__ list, uint32_t n, int32_t spp,
                                                         int32_t s0, int32_t s1, float lim4,
                                                         AdaptState* __restrict__ state, uint8_t* __restrict__ own,
                                                         const float4* __restrict__ prior)
{
    constexpr int kC = 16;               // samples per staged chunk
    __shared__ float4 tile[64][kC + 1];  // +1: a lane's row starts on another bank
    __shared__ uint32_t s_pix[64];
    const uint32_t p0 = blockIdx.x * 64u;
    const int t = (int)threadIdx.x;
    const int np = (int)min(64u, n - p0);
    const uint32_t pix = t < np ? (list ? list[p0 + t] : p0 + (uint32_t)t) : 0u;
    s_pix[t] = pix;
    AdaptState st{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, {0u, 0u}};
    if (s0 > 0 && t < np) st = state[pix];
    __syncthreads();
    for (int32_t c0 = s0; c0 < s1; c0 += kC) {
        const int nc = min(kC, s1 - c0);
        for (int e = t; e < 64 * kC; e += 64) {
            const int i = e / kC, j = e - i * kC;
            if (i < np && j < nc) tile[i][j] = sbuf[(size_t)s_pix[i] * (size_t)spp + (size_t)(c0 + j)];
        }
        __syncthreads();
        if (t < np)
            for (int j = 0; j < nc; ++j) {
                const float4 c = tile[t][j];
                st.r = st.r + c.x;
                st.g = st.g + c.y;
                st.b = st.b + c.z;
                const float y = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z;
                st.m1 = st.m1 + y;
                st.m2 = st.m2 + y * y;
            }
        __syncthreads();
    }
    if (t < np) {
        const float fn = (float)s1;
        const float mean = st.m1 / fn;
        const float var = fmaxf(0.0f, st.m2 / fn - mean * mean);
        float se2 = var / (fn - 1.0f);
        float meanb = mean;
        if (PRIOR) {  // as in k_adapt_update
            const float4 pr = prior[pix];
            se2 = pr.y + (pr.z * pr.z) * se2;
            meanb = pr.x + (mean - pr.x) * pr.z;
        }
        const float lim = lim4 * fmaxf(meanb, 1.0f / 256.0f);
        st.n = s1;
        state[pix] = st;
        own[pix] = s1 < spp && se2 > lim ? 1 : 0;  // a NaN compares false
    }
}

// ---- the neighbourhood rule (radius r > 0): a listed pixel stays active iff
// the own test held for some pixel within r columns and r rows of it, inside
// the frame and inside its band.  The own plane is packed into one bit per
// pixel, rows of wpr = ceil(W / 64) 64-bit words (bit b of word j = column
// 64 j + b; the bits past W are 0), dilated word by word, and read back per
// list position.  The tile's rows of one band are consecutive and tile row t
// lies in the shard's band t / band_rows (only the last band may be short),
// so the band clip is a clip of tile rows.

// One wave per word of the bit plane: a ballot over 64 pixels of a row.
__global__ void __launch_bounds__(256) k_adapt_pack(const uint8_t* __restrict__ own, int32_t W, uint32_t wpr,
                                                    uint32_t nwords, uint64_t* __restrict__ bits)
{
    const uint32_t wi = blockIdx.x * 4u + (threadIdx.x >> 6);  // wave-uniform
    if (wi >= nwords) return;
    const uint32_t row = wi / wpr, j = wi - row * wpr;
    const uint32_t x = j * 64u + (uint32_t)lane_id();
    const bool on = x < (uint32_t)W && own[(size_t)row * (size_t)W + x] != 0;
    const uint64_t m = wballot(on);
    if (lane_id() == 0) bits[wi] = m;
}

// One lane per word: OR over the rows of the band within r (the word and its
// two neighbours in the row), then the OR of the shifts by 1 .. r with the
// neighbour words' bits carried in.  r <= 8 < 64: every shift count is in
// 1 .. 63.  A word left of column 0 or right of the row's last is 0, as are
// the last word's bits past W: the frame clips the neighbourhood.
__global__ void __launch_bounds__(256) k_adapt_dilate(const uint64_t* __restrict__ bits, uint32_t wpr, uint32_t nwords,
                                                      int32_t tile_rows, int32_t band_rows, int32_t r,
                                                      uint64_t* __restrict__ dil)
{
    const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
    if (wi >= nwords) return;
    const int32_t row = (int32_t)(wi / wpr);
    const uint32_t j = wi - (uint32_t)row * wpr;
    const int32_t b0 = (row / band_rows) * band_rows, b1 = min(tile_rows, b0 + band_rows);  // the band's rows [b0, b1)
    const int32_t lo = max(b0, row - r), hi = min(b1 - 1, row + r);
    uint64_t vl = 0, vc = 0, vr = 0;
    for (int32_t t = lo; t <= hi; ++t) {
        const uint64_t* w = bits + (size_t)t * wpr + j;
        vc |= w[0];
        if (j > 0) vl |= w[-1];
        if (j + 1 < wpr) vr |= w[1];
    }
    uint64_t d = vc;
    for (int32_t k = 1; k <= r; ++k) d |= (vc << k) | (vl >> (64 - k)) | (vc >> k) | (vr << (64 - k));
    dil[wi] = d;
}

// One lane per list position, as k_adapt_update: the dilated bit at the
// pixel's slot, balloted into the mask[block] / cnt[block] that k_adapt_scan
// and k_adapt_scatter consume.
__global__ void __launch_bounds__(64) k_adapt_gather(const uint32_t* __restrict__ list, uint32_t n, int32_t W,
                                                     uint32_t wpr, const uint64_t* __restrict__ dil,
                                                     uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    bool active = false;
    if (i < n) {
        const uint32_t pix = list ? list[i] : i;
        const uint32_t row = pix / (uint32_t)W, x = pix - row * (uint32_t)W;
        active = ((dil[(size_t)row * wpr + (x >> 6)] >> (x & 63u)) & 1ull) != 0;
    }
    const uint64_t m = wballot(active);
    if (threadIdx.x == 0) {
        mask[blockIdx.x] = m;
        cnt[blockIdx.x] = (uint32_t)__popcll(m);
    }
}

// Exclusive scan of the nb block counts, in place, by one block: every thread
// sums a contiguous piece, the pieces' sums are scanned in LDS, and the piece
// is walked again.  total[0] = the next list's length.
__global__ void __launch_bounds__(kScanBlock) k_adapt_scan(uint32_t* __restrict__ cnt, uint32_t nb,
                                                           uint32_t* __restrict__ total)
{
    __shared__ uint32_t s_sum[kScanBlock];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nb + kScanBlock - 1u) / kScanBlock;
    const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += cnt[b];
    s_sum[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kScanBlock; off <<= 1) {  // inclusive, Hillis-Steele
        const uint32_t v = t >= off ? s_sum[t - off] : 0u;
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    uint32_t run = s_sum[t] - sum;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t c = cnt[b];
        cnt[b] = run;
        run += c;
    }
    if (t == kScanBlock - 1u) total[0] = s_sum[t];
}

// The next list: block b's active pixels, in lane order, from off[b] on --
// positions keep their order, and the lists are ascending in the slot from the
// first (the identity) on, with no dependence on which block ran first.
__global__ void __launch_bounds__(64) k_adapt_scatter(const uint32_t* __restrict__ list, uint32_t n,
                                                      const uint64_t* __restrict__ mask,
                                                      const uint32_t* __restrict__ off, uint32_t* __restrict__ next)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const uint64_t m = mask[blockIdx.x];
    if (i >= n || ((m >> threadIdx.x) & 1ull) == 0) return;
    const uint32_t below = (uint32_t)__popcll(m & ((1ull << threadIdx.x) - 1ull));
    next[off[blockIdx.x] + below] = list ? list[i] : i;
}

// The three outputs from the state (any of them may be null): the float pixel
// {sum * (1.0f / (float)n), 1.0f} as k_radiance_scale forms it, the packed
// pixel as every render packs its own, and n.
__global__ void __launch_bounds__(256) k_adapt_final(const AdaptState* __restrict__ state, int64_t n,
                                                     float4* __restrict__ o32, uint32_t* __restrict__ o8,
                                                     int32_t* __restrict__ ospp)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const AdaptState st = state[i];
    const float recip = 1.0f / (float)st.n;
    const f3 sum = mk(st.r, st.g, st.b);
    if (o32) {
        const f3 col = sum * recip;
        o32[i] = make_float4(col.x, col.y, col.z, 1.0f);
    }
    if (o8) o8[i] = pack_pixel(sum, recip);
    if (ospp) ospp[i] = st.n;
}

// k_adapt_final with the pixel's luminance moments beside the three outputs
// (tmpt_render_moments; include/tmpt.h): {m1 / fn, m2 / fn, 1.0f / fn, 1.0f},
// fn = (float)n -- a kernel of its own, so that tmpt_render_adaptive keeps
// k_adapt_final's code as it is.  mom is never null.
__global__ void __launch_bounds__(256) k_adapt_final_mom(const AdaptState* __restrict__ state, int64_t n,
                                                         float4* __restrict__ o32, uint32_t* __restrict__ o8,
                                                         int32_t* __restrict__ ospp, float4* __restrict__ mom)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const AdaptState st = state[i];
    const float fn = (float)st.n;
    const float recip = 1.0f / fn;
    const f3 sum = mk(st.r, st.g, st.b);
    if (o32) {
        const f3 col = sum * recip;
        o32[i] = make_float4(col.x, col.y, col.z, 1.0f);
    }
    if (o8) o8[i] = pack_pixel(sum, recip);
    if (ospp) ospp[i] = st.n;
    mom[i] = make_float4(st.m1 / fn, st.m2 / fn, recip, 1.0f);
}

static size_t align256(size_t v) { return (v + 255u) & ~(size_t)255u; }

// ad: the resolved descriptor (defaults applied, ranges checked by the
// caller); d_f32 / d_u8 / d_spp: device tiles or null.  d_mom (tmpt_render_moments,
// `what` its name): the moments tile, or null.  d_prior (tmpt_render_guided): the
// prior tile, one float4 per slot, or null -- the update kernels' PRIOR = false
// instantiations then, which are the kernels as they were.
int render_adaptive(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, const tmpt_adaptive_desc* ad,
                    float4* d_f32, uint32_t* d_u8, int32_t* d_spp, tmpt_adaptive_info* info, uint64_t* ray_count,
                    float4* d_mom, const char* what, const float4* d_prior)
{
    RenderArgs a = make_args(cam, d);
    s.row_render = false;
    s.pixel_render = false;
    if (int rc = ensure_sample_tables(s, a.spp, what)) return rc;
    a.jt = s.jt;
    if (int rc = wait_caller_stream(s, d, what)) return rc;
    if (ensure_counters(s)) return -1;
    a.root_check = camera_root_check(s, a.cam);
    tmpt_adaptive_info inf;
    memset(&inf, 0, sizeof(inf));
    unsigned long long c[kRenderCounters] = {};
    double extend_ms = 0.0, redo_ms = 0.0;
    int64_t launches = 0, redo_samples = 0, redo_late = 0;
    int32_t redo_launches = 0, tie_path = 0, cam_used = 0;
    reset_render_stats(s);
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    if (a.slots > 0) {
        const size_t slots = (size_t)a.slots, nb_max = (slots + 63) / 64;
        const size_t o_list0 = align256(sizeof(AdaptState) * slots), o_list1 = o_list0 + align256(4 * slots);
        const size_t o_mask = o_list1 + align256(4 * slots), o_cnt = o_mask + align256(8 * nb_max);
        const size_t o_total = o_cnt + align256(4 * nb_max);
        // the neighbourhood rule's planes (radius > 0): own bytes, the bit plane and its dilation
        const int32_t radius = ad->radius;
        const uint32_t wpr = ((uint32_t)a.W + 63u) / 64u, nwords = wpr * (uint32_t)a.tile_rows;
        const size_t o_own = o_total + 256, o_bits = o_own + align256(slots), o_dil = o_bits + align256(8 * (size_t)nwords);
        const size_t need = radius > 0 ? o_dil + align256(8 * (size_t)nwords) : o_total + 256;
        if (!s.adapt_buf.reserve(need)) {
            set_error(std::string(what) + ": out of device memory (the per-pixel state and lists)");
            return -12;
        }
        TMPT_HIP(s.adapt_host.ensure(64));
        char* base = s.adapt_buf.as<char>();
        AdaptState* state = reinterpret_cast<AdaptState*>(base);
        uint32_t* lists[2] = {reinterpret_cast<uint32_t*>(base + o_list0), reinterpret_cast<uint32_t*>(base + o_list1)};
        uint64_t* mask = reinterpret_cast<uint64_t*>(base + o_mask);
        uint32_t* cnt = reinterpret_cast<uint32_t*>(base + o_cnt);
        uint32_t* total = reinterpret_cast<uint32_t*>(base + o_total);
        uint8_t* own = reinterpret_cast<uint8_t*>(base + o_own);  // radius > 0 only: inside the buffer then
        uint64_t* bits = reinterpret_cast<uint64_t*>(base + o_bits);
        uint64_t* dil = reinterpret_cast<uint64_t*>(base + o_dil);
        const float lim4 = 4.0f * (ad->threshold * ad->threshold);
        const uint32_t* list = nullptr;  // pass 0: every slot
        int64_t n_list = a.slots;
        int32_t n0 = 0, n1 = ad->spp_min;
        int rc = 0;
        for (int k = 0;; ++k) {
            RenderArgs ap = a;
            ap.smp_begin = n0;
            ap.smp_end = n1;
            reset_render_stats(s);
            TMPT_HIP(hipMemsetAsync(s.counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
            s.adapt_on = true;
            s.adapt_list = list;
            s.adapt_n = n_list;
            rc = render_persistent(s, ap, d_u8, false, s.counters);
            s.adapt_on = false;
            s.adapt_list = nullptr;
            s.adapt_n = 0;
            if (rc) break;
            const uint32_t n = (uint32_t)n_list, nb = (n + 63u) / 64u;
            const bool last = n1 >= a.spp;
            if (radius > 0)
                (d_prior ? k_adapt_update_own<true> : k_adapt_update_own<false>)<<<nb, 64, 0, s.stream>>>(
                    s.sbuf, list, n, a.spp, n0, n1, lim4, state, own, d_prior);
            else
                (d_prior ? k_adapt_update<true> : k_adapt_update<false>)<<<nb, 64, 0, s.stream>>>(
                    s.sbuf, list, n, a.spp, n0, n1, lim4, state, mask, cnt, d_prior);
            TMPT_HIP(hipGetLastError());
            uint32_t* next = lists[k & 1];
            if (!last && radius > 0) {  // the neighbourhood rule: mask / cnt from the dilated own plane
                k_adapt_pack<<<(nwords + 3u) / 4u, 256, 0, s.stream>>>(own, a.W, wpr, nwords, bits);
                TMPT_HIP(hipGetLastError());
                k_adapt_dilate<<<(nwords + 255u) / 256u, 256, 0, s.stream>>>(bits, wpr, nwords, a.tile_rows, a.band_rows,
                                                                           radius, dil);
                TMPT_HIP(hipGetLastError());
                k_adapt_gather<<<nb, 64, 0, s.stream>>>(list, n, a.W, wpr, dil, mask, cnt);
                TMPT_HIP(hipGetLastError());
            }
            if (!last) {
                k_adapt_scan<<<1, kScanBlock, 0, s.stream>>>(cnt, nb, total);
                TMPT_HIP(hipGetLastError());
                k_adapt_scatter<<<nb, 64, 0, s.stream>>>(list, n, mask, cnt, next);
                TMPT_HIP(hipGetLastError());
                TMPT_HIP(hipMemcpyAsync(s.adapt_host, total, 4, hipMemcpyDeviceToHost, s.stream));
            }
            // the host waits here, once per pass: for the pass's counters and,
            // unless the pass is the last, the next list's length
            TMPT_HIP(hipMemcpyAsync(s.counters_host, s.counters, kRenderCounters * sizeof(unsigned long long),
                                    hipMemcpyDeviceToHost, s.stream));
            TMPT_HIP(hipStreamSynchronize(s.stream));
            for (int i = 0; i < kRenderCounters; ++i) c[i] += s.counters_host[i];
            float k1 = 0.0f;
            (void)hipEventElapsedTime(&k1, s.path_ev[2], s.path_ev[3]);
            extend_ms += k1;
            if (s.redo_launches) {
                float kr = 0.0f;
                (void)hipEventElapsedTime(&kr, s.path_ev[0], s.path_ev[1]);
                redo_ms += kr;
            }
            launches += s.path_launches;
            redo_samples += s.redo_samples;
            redo_late += s.redo_late;
            redo_launches += s.redo_launches;
            if (k == 0) tie_path = s.tie_path;
            cam_used |= s.cam_rays_used;
            inf.pass_pixels[k] = n_list;
            inf.samples += (uint64_t)n_list * (uint64_t)(n1 - n0);
            inf.passes = k + 1;
            if (last) break;
            n_list = (int64_t)s.adapt_host[0];
            if (n_list == 0) break;
            list = next;
            n0 = n1;
            n1 = std::min(n1 + ad->spp_step, a.spp);
        }
        if (rc) return rc;
        const unsigned fb = (unsigned)((a.slots + 255) / 256);
        if (d_mom)
            k_adapt_final_mom<<<fb, 256, 0, s.stream>>>(state, a.slots, d_f32, d_u8, d_spp, d_mom);
        else
            k_adapt_final<<<fb, 256, 0, s.stream>>>(state, a.slots, d_f32, d_u8, d_spp);
        TMPT_HIP(hipGetLastError());
    }
    TMPT_HIP(hipEventRecord(e1, s.stream));
    TMPT_HIP(hipStreamSynchronize(s.stream));
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    reset_render_stats(s);
    s.render_ms = ms;
    s.extend_ms = extend_ms;
    s.redo_ms = redo_ms;
    s.redo_rays = c[kRedoRaysCounter];
    s.redo_samples = redo_samples;
    s.redo_late = redo_late;
    s.redo_launches = redo_launches;
    s.tie_path = tie_path;
    s.cam_rays_used = cam_used;
    s.tie_queries = c[kTieCounter];
    s.root_misses = c[kTieCounter + 1];
    s.crack_queries = c[kCrackCounter];
    s.extend_rays = c[3];
    s.shadow_rays = c[0] - c[3];
    s.extend_launches = launches;
    s.iterations = inf.passes;
    if (info) *info = inf;
    if (ray_count) *ray_count = c[0];
    return 0;
}

}  // namespace tmpt
