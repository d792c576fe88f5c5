// tmpt_denoise.hip -- the denoiser (tmpt_denoise, include/tmpt.h
// tmpt_denoise_desc): an edge-avoiding a-trous wavelet filter over a float
// radiance frame (tmpt_render_radiance), its weights from the AOV records of
// the same frame (tmpt_render_aov).  The header states the arithmetic, and
// that statement is the contract: float32, one rounding per operation, a fixed
// order, no exp or pow -- this file only schedules it.
//
// k_dn_guides packs what a tap needs, once per call: 20 B per pixel in two
// planes, {nh.xyz, zb} (16 B) and dl (4 B).  Coverage has no word of its own:
// an uncovered pixel's nh, zb and dl are never read (its taps take the plain
// B3 weights), so its zb word holds kNoCov, a NaN pattern no arithmetic gives
// (a covered pixel whose zb is a NaN is stored as the canonical one).
//
// k_dn_level is one level: a 32 x 8 tile of pixels per 256-thread block, one
// pixel per lane, the 25 taps unrolled.  STAGE 1 / 2 (strides 1 and 2): the
// tile and its 2-stride halo -- colour, guides -- are staged in LDS once per
// block (36 x 12 or 40 x 16 pixels, 36 B each: 15.2 / 22.5 KB) and the taps
// read LDS; STAGE 0 (any stride): the taps are global loads, 16 B + 16 B + 4 B
// each, contiguous across the lanes of a tile row.  Which strides use the
// staged form: dn_staged() below.  The levels ping-pong two float4 planes of
// the scene's workspace; the last one writes the caller's buffer and packs the
// 8-bit pixels in the same pass.
//
// The noise-aware form (tmpt_denoise_moments; the header states it too) is the
// same level kernel with the template flag VAR: beside c_L it carries v_L, the
// variance of the pixel's mean luminance (k_dn_v0 forms v_0 from the moments),
// and a keep plane, the detail each level removed that the noise estimate does
// not explain.  STAGE 1 / 2 stage v_L with the tile (40 B per staged pixel,
// 17.3 / 25.6 KB); the 3 x 3 prefilter of v_L reads the staged tile (halo >= 2)
// or, STAGE 0, global memory.  The last level adds keep and packs.  The three
// VAR = false instantiations are the code they were without the flag.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "tmpt_render.h"

namespace tmpt {

constexpr int kDnTX = 32, kDnTY = 8;       // a block's tile: one lane per pixel
constexpr uint32_t kNoCov = 0xFFFFFFFFu;   // zb word of a pixel no sample hit (hits == 0)
constexpr uint32_t kNoPixel = 0xFFFFFFFEu; // zb word of a staged halo entry outside the frame
constexpr uint32_t kNaN = 0x7FC00000u;

struct DnArgs {
    int32_t W, H, stride, normal_exp;
    float sigma_depth, sigma_direct;
};
// the arguments of a VAR level: v_L, v_(L+1), the keep plane (not read at the
// first level, not written at the last), shrink
struct DnVarArgs : DnArgs {
    const float* vin;
    float* vout;
    float4* keep;
    float shrink;
    int32_t first, last;
};
template <bool VAR>
using DnArgsT = std::conditional_t<VAR, DnVarArgs, DnArgs>;

__global__ void __launch_bounds__(256) k_dn_guides(const float4* __restrict__ aov, int64_t n, float spp,
                                                   float4* __restrict__ g0, float* __restrict__ g1)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float4 a = aov[2 * p], b = aov[2 * p + 1];  // {normal.xyz, depth}, {direct, tri_id, hits, lit}
    const uint32_t hits = __float_as_uint(b.z);
    const f3 nrm = mk(a.x, a.y, a.z);
    const float dd = (nrm.x * nrm.x + nrm.y * nrm.y) + nrm.z * nrm.z;
    const f3 nh = nrm * (1.0f / sqrtf(fmaxf(dd, 1e-30f)));
    uint32_t zw = kNoCov;
    if (hits > 0) {
        const float zb = a.w * (spp / (float)hits);
        zw = zb != zb ? kNaN : __float_as_uint(zb);
    }
    g0[p] = make_float4(nh.x, nh.y, nh.z, __uint_as_float(zw));
    g1[p] = b.x;
}

// v_0 of the noise-aware filter, per pixel, from the frame's moments
// {mu1, mu2, mean 1/n, history length}: in the header's order.
__global__ void __launch_bounds__(256) k_dn_v0(const float4* __restrict__ mom, int64_t n, float* __restrict__ v0)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float4 m = mom[p];
    const float ne = m.w / m.z;
    const float sq = m.x * m.x;
    v0[p] = fmaxf(0.0f, m.y - sq) / fmaxf(ne - 1.0f, 1.0f);
}

// the staged v_L of a VAR level (a function's own LDS array: the VAR = false
// instantiations never name it)
template <int N>
__device__ __forceinline__ float* dn_lds_v()
{
    __shared__ float s_v[N];
    return s_v;
}

// the pixel a lane filters
struct DnCentre {
    f3 nh;
    float zb, dl;
    bool cov;
};

// One tap other than the centre, already known to lie in the frame with
// cov_q == cov_p: its weight, in the header's order, and the two sums.  Returns
// the weight.
__device__ __forceinline__ float dn_tap(const DnArgs& a, const DnCentre& p, float hw, float dist, float4 cq, float4 gq,
                                        float dlq, f3& csum, float& wsum)
{
    float w = hw;
    if (p.cov) {
        const float d = (p.nh.x * gq.x + p.nh.y * gq.y) + p.nh.z * gq.z;
        float c = d > 0.0f ? d : 0.0f;  // fmaxf(0.0f, d)
        for (int k = 0; k < a.normal_exp; ++k) c = c * c;
        w = w * c;
        const float rz = (p.zb - gq.w) / ((a.sigma_depth * fminf(p.zb, gq.w)) * dist);
        w = w * (1.0f / (1.0f + rz * rz));
        const float rd = (p.dl - dlq) / a.sigma_direct;
        w = w * (1.0f / (1.0f + rd * rd));
    }
    csum = csum + mk(cq.x * w, cq.y * w, cq.z * w);
    wsum = wsum + w;
    return w;
}

// STAGE: 0 = global loads at the run-time stride a.stride; 1, 2 = that stride,
// the block's tile + halo staged in LDS.  out8 (last level only, may be null):
// the packed pixels.  VAR: the noise-aware form (a: DnVarArgs).
template <int STAGE, bool VAR = false>
__global__ void __launch_bounds__(256) k_dn_level(const float4* __restrict__ in, const float4* __restrict__ g0,
                                                  const float* __restrict__ g1, float4* __restrict__ out,
                                                  uint32_t* __restrict__ out8, DnArgsT<VAR> a)
{
    constexpr int HALO = 2 * STAGE;
    constexpr int TW = kDnTX + 2 * HALO, TH = kDnTY + 2 * HALO;
    __shared__ float4 s_col[STAGE ? TW * TH : 1];
    __shared__ float4 s_g0[STAGE ? TW * TH : 1];
    __shared__ float s_g1[STAGE ? TW * TH : 1];
    float* s_v = nullptr;
    if constexpr (VAR && STAGE != 0) s_v = dn_lds_v<TW * TH>();
    const int tx = (int)threadIdx.x % kDnTX, ty = (int)threadIdx.x / kDnTX;
    const int x0 = (int)blockIdx.x * kDnTX, y0 = (int)blockIdx.y * kDnTY;
    const int x = x0 + tx, y = y0 + ty;
    const int s = STAGE ? STAGE : a.stride;
    if (STAGE) {
        for (int e = (int)threadIdx.x; e < TW * TH; e += 256) {
            const int ly = e / TW, lx = e - ly * TW;
            const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
            if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
                const int64_t q = (int64_t)gy * a.W + gx;
                s_col[e] = in[q];
                s_g0[e] = g0[q];
                s_g1[e] = g1[q];
                if constexpr (VAR) s_v[e] = a.vin[q];
            } else {
                s_g0[e] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kNoPixel));
            }
        }
        __syncthreads();
    }
    if (x >= a.W || y >= a.H) return;
    const int64_t pi = (int64_t)y * a.W + x;
    const int lc = STAGE ? (ty + HALO) * TW + tx + HALO : 0;
    const float4 cp = STAGE ? s_col[lc] : in[pi];
    const float4 gp = STAGE ? s_g0[lc] : g0[pi];
    DnCentre p;
    p.nh = mk(gp.x, gp.y, gp.z);
    p.zb = gp.w;
    p.dl = STAGE ? s_g1[lc] : g1[pi];
    p.cov = __float_as_uint(gp.w) != kNoCov;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    f3 csum = mk(0.0f, 0.0f, 0.0f);
    float wsum = 0.0f;
    float vsum = 0.0f;  // VAR only
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            if (i == 0 && j == 0) {
                const float w = h[2] * h[2];
                csum = csum + mk(cp.x * w, cp.y * w, cp.z * w);
                wsum = wsum + w;
                if constexpr (VAR) vsum = vsum + (STAGE ? s_v[lc] : a.vin[pi]) * (w * w);
                continue;
            }
            const float hw = h[i + 2] * h[j + 2];
            const float dist = (float)(s * ((i < 0 ? -i : i) > (j < 0 ? -j : j) ? (i < 0 ? -i : i) : (j < 0 ? -j : j)));
            if (STAGE) {
                const int e = lc + (j * TW + i) * STAGE;
                const float4 gq = s_g0[e];
                const uint32_t zw = __float_as_uint(gq.w);
                if (zw == kNoPixel || (zw != kNoCov) != p.cov) continue;
                const float w = dn_tap(a, p, hw, dist, s_col[e], gq, s_g1[e], csum, wsum);
                if constexpr (VAR) vsum = vsum + s_v[e] * (w * w);
            } else {
                const int qx = x + s * i, qy = y + s * j;
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const int64_t q = (int64_t)qy * a.W + qx;
                const float4 gq = g0[q];
                if ((__float_as_uint(gq.w) != kNoCov) != p.cov) continue;
                const float w = dn_tap(a, p, hw, dist, in[q], gq, g1[q], csum, wsum);
                if constexpr (VAR) vsum = vsum + a.vin[q] * (w * w);
            }
        }
    }
    const f3 o = mk(csum.x / wsum, csum.y / wsum, csum.z / wsum);
    if constexpr (VAR) {
        a.vout[pi] = vsum / (wsum * wsum);
        // the 3 x 3 Gaussian of v_L, distance 1 at every level; the centre always counts
        const float k3[3] = {0.25f, 0.5f, 0.25f};
        float gsum = 0.0f, ksum = 0.0f;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                float vq;
                if (STAGE) {
                    const int e = lc + j * TW + i;
                    const uint32_t zw = __float_as_uint(s_g0[e].w);
                    if (zw == kNoPixel || (zw != kNoCov) != p.cov) continue;
                    vq = s_v[e];
                } else {
                    const int qx = x + i, qy = y + j;
                    if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                    const int64_t q = (int64_t)qy * a.W + qx;
                    if ((__float_as_uint(g0[q].w) != kNoCov) != p.cov) continue;
                    vq = a.vin[q];
                }
                const float k = k3[i + 1] * k3[j + 1];
                gsum = gsum + vq * k;
                ksum = ksum + k;
            }
        }
        const float g = gsum / ksum;
        const f3 d = mk(cp.x - o.x, cp.y - o.y, cp.z - o.z);  // the detail this level removed
        const float dy = (0.2126f * d.x + 0.7152f * d.y) + 0.0722f * d.z;
        const float en = dy * dy, nn = a.shrink * g;
        const float gain = en > nn ? (en - nn) / en : 0.0f;  // a NaN compares false
        float4 kp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!a.first) kp = a.keep[pi];
        kp.x = kp.x + d.x * gain;
        kp.y = kp.y + d.y * gain;
        kp.z = kp.z + d.z * gain;
        if (a.last) {
            const f3 r = mk(o.x + kp.x, o.y + kp.y, o.z + kp.z);
            out[pi] = make_float4(r.x, r.y, r.z, cp.w);
            if (out8) out8[pi] = pack_pixel(r, 1.0f);
        } else {
            a.keep[pi] = kp;
            out[pi] = make_float4(o.x, o.y, o.z, cp.w);
        }
    } else {
        out[pi] = make_float4(o.x, o.y, o.z, cp.w);
        if (out8) out8[pi] = pack_pixel(o, 1.0f);
    }
}

// Which strides read the staged LDS tile (option denoise_lds = -1): 1 and 2.
// Measured on the bench frame (1920 x 1080, AOVs at 64 spp; tools/denoise_time.py,
// profiles/denoise_time.log, DESIGN.md "Denoiser"), a level's time, direct /
// staged, medians of 5: stride 1 (with the guide preparation) 0.134 / 0.116 ms,
// stride 2 0.109 / 0.094 ms; at the 1/8 shard's height 0.031 / 0.027 and 0.022 /
// 0.020 ms (run-to-run spread of the one-level call: 0.011 and 0.001 ms).  From stride 4 the halo
// (4 strides of rows and columns around an 8-row tile) outgrows the tile, and
// the direct form is the only one built.
static bool dn_staged(const Options& o, int stride)
{
    if (stride > 2) return false;
    if (o.denoise_lds >= 0) return o.denoise_lds != 0;
    return true;
}

// Both filters' host side.  VAR: tmpt_denoise_moments (d_mom, shrink); the
// workspace then holds two float planes (v_L, ping-pong) and the keep plane too.
template <bool VAR>
static int dn_run(Scene& s, const char* what, const tmpt_denoise_desc* d, float shrink, const float4* d_in,
                  const tmpt_aov_pixel* d_aov, const float4* d_mom, float4* d_out32, uint32_t* d_out8)
{
    const int64_t n = (int64_t)d->width * d->height;
    // workspace: two colour planes, then the guide planes (VAR: keep, then two variance planes)
    const size_t plane = sizeof(float4) * (size_t)n, fplane = sizeof(float) * (size_t)n;
    if (ensure_ws(s, VAR ? 4 * plane + 3 * fplane : 3 * plane + fplane)) return -1;
    float4* pl[2] = {s.ws.as<float4>(), reinterpret_cast<float4*>(s.ws.as<char>() + plane)};
    float4* g0 = reinterpret_cast<float4*>(s.ws.as<char>() + 2 * plane);
    float* g1 = reinterpret_cast<float*>(s.ws.as<char>() + 3 * plane);
    float4* keep = reinterpret_cast<float4*>(s.ws.as<char>() + 3 * plane + fplane);  // VAR only, as vp
    float* vp[2] = {reinterpret_cast<float*>(s.ws.as<char>() + 4 * plane + fplane),
                    reinterpret_cast<float*>(s.ws.as<char>() + 4 * plane + 2 * fplane)};
    tmpt_render_desc wd{};
    wd.flags = d->flags;
    wd.wait_stream = d->wait_stream;
    if (int rc = wait_caller_stream(s, &wd, what)) return rc;
    if (ensure_counters(s)) return -1;  // the scene's timing events
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    k_dn_guides<<<(unsigned)((n + 255) / 256), 256, 0, s.stream>>>(reinterpret_cast<const float4*>(d_aov), n,
                                                                   (float)d->spp, g0, g1);
    TMPT_HIP(hipGetLastError());
    if (VAR) {
        k_dn_v0<<<(unsigned)((n + 255) / 256), 256, 0, s.stream>>>(d_mom, n, vp[1]);
        TMPT_HIP(hipGetLastError());
    }
    DnArgsT<VAR> a{};
    static_cast<DnArgs&>(a) = DnArgs{d->width, d->height, 1, d->normal_exp, d->sigma_depth, d->sigma_direct};
    const dim3 grid((unsigned)((d->width + kDnTX - 1) / kDnTX), (unsigned)((d->height + kDnTY - 1) / kDnTY));
    const float4* src = d_in;
    for (int L = 0; L < d->levels; ++L) {
        const bool last = L == d->levels - 1;
        // the last level writes the caller's buffer, unless that is the buffer
        // this level's taps still read (one level, in place) or there is none
        float4* dst = pl[L & 1];
        if (last && d_out32 && (const float4*)d_out32 != src) dst = d_out32;
        uint32_t* o8 = last ? d_out8 : nullptr;
        a.stride = 1 << L;
        if constexpr (VAR) {
            a.vin = vp[(L + 1) & 1];
            a.vout = vp[L & 1];
            a.keep = keep;
            a.shrink = shrink;
            a.first = L == 0;
            a.last = last;
        }
        if (a.stride == 1 && dn_staged(s.opt, 1))
            k_dn_level<1, VAR><<<grid, 256, 0, s.stream>>>(src, g0, g1, dst, o8, a);
        else if (a.stride == 2 && dn_staged(s.opt, 2))
            k_dn_level<2, VAR><<<grid, 256, 0, s.stream>>>(src, g0, g1, dst, o8, a);
        else
            k_dn_level<0, VAR><<<grid, 256, 0, s.stream>>>(src, g0, g1, dst, o8, a);
        TMPT_HIP(hipGetLastError());
        if (last && d_out32 && dst != d_out32)
            TMPT_HIP(hipMemcpyAsync(d_out32, dst, plane, hipMemcpyDeviceToDevice, s.stream));
        src = dst;
    }
    (void)hipEventRecord(e1, s.stream);
    const hipError_t se = hipStreamSynchronize(s.stream);
    if (se != hipSuccess) {
        set_error(std::string(what) + ": " + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    s.render_ms = ms;
    return 0;
}

int denoise(Scene& s, const tmpt_denoise_desc* d, const float4* d_in, const tmpt_aov_pixel* d_aov, float4* d_out32,
            uint32_t* d_out8)
{
    return dn_run<false>(s, "tmpt_denoise", d, 0.0f, d_in, d_aov, nullptr, d_out32, d_out8);
}

int denoise_moments(Scene& s, const tmpt_denoise_desc* d, float shrink, const float4* d_in, const tmpt_aov_pixel* d_aov,
                    const float4* d_mom, float4* d_out32, uint32_t* d_out8)
{
    return dn_run<true>(s, "tmpt_denoise_moments", d, shrink, d_in, d_aov, d_mom, d_out32, d_out8);
}

}  // namespace tmpt
