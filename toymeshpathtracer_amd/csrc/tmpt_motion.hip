// tmpt_motion.hip -- temporal accumulation (include/tmpt.h "Temporal
// accumulation"): the motion pass (tmpt_render_motion, tmpt_motion_pixel) and
// the reprojected history (tmpt_temporal, tmpt_temporal_desc).  The header
// states the arithmetic, and that statement is the contract: float32, one
// rounding per operation, a fixed order -- this file only schedules it.
//
// k_motion: one lane per pixel, one closest-hit query per lane through the
// traversal every engine steps (tmpt_traverse.h), with the scene's tie, crack
// and flat handling and the octree root test, as k_aov's camera rays get them;
// then the hit's material point in the previous pose (the same triangle slot,
// the same barycentrics) projected through the previous camera.  No jump
// tables, no shadow query.  A wave takes 64 pixels per ticket: TILE = false,
// 64 consecutive pixels of the tile in row order; TILE = true, an 8 x 8 block
// of them, so that the wave's rays span a square of the image instead of a
// line.  Which one runs: motion_tiled() below (the row: the two measured alike).
//
// k_temporal: one lane per pixel, a 32 x 8 block of pixels per 256-thread
// block as the denoiser's levels; four history taps and four previous motion
// records per pixel, global loads.
//
// k_temporal_clip<R> (tmpt_temporal_clip): k_temporal's fetch, then the history
// clipped to the mean +- gamma * sigma of the (2R+1)^2 window of the statistics
// frame, which the block stages in LDS with its halo; optionally a second (aux)
// frame through the same taps and blend factor.
//
// k_sample_plan (tmpt_sample_plan): k_temporal's fetch over the accumulated
// moments frame, then the per-pixel prior of tmpt_render_guided.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "tmpt_render.h"

namespace tmpt {

static_assert(sizeof(tmpt_motion_pixel) == 32, "motion record: two 16-byte stores");
static_assert(sizeof(tmpt_temporal_desc) == 48, "tmpt_temporal_desc: 48 bytes");
static_assert(sizeof(tmpt_temporal_clip_desc) == 56, "tmpt_temporal_clip_desc: 56 bytes");

constexpr int kMotionTicket = 8;  // counters[]: the next 64-pixel unit no wave has taken

struct MotionArgs {
    Camera prev;            // the previous frame's camera
    const float* prev9;     // the previous pose, 9 floats per triangle; null: the scene's own vertices
    float fw, fh;           // (float)width, (float)height
    int32_t tiles_x;        // TILE: 8 x 8 units per row of units
    int64_t units;          // tickets of the tile
};

template <bool TILE, int BLOCK, int SL>
__global__ void __launch_bounds__(BLOCK) k_motion(SceneView sv, RenderArgs a, MotionArgs m, float4* __restrict__ out,
                                                  uint32_t* __restrict__ ovf,
                                                  unsigned long long* __restrict__ counters)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    TravCount cnt;
    const int lane = lane_id();
    uint32_t rays = 0;
    for (;;) {
        // one ticket per wave (at most 10^8 pixels, so fewer units: 32 bits hold them)
        uint32_t tk = 0;
        if (lane == 0) tk = (uint32_t)atomicAdd(&counters[kMotionTicket], 1ull);
        const int64_t unit = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)tk);
        if (unit >= m.units) break;
        int lr;
        int64_t xi;
        if (TILE) {
            const int uy = (int)(unit / m.tiles_x), ux = (int)(unit - (int64_t)uy * m.tiles_x);
            lr = uy * 8 + (lane >> 3);
            xi = (int64_t)ux * 8 + (lane & 7);
        } else {
            const int64_t pix = unit * 64 + lane;
            lr = (int)(pix / a.W);
            xi = pix - (int64_t)lr * a.W;
        }
        const bool live = lr < a.tile_rows && xi < a.W;
        if (!live) continue;  // the wave's other lanes go on; nothing below crosses lanes
        const uint32_t x = (uint32_t)xi;
        const uint32_t y = (uint32_t)tile_row_to_y(a, lr);
        // the centre ray: the camera's expression with no lens offset at all
        const float cs = ((float)x + 0.5f) * a.invW, ct = ((float)y + 0.5f) * a.invH;
        const f3 o = a.cam.origin;
        const f3 d = normalize(a.cam.lower_left + cs * a.cam.horizontal + ct * a.cam.vertical - a.cam.origin);
        ++rays;
        float t = 0.0f, u = 0.0f, v = 0.0f;
        int id = -1;
        if (a.root_check && !octree_root_hit(sv, o, d, kMinT, kMaxT)) {
            atomicAdd(&sv.oct->ties[1], 1ull);  // the ray misses the reference's root box
        } else {
            id = traverse<false, false, BLOCK, SL>(sv, make_trav_ray(o, d), kMinT, kMaxT, t, u, v, st, cnt);
        }
        float4* p = out + 2 * ((int64_t)lr * a.W + xi);
        if (id < 0 || TMPT_CHK(sv.chk, (uint32_t)id < (uint32_t)max(sv.n, 1), kChkTri, id)) {
            p[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            p[1] = make_float4(0.0f, 0.0f, __int_as_float(-1), __uint_as_float(0u));
            continue;
        }
        f3 v0, v1, v2;
        if (m.prev9) {
            const float* q = m.prev9 + 9 * (int64_t)id;
            v0 = mk(q[0], q[1], q[2]);
            v1 = mk(q[3], q[4], q[5]);
            v2 = mk(q[6], q[7], q[8]);
        } else {
            const float4* q = reinterpret_cast<const float4*>(sv.tri_orig + id);
            const float4 qa = q[0], qb = q[1], qc = q[2];
            v0 = mk(qa.x, qa.y, qa.z);
            v1 = mk(qa.w, qb.x, qb.y);
            v2 = mk(qb.z, qb.w, qc.x);
        }
        const f3 pp = hit_pos(v0, v1, v2, u, v);
        const Camera& c = m.prev;
        const f3 dd = pp - c.origin, q = c.lower_left - c.origin;
        const float den = dot(dd, c.w), num = dot(q, c.w);
        float px = 0.0f, py = 0.0f, dp = 0.0f;
        uint32_t flags = 1u;
        if (den < 0.0f) {
            const float k = num / den;
            const f3 r = mk(k * dd.x - q.x, k * dd.y - q.y, k * dd.z - q.z);
            px = (dot(r, c.horizontal) / dot(c.horizontal, c.horizontal)) * m.fw;
            py = (dot(r, c.vertical) / dot(c.vertical, c.vertical)) * m.fh;
            dp = sqrtf(dot(dd, dd));
            flags |= 2u;
        }
        p[0] = make_float4(px, py, t, dp);
        p[1] = make_float4(u, v, __int_as_float(id), __uint_as_float(flags));
    }
    // [0] every query, [3] the closest-hit ones (as the path kernels count)
    const uint32_t r0 = wave_sum(rays);
    if (lane == 0) {
        atomicAdd(&counters[0], (unsigned long long)r0);
        atomicAdd(&counters[3], (unsigned long long)r0);
    }
}

// motion_tile = -1: which unit a wave takes.  Measured on the bench frame
// (1920 x 1080, 2.07 M rays; tools/temporal_time.py, profiles/temporal_time.log,
// DESIGN.md "Temporal accumulation"), medians of 9 interleaved rounds, row of
// 64 / 8 x 8 block: 0.5667 / 0.5681 ms with the scene's own vertices, 0.5612 /
// 0.5708 ms with a previous pose given, each with a spread of 0.03 - 0.04 ms --
// the block buys nothing the spread does not cover, so the row, whose pixel
// index is one division, is what runs.
static bool motion_tiled(const Options& o)
{
    if (o.motion_tile >= 0) return o.motion_tile != 0;
    return false;
}

template <bool TILE>
static int launch_motion(Scene& s, const RenderArgs& a, MotionArgs m, tmpt_motion_pixel* d_out)
{
    auto fn = k_motion<TILE, kBlk, kSL>;
    m.tiles_x = (a.W + 7) / 8;
    m.units = TILE ? (int64_t)m.tiles_x * ((a.tile_rows + 7) / 8) : (a.slots + 63) / 64;
    const int resident = occupancy_grid((const void*)fn, kBlk, 0, s.device);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(resident, (m.units * 64 + kBlk - 1) / kBlk));
    const size_t ovf_bytes = (size_t)grid * kBlk * (kStackTotal - kSL) * sizeof(uint32_t);
    if (ensure_ws(s, ovf_bytes)) return -1;
    fn<<<grid, kBlk, 0, s.stream>>>(view(s), a, m, reinterpret_cast<float4*>(d_out), s.ws.as<uint32_t>(), s.counters);
    TMPT_HIP(hipGetLastError());
    return 0;
}

// The call leaves the progressive state, the colour buffer, the redo list and
// the jump tables alone; it shares the workspace and the counters with render().
// d_prev: the previous pose on the device (9 floats per triangle), or null.
int render_motion(Scene& s, const tmpt_camera* cam, const tmpt_camera* prev_cam, const float* d_prev,
                  const tmpt_render_desc* d, tmpt_motion_pixel* d_out, uint64_t* ray_count)
{
    tmpt_render_desc rd = *d;  // spp is not read: make_args divides by it
    rd.spp = 1;
    rd.spp_begin = rd.spp_count = 0;
    RenderArgs a = make_args(cam, &rd);
    const RenderArgs pa = make_args(prev_cam, &rd);
    MotionArgs m{pa.cam, d_prev, (float)d->width, (float)d->height, 0, 0};
    s.row_render = s.pixel_render = false;  // the walk's defaults as the AOV pass has them
    if (int rc = wait_caller_stream(s, d, "tmpt_render_motion")) return rc;
    if (ensure_counters(s)) return -1;
    a.root_check = camera_root_check(s, a.cam);
    TMPT_HIP(hipMemsetAsync(s.counters, 0, kRenderCounters * sizeof(unsigned long long), s.stream));
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    reset_render_stats(s);
    int rc = 0;
    if (a.slots > 0) rc = motion_tiled(s.opt) ? launch_motion<true>(s, a, m, d_out) : launch_motion<false>(s, a, m, d_out);
    (void)hipEventRecord(e1, s.stream);
    hipError_t se = rc == 0 ? hipMemcpyAsync(s.counters_host, s.counters, kRenderCounters * sizeof(unsigned long long),
                                             hipMemcpyDeviceToHost, s.stream)
                            : hipSuccess;
    const hipError_t se2 = hipStreamSynchronize(s.stream);
    if (se == hipSuccess) se = se2;
    if (rc) return rc;
    if (se != hipSuccess) {
        set_error(std::string("tmpt_render_motion: ") + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const unsigned long long* c = s.counters_host;
    s.render_ms = ms;
    s.extend_ms = ms;
    s.extend_rays = c[3];
    s.shadow_rays = 0;
    s.extend_launches = a.slots > 0 ? 1 : 0;
    s.iterations = s.extend_launches;
    s.tie_queries = c[kTieCounter];
    s.root_misses = c[kTieCounter + 1];
    s.crack_queries = c[kCrackCounter];
    if (ray_count) *ray_count = c[0];
    return 0;
}

// ---------------------------------------------------------------- the blend
constexpr int kTpTX = 32, kTpTY = 8;  // a block's pixels: one lane each

struct TemporalArgs {
    int32_t W, H;
    float n_max, sigma_depth;
};

__global__ void __launch_bounds__(256) k_temporal(const float4* cur, const float4* __restrict__ motion,
                                                  const float4* __restrict__ pmotion, const float4* __restrict__ hist,
                                                  float4* out, uint32_t* __restrict__ out8, TemporalArgs a)
{
    const int x = (int)blockIdx.x * kTpTX + (int)threadIdx.x % kTpTX;
    const int y = (int)blockIdx.y * kTpTY + (int)threadIdx.x / kTpTX;
    if (x >= a.W || y >= a.H) return;
    const int64_t pi = (int64_t)y * a.W + x;
    const float4 c = cur[pi];  // (out may be cur: this lane alone reads and writes pixel pi)
    const float4 m0 = motion[2 * pi], m1 = motion[2 * pi + 1];  // {px, py, depth, depth_prev}, {u, v, tri, flags}
    f3 o = mk(c.x, c.y, c.z);
    float n = 1.0f;
    const float mpx = m0.x, mpy = m0.y, dprev = m0.w;
    const bool valid = (__float_as_uint(m1.w) & 2u) != 0 && mpx >= -1.0f && mpx < (float)a.W + 1.0f && mpy >= -1.0f &&
                       mpy < (float)a.H + 1.0f;
    if (valid) {
        const float fx = mpx - 0.5f, fy = mpy - 0.5f;
        const float x0 = floorf(fx), y0 = floorf(fy);
        const float ax = fx - x0, ay = fy - y0;
        const int ix = (int)x0, iy = (int)y0;
        f3 csum = mk(0.0f, 0.0f, 0.0f);
        float nsum = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int qx = ix + i, qy = iy + j;
                const float wgt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const int64_t q = (int64_t)qy * a.W + qx;
                const float4 p0 = pmotion[2 * q], p1 = pmotion[2 * q + 1];
                if (!(__float_as_uint(p1.w) & 1u)) continue;
                if (fabsf(p0.z - dprev) > a.sigma_depth * dprev) continue;
                const float4 hq = hist[q];
                csum = csum + mk(hq.x * wgt, hq.y * wgt, hq.z * wgt);
                nsum = nsum + hq.w * wgt;
                wsum = wsum + wgt;
            }
        }
        if (wsum > 0.0f) {
            const f3 h = mk(csum.x / wsum, csum.y / wsum, csum.z / wsum);
            n = fminf(nsum / wsum + 1.0f, a.n_max);
            const float al = 1.0f / n;
            o = mk(h.x + (c.x - h.x) * al, h.y + (c.y - h.y) * al, h.z + (c.z - h.z) * al);
        }
    }
    if (out) out[pi] = make_float4(o.x, o.y, o.z, n);
    if (out8) out8[pi] = pack_pixel(o, 1.0f);
}

// d (checked by the caller) holds the resolved n_max and sigma_depth; every
// pointer on the device; d_out32 or d_out8 may be null; d_out32 may be d_cur.
int temporal(Scene& s, const tmpt_temporal_desc* d, const float4* d_cur, const tmpt_motion_pixel* d_motion,
             const tmpt_motion_pixel* d_pmotion, const float4* d_hist, float4* d_out32, uint32_t* d_out8)
{
    tmpt_render_desc wd{};
    wd.flags = d->flags;
    wd.wait_stream = d->wait_stream;
    if (int rc = wait_caller_stream(s, &wd, "tmpt_temporal")) return rc;
    if (ensure_counters(s)) return -1;  // the scene's timing events
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    const TemporalArgs a{d->width, d->height, d->n_max, d->sigma_depth};
    const dim3 grid((unsigned)((d->width + kTpTX - 1) / kTpTX), (unsigned)((d->height + kTpTY - 1) / kTpTY));
    k_temporal<<<grid, 256, 0, s.stream>>>(d_cur, reinterpret_cast<const float4*>(d_motion),
                                           reinterpret_cast<const float4*>(d_pmotion), d_hist, d_out32, d_out8, a);
    TMPT_HIP(hipGetLastError());
    (void)hipEventRecord(e1, s.stream);
    const hipError_t se = hipStreamSynchronize(s.stream);
    if (se != hipSuccess) {
        set_error(std::string("tmpt_temporal: ") + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    s.render_ms = ms;
    return 0;
}

// ---------------------------------------------------------------- the sample plan
// k_sample_plan (tmpt_sample_plan): k_temporal's fetch, statement for statement,
// over the accumulated moments frame, then the prior the guided render's test
// reads -- {history luminance, the history's share of the blended variance, this
// frame's blend factor, history length}.  One lane per pixel, a block's 32 x 8
// pixels as k_temporal; no colour frame is read.  A kernel of its own, so that
// k_temporal and k_temporal_clip keep their code as it is.
__global__ void __launch_bounds__(256) k_sample_plan(const float4* __restrict__ motion,
                                                     const float4* __restrict__ pmotion,
                                                     const float4* __restrict__ hist, float4* __restrict__ out,
                                                     TemporalArgs a)
{
    const int x = (int)blockIdx.x * kTpTX + (int)threadIdx.x % kTpTX;
    const int y = (int)blockIdx.y * kTpTY + (int)threadIdx.x / kTpTX;
    if (x >= a.W || y >= a.H) return;
    const int64_t pi = (int64_t)y * a.W + x;
    const float4 m0 = motion[2 * pi], m1 = motion[2 * pi + 1];  // {px, py, depth, depth_prev}, {u, v, tri, flags}
    float4 pr = make_float4(0.0f, 0.0f, 1.0f, 0.0f);            // the null prior
    const float mpx = m0.x, mpy = m0.y, dprev = m0.w;
    const bool valid = (__float_as_uint(m1.w) & 2u) != 0 && mpx >= -1.0f && mpx < (float)a.W + 1.0f && mpy >= -1.0f &&
                       mpy < (float)a.H + 1.0f;
    if (valid) {
        const float fx = mpx - 0.5f, fy = mpy - 0.5f;
        const float x0 = floorf(fx), y0 = floorf(fy);
        const float ax = fx - x0, ay = fy - y0;
        const int ix = (int)x0, iy = (int)y0;
        f3 asum = mk(0.0f, 0.0f, 0.0f);
        float nsum = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int qx = ix + i, qy = iy + j;
                const float wgt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const int64_t q = (int64_t)qy * a.W + qx;
                const float4 p0 = pmotion[2 * q], p1 = pmotion[2 * q + 1];
                if (!(__float_as_uint(p1.w) & 1u)) continue;
                if (fabsf(p0.z - dprev) > a.sigma_depth * dprev) continue;
                const float4 hq = hist[q];
                asum = asum + mk(hq.x * wgt, hq.y * wgt, hq.z * wgt);
                nsum = nsum + hq.w * wgt;
                wsum = wsum + wgt;
            }
        }
        if (wsum > 0.0f) {
            const float hY = asum.x / wsum, h2 = asum.y / wsum, hz = asum.z / wsum, nh = nsum / wsum;
            const float ne = nh / hz;
            const float vh = fmaxf(0.0f, h2 - hY * hY) / fmaxf(ne - 1.0f, 1.0f);
            const float n = fminf(nh + 1.0f, a.n_max);
            const float al = 1.0f / n, be = 1.0f - al;
            pr = make_float4(hY, (be * be) * vh, al, nh);
        }
    }
    out[pi] = pr;
}

// d (checked by the caller) holds the resolved n_max and sigma_depth; every
// pointer on the device; d_out overlaps no input (the caller's check).
int sample_plan(Scene& s, const tmpt_temporal_desc* d, const tmpt_motion_pixel* d_motion,
                const tmpt_motion_pixel* d_pmotion, const float4* d_hist, float4* d_out)
{
    tmpt_render_desc wd{};
    wd.flags = d->flags;
    wd.wait_stream = d->wait_stream;
    if (int rc = wait_caller_stream(s, &wd, "tmpt_sample_plan")) return rc;
    if (ensure_counters(s)) return -1;  // the scene's timing events
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    const TemporalArgs a{d->width, d->height, d->n_max, d->sigma_depth};
    const dim3 grid((unsigned)((d->width + kTpTX - 1) / kTpTX), (unsigned)((d->height + kTpTY - 1) / kTpTY));
    k_sample_plan<<<grid, 256, 0, s.stream>>>(reinterpret_cast<const float4*>(d_motion),
                                              reinterpret_cast<const float4*>(d_pmotion), d_hist, d_out, a);
    TMPT_HIP(hipGetLastError());
    (void)hipEventRecord(e1, s.stream);
    const hipError_t se = hipStreamSynchronize(s.stream);
    if (se != hipSuccess) {
        set_error(std::string("tmpt_sample_plan: ") + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    s.render_ms = ms;
    return 0;
}

// ---------------------------------------------------------------- the clipped blend
struct TemporalClipArgs {
    int32_t W, H;
    float n_max, sigma_depth, gamma;
};

// R: the window's radius.  The block's 32 x 8 pixels of the statistics frame and
// a halo of R around them are staged in LDS, the coverage of each slot in .w:
// 1.0f covered, 0.0f not, -1.0f outside the frame (no load is issued there), so
// that "skipped" is one comparison with the pixel's own coverage.  Every lane of
// the block stages and takes the barrier, the ones outside the frame too.
template <int R>
__global__ void __launch_bounds__(256)
    k_temporal_clip(const float4* cur, const float4* stat, const float4* __restrict__ motion,
                    const float4* __restrict__ pmotion, const float4* __restrict__ hist, const float4* aux_cur,
                    const float4* __restrict__ aux_hist, float4* aux_out, float4* __restrict__ out,
                    uint32_t* __restrict__ out8, TemporalClipArgs a)
{
    constexpr int TW = kTpTX + 2 * R, TH = kTpTY + 2 * R;
    __shared__ float4 s_tile[TW * TH];
    const int tx = (int)threadIdx.x % kTpTX, ty = (int)threadIdx.x / kTpTX;
    const int bx0 = (int)blockIdx.x * kTpTX - R, by0 = (int)blockIdx.y * kTpTY - R;
    const uint32_t* mwords = reinterpret_cast<const uint32_t*>(motion);
    for (int s = (int)threadIdx.x; s < TW * TH; s += 256) {
        const int sy = s / TW, sx = s - sy * TW;
        const int gx = bx0 + sx, gy = by0 + sy;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const int64_t q = (int64_t)gy * a.W + gx;
            const float4 sq = stat[q];
            v = make_float4(sq.x, sq.y, sq.z, (mwords[8 * q + 7] & 1u) ? 1.0f : 0.0f);
        }
        s_tile[s] = v;
    }
    __syncthreads();
    const int x = (int)blockIdx.x * kTpTX + tx;
    const int y = (int)blockIdx.y * kTpTY + ty;
    if (x >= a.W || y >= a.H) return;
    const int64_t pi = (int64_t)y * a.W + x;
    const float4 c = cur[pi];
    const float4 m0 = motion[2 * pi], m1 = motion[2 * pi + 1];  // {px, py, depth, depth_prev}, {u, v, tri, flags}
    float4 ac = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (aux_cur) ac = aux_cur[pi];  // (aux_out may be aux_cur: this lane alone reads and writes pixel pi)
    f3 o = mk(c.x, c.y, c.z), ao = mk(ac.x, ac.y, ac.z);
    float n = 1.0f;
    const float mpx = m0.x, mpy = m0.y, dprev = m0.w;
    const bool valid = (__float_as_uint(m1.w) & 2u) != 0 && mpx >= -1.0f && mpx < (float)a.W + 1.0f && mpy >= -1.0f &&
                       mpy < (float)a.H + 1.0f;
    if (valid) {
        const float fx = mpx - 0.5f, fy = mpy - 0.5f;
        const float x0 = floorf(fx), y0 = floorf(fy);
        const float ax = fx - x0, ay = fy - y0;
        const int ix = (int)x0, iy = (int)y0;
        f3 csum = mk(0.0f, 0.0f, 0.0f), asum = mk(0.0f, 0.0f, 0.0f);
        float nsum = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int qx = ix + i, qy = iy + j;
                const float wgt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const int64_t q = (int64_t)qy * a.W + qx;
                const float4 p0 = pmotion[2 * q], p1 = pmotion[2 * q + 1];
                if (!(__float_as_uint(p1.w) & 1u)) continue;
                if (fabsf(p0.z - dprev) > a.sigma_depth * dprev) continue;
                const float4 hq = hist[q];
                csum = csum + mk(hq.x * wgt, hq.y * wgt, hq.z * wgt);
                nsum = nsum + hq.w * wgt;
                wsum = wsum + wgt;
                if (aux_hist) {
                    const float4 aq = aux_hist[q];
                    asum = asum + mk(aq.x * wgt, aq.y * wgt, aq.z * wgt);
                }
            }
        }
        if (wsum > 0.0f) {
            const f3 h = mk(csum.x / wsum, csum.y / wsum, csum.z / wsum);
            // the window, rows outer: the statement's order
            const float covp = (__float_as_uint(m1.w) & 1u) ? 1.0f : 0.0f;
            f3 s1 = mk(0.0f, 0.0f, 0.0f), s2 = mk(0.0f, 0.0f, 0.0f);
            float cnt = 0.0f;
#pragma unroll
            for (int j = 0; j <= 2 * R; ++j) {
#pragma unroll
                for (int i = 0; i <= 2 * R; ++i) {
                    const float4 t = s_tile[(ty + j) * TW + (tx + i)];
                    if (t.w != covp) continue;
                    s1 = s1 + mk(t.x, t.y, t.z);
                    s2 = s2 + mk(t.x * t.x, t.y * t.y, t.z * t.z);
                    cnt = cnt + 1.0f;
                }
            }
            const f3 mu = mk(s1.x / cnt, s1.y / cnt, s1.z / cnt);
            const f3 g = mk(a.gamma * sqrtf(fmaxf(0.0f, s2.x / cnt - mu.x * mu.x)),
                            a.gamma * sqrtf(fmaxf(0.0f, s2.y / cnt - mu.y * mu.y)),
                            a.gamma * sqrtf(fmaxf(0.0f, s2.z / cnt - mu.z * mu.z)));
            const f3 hc = mk(fminf(fmaxf(h.x, mu.x - g.x), mu.x + g.x), fminf(fmaxf(h.y, mu.y - g.y), mu.y + g.y),
                             fminf(fmaxf(h.z, mu.z - g.z), mu.z + g.z));
            const float e = fmaxf(fmaxf(fabsf(h.x - hc.x), fabsf(h.y - hc.y)), fabsf(h.z - hc.z));
            const float span = fmaxf(fmaxf(g.x, g.y), g.z);
            float nh = nsum / wsum;
            if (e > 0.0f) nh = nh * (span / (span + e));
            n = fminf(nh + 1.0f, a.n_max);
            const float al = 1.0f / n;
            o = mk(hc.x + (c.x - hc.x) * al, hc.y + (c.y - hc.y) * al, hc.z + (c.z - hc.z) * al);
            if (aux_cur) {
                const f3 ha = mk(asum.x / wsum, asum.y / wsum, asum.z / wsum);
                ao = mk(ha.x + (ac.x - ha.x) * al, ha.y + (ac.y - ha.y) * al, ha.z + (ac.z - ha.z) * al);
            }
        }
    }
    if (out) out[pi] = make_float4(o.x, o.y, o.z, n);
    if (aux_out) aux_out[pi] = make_float4(ao.x, ao.y, ao.z, n);
    if (out8) out8[pi] = pack_pixel(o, 1.0f);
}

// d (checked by the caller) holds the resolved n_max, sigma_depth, gamma and
// radius (1..3); every pointer on the device; d_stat is a frame (d_cur where the
// caller gave none); the three aux pointers all or none; d_out32 or d_out8 may be
// null.  The outputs overlap no frame whose neighbours are read (the caller's check).
int temporal_clip(Scene& s, const tmpt_temporal_clip_desc* d, const float4* d_cur, const float4* d_stat,
                  const tmpt_motion_pixel* d_motion, const tmpt_motion_pixel* d_pmotion, const float4* d_hist,
                  const float4* d_aux_cur, const float4* d_aux_hist, float4* d_aux_out, float4* d_out32,
                  uint32_t* d_out8)
{
    tmpt_render_desc wd{};
    wd.flags = d->flags;
    wd.wait_stream = d->wait_stream;
    if (int rc = wait_caller_stream(s, &wd, "tmpt_temporal_clip")) return rc;
    if (ensure_counters(s)) return -1;  // the scene's timing events
    hipEvent_t e0 = s.render_ev[0], e1 = s.render_ev[1];
    TMPT_HIP(hipEventRecord(e0, s.stream));
    const TemporalClipArgs a{d->width, d->height, d->n_max, d->sigma_depth, d->gamma};
    const dim3 grid((unsigned)((d->width + kTpTX - 1) / kTpTX), (unsigned)((d->height + kTpTY - 1) / kTpTY));
    auto fn = d->radius == 1 ? k_temporal_clip<1> : d->radius == 2 ? k_temporal_clip<2> : k_temporal_clip<3>;
    fn<<<grid, 256, 0, s.stream>>>(d_cur, d_stat, reinterpret_cast<const float4*>(d_motion),
                                   reinterpret_cast<const float4*>(d_pmotion), d_hist, d_aux_cur, d_aux_hist, d_aux_out,
                                   d_out32, d_out8, a);
    TMPT_HIP(hipGetLastError());
    (void)hipEventRecord(e1, s.stream);
    const hipError_t se = hipStreamSynchronize(s.stream);
    if (se != hipSuccess) {
        set_error(std::string("tmpt_temporal_clip: ") + hipGetErrorString(se));
        return -1;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    s.render_ms = ms;
    return 0;
}

}  // namespace tmpt
