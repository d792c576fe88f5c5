// tmpt_wavefront.hip -- the wavefront engine and its driver, render_wavefront
// (render() in tmpt_render.hip calls it):
//  * wavefront (pixel mode): per-pixel path state in HBM (SoA), one slot per
//    pixel of the tile; every iteration runs
//        extend  closest-hit traversal of the active queue     (persistent waves)
//        shade   hit -> shadow ray + next bounce; miss/max depth -> backward
//                recurrence, accumulate, next camera sample or pixel write
//        shadow  any-hit traversal of the shadow queue          (persistent waves)
//    queues are compacted with wave64 ballot + mbcnt prefix and ONE atomic per
//    wave.  Samples of a pixel stay sequential (its RNG stream threads through
//    them, main.cpp:204-218), so parallelism is over pixels.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "tmpt_render.h"

namespace tmpt {

// ============================================================ wavefront
// (the segmented queues' constants kSeg, kCtr, kChunk: tmpt_render.h, shared with k_path's pixel supply)
constexpr uint32_t kSkip = 0x80000000u;  // queue-entry flag: path stopped at kMaxDepth
constexpr uint32_t kDone = 0xFFFFFFFFu;  // depth value of a finished pixel

struct WfState {
    uint32_t* rng;
    uint32_t* smp;
    uint32_t* depth;
    float* col;    // [3][P]
    float* light;  // [kMaxDepth][P]
    float* ray;    // [6][P]  o.xyz d.xyz
    float* hit;    // [3][P]  t u v
    int32_t* hid;  // [P]
    float* sho;    // [3][P] shadow origin
    // Extend queues (per parity): kSeg * nbins sub-queues of seg_cap entries,
    // sub-queue seg * nbins + bin holding the rays of segment seg whose
    // direction falls in octant bin (the low log2(nbins) bits of the sign
    // mask; nbins = 1: no binning), so a wave's 64-entry reservation holds
    // rays from nearby pixels in one octant (sort-by-bounce: every iteration's
    // queue is one bounce).  Counters and fetch heads per sub-queue.
    uint32_t* q[2];
    uint32_t* qs;    // shadow queue: kSeg segments (shadow rays share one direction)
    uint32_t* cnt[2];  // extend sub-queue counts per parity, kSeg * nbins counters (stride kCtr)
    uint32_t* cnt_s;   // shadow queue counts
    uint32_t* head_e;  // fetch heads
    uint32_t* head_s;
    uint32_t* total;   // [0]: entries of the queue the next iteration consumes
    uint32_t* iter_log;  // optional (TMPT_ITER_LOG): per-iteration queue sizes
    unsigned long long* tot;  // [0] extend rays [1] shadow rays [2,3] extend node/tri visits [4,5] shadow
    int64_t P;
    uint32_t seg_cap;
    uint32_t nbins;  // 1, 2, 4 or 8
    int walk_check;  // relaxed head check before a walking wave's atomic (low load, binned queues)
    int root_check;  // RenderArgs::root_check: camera rays (depth 0) take the root box test
};

// octant bin of a direction: bit 0 = x < 0, bit 1 = y < 0, bit 2 = z < 0, low bits only
__device__ __forceinline__ uint32_t dir_bin(f3 d, uint32_t nbins)
{
    const uint32_t o = (uint32_t)signbit(d.x) | ((uint32_t)signbit(d.y) << 1) | ((uint32_t)signbit(d.z) << 2);
    return o & (nbins - 1u);
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_wf_generate(RenderArgs a, WfState s)
{
    int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < kSeg) {  // initial queue: every slot, in slot order, in bin 0 of its segment
        int64_t lo = p * s.seg_cap;
        int64_t c = s.P - lo;
        s.cnt[0][p * s.nbins * kCtr] = (uint32_t)(c < 0 ? 0 : (c > s.seg_cap ? s.seg_cap : c));
    }
    if (p >= s.P) return;
    int lr = (int)(p / a.W), x = (int)(p - (int64_t)lr * a.W);
    int y = tile_row_to_y(a, lr);
    uint32_t rng = pixel_seed((uint32_t)x, (uint32_t)y, (uint32_t)a.W);
    f3 o, d;
    camera_sample(a.cam, (uint32_t)x, (uint32_t)y, a.invW, a.invH, rng, o, d);
    const int64_t P = s.P;
    s.rng[p] = rng;
    s.smp[p] = 0;
    s.depth[p] = 0;
    s.col[p] = 0.0f; s.col[P + p] = 0.0f; s.col[2 * P + p] = 0.0f;
    s.ray[p] = o.x; s.ray[P + p] = o.y; s.ray[2 * P + p] = o.z;
    s.ray[3 * P + p] = d.x; s.ray[4 * P + p] = d.y; s.ray[5 * P + p] = d.z;
    const int64_t seg = p / s.seg_cap;  // sub-queue (seg, 0) starts at seg * nbins * seg_cap
    s.q[0][seg * s.nbins * s.seg_cap + (p - seg * s.seg_cap)] = (uint32_t)p;
}

// Persistent traversal with lane refill ("dynamic fetch", Aila & Laine 2009,
// re-derived for wave64 and segmented queues): every lane keeps a resumable
// traversal state in registers.  A wave holds a reservation of up to kChunk
// queue entries (uniform, in SGPRs); whenever >= REFILL lanes are idle they
// take the next entries of the reservation (ballot + mbcnt ranks).  An empty
// reservation is renewed by ONE atomic on the head of the wave's current
// segment; exhausted segments are skipped, starting from the wave's own, so
// waves work on nearby pixels and the heads see few atomics.  Lanes run
// STEPS traversal steps between refill checks, each step of the kind (node or
// leaf) more lanes are waiting for.
template <bool ANY, bool COUNT, int BLOCK, int SL, bool TOPC, int MINW, int STEPS = 4, int REFILL = 8>
__global__ void __launch_bounds__(BLOCK, MINW) k_wf_trace(SceneView sv, WfState s, int parity,
                                                          uint32_t* __restrict__ ovf)
{
    __shared__ uint32_t s_stack[SL * BLOCK];
    const int64_t gtid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, SL> st{&s_stack[threadIdx.x], ovf + gtid * (kStackTotal - SL)};
    if (TOPC) {  // the top BVH4 levels in LDS (as k_path)
        __shared__ uint4 s_top[TOPC ? kTopNodes * 4 : 1];
        const uint32_t ntop = (uint32_t)min(kTopNodes, sv.n_nodes4);
        const uint4* g = reinterpret_cast<const uint4*>(sv.nodes4);
        for (uint32_t i = threadIdx.x; i < ntop * 4; i += BLOCK) s_top[i] = g[i];
        __syncthreads();
        st.top = (const lds_u4*)s_top;
        st.ntop = ntop;
    }
    TravCount cnt;
    uint32_t traced = 0;
    const uint32_t* q = ANY ? s.qs : s.q[parity];
    const uint32_t* counts = ANY ? s.cnt_s : s.cnt[parity];
    uint32_t* heads = ANY ? s.head_s : s.head_e;
    const int64_t P = s.P;
    const f3 ldir = light_dir();
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    const uint32_t wave_gid = (uint32_t)(gtid >> 6);
    const uint32_t nq = ANY ? (uint32_t)kSeg : (uint32_t)kSeg * s.nbins;  // sub-queues
    uint32_t seg = wave_gid % nq;  // current sub-queue; starts spread over the frame
    bool drained = false;
    uint32_t walked = 0;
    uint32_t res = 0, res_end = 0;          // reservation [res, res_end) of queue positions
    bool active = false;
    uint32_t p = 0;
    uint32_t steps = 0, max_steps = 0;  // COUNT builds: longest query of this lane
    TravRay r;
    TravState ts;
    for (;;) {
        uint64_t idle = wballot(!active);
        uint32_t nidle = (uint32_t)__popcll(idle);
        if (nidle >= (uint32_t)REFILL && (res < res_end || !drained)) {
            while (res >= res_end && !drained) {  // renew the reservation (wave-uniform)
                const uint32_t c = counts[seg * kCtr];
                uint32_t b = c;
                // at low load (walk_check) a wave walking past its own
                // sub-queue takes a relaxed look at the head first, so an
                // exhausted sub-queue costs no atomic (every wave walks all of
                // them at the end of an iteration: 1/8 shard 310 -> 193 ms);
                // at full load that extra round trip per renewal costs more
                // than it saves (N = 1: 550 -> 773 ms), so the atomic alone
                if (c != 0 && (walked == 0 || !s.walk_check ||
                               __hip_atomic_load(&heads[seg * kCtr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c)) {
                    if (lane_id() == 0) b = atomicAdd(&heads[seg * kCtr], kChunk);
                    b = (uint32_t)__shfl((int)b, 0);
                }
                if (b < c) {
                    res = seg * s.seg_cap + b;
                    res_end = seg * s.seg_cap + min(b + kChunk, c);
                    walked = 0;
                } else {  // sequential walk: try the next sub-queue, give up after all of them
                    seg = seg + 1 == nq ? 0u : seg + 1;
                    if (++walked == nq) drained = true;
                }
            }
            uint32_t take = min(nidle, res_end - res);
            uint32_t k = (uint32_t)__popcll(idle & lt);
            if (!active && k < take) {
                uint32_t e = q[res + k];
                if (!(e & kSkip)) {  // flagged entries: stopped at kMaxDepth, nothing to trace
                    p = e;
                    f3 o, d;
                    if (ANY) {
                        o = mk(s.sho[p], s.sho[P + p], s.sho[2 * P + p]);
                        d = ldir;
                    } else {
                        o = mk(s.ray[p], s.ray[P + p], s.ray[2 * P + p]);
                        d = mk(s.ray[3 * P + p], s.ray[4 * P + p], s.ray[5 * P + p]);
                    }
                    r = make_trav_ray(o, d);
                    trav_init(ts, kMaxT);
                    ++traced;
                    steps = 0;
                    const bool root_miss = !ANY && s.root_check && s.depth[p] == 0 &&
                                           !octree_root_hit(sv, o, d, kMinT, kMaxT);
                    if (root_miss) atomicAdd(&sv.oct->ties[1], 1ull);
                    if (sv.n > 0 && !ray_has_nan(o, d) && !root_miss) {
                        active = true;
                    } else if (!ANY) {  // provably no hit (NaN ray, empty scene, root box): a counted miss
                        s.hid[p] = -1;
                    }
                }
            }
            res += take;
        }
        if (!wany(active)) {
            if (res >= res_end && drained) break;
            continue;
        }
        if (active) {
            bool done = false;
            for (int k = 0; k < STEPS; ++k) {
                // one step kind per round: inner nodes or leaves, whichever more
                // lanes are waiting for, so each load issues with more lanes
                const uint64_t at_leaf = wballot(!done && ts.node < 0);
                const uint64_t at_node = wballot(!done && ts.node >= 0);
                if (at_leaf == 0 && at_node == 0) break;
                const bool leaf_round = __popcll(at_leaf) > __popcll(at_node);
                // the kind is wave-uniform: a scalar branch to the step that has
                // only that kind's code (as in k_path's voted rounds)
                if (leaf_round) {
                    if (!done && ts.node < 0) {
                        done = trav_step4q2_mixed<COUNT, BLOCK, SL, TOPC, 2>(sv, r, ANY, ts, st, cnt);
                        if (COUNT) ++steps;
                    }
                } else if (!done && ts.node >= 0) {
                    done = trav_step4q2_mixed<COUNT, BLOCK, SL, TOPC, 1>(sv, r, ANY, ts, st, cnt);
                    if (COUNT) ++steps;
                }
            }
            if (done) {
                active = false;
                if (COUNT) max_steps = max(max_steps, steps);
                if (ANY) {
                    if (octree_flag(sv, r, ts)) settle_any(sv, r, kMinT, kMaxT, ts);  // a flat triangle, a crack
                    if (ts.best >= 0) s.light[(int64_t)(s.depth[p] - 1) * P + p] = 0.0f;
                } else {
                    settle_closest<BLOCK, SL, TOPC, false, false>(sv, r, 0.0f, kMinT, kMaxT, ts, st);
                    s.hid[p] = ts.best;
                    s.hit[P + p] = ts.bu;
                    s.hit[2 * P + p] = ts.bv;
                }
            }
        }
    }
    uint32_t rr = wave_sum(traced);
    uint32_t nv = COUNT ? wave_sum(cnt.nodes) : 0u;
    uint32_t nt = COUNT ? wave_sum(cnt.tris) : 0u;
    if (lane_id() == 0) {
        atomicAdd(&s.tot[ANY ? 1 : 0], (unsigned long long)rr);
        if (COUNT) {
            atomicAdd(&s.tot[ANY ? 4 : 2], (unsigned long long)nv);
            atomicAdd(&s.tot[ANY ? 5 : 3], (unsigned long long)nt);
        }
    }
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) max_steps = max(max_steps, (uint32_t)__shfl_xor((int)max_steps, off));
        if (lane_id() == 0) atomicMax(&s.tot[ANY ? 7 : 6], (unsigned long long)max_steps);
    }
}

// shade: one lane per path slot, in slot order, so every state access is
// coalesced.  Every unfinished path was extended this iteration (or stopped at
// kMaxDepth), so each needs exactly one shading step.  Appends (wave-compacted)
// to the block's segment of the other parity's extend queue and of the shadow
// queue; writes finished pixels.
template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_wf_shade(SceneView sv, RenderArgs a, WfState s,
                                                    int parity, uint32_t* __restrict__ out)
{
    const int64_t P = s.P;
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t p = (uint32_t)p64;
    const uint32_t seg = (uint32_t)(((int64_t)blockIdx.x * BLOCK) / s.seg_cap);
    uint32_t depth = p64 < P ? s.depth[p] : kDone;
    bool cont = false, shadow = false;
    uint32_t bin = 0;  // octant bin of the next extend ray
    if (depth != kDone) {
        uint32_t rng = s.rng[p];
        f3 d = mk(s.ray[3 * P + p], s.ray[4 * P + p], s.ray[5 * P + p]);
        int id = depth < (uint32_t)kMaxDepth ? s.hid[p] : -1;
        bool finish = true;
        f3 color = mk(0.0f, 0.0f, 0.0f);
        if (depth < (uint32_t)kMaxDepth) {
            if (id >= 0) {  // Scatter, main.cpp:44-73
                f3 pos, nrm;
                hit_record(sv, id, s.hit[P + p], s.hit[2 * P + p], pos, nrm);
                s.light[(int64_t)depth * P + p] = light_cosine(nrm, d);  // zeroed by shadow if occluded
                s.sho[p] = pos.x; s.sho[P + p] = pos.y; s.sho[2 * P + p] = pos.z;
                f3 rnd = random_unit_vector(rng);
                f3 target = pos + nrm + rnd;
                d = normalize(target - pos);
                s.ray[p] = pos.x; s.ray[P + p] = pos.y; s.ray[2 * P + p] = pos.z;
                s.ray[3 * P + p] = d.x; s.ray[4 * P + p] = d.y; s.ray[5 * P + p] = d.z;
                ++depth;
                shadow = true;
                cont = true;  // depth == kMaxDepth: finished next iteration, after its shadow
                finish = false;
            } else {
                color = sky(d);  // main.cpp:106-107
            }
        }
        if (finish) {
            for (int k = (int)depth - 1; k >= 0; --k)
                color = backward_step(color, s.light[(int64_t)k * P + p]);
            f3 col = mk(s.col[p], s.col[P + p], s.col[2 * P + p]) + color;
            uint32_t smp = s.smp[p] + 1;
            s.smp[p] = smp;
            depth = 0;
            if (smp < (uint32_t)a.spp) {
                s.col[p] = col.x; s.col[P + p] = col.y; s.col[2 * P + p] = col.z;
                int lr = (int)(p / (uint32_t)a.W), x = (int)(p - (uint32_t)lr * (uint32_t)a.W);
                int y = tile_row_to_y(a, lr);
                f3 o;
                if (a.jt) rng = sample_seed(a.jt, smp, pixel_seed((uint32_t)x, (uint32_t)y, (uint32_t)a.W));
                camera_sample(a.cam, (uint32_t)x, (uint32_t)y, a.invW, a.invH, rng, o, d);
                s.ray[p] = o.x; s.ray[P + p] = o.y; s.ray[2 * P + p] = o.z;
                s.ray[3 * P + p] = d.x; s.ray[4 * P + p] = d.y; s.ray[5 * P + p] = d.z;
                cont = true;
            } else {
                out[p] = pack_pixel(col, a.spp_recip);
                depth = kDone;
            }
        }
        s.depth[p] = depth;
        s.rng[p] = rng;
        if (cont && depth != (uint32_t)kMaxDepth) bin = dir_bin(d, s.nbins);
    }
    // the next extend ray into its (segment, octant) sub-queue: one ballot
    // and at most one atomic per wave and bin
    for (uint32_t b = 0; b < s.nbins; ++b) {
        const bool mine = cont && bin == b;
        const uint32_t sq = seg * s.nbins + b;
        const uint32_t qi = wave_append(&s.cnt[parity ^ 1][sq * kCtr], mine);
        if (mine) s.q[parity ^ 1][sq * s.seg_cap + qi] = depth == (uint32_t)kMaxDepth ? (p | kSkip) : p;
    }
    uint32_t si = wave_append(&s.cnt_s[seg * kCtr], shadow);
    if (shadow) s.qs[seg * s.seg_cap + si] = p;
}

// after the extend of `parity` was consumed: zero its counts and the heads;
// publish the size of the next queue for the host's termination check
__global__ void __launch_bounds__(kSeg) k_wf_advance(WfState s, int parity, int it)
{
    int j = threadIdx.x;
    uint32_t next = 0, cur = 0;
    for (uint32_t k = (uint32_t)j; k < (uint32_t)kSeg * s.nbins; k += kSeg) {  // extend sub-queues
        next += s.cnt[parity ^ 1][k * kCtr];
        cur += s.cnt[parity][k * kCtr];
        s.cnt[parity][k * kCtr] = 0;
        s.head_e[k * kCtr] = 0;
    }
    if (s.iter_log) {  // debug: rays of this iteration's extend (consumed queue) and shadow
        uint32_t e = wave_sum(cur);
        uint32_t sh = wave_sum(s.cnt_s[j * kCtr]);
        if (j == 0) {
            s.iter_log[2 * it] = e;
            s.iter_log[2 * it + 1] = sh;
        }
    }
    s.cnt_s[j * kCtr] = 0;
    s.head_s[j * kCtr] = 0;
    next = wave_sum(next);
    if (j == 0) s.total[0] = next;
}

// Wavefront driver.  The host enqueues iterations without reading the queue
// sizes (the kernels read them from device memory) and checks for completion
// every kCheck iterations.
int render_wavefront(Scene& s, const RenderArgs& a, uint32_t* d_out, bool count)
{
    const int64_t P = a.slots;
    if (P >= (int64_t)kSkip) {
        set_error("wavefront: tile too large");
        return -22;
    }
    // top BVH levels from LDS in both passes, no occupancy floor: measured best
    // against no LDS copy and 5-8 waves per SIMD (profiles/r03_wavefront_ab/)
    constexpr bool kTopE = true, kTopS = true;
    constexpr int kWE = 1, kWS = 1;
    auto trace_e = count ? k_wf_trace<false, true, kBlk, kSL, kTopE, kWE> : k_wf_trace<false, false, kBlk, kSL, kTopE, kWE>;
    auto trace_s = count ? k_wf_trace<true, true, kBlk, kSL, kTopS, kWS> : k_wf_trace<true, false, kBlk, kSL, kTopS, kWS>;
    const int sl = kSL;
    int grid_t = occupancy_grid((const void*)trace_e, kBlk, 0, s.device);
    const int grid_sh = (int)((P + kBlk - 1) / kBlk);
    const size_t seg_cap = (size_t)(((P + kSeg - 1) / kSeg + kBlk - 1) / kBlk) * kBlk;
    const uint32_t nbins = (uint32_t)s.opt.wf_bins;  // extend sub-queues per segment (octant bins)
    const size_t qcap = seg_cap * kSeg * nbins, qcap_s = seg_cap * kSeg;
    const size_t Pz = (size_t)P;
    size_t ovf_words = (size_t)grid_t * kBlk * (kStackTotal - sl);
    // layout of the workspace
    size_t words = 0;
    auto take = [&](size_t w) { size_t o = words; words += (w + 63) & ~size_t(63); return o; };
    const size_t ctr_words = (size_t)kSeg * kCtr, ectr_words = ctr_words * nbins;
    size_t o_rng = take(Pz), o_smp = take(Pz), o_depth = take(Pz), o_col = take(3 * Pz),
           o_light = take(kMaxDepth * Pz), o_ray = take(6 * Pz), o_hit = take(3 * Pz),
           o_hid = take(Pz), o_sho = take(3 * Pz), o_q0 = take(qcap), o_q1 = take(qcap),
           o_qs = take(qcap_s), o_ctl = take(3 * ectr_words + 2 * ctr_words + 64), o_tot = take(16),
           o_ovf = take(ovf_words);
#ifdef TMPT_DIAG
    const bool log_iters = getenv("TMPT_ITER_LOG") != nullptr;  // diagnostic build: queue sizes per iteration
#else
    const bool log_iters = false;
#endif
    const int64_t max_log = (int64_t)a.spp * (kMaxDepth + 2) + 64 + 16;
    size_t o_log = log_iters ? take(2 * (size_t)max_log) : 0;
    if (ensure_ws(s, words * 4)) return -1;
    uint32_t* w = s.ws.as<uint32_t>();
    WfState st;
    st.rng = w + o_rng;
    st.smp = w + o_smp;
    st.depth = w + o_depth;
    st.col = (float*)(w + o_col);
    st.light = (float*)(w + o_light);
    st.ray = (float*)(w + o_ray);
    st.hit = (float*)(w + o_hit);
    st.hid = (int32_t*)(w + o_hid);
    st.sho = (float*)(w + o_sho);
    st.q[0] = w + o_q0;
    st.q[1] = w + o_q1;
    st.qs = w + o_qs;
    st.cnt[0] = w + o_ctl;
    st.cnt[1] = st.cnt[0] + ectr_words;
    st.head_e = st.cnt[1] + ectr_words;
    st.cnt_s = st.head_e + ectr_words;
    st.head_s = st.cnt_s + ctr_words;
    st.total = st.head_s + ctr_words;
    st.tot = (unsigned long long*)(w + o_tot);
    st.iter_log = log_iters ? w + o_log : nullptr;
    st.P = P;
    st.seg_cap = (uint32_t)seg_cap;
    st.nbins = nbins;
    // low load: under two queue entries per resident traversal lane; binned
    // queues always (most of their sub-queues are empty)
    st.walk_check = nbins > 1 || P < 2 * (int64_t)grid_t * kBlk;
    st.root_check = a.root_check;
    uint32_t* ovf = w + o_ovf;
    hipStream_t str = s.stream;

    TMPT_HIP(hipMemsetAsync(w + o_ctl, 0, (3 * ectr_words + 2 * ctr_words + 64) * 4, str));
    TMPT_HIP(hipMemsetAsync(st.tot, 0, 8 * sizeof(unsigned long long), str));
    if (st.iter_log) TMPT_HIP(hipMemsetAsync(st.iter_log, 0, 8 * (size_t)max_log, str));
    k_wf_generate<kBlk><<<(int)((std::max<int64_t>(P, kSeg) + kBlk - 1) / kBlk), kBlk, 0, str>>>(a, st);

    // per-launch timing of the traversal kernels
    std::vector<Event> ev;
    auto new_ev = [&]() {
        ev.emplace_back();
        (void)ev.back().ensure();
        return ev.back().get();
    };
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ext_ev, sh_ev;
    PinnedBuffer<uint32_t> h_cnt;
    TMPT_HIP(h_cnt.ensure(16));
    const int kCheck = 8;
    int parity = 0;
    int64_t it = 0;
    int rc = 0;
    for (;;) {
        for (int k = 0; k < kCheck; ++k, ++it) {
            hipEvent_t e0 = new_ev(), e1 = new_ev(), e2 = new_ev(), e3 = new_ev();
            (void)hipEventRecord(e0, str);
            trace_e<<<grid_t, kBlk, 0, str>>>(view(s), st, parity, ovf);
            (void)hipEventRecord(e1, str);
            k_wf_shade<kBlk><<<grid_sh, kBlk, 0, str>>>(view(s), a, st, parity, d_out);
            (void)hipEventRecord(e2, str);
            trace_s<<<grid_t, kBlk, 0, str>>>(view(s), st, parity, ovf);
            (void)hipEventRecord(e3, str);
            k_wf_advance<<<1, kSeg, 0, str>>>(st, parity, (int)std::min<int64_t>(it, max_log - 1));
            ext_ev.push_back({e0, e1});
            sh_ev.push_back({e2, e3});
            parity ^= 1;
        }
        if (hipGetLastError() != hipSuccess) { rc = -1; break; }
        if (hipMemcpyAsync(h_cnt, st.total, 4, hipMemcpyDeviceToHost, str) != hipSuccess ||
            hipStreamSynchronize(str) != hipSuccess) { rc = -1; break; }
        if (h_cnt[0] == 0) break;
        if (it > (int64_t)a.spp * (kMaxDepth + 2) + 64) {  // each pixel needs <= spp*(kMaxDepth+1) iterations
            set_error("wavefront: iteration bound exceeded");
            rc = -3;
            break;
        }
    }
    unsigned long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rc == 0) {
        TMPT_HIP(hipMemcpyAsync(tot, st.tot, sizeof(tot), hipMemcpyDeviceToHost, str));
        TMPT_HIP(hipStreamSynchronize(str));
        if (log_iters) {
            std::vector<uint32_t> lg(2 * (size_t)std::min<int64_t>(it, max_log));
            TMPT_HIP(hipMemcpy(lg.data(), st.iter_log, lg.size() * 4, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < lg.size() / 2; ++k)
                fprintf(stderr, "tmpt-iter %zu extend %u shadow %u\n", k, lg[2 * k], lg[2 * k + 1]);
            if (count) fprintf(stderr, "tmpt-max-steps extend %llu shadow %llu\n", tot[6], tot[7]);
        }
    }
    double ems = 0, sms = 0;
    for (auto& pr : ext_ev) { float ms = 0; (void)hipEventElapsedTime(&ms, pr.first, pr.second); ems += ms; }
    for (auto& pr : sh_ev) { float ms = 0; (void)hipEventElapsedTime(&ms, pr.first, pr.second); sms += ms; }
    if (rc) {
        if (rc == -1) set_error("wavefront: HIP error");
        return rc;
    }
    s.extend_ms = ems;
    s.shadow_ms = sms;
    s.extend_rays = tot[0];
    s.shadow_rays = tot[1];
    s.node_visits = tot[2];
    s.tri_tests = tot[3];
    s.shadow_node_visits = tot[4];
    s.shadow_tri_tests = tot[5];
    s.extend_launches = it;
    s.shadow_launches = it;
    s.iterations = it;
    return 0;
}

}  // namespace tmpt
