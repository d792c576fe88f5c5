// tmpt_path.h -- the contract between k_path (tmpt_render.hip) and its three
// launchers (render_persistent there; render_rowstream and render_rowspec in
// tmpt_rows.hip): the kernel's control block and what it carries for the row
// engines, the variants the library instantiates and their lookup, the
// cadences, and the host functions beside k_path that the row engines call.
#pragma once

#include "tmpt_render.h"

namespace tmpt {

// Streaming row engine (SAMP 4, render_rowstream): the speculative row chains
// of render_rowspec without iterations.  One persistent launch: chaser waves
// (the first blocks, one lane per row) walk each row's chain as soon as the
// unit it needs is done and plan pixel windows ahead of it; worker waves take
// units from the rows' windows and trace them shadow-free.  A unit (row,
// pixel p, offset j) starts at M^(2j) row_seed, like render_rowspec's.
//   slots[row][kRssT + 1]: pixel windows, word = (p+1) << 48 | q << 24 | hi
//     (offsets [q, hi) of pixel p not handed out yet; slot p % kRssT; the last
//     slot is the chain's demand window for the current pixel); workers take
//     offsets by CAS, the chaser plans and extends by CAS
//   res[row][p % kRssT][j % R]: a finished unit, word = ((p+1) << 24 | j) << 28
//     | draws | rays << 14 | closest-hit rays << 19, written by atomicMax, so a
//     late unit of a pixel kRssT back never overwrites a live one
//   chainpos[row] = x << 32 | c: the chain's pixel and next sample's offset
//   list[(row * W + x) * spp + k] = offset of sample k of pixel x on the chain
//   ctl: [0] rows done, [1] abort, [2] chain progress ticks, [3] error, [4] P,
//        [5..11] statistics, [12] block arrival tickets (the first nchase are chasers)
#ifndef TMPT_RSS_T
#define TMPT_RSS_T 8
#endif
constexpr int kRssT = TMPT_RSS_T;  // live pixel windows per row at most kRssT - 1 (plus the demand slot)
static_assert(kRssT >= 4 && kRssT <= 31, "the worker's pick key holds the slot in 5 bits");
constexpr uint32_t kRssM24 = 0xFFFFFFu;
struct RsStream {
    unsigned long long* __restrict__ slots;
    unsigned long long* __restrict__ res;
    unsigned long long* __restrict__ chainpos;
    uint32_t* __restrict__ list;
    uint32_t* __restrict__ rowrays;    // [row][2]: chain rays, closest-hit
    uint32_t* __restrict__ lo;         // [row][kRssT]: chaser-private window starts
    uint32_t* __restrict__ ctl;
    const uint32_t* __restrict__ anchors;  // [row][na]: M^(2^15 a) row_seed
    const uint32_t* __restrict__ t1;       // M^(2c), c < 128 (byte tables)
    const uint32_t* __restrict__ t2;       // M^(256 b), b < 128
    uint32_t na, R, rmask;
    uint32_t jlimit;        // na * 2^14: offsets with an anchor
    int nrows, nchase, nw;  // rows, chaser blocks, live pixel windows per row
    float spread;
    // live windows and spread follow the live rows (the load law of the
    // launch-time rule, applied as rows finish): room = room_lanes / live rows;
    // dyn bit 0: windows, bit 1: spread (an option fixes either)
    float room_lanes;
    uint32_t dyn;
    uint32_t watchdog;      // 100-MHz ticks without chain progress before the workers abort
    int test_abort;         // option rowstream_test_abort: chasers leave at once (the abort path's test)
};

// M^(2j) row_seed of row `row` (j < na * 2^14)
__device__ __forceinline__ uint32_t rss_state(const RsStream& S, int row, uint32_t j)
{
    uint32_t s = S.anchors[(size_t)row * S.na + (j >> 14)];
    s = sample_seed(S.t2, (j >> 7) & 127u, s);
    return sample_seed(S.t1, j & 127u, s);
}

// One camera sample of sample seeding, as k_cam_rays leaves it for the CAM
// kernels (32 B, two 16-byte halves): the ray of main.cpp:212-216 and the RNG
// state after the camera's draws -- a function of (pixel, sample) alone, so
// the whole pass's are made before k_path starts, on full waves.  flags:
// kCamNan the ray holds a NaN (ray_has_nan: a counted miss; k_path's query
// set-up tests every starting ray itself, scattered ones among them, so it
// does not read this bit); kCamRootMiss, set only under
// RenderArgs::root_check, the ray misses the reference's root box
// (octree_root_hit), which k_path CAM reads instead of making the test.
// include/tmpt.h states the words (tmpt_camera_rays).
struct alignas(16) CamRay {
    float ox, oy, oz, dx;
    float dy, dz;
    uint32_t rng, flags;
};
static_assert(sizeof(CamRay) == 32, "camera entry: two dwordx4 accesses");
constexpr uint32_t kCamNan = 1u, kCamRootMiss = 2u;

struct PathCtl {
    uint32_t* heads;  // kSeg chunk counters, stride kCtr
    uint32_t nchunks;
    // SIMD-balanced first chunks (ordered pass, cost-descending chunks): the
    // wave of rank r on the d-th SIMD to register takes chunk r*nsimd + d (r
    // even) or r*nsimd + nsimd-1-d (r odd), so every SIMD's resident waves sum
    // to about the same work.  Every chunk has a claim word: the first chunk
    // and the segment supply both claim, so a chunk the placement left
    // unassigned (uneven waves per SIMD) is still taken, and none twice.
    // simd_reg = 2 words per hardware SIMD key (waves seen, dense index + 1)
    // plus a dense counter at kSimdKeys*2.  null = off.
    uint32_t* simd_reg;
    uint32_t* claim;  // nchunks words, zeroed per launch
    uint32_t nsimd, wps;
    int64_t P;
    // rank -> pixel, or null (pixel seeding's cost order).  Sample seeding, a
    // pass over a list of pixels (k_path LIST; tmpt_render_adaptive's later
    // passes): the units are (list position, block) -- P counts them by the
    // list's length -- and the quotient of the unit decode indexes this list of
    // tile pixel slots; everything after the decode works on the pixel.  No
    // other sample kernel reads it.
    const uint32_t* __restrict__ order;
    uint32_t* __restrict__ cost_out;     // per-pixel traversal steps of this call, or null
    // dynamic issue priority (longest remaining first): each shading round the
    // wave estimates its lanes' remaining traversal steps (steps so far per
    // finished sample x samples left) and sets s_setprio 3/2/1/0 at the
    // thresholds dprio[0] > dprio[1] > dprio[2] (steps); dprio[0] = 0: off.
    // With dprio_cost (the pilot pass's per-pixel steps), the thresholds are
    // fractions of the heaviest pixel's (order[0]) projected remaining steps.
    float dprio[3];
    const uint32_t* __restrict__ dprio_cost;
    uint32_t lane_cap;  // pixels a wave holds at once (64: all lanes)
    uint32_t chunk;     // ranks per chunk (kChunk, or lane_cap when capped)
    // Sample seeding: the supply hands out units = (pixel, block of blk
    // samples), nblk blocks per pixel, unit u = pixel * nblk + block (P counts
    // units).  With nblk > 1 each sample's colour goes to sbuf[s * slots + pixel]
    // and k_resolve sums them in sample order (main.cpp:218's col += Trace).
    uint32_t nblk, blk;
    FastDiv div_nblk, div_blk;  // their dividers (the unit decode)
    uint32_t blk0;  // progressive pass: the block of its first sample (units = the pass's blocks)
    // the frame's tail (option sample_tail): units >= ua are single samples,
    // unit ua + v = sample v % blk of block ua + v / blk, so the last units
    // handed out are one sample long, not one block
    uint32_t ua;
    float4* __restrict__ sbuf;
    uint32_t sb_ss, sb_sp;  // sbuf index = sample * sb_ss + pixel * sb_sp ([pixel][sample]: 1, spp)
    uint32_t pair;          // sample pairs (2k, 2k+1) of a unit written back to back (one 32-B sector)
    // Speculative row seeding (SAMP 2, render_rowspec): unit u traces ONE
    // sample of tile pixel upix[u] from RNG state ustate[u] and writes its
    // colour with w = draws | rays << 27 to rs_out[u], and its final RNG state
    // to rs_end[u]
    const uint32_t* __restrict__ upix;
    const uint32_t* __restrict__ ustate;
    float4* __restrict__ rs_out;
    uint32_t* __restrict__ rs_end;
    const uint32_t* __restrict__ p_dev;  // the unit count (replaces P, nchunks at launch)
    // no-shadow speculation (option rowspec_noshadow): the speculative pass skips
    // shadow traversals (they never change a sample's draws); the chain's
    // samples are traced again in full at the end of the frame, unit u as
    // sample uslot[u] of its pixel, colour into sbuf (resolved in order)
    int rs_noshadow;
    const uint32_t* __restrict__ uslot;
    RsStream rss;  // SAMP 4
    // Deferred ties (SAMP 1, k_path DEFER): the main loop carries no octree
    // walk; a sample whose closest-hit query ends on a flagged tie is dropped
    // and (pixel, sample) appended to redo (counters[kRedoCounter] counts them,
    // redo_cap entries are kept, kRedoEmpty until written).  Waves past the
    // main loop trace the listed samples again, ties settled (redo_sample);
    // k_redo takes any they leave.
    uint2* __restrict__ redo;
    float4* __restrict__ redo_state;  // kRedoState4 float4 per slot: where the dropped path stopped
    uint32_t redo_cap;
    uint32_t redo_inline;  // 0 (test hook, option redo_inline): no redo phase, k_redo takes every entry
    uint32_t redo_lanes;   // lanes per wave that take redo tickets (1..64)
    // With the octree: shadow answers can need it too (a flat triangle in the
    // scene, or the light direction can run along a crack; render_persistent
    // decides) -- the finished shadow queries are checked as closest hits are
    // (octree_flag), so HELP and DEFER are off then.
    uint32_t oct_shadow;
    // Top-walk rounds (option top_walk): at the end of a shading round, up to
    // this many wave-uniform node rounds for the lanes standing on a node of
    // the block's LDS copy of the top levels -- every query starts at node 0
    // -- with no global load in them (trav_step4q2_mixed TOPONLY).  0 = off.
    uint32_t top_walk;
    // The camera pre-pass (k_cam_rays; k_path CAM): the pass's camera samples,
    // one CamRay per (tile pixel slot, sample of the pass) at slot * cam_count +
    // (sample - smp_begin), as sbuf is laid out, so a unit's samples are
    // contiguous.  Read by the CAM kernels only.
    const CamRay* __restrict__ cam_rays;
    uint32_t cam_count;  // samples of the pass, smp_end - smp_begin
    // The shadow split (option shadow_split; k_path SPLIT, k_shadow,
    // k_split_resolve): a bounce whose light cosine is > 0 appends its shadow
    // query {hit point, record << 4 | bounce} to sq instead of tracing it, and
    // a finished sample leaves its record (SplitRec) in srec instead of a
    // colour.  Record r = pixel slot * cam_count + (sample - smp_begin), as
    // the pre-pass's entries.  A wave reserves kSplitChunk entries of sq per
    // atomic on sq_ctl[0] and fills what it leaves unused with kSplitEmpty, so
    // every entry below the counter is a query or empty.  sq_cap holds the
    // worst case; an entry past it would not be written and counted in
    // counters[kSplitOverflowCounter], the render call's error.
    uint4* __restrict__ sq;
    uint32_t* __restrict__ sq_ctl;
    uint32_t sq_cap;
    float4* __restrict__ srec;
};

// The shadow split's sample record, four 16-byte quarters: the path's end
// colour (sky() of the last ray, or 0 after kMaxDepth hits) and its depth, then
// the light cosines of its bounces -- the terms of the backward recurrence
// (backward_step), which k_split_resolve runs once k_shadow has zeroed the
// cosines of the occluded bounces.  A quarter past the depth is not written.
struct alignas(16) SplitRec {
    float end[3];
    uint32_t depth;
    float cosine[12];  // [0, depth); kMaxDepth <= 10
};
static_assert(sizeof(SplitRec) == 64 && kMaxDepth <= 12, "sample record: four dwordx4 quarters");
constexpr uint32_t kSplitChunk = 1024u;        // queue entries a k_path wave reserves per atomic
constexpr uint32_t kSplitEmpty = 0xFFFFFFFFu;  // .w of an entry no query was written to
constexpr int64_t kSplitMaxRecs = 1ll << 28;   // records a queue entry's word can name (4 bits: the bounce)

// ---- k_path's variants
// What varies between k_path's instantiations, by its template parameters'
// names (BLOCK is kBlk in all of them; TAIL follows samp, path_tail below).
// The table after k_path (kPathVariants) lists the ones the library instantiates.
struct PathVariant {
    bool count;                     // COUNT: the visit counters
    int sl, steps, shade_min, occ;  // LDS stack entries per lane, rounds per shading check, lanes that trigger one, blocks per CU
    int prof;                       // PROF (TMPT_DIAG builds): the wave-time split
    int help;                       // HELP: idle lanes trace other lanes' shadow queries
    int samp;                       // SAMP: 0 pixel, 1 sample seeding; 2 / 3 / 4 the row engines' units
    bool soa;                       // the SoA planes (layout=soa)
    int ties;                       // TIES: 0 lowest index, 2 flag for the octree, 1 flag and defer
    bool sums;                      // SUMS: the float sums beside the packed pixels
    int cam;                        // CAM: 0 the camera block, 1 the pre-pass's entries (PathCtl::cam_rays)
    bool list;                      // LIST: the unit decode's pixel is an index into PathCtl::order
    int split;                      // SPLIT: shadow queries queued for k_shadow, sample records for k_split_resolve
};

// The LDS stack: 16 entries per lane; the 5-wave kernels of sample and pixel
// seeding and the rows' full re-trace (OCC 5): 30 KB of LDS per block -- a
// 12-entry LDS stack, the scattered ray's direction only, kTopNodes5 top nodes
constexpr int kPathSL = 16, kPathSL5 = 12;
// the 6-wave twins of the shadow split (OCC 6): the same 12 entries, kTopNodes6 top nodes
constexpr int kPathSL6 = 12;
// path_waves = 0 (auto) in sample seeding where the shadow split runs with the
// deferring twin (TIES 1): 1 = its 6-wave form from kPathWaves6MinLoad samples
// of the pass per lane of the 5-wave grid, 0 = always the 5-wave one (A/B
// macro).  Whole renders of the bench frame, 5 / 6 waves, same box
// (profiles/README_r13.md): N=1 (405 samples per lane) 143.41 / 140.87 ms,
// 1/2 shard (202) 73.36 / 72.50, 1/4 (101) 38.78 / 38.52 -- -0.68 %, at the
// edge of three times that run's spread --, 1/8 (51) 20.37 / 20.59 and 20.48 /
// 20.55 in two runs: level or losing.  So from 150 per lane, between the 1/4
// shard's load and the 1/2 shard's.
#ifndef TMPT_PATH_WAVES6
#define TMPT_PATH_WAVES6 1
#endif
constexpr int kPathWaves6Auto = TMPT_PATH_WAVES6;
constexpr int64_t kPathWaves6MinLoad = 150;

// The cadences, each with its A/B macro (tools/ab_build.sh, tools/ab_kpath.py).
#ifndef TMPT_PATH_STEPS
#define TMPT_PATH_STEPS 16
#endif
#ifndef TMPT_PIX_STEPS
#define TMPT_PIX_STEPS 24
#endif
#ifndef TMPT_ROW_STEPS
#define TMPT_ROW_STEPS 16
#endif
#ifndef TMPT_ROW_SHADE_MIN
#define TMPT_ROW_SHADE_MIN 24
#endif
#ifndef TMPT_SHADE_MIN
#define TMPT_SHADE_MIN 16
#endif
#ifndef TMPT_SPARSE
#define TMPT_SPARSE 2
#endif
#ifndef TMPT_RS_OCC
#define TMPT_RS_OCC 5
#endif
// Sample and pixel seeding (render_persistent): traversal rounds between
// shading checks / lanes waiting that trigger a shading round (A/B on the
// bench frame at 1 and 8 shards);
// sparse-wave shading threshold divisor (k_path TAIL): 2 -- bench frame,
// pixel seeding 235.2 -> 231.9 ms at N=1, 1/8 shard unchanged (41.0 ms);
// sample seeding 220.4 -> 218.2 ms at N=1, 29.4 -> 29.0 ms at 1/8
// (TMPT_PATH_STEPS / TMPT_SHADE_MIN / TMPT_SPARSE: A/B builds, tools/ab_build.sh)
constexpr int kSampleSteps = TMPT_PATH_STEPS, kShadeMin = TMPT_SHADE_MIN, kSparse = TMPT_SPARSE;
// pixel seeding's kernels: 24 rounds between shading checks -- re-swept at
// 5 waves per SIMD (whole renders, steps 16 / 24 / 32: 1/8 shard 36.4 /
// 35.2 / 36.1 ms, 1/4 63.7 / 63.2 / 65.1, N=1 198.0 / 196.0 / 208.9; the
// sample kernels 172.3 / 172.8 / 182.9 keep 16; 20 and 28 both lose to 24,
// +1.4 % at 1/8; profiles/r06_experiments/cadence_5waves*.log,
// cadence_pixel_20_24_28.log)
constexpr int kPixSteps = TMPT_PIX_STEPS;
// The streaming row engine (render_rowstream), SAMP 2 and 4:
// a shading round once 24 lanes wait (16 before round 6): whole row renders,
// 16 / 24 / 28 / 32, N=1 1835.9 / 1811.4 / 1811.9 / 1833.8 ms, 1/2 1034.8 /
// 1023.5 / 1023.6, 1/8 432.1 / 430.4 / 427.6 / 428.3; 24 or 32 rounds per
// check instead of 16: -0.8 / +1.2 % at N=1 (profiles/r06_experiments/row_cadence*.log)
constexpr int kRowSteps = TMPT_ROW_STEPS, kRowShadeMin = TMPT_ROW_SHADE_MIN;
// the iterated row engine (render_rowspec), SAMP 2 and 3: no macro
constexpr int kRowIterSteps = 16, kRowIterShadeMin = 16;
// blocks per CU of the shadow-free row units, SAMP 3 and 4 (5 waves per SIMD)
constexpr int kRsOcc3 = TMPT_RS_OCC;
// TAIL of a variant: kSparse in sample and pixel seeding, 2 in the row engines
constexpr int path_tail(int samp) { return samp <= 1 ? kSparse : 2; }

using PathFn = void (*)(SceneView, RenderArgs, PathCtl, uint32_t*, uint32_t*, unsigned long long*);

// The kernel of a variant, or null when the table does not hold it.
PathFn path_kernel(const PathVariant& v);
// The same for a render call: 0 and the kernel, or -22 with the variant's
// fields in the error (set_error) -- never a neighbouring kernel.
int find_path_kernel(const PathVariant& v, const char* who, PathFn& fn);

// The heaviest pixels of a pixel-seeded frame as speculative chains
// (render_rowspec's engine with a chain = one pixel): pixel cpix[r], its
// samples smp0 .. smp0 + cspp - 1, from the state the pilot pass left in
// cinit[pixel] (colour sum of samples 0 .. smp0-1, RNG state in .w).
struct PixelChains {
    const uint32_t* cpix;
    const float4* cinit;
    int n, smp0, cspp;
};

// PathCtl::top_walk and PathCtl::oct_shadow of a launch (beside render_persistent)
uint32_t top_walk_cap(const Options& o, int seeding);
uint32_t oct_shadow_check(const Scene& s);

// k_resolve_px (beside k_path) over a whole tile's colour buffer, for the row engines
void launch_resolve_px(hipStream_t stream, const float4* sbuf, int64_t P, int32_t spp, float spp_recip,
                       uint32_t* out);

// tmpt_shadow.hip: the shadow split's two kernels after k_path SPLIT.
// k_shadow answers the queued shadow queries (entries [0, min(*count, cap)) of
// sq) and stores 0 into the record's cosine of an occluded bounce; `head` is
// its fetch counter (zeroed by the caller), n_rec the records of srec, ovf the
// lanes' stack spill areas (shadow_ovf_words() words).  k_split_resolve then runs each sample's backward
// recurrence from its record, sums a pixel's cnt samples in sample order and
// packs the pixel, as k_resolve_px does from the colour buffer: onto the sums
// in carry_in where given (a pass after the first), the new sums left in
// carry_out where given.
size_t shadow_ovf_words(int device);
int launch_shadow(hipStream_t stream, int device, const SceneView& sv, const uint4* sq, const uint32_t* count,
                  uint32_t cap, uint32_t* head, float4* srec, uint32_t n_rec, uint32_t* ovf);
void launch_split_resolve(hipStream_t stream, const float4* srec, int64_t P, int32_t cnt, float spp_recip,
                          uint32_t* out, const float4* carry_in = nullptr, float4* carry_out = nullptr);

#ifdef TMPT_EXP_WAVETIME  // timeline experiment: per wave, s_memrealtime at start / main loop end / exit
constexpr int kWaveTimeMax = 16384;
// g_wavetime (3 * kWaveTimeMax words) / g_rowtime and g_claimtime (kWaveTimeMax
// words each), defined beside k_path: copied to the host (false: a copy failed), set from it
bool wavetime_get(unsigned long long* w);
bool rowtime_get(unsigned long long* r, unsigned long long* cl);
void wavetime_put(const unsigned long long* w);
void rowtime_put(const unsigned long long* r);  // both arrays from r
#endif

}  // namespace tmpt
