// tmpt_internal.h -- device data layout and the scene object behind the C ABI.
//
// HBM layout of one scene (DESIGN.md "Data layout in HBM"):
//   nodes4   Bvh4Node[<= n-1]     64 B  4-wide BVH, quantised child boxes,
//                                        numbered level by level (the top
//                                        kTopNodes are copied to LDS); within
//                                        a level in the order of an atomic
//                                        counter, so two builds are equal only
//                                        renumbered breadth-first, not raw
//                                        (include/tmpt.h tmpt_scene_dump_bvh)
//   tri_pre  TriPre[n + 1]        48 B  leaf order: v0, e1 = v1-v0, e2 = v2-v0,
//                                        original index (the Moller-Trumbore operands)
//   tri_orig TriOrig[n]           48 B  original order: v0, v1, v2 and the geometric
//                                        normal, read once per accepted hit
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "tmpt_device.h"
#include "tmpt_math.h"

namespace tmpt {

// 4-wide node with quantised child boxes (DESIGN.md "BVH4Q"): 64 B, one
// half cache line, 4 x dwordx4 loads for FOUR child boxes.
//   a: origin.xyz (node box min, f32), w = exponents ex,ey,ez (bytes 0-2,
//      signed: scale = 2^e) | child-valid mask (byte 3)
//   b: qlo.x[4], qhi.x[4], qlo.y[4], qhi.y[4]   (uint8 per child, child k in byte k)
//   c: qlo.z[4], qhi.z[4], 0, 0
//   d: child links: >=0 node index; <0 leaf = 0x80000000 | (count-1)<<count_shift | first slot
//      (count_shift per scene: link_layout below)
// A child box decodes as origin + q*scale (q*scale exact), quantised outward
// from the padded boxes, so culling stays conservative.
struct alignas(16) Bvh4Node {
    float4 a;
    uint4 b;
    uint4 c;
    int4 d;
};
static_assert(sizeof(Bvh4Node) == 64, "BVH4Q node is one half cache line");

constexpr int kLeafMaxTris = 16;

// Child links and stack entries ("Link layout").  A link
// is 32 bits: an internal child is its node index; a leaf is
//   bit 31 | (count - 1) << count_shift | first record
// with the fields only as wide as the scene needs: count_shift = bits(n), n
// the highest record a leaf can name (the null leaf's), and a count field of
// bits(leaf_max - 1) bits.  Bits 30..link_bits of every link are therefore 0,
// and a traversal stack entry carries there the top K bits of the f32 pattern
// of its child's entry distance tn >= 0 (sign bit 0: it coincides with the leaf
// flag): 8 exponent bits and K - 8 of the mantissa, truncated, so a lower bound
// of tn.  Pop culling compares it with the best hit (tmpt_traverse.h trav_pop).
constexpr int kPopKeyMin = 9;   // fewer bits than the exponent and one more: no key, culling off
constexpr int kPopKeyMax = 16;
TMPT_HD constexpr int bits_for(uint32_t v)
{
    int b = 0;
    for (; v; v >>= 1) ++b;
    return b;
}
struct LinkLayout {
    int count_shift;  // of a leaf link's count - 1; the first-record field lies below it
    int link_bits;    // bits 0..link_bits-1 (and bit 31) are all a link uses
};
TMPT_HD constexpr LinkLayout link_layout(uint32_t n_tris, int leaf_max, uint32_t n_nodes4)
{
    const int cs = bits_for(n_tris), leaf = cs + bits_for((uint32_t)leaf_max - 1u);
    const int node = bits_for(n_nodes4 ? n_nodes4 - 1u : 0u);
    return LinkLayout{cs, leaf > node ? leaf : node};
}
// K, the key's width: what the link leaves free below bit 31, at most
// kPopKeyMax and at most `cap` (option pop_key_cap, < 0 = none); 0 below kPopKeyMin
TMPT_HD constexpr int pop_key_bits(int link_bits, int cap)
{
    int k = 31 - link_bits;
    k = k > kPopKeyMax ? kPopKeyMax : k;
    k = cap >= 0 && k > cap ? cap : k;
    return k < kPopKeyMin ? 0 : k;
}
TMPT_HD constexpr uint32_t pop_key_mask(int k) { return k ? ((1u << k) - 1u) << (31 - k) : 0u; }
TMPT_HD constexpr uint32_t leaf_link(uint32_t count, uint32_t first, int count_shift)
{
    return 0x80000000u | ((count - 1u) << count_shift) | first;
}
TMPT_HD constexpr uint32_t leaf_first(uint32_t link, int count_shift) { return link & ((1u << count_shift) - 1u); }
TMPT_HD constexpr uint32_t leaf_count(uint32_t link, int count_shift)
{
    return ((link >> count_shift) & (uint32_t)(kLeafMaxTris - 1)) + 1u;
}
// a stack entry from a clean link and the f32 bits of its key; and back
TMPT_HD constexpr uint32_t entry_pack(uint32_t link, uint32_t key_f32, uint32_t key_mask)
{
    return (key_f32 & key_mask) | link;
}
TMPT_HD constexpr uint32_t entry_key(uint32_t e, uint32_t key_mask) { return e & key_mask; }
TMPT_HD constexpr uint32_t entry_link(uint32_t e, uint32_t key_mask) { return e ^ (e & key_mask); }

namespace link_checks {
// the bench scene (stand-in sponza: 66,453 records, leaves of <= 2, 16.7 k nodes): 13 key bits
constexpr LinkLayout kBench = link_layout(66453u, 2, 16700u);
static_assert(kBench.count_shift == 17 && kBench.link_bits == 18, "bench scene: 18-bit links");
static_assert(pop_key_bits(kBench.link_bits, -1) == 13 && pop_key_mask(13) == 0x7FFC0000u, "bench scene: bits 30..18");
static_assert(pop_key_bits(kBench.link_bits, 9) == 9 && pop_key_mask(9) == 0x7FC00000u, "capped key");
static_assert(pop_key_bits(kBench.link_bits, 0) == 0 && pop_key_bits(kBench.link_bits, 8) == 0 &&
                  pop_key_mask(0) == 0u, "no key below 9 bits");
// the same scene with leaves of <= 16: four count bits, 10 key bits
static_assert(link_layout(66453u, 16, 9000u).link_bits == 21 && pop_key_bits(21, -1) == 10, "leaf_max 16");
// 2^21 triangles: the null leaf's record needs 22 bits; with leaves of <= 2 only 8 bits stay, so no key
static_assert(link_layout(1u << 21, 2, 1u << 20).link_bits == 23 && pop_key_bits(23, -1) == 0, "2^21 triangles");
static_assert(link_layout(1u << 21, 1, 1u << 21).link_bits == 22 && pop_key_bits(22, -1) == 9, "2^21, leaf_max 1");
// tiny scenes: the key is capped at 16 bits; a tree of many nodes and few records is sized by its nodes
static_assert(pop_key_bits(link_layout(12u, 2, 5u).link_bits, -1) == 16 && pop_key_mask(16) == 0x7FFF8000u, "cap 16");
static_assert(link_layout(3u, 1, 1000u).link_bits == 10, "node index decides");
// the widest layout is the old fixed one: count at bit 27, all of bits 30..0 used
static_assert(link_layout((1u << 27) - 1u, 16, 1u << 26).link_bits == 31, "2^27 - 1 triangles still fit");
// pack / unpack: the link comes back clean, the key is the f32 pattern truncated (a lower bound for tn >= 0)
constexpr uint32_t kLeaf = leaf_link(2u, 66452u, kBench.count_shift), kMask = pop_key_mask(13);
constexpr uint32_t kTn = 0x4129999Au;  // 10.6f
static_assert(leaf_first(kLeaf, kBench.count_shift) == 66452u && leaf_count(kLeaf, kBench.count_shift) == 2u,
              "leaf decode");
static_assert(entry_link(entry_pack(kLeaf, kTn, kMask), kMask) == kLeaf, "leaf link survives its key");
static_assert(entry_link(entry_pack(16699u, kTn, kMask), kMask) == 16699u, "node link survives its key");
static_assert(entry_key(entry_pack(kLeaf, kTn, kMask), kMask) == 0x41280000u, "key = tn truncated (10.5 <= 10.6)");
static_assert(entry_key(entry_pack(kLeaf, 0x7F800000u, kMask), kMask) == 0x7F800000u, "+inf stays +inf");
static_assert(entry_pack(kLeaf, kTn, 0u) == kLeaf && entry_key(kLeaf, 0u) == 0u, "no key field: plain links");
}  // namespace link_checks

// Division by a divisor the host knows (the frame's width, a unit's block
// counts: wave-uniform, fixed per launch) as a multiply and a shift, in place
// of the ~25-instruction u32 division sequence the compiler emits for a
// run-time divisor.  For d >= 1 with l = ceil(log2 d):
//   mul = ceil(2^(31 + l) / d)  (< 2^32: d > 2^(l-1)),  shift = l,
//   x / d = (x * mul) >> (31 + l) = mulhi(2x, mul) >> l     for every x < 2^31
// (Granlund & Montgomery 1994, N = 31: mul * d = 2^(31+l) + e with 0 <= e < d
// <= 2^l, so x * mul / 2^(31+l) exceeds x / d by x * e / (d * 2^(31+l)) < 1/d,
// too little to reach the next integer).  2x fits 32 bits, so the device needs
// no 64-bit product.  Every dividend here is a pixel, row or unit index, and
// the host keeps those below 2^31 (render_persistent).
struct FastDiv {
    uint32_t mul, shift;
};
inline FastDiv fastdiv_make(uint32_t d)
{
    const uint32_t l = (uint32_t)bits_for(d > 1u ? d - 1u : 0u);
    const uint64_t p = 1ull << (31u + l);
    return FastDiv{(uint32_t)((p + d - 1u) / d), l};
}
TMPT_HD uint32_t fastdiv(uint32_t x, FastDiv f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(x << 1, f.mul) >> f.shift;
#else
    return (uint32_t)(((uint64_t)(x << 1) * f.mul) >> 32) >> f.shift;
#endif
}

constexpr int kTopNodes = 120;  // BVH4 nodes held in LDS per path block (7.5 KB)
// The same in the 5-wave path kernels (OCC 5): 5 KB, so a block's LDS is 30 KB
// (12-entry stack 12 KB, light terms 10 KB, pending ray 3 KB, top nodes 5 KB).
// Five such blocks fit a CU; with 104 nodes (31.5 KB) they did not (the
// occupancy API still said 5, and the launch's tail waited for blocks that
// were never resident), 72-96 nodes measured alike.
constexpr int kTopNodes5 = 80;
// The 6-wave twins of the shadow split (OCC 6, SPLIT: no pending ray): six
// blocks per CU.  The CU hands out its 160 KB of LDS in units of kLdsGranule
// bytes -- the boundary round 6 measured fits no other unit: 31,744 B (25
// units, 5 x 25 = 125 of 128) ran five blocks, 32,256 B (26, 130) did not,
// whatever the occupancy query said -- so a sixth block needs 21 units or
// fewer, 26,880 B, not 163,840 / 6.  A 12-entry stack (12 KB), the light terms
// (10 KB) and 64 top nodes (4 KB) are 26,640 B (k_path asserts the bound).
constexpr int kLdsGranule = 1280, kLdsBytes = 163840;
constexpr int kTopNodes6 = 64;

struct alignas(16) TriPre {
    float4 a;  // v0.xyz, e1.x
    float4 b;  // e1.yz, e2.xy
    float4 c;  // e2.z, 2 x original index (int bits; bit 0 is the traversal's tie flag), 0, 0
};
struct alignas(16) TriOrig {
    float4 a;  // v0.xyz, v1.x
    float4 b;  // v1.yz, v2.xy
    float4 c;  // v2.z, normal.xyz
};

// The reference's own octree (Scene::BuildOctree, scene.cpp:75-83, 99-160),
// kept for the answers the BVH cannot give by itself: which of several
// triangles that tie on t the reference returns (its first strict '<' in
// depth-first child order 0..7, scene.cpp:29-48) and the rays its root box
// test drops.  Nodes in depth-first preorder, 32 B each:
//   lo = box min.xyz, w = skip (int bits): the node after this subtree
//   hi = box max.xyz, w = ref  (int bits): -1 for an inner node; a leaf's
//        triangles are refs[ref + 1 .. ref + refs[ref]] in the reference's order
// Built on the host (the reference's build is untimed too, main.cpp:312 vs
// :319) by tmpt_octree.cpp, or under option octree_build=device by
// tmpt_octree_dev.hip, word for word the same; read by the device only for
// flagged queries.
struct alignas(16) OctNode {
    float4 lo;
    float4 hi;
};
static_assert(sizeof(OctNode) == 32, "octree node: two dwordx4 loads");

// The octree's cracks ("cracks"): a child box is its
// parent's min plus half the parent's size, its max that plus half again, so
// the boxes of two neighbouring subtrees need not share a face bit for bit --
// one subtree can end an ulp or two before the next begins.  A ray that runs
// inside such a gap, nearly parallel to it, passes no leaf there, and the
// reference misses a triangle the exact closest hit finds; a triangle lying
// flat inside a gap is in no leaf at all.  The planes of the octree are the
// grid r0 + j * cell (cell = root size / 2^depth) to within `band`, so the
// queries that can land in a gap are known from the hit alone:
//   crack  hit point within band[k] of a plane of axis k, and the ray moved
//          less than 2 band[k] along k over min(t, reach) -- it ran along
//          the gap -- for some axis k;
//   flat   the hit triangle lies within 2 band[k] of one plane (its TriPre
//          index is odd: marked when the octree is built).
// Both are answered over the octree, as ties are.
struct OctGrid {
    // first 16 B: what every finished query reads (one scalar dwordx4 load)
    float reach;        // half the smallest cell: t beyond which a ray's drift along k is judged
    float drift[3];     // 2 x band: the drift along k that counts as running along a plane
    float r0[3];        // root box min
    float inv_cell[3];  // 2^depth / root size
    float cell[3];      // root size / 2^depth
    float band[3];      // 4 x the largest plane offset of any node box + 8 ulp of the root's coordinates
};

// What the kernels see of it (one device-side struct, so a kernel keeps one
// pointer live): nodes, leaf lists, node count, the counters of the queries
// it answered ([0] ties, [1] root-box misses, [6] crack / flat-triangle
// queries; Scene::ties), the crack grid.
struct OctView {
    const OctNode* nodes;
    const int32_t* refs;
    int32_t n;
    int32_t flat;  // triangles marked flat (0: the any-hit answers need no check)
    unsigned long long* ties;
    OctGrid grid;
    int64_t n_refs;  // entries of refs (the checked build's bound)
};

// Device bounds checks, the checked build only (make CHECK=1: -DTMPT_CHECK,
// ../_lib_check; tools/check_build.sh).  The traversal, both octree walks and
// the hit-record loads test each index before they use it -- BVH node, leaf
// range, stack depth, octree skip link and reference list, triangle id --
// and a failed test ends that query and ORs its code into Scene::chk
// ({codes, count, last offending value}); the API call then fails with
// kCheckError and names the codes (tmpt_last_error).  The product build
// compiles none of it.
constexpr uint32_t kChkNode = 1u, kChkLeaf = 2u, kChkStack = 4u, kChkOctSkip = 8u, kChkOctRef = 16u,
                   kChkTri = 32u;
constexpr int kCheckError = -30;

struct OctreeHost {
    std::vector<OctNode> nodes;
    std::vector<int32_t> refs;
    int32_t leaves = 0, depth = 0;
};

// Subdivide / InternalDivide of scene.cpp:99-160 from the root box [bmin, bmax]
// (main.cpp:312: the scene bounds +- 0.7 x their size)
void build_octree(const float* tris9, int32_t n, const float bmin[3], const float bmax[3], OctreeHost& out);
// FNV-1a over the preorder walk (node boxes' bits, leaf triangle lists): the
// structure check the CPU tests compare with the oracle's octree
uint64_t octree_digest(const OctreeHost& t);
// The crack grid of an octree (tmpt_octree.cpp) and the triangles that lie
// flat on one of its planes (flat[i] = 1).
void octree_grid(const OctreeHost& t, const float bmin[3], const float bmax[3], OctGrid& g);
int32_t octree_flat_triangles(const float* tris9, int32_t n, const OctGrid& g, std::vector<uint8_t>& flat);
// octree_grid in its two halves: the cell of axis k at `depth`, and the grid
// from the largest plane offset per axis (what octree_grid finds over t.nodes;
// the device build reduces it on the device)
double octree_cell(int32_t depth, const float bmin[3], const float bmax[3], int k);
void octree_grid_from_offsets(int32_t depth, const double wmax[3], const float bmin[3], const float bmax[3], OctGrid& g);
// The device build's passes (tmpt_octree_build.h) as host loops: the same
// arrays as build_octree (0), or -1 where a level or the result passes
// INT32_MAX; and its plane-offset reduction.  tmpt_octree_arrays method 1.
int build_octree_levels(const float* tris9, int32_t n, const float bmin[3], const float bmax[3], OctreeHost& out);
void octree_offsets_levels(const OctreeHost& t, const float bmin[3], const float bmax[3], double w[3]);

// Build option layout=soa (the north star's "SoA" A/B):
// the BVH4Q nodes and the leaf-ordered triangle records as planes, each plane
// one load of a step -- node planes a (origin, exponents), b (x / y byte
// planes), c (z byte planes, 8 B: no padding), d (child links); triangle
// planes a (v0, e1.x), b (e1.yz, e2.xy), c (e2.z, index: 8 B).  56 B per node
// and 40 B per triangle instead of 64 and 48, in 4 and 3 separate lines.
struct SoaScene {
    const uint4* __restrict__ na = nullptr;
    const uint4* __restrict__ nb = nullptr;
    const uint2* __restrict__ nc = nullptr;
    const int4* __restrict__ nd = nullptr;
    const float4* __restrict__ ta = nullptr;
    const float4* __restrict__ tb = nullptr;
    const float2* __restrict__ tc = nullptr;
};

// Box culling is conservative (DESIGN.md "Scene query contract"): leaf boxes are
// inflated by kBoxPadRel * (|coord| + extent) and the far slab distance is
// stretched by kTfarSlack, so every triangle the reference would accept is
// reached and Moller-Trumbore alone decides.
constexpr float kBoxPadRel = 1e-5f;
constexpr float kTfarSlack = 1.00001f;

// Stack: SL entries per lane live in LDS, the rest spill to a global per-lane
// area.  BVH4Q: <= 3 entries per level.  The build rejects trees that could
// exceed kStackTotal (DESIGN.md "Traversal").
constexpr int kStackTotal = 128;

// Option shadow_order's default (-1) in sample and pixel seeding and for the
// batched queries: largest exit first ("The walk over
// the same tree"); row seeding keeps nearest first (tmpt_render.hip view()).
constexpr int kShadowOrderDefault = 2;
// Option pop_cull's default (-1) per seeding mode, from the same-box A/B
// ("A key in the entry's spare bits"): on everywhere.
// Sample and row seeding gain on the parent by more than three times the A/A
// spread; pixel seeding only draws level with it, but with the pop's extra
// instructions in the kernel either way, off would cost it 7 %.  The batched
// queries and the AOV pass go by sample seeding's.
constexpr int kPopCullSample = 1, kPopCullPixel = 1, kPopCullRow = 1;

// tmpt_scene_hit_device's two measured defaults (options query_top / query_sort = -1;
// DESIGN.md section 4, "Device-resident queries", has the table and the rule):
// the LDS top levels, and the smallest batch that is sorted (0: never)
constexpr int kQueryTopDefault = 1;
constexpr int64_t kQuerySortMinN = 0;
constexpr int kQuerySortTimed = 32;  // chunks of a sorted call whose keys + sort are timed (query_sort_ms)

constexpr int kRowSpecMaxGroups = 8;  // speculative row engine: row groups (streams)
constexpr int kRenderCounters = 48;   // ray / visit / round counters of one render
constexpr int kWalkCounter = 42;      // [42] stack entries pop culling discarded, [43] of them followed by
                                      // another stale entry (counting instantiations only)
constexpr int kCamCounter = 44;       // [44..46] k_path PROF >= 2: shading rounds, those whose camera block runs,
                                      // the lanes in it
constexpr int kTopCounter = 32;      // [32..41] k_path's top-level visit and top-walk round statistics
                                      // (instrumented instantiations only)
constexpr int kTieCounter = 24;       // [24] tied queries re-answered over the octree, [25] root-box misses,
                                      // [30] crack / flat-triangle queries re-answered over it (ties[6])
constexpr int kCrackCounter = 30;
constexpr int kRedoRaysCounter = 31;  // rays of the k_redo launch (part of [0])
constexpr int kSplitOverflowCounter = 47;  // shadow-split queue entries that found the queue full (none: an error)
constexpr int kRedoCounter = 26;      // samples the deferred-tie sample kernel left to the redo pass

// Per-scene options: the library's control plane in place of environment
// variables (include/tmpt.h documents each key).  Build options are fixed when
// the scene is created; render options apply to the renders after they are set.
struct Options {
    // build (tmpt_scene_create_ex)
    int builder = 0;      // 0 = PLOC (Meister & Bittner 2018), 1 = LBVH (Karras 2012)
    int layout = 0;       // 0 = AoS records (64-B nodes, 48-B triangles), 1 = also SoA planes (SoaScene)
    int leaf_max = 2;     // triangles per BVH4 leaf, 1..kLeafMaxTris
    int collapse = 0;     // BVH2 -> BVH4: 0 = greedy largest-area opening, 1 = SAH-optimal
    int ploc_radius = 32; // PLOC nearest-neighbour search radius
    float sah_c_leaf = 0.7f, sah_c_tri = 0.5f;  // SAH collapse costs (inner node = 1)
    // render (tmpt_scene_set_option)
    int sample_base = 0;      // sample seeding: sample s starts 2^16 (s + sample_base) steps into the pixel's stream
                              // (host only: ensure_sample_tables builds J_(s + B); 0 .. 64512)
    int sample_block = 0;    // sample seeding: samples per work unit, a power of two (0 = auto)
    int rowstream_dynamic = 1;  // row seeding, streaming: windows and spread follow the live rows
    int row_flag_leaves = 1;    // row seeding, streaming, octree answering: flag-only leaves (TIES 2)
    int row_occ = 0;            // row seeding, streaming: worker waves per SIMD (0 = by load, 4, 5)
    int sample_tail = -1;     // sample seeding: blocks per resident lane run as single samples at the end (-1 auto)
    double sbuf_max = 0.0;    // sample seeding: cap on the per-sample colour buffer, bytes (0 = 3/4 of free HBM)
    int sbuf_pair = 1;        // sample seeding: a unit's sample pairs written back to back into one 32-B sector
    int cam_pre = -1;         // sample seeding, 5 waves: the pass's camera samples made by a pre-pass on full
                              // waves, k_path reads them (-1 = the measured default, 0 off, 1 on where it fits)
    double cam_pre_max = 0.0; // cam_pre: cap on the pre-pass's buffer, bytes (0 = half of the free HBM)
    int shadow_split = 1;     // sample seeding, 5 waves, with the camera pre-pass: the shadow queries traced by a
                              // kernel of their own after k_path (k_shadow), the samples resolved from records
    double shadow_split_max = 0.0;  // shadow_split: cap on its queue and records, bytes (0 = half of the free HBM)
    int shadow_split_pass = 0;      // shadow_split: at most this many samples of every pixel per pass (0 = what fits)
    int pilot = -1;           // pixel seeding: pilot-pass samples of the cost ordering (-1 auto, 0 off)
    int help = -1;            // pixel seeding: shadow offload to idle lanes (-1 auto, 0 off, 1 on)
    int pair = -1;            // pixel seeding: expensive ranks per 64-rank chunk with offload (-1 auto)
    int balance = 1;          // pixel seeding: SIMD-balanced first chunks
    int dprio = 1;            // pixel seeding: longest-remaining-first wave priority with offload
    int wave_cap = 0;         // pixel seeding: pixels a wave holds at once (0 auto, else 1..64)
    int pixel_chains = -1;    // pixel seeding, ordered: heaviest pixels per 1024 run as speculative chains (-1 auto)
    int rowspec = 1;          // row seeding: speculative row engine (0 = one lane per row chain)
    int rowspec_wmax = 0;     // row seeding: units per window (0 = auto: 24 x spp)
    int rowspec_windows = 0;  // row seeding: windows per row and iteration (0 = auto)
    float rowspec_spread = -1.0f;  // row seeding: window spread in pixels (-1 = auto)
    int rowspec_groups = 2;   // row seeding: row groups on their own streams
    int rowspec_noshadow = 1; // row seeding: shadow-free speculation + one full re-trace of the chain
    int rowspec_chase = 1;    // row seeding, shadow-free: the chase walks LDS-staged units, one wave per row
    int rowspec_stream = 1;   // row seeding: the streaming row engine (one launch; 0 = iterations)
    int rowstream_test_abort = 0;  // test hook: the streaming engine's chasers leave at once, so its
                                   // watchdog aborts the launch and the iterated engine renders the frame
    int wf_bins = 1;          // wavefront engine: extend sub-queues per segment by direction octant (1, 2, 4, 8)
    int tie_rule = 0;         // closest hits tied on t: 0 = the reference's octree visit order (needs
                              // tmpt_scene_build_octree), 1 = the lowest triangle index
    int tie_defer = -1;       // sample seeding, octree rule: tied samples left to a redo pass, so the
                              // main kernel carries no octree walk (-1 auto, 0 off, 1 on)
    int redo_cap = 0;         // test hook: the redo list's capacity in entries (0 = auto; a small one
                              // overflows, and the frame is rendered again with the list grown)
    int redo_lanes = 4;       // tie_defer: lanes per wave that take re-traces in the launch's tail
    int path_waves = 0;       // path-kernel waves per SIMD (0 = auto: 5 in sample seeding, in pixel seeding
                              // from 3 pixels per 4-wave lane; 4, 5 or 6 -- 6: the shadow split's twins,
                              // 5 wherever there is no 6-wave kernel)
    int redo_inline = 1;      // test hook: 0 = the deferring kernel's waves leave every dropped sample
                              // to the k_redo launch (its fallback) instead of tracing them in their tail
    int top_walk = -1;        // path kernels: node rounds over the LDS-cached top levels at the end of a
                              // shading round, with no global load in them (-1 = per seeding, 0 off, 1..8)
    int shadow_order = -1;    // any-hit queries: the order a node's children are visited in (-1 = default,
                              // 0 nearest entry first, 1 longest overlap tf - tn first, 2 largest exit tf first)
    int pop_cull = -1;        // closest-hit queries: a popped stack entry whose key (a lower bound of its child's
                              // entry distance) already exceeds the best hit is discarded unvisited, and one
                              // more entry popped (-1 = the seeding's measured default, 0 off, 1 on)
    int pop_key_cap = -1;     // test hook: at most this many key bits in a stack entry (-1 = no cap; below
                              // kPopKeyMin there is no key and nothing is culled)
    int aov_group = 0;        // AOV pass: lanes that share a pixel (0 = auto, else 1, 2, 4, 8 or 16)
    int motion_tile = -1;     // tmpt_render_motion: a wave takes an 8 x 8 block of pixels (1), 64 pixels of a row
                              // (0), or the measured choice (-1)
    int octree_build = 0;     // tmpt_scene_build_octree: 0 = the host build (tmpt_octree.cpp), 1 = the level-order
                              // build on the device (tmpt_octree_dev.hip); the same octree word for word
    double octree_dev_max = 0.0;  // octree_build=device: cap on its scratch and result, bytes (0 = half of the free HBM)
    int query_sort = -1;      // tmpt_scene_hit_device: rays traced in the order of a 24-bit origin-cell / direction key
                              // (tmpt_query_key.h), in chunks (-1 = the measured rule, 0 off, 1 on)
    int query_top = -1;       // tmpt_scene_hit_device: the top BVH4 levels read from LDS (-1 = the measured default)
    double query_max = 0.0;   // tmpt_scene_hit_device: cap on the scene's query scratch, bytes (0 = half of the free HBM)
    int query_chunk = 1 << 22;  // test hook: rays per sorted chunk
    int query_grid = 0;       // test hook: cap on the blocks of a k_query launch (0 = the occupancy grid)
    int query_legacy = 0;     // tool hook: 1 = tmpt_scene_hit_device launches k_intersect on the caller's device
                              // data instead (tools/hit_device_time.py's kernel-only comparison; no uv)
    int denoise_lds = -1;     // tmpt_denoise: levels of stride 1 and 2 read an LDS tile + halo (1), every level
                              // reads global memory directly (0), or the measured choice per stride (-1)
};
int options_parse(Options& o, const char* text, bool allow_build);
int options_set(Options& o, const char* key, double value, bool allow_build);
int options_get(const Options& o, const char* key, double* value);

// What a BVH build makes (build_lbvh, build_soa) and a refit rewrites: built
// into a local one and moved into the scene on success (tmpt_scene_update).
struct Bvh {
    int32_t n = 0;          // triangles incl. the floor
    int32_t n_nodes = 0;    // internal nodes of the binary tree the BVH4 is collapsed from
    int32_t max_depth = 0;  // of the LBVH (Karras builder)
    DeviceBuffer<Bvh4Node> nodes4;
    int32_t n_nodes4 = 0, depth4 = 0, leaf_max = 0, ploc_iters = 0;
    int32_t count_shift = 0, link_bits = 31;  // the links' layout (link_layout), fixed by the build
    DeviceBuffer<TriPre> tri_pre;
    DeviceBuffer<TriOrig> tri_orig;
    DeviceBuffer<> soa_buf;  // layout=soa: the planes of SoaScene, one allocation
    SoaScene soa;
    // scene updates (tmpt_scene_update): BVH4 level L is nodes [level_begin[L],
    // level_begin[L + 1]) (depth4 + 1 entries); every node's own exact f32 box
    // (6 floats per node, written by the build and by every refit); the padded
    // box of every leaf-ordered record (6 floats, a refit's scratch, allocated
    // by the first one)
    std::vector<int32_t> level_begin;
    DeviceBuffer<float> node_box;
    DeviceBuffer<float> rec_box;
    double build_ms = 0.0;
};

// The reference's octree on the device (tmpt_scene_build_octree): built into a
// local one and moved into the scene on success; Octree{} drops it.
struct Octree {
    DeviceBuffer<OctNode> oct;
    DeviceBuffer<int32_t> oct_refs;
    DeviceBuffer<OctView> oct_view;  // device copy of {oct, oct_refs, n_oct, ties}
    int32_t n_oct = 0, oct_leaves = 0, oct_depth = 0;
    int32_t oct_flat = 0;  // triangles flat on one of the octree's planes (OctView::flat)
    OctGrid oct_grid{};    // its crack grid (OctView::grid)
    int64_t n_oct_refs = 0;
    double oct_build_ms = 0.0;
    float oct_lo[3] = {0, 0, 0}, oct_hi[3] = {0, 0, 0};
};

// Every buffer, event and stream below is an owner (tmpt_device.h): deleting
// the scene releases them, in reverse order of declaration -- the streams,
// declared first, last.  DESIGN.md "Owners" lists the kept buffers' budgets.
struct Scene {
    int device = 0;
    Stream stream;
    Stream rs_stream[kRowSpecMaxGroups];  // speculative row seeding: one per row group
    Bvh bvh;
    std::vector<float> tris_host;  // the triangles as given (Scene::Scene keeps its copy too)
    // the last update's kind (0 none, 1 refit, 2 rebuild) and device time;
    // option bvh_cost's cached value (valid: cost_known)
    int32_t update_kind = 0;
    double update_ms = 0.0;
    double cost = 0.0;
    bool cost_known = false;
    Event update_ev[2];
    // the reference's octree, and the counter of closest-hit queries answered
    // through it in the current call
    Octree octree;
    // octree_build=device: the build's scratch, bump-allocated chunks (kept, and
    // grown by further chunks; counted against octree_dev_max)
    std::vector<DeviceBuffer<>> oct_scratch;
    DeviceBuffer<uint32_t> oct_flags;  // and its overlap flags, one level's at a time (kept, grown)
    unsigned long long* ties = nullptr;  // [0] re-answered ties, [1] root-box misses (inside counters)
    uint64_t tie_queries = 0, root_misses = 0, crack_queries = 0;
    // row seeding: the engine of the last render (0 none, 1 one lane per row,
    // 2 iterated speculative, 3 streaming) and whether the streaming engine's
    // launch aborted and was re-rendered by the iterated one
    int32_t row_engine = 0, stream_fallbacks = 0;
    int64_t chain_pixels = 0;  // pixel seeding: pixels of the last render run as speculative chains
    Options opt;  // build and render options (tmpt_scene_create_ex / tmpt_scene_set_option)
    Event wait_ev;  // TMPT_FLAG_WAIT_STREAM: reused across renders
    DeviceBuffer<unsigned long long> counters;       // a render's ray / visit counters (device)
    PinnedBuffer<unsigned long long> counters_host;  // their pinned host copy
    DeviceBuffer<uint32_t> chk;  // the checked build's device word triple (kChk* codes), else unused
    Event render_ev[2];          // first / last kernel of a render
    DeviceBuffer<> ws;           // render workspace, kept and grown on demand
    DeviceBuffer<float> motion_prev;  // tmpt_render_motion: a host prev_tris uploaded (kept, grown, never shrunk)
    DeviceBuffer<> clip_stage;        // tmpt_temporal_clip: the host form's frames on the device (kept, grown)
    // progressive spp: per-pixel {colour sum xyz, rng} of the last pass (kept,
    // grown), and the shard it belongs to (width, height, spp, band_rows,
    // shard, num_shards, next sample)
    DeviceBuffer<float4> prog;
    int32_t prog_key[7] = {0, 0, 0, 0, 0, 0, -1};
    uint64_t prog_cam = 0;  // FNV-1a of the camera (and seed mode) of that pass
    // sample seeding: sample_seed's jump tables for samples [0, jt_spp), and the
    // per-sample colour buffer of block-split pixels (tmpt_render.hip k_resolve; kept, grown)
    DeviceBuffer<uint32_t> jt;
    int32_t jt_spp = 0;
    DeviceBuffer<float4> sbuf;
    // the camera pre-pass's entries (tmpt_render.hip k_cam_rays; 32 B per sample
    // of a pass; kept, grown), and whether the last render ran it
    DeviceBuffer<> cam_rays;
    int32_t cam_rays_used = 0;
    // the shadow split's queue (16 B per entry) and sample records (64 B per
    // sample of a pass; kept, grown); whether the last render ran it, its
    // passes, and its kernels' times
    DeviceBuffer<> split_buf;
    int32_t split_used = 0, split_passes = 0;
    // waves per SIMD the last render's path kernel was built for and launched at (0: no k_path ran)
    int32_t path_waves_used = 0;
    // a shadow-split render in several passes of samples (render_split_passes):
    // the pixels' float sums carried from pass to pass (RenderArgs::prog of
    // its passes; kept, grown) and the passes' summed statistics
    DeviceBuffer<float4> split_carry;
    bool split_sub = false;
    struct SplitAcc {
        double extend_ms = 0.0, shadow_ms = 0.0, resolve_ms = 0.0, redo_ms = 0.0;
        int64_t redo_samples = 0, redo_late = 0;
        int32_t redo_launches = 0, launches = 0, used = 0;
    } split_acc;
    Event split_ev[3];  // before k_shadow, between, after k_split_resolve
    double split_resolve_ms = 0.0;
    // deferred ties (PathCtl::redo): the redo list, its capacity in entries,
    // and the samples the last render left to the redo pass
    DeviceBuffer<uint2> redo;
    uint32_t redo_cap = 0;
    DeviceBuffer<float4> redo_state;  // per redo slot: where its path stopped (tmpt_render.hip kRedoState4)
    int64_t redo_samples = 0;
    int64_t redo_late = 0;   // of them, left by the launch's tail to the k_redo launch
    int32_t redo_launches = 0;  // k_redo launches of the last render
    int32_t tie_path = 0;       // tmpt_stats.tie_path of the last render
    bool row_render = false;    // the render in progress is row-seeded (view(): shadow_order's default)
    bool pixel_render = false;  // ... is pixel-seeded (view(): pop_cull's default)
    double redo_ms = 0.0;       // and their time (not in extend_ms)
    uint64_t redo_rays = 0;     // and their rays (in the render's count)
    // speculative row seeding (tmpt_rows.hip render_rowspec): jump tables
    // M^(2j) for j in [0, jt2_n), and its row/unit buffers (kept, grown)
    DeviceBuffer<uint32_t> jt2;
    int32_t jt2_n = 0;
    DeviceBuffer<> rs_buf;
    Event rs_event[kRowSpecMaxGroups + 1];  // group ends; [max]: the start
    PinnedBuffer<uint32_t> rs_host;         // each group's last unit count
    DeviceBuffer<> rs_list;                 // no-shadow speculation: the chain list (kept, grown)
    // streaming row engine (render_rowstream): rings, windows, anchors (kept,
    // grown); its jump tables (M^(2c), M^(256b), M^(2^15 a0), M^(2^20 a1));
    // pinned control words
    DeviceBuffer<> rss_buf;
    DeviceBuffer<uint32_t> rss_tab;
    PinnedBuffer<uint32_t> rss_host;
    // adaptive sampling (tmpt_adaptive.hip render_adaptive): set around each of
    // its passes for render_persistent -- adapt_on: the pass keeps its samples
    // in the colour buffer and resolves nothing; adapt_list / adapt_n: the
    // pixels of a pass after the first (device list of tile slots, ascending,
    // inside adapt_buf) -- and the call's buffers (per-pixel state, the two
    // lists, the block masks and counts; kept, grown), with the pinned
    // next-list length
    bool adapt_on = false;
    const uint32_t* adapt_list = nullptr;
    int64_t adapt_n = 0;
    DeviceBuffer<> adapt_buf;
    PinnedBuffer<uint32_t> adapt_host;
    // tmpt_scene_hit_device (tmpt_query.hip query_batch): the overflow stacks and
    // sort buffers of its launches (kept, grown, counted against query_max), its
    // events (the call; keys + sort of the first kQuerySortTimed chunks), and the
    // last call's read-only options
    DeviceBuffer<> query_buf;
    Event query_ev[2];
    std::vector<Event> query_sort_ev;
    double query_ms = 0.0, query_sort_ms = 0.0;
    int64_t query_chunks = 0;
    int32_t query_sorted = 0;
    int path_launches = 1;  // k_path launches of the last persistent render (pilot ordering: 2)
    Event path_ev[4];       // around the pilot / final k_path
    // statistics of the last render
    double render_ms = 0.0;
    double extend_ms = 0.0;
    double shadow_ms = 0.0;
    uint64_t extend_rays = 0, shadow_rays = 0;
    int64_t extend_launches = 0, shadow_launches = 0, iterations = 0;
    uint64_t node_visits = 0, tri_tests = 0;  // only with TMPT_FLAG_COUNT_VISITS
    uint64_t shadow_node_visits = 0, shadow_tri_tests = 0;
};

// error plumbing: last error is thread-local, ints cross the ABI, never exceptions
void set_error(const std::string& msg);
const char* last_error();

#define TMPT_HIP(call)                                                                  \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ::tmpt::set_error(std::string(#call) + ": " + hipGetErrorString(e_));       \
            return -1;                                                                  \
        }                                                                               \
    } while (0)

// an owner's alloc / reserve (tmpt_device.h) that must succeed
#define TMPT_ALLOC(ok, what)                                                            \
    do {                                                                                \
        if (!(ok)) {                                                                    \
            ::tmpt::set_error(std::string(what) + ": out of device memory");            \
            return -1;                                                                  \
        }                                                                               \
    } while (0)

// tmpt_bvh.hip
// the build of bvh.n triangles (device, 9 floats each) into an empty Bvh, on a
// stream the caller owns
int build_lbvh(Bvh& bvh, const Options& opt, hipStream_t st, const float* d_tris9);
int build_soa(Bvh& bvh, hipStream_t st);  // layout=soa planes from the built AoS records
// tmpt_scene_update's refit: the built tree fitted to its n new triangles
// (device, 9 floats each), launched on st; and option bvh_cost,
// tests/bvh_check.py cost() by a float64 reduction kernel
int refit_bvh(Bvh& bvh, hipStream_t st, const float* d_tris9);
int bvh_cost(Scene& s, double* out);
// the octree's flat triangles marked in the leaf-ordered records (bit 0 of the
// doubled index), the others cleared; flat has s.n entries (empty: clear all)
int mark_flat_triangles(Scene& s, const std::vector<uint8_t>& flat);
// tmpt_octree_dev.hip: option octree_build=device.  The reference's octree of
// the scene's triangles (bvh.tri_orig) built on s.stream into o (oct, oct_refs,
// the counts, leaves, depth) and the largest plane offset per axis for
// octree_grid_from_offsets.  0; -12 over octree_dev_max or out of device memory
// (the scene unchanged); -22 for a tree the host path refuses too; -1 HIP error.
int build_octree_device(Scene& s, const float bmin[3], const float bmax[3], Octree& o, double wmax[3]);
// tmpt_render.hip: the scene's counters, pinned copy and render events (once)
int ensure_counters(Scene& s);
int check_report(Scene& s, const char* what);
// tmpt_render.hip: sample_seed's byte tables for samples [0, spp) (1024 words each)
void sample_jump_tables(int32_t spp, std::vector<uint32_t>& tab);
// device radix sort of (key, value) pairs (tmpt_bvh.hip); returns 0 if the
// result is in (keys, vals), 1 if in (tkeys, tvals)
int radix_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* tkeys, uint32_t* tvals, int32_t n,
                     int bits, uint32_t* hist, hipStream_t st);
size_t radix_sort_hist_words(int32_t n);
// check hooks (tmpt_bvh.hip): the built nodes (16 words each) and triangle
// records (12 words each) copied to the host, from the AoS records or put
// together again from the SoA planes; and radix_sort_pairs over host data
constexpr int32_t kRadixSortHookMax = 1 << 22;
int dump_bvh(Scene& s, bool soa, uint32_t* nodes, uint32_t* tris);
int radix_sort_host(Scene& s, uint32_t* keys, uint32_t* vals, int32_t n, int bits);

TMPT_HD float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }

}  // namespace tmpt
