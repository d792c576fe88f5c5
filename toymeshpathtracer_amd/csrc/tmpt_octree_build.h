// tmpt_octree_build.h -- the arithmetic of the reference's octree build, one
// body for the host and for gfx950.
//
// First half: the box and overlap rules of Subdivide / InternalDivide
// (scene.cpp:99-160, maths.cpp:165-298), moved here from tmpt_octree.cpp so
// that the host recursion (build_octree) and the device build
// (tmpt_octree_dev.hip) run the same expressions in the same rounding order
// (-ffp-contract=off on both sides, csrc/Makefile NUMERIC).
//
// Second half: the level-order build (option octree_build=device) as passes
// over one level's nodes or list entries.  Every pass is a function of one
// index; a device kernel calls it for its thread's index, and the host
// restatement (tmpt_octree.cpp build_octree_levels, tmpt_octree_arrays method
// 1) calls it in a loop, so the relayout arithmetic is the same code on both
// sides and is checked without a device (tests/test_octree_arrays.py).
//
//   level d   nodes [0, n): box, list = ids[start .. start + cnt), owner[e] the
//             node of list entry e.  The lists of a level lie back to back in
//             node order.
//   split     node i splits when cnt > 10 and d < 10 (scene.cpp:101).  `split`
//             and `fstart` hold, after an exclusive scan over n + 1 words, the
//             number of split nodes before i and the list entries of split
//             nodes before i; node i's children are nodes 8 s + k of level
//             d + 1, s = split[i].
//   flags     F[8 fstart[i] + k cnt + j] = 1 when entry j of node i's list
//             overlaps child k's box: the order (node, child, position) is the
//             order of level d + 1's lists, so one exclusive scan of F gives
//             every kept entry its place there and every child its start and
//             count.  A child's list is its parent's, filtered in order; no
//             atomics, nothing depends on scheduling.
//   sizes     bottom-up: subn = nodes of the subtree, subr = its words in refs
//             (1 + count per leaf).
//   preorder  top-down: child k's index = parent's + 1 + subn of children
//             0..k-1, its list offset = parent's + subr of children 0..k-1.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tmpt_math.h"

namespace tmpt {

TMPT_HD float comp(f3 v, int q) { return q == 0 ? v.x : (q == 1 ? v.y : v.z); }

// PlaneIntersectAabb (maths.cpp:165-197): does the plane through `vert` with
// normal `n` meet the box [-half, half]?  The nearest and farthest box corners
// along n, offset by -vert, tested with glm::dot's (x*x' + y*y') + z*z'.
TMPT_HD bool plane_meets_box(f3 n, f3 vert, f3 half)
{
    float near_c[3], far_c[3];
    for (int q = 0; q < 3; ++q) {
        const float h = comp(half, q), v = comp(vert, q);
        const bool pos = comp(n, q) > 0.0f;
        near_c[q] = pos ? -h - v : h - v;
        far_c[q] = pos ? h - v : -h - v;
    }
    if (dot(n, mk(near_c[0], near_c[1], near_c[2])) > 0.0f) return false;
    return dot(n, mk(far_c[0], far_c[1], far_c[2])) >= 0.0f;
}

// One cross-product axis of the separating-axis test (the AXISTEST_* macros,
// maths.cpp:112-156): the two distinct vertex projections pa, pb (ordered as
// the macro orders its pair) against the box's projected radius.
TMPT_HD bool axis_separates(float pa, float pb, float rad)
{
    const float lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    return lo > rad || hi < -rad;
}

// The triangle's extent on one box axis (FINDMINMAX, maths.cpp:158-163) against
// the half size.
TMPT_HD bool extent_separates(float a, float b, float c, float h)
{
    float lo = a, hi = a;
    if (b < lo) lo = b;
    if (b > hi) hi = b;
    if (c < lo) lo = c;
    if (c > hi) hi = c;
    return lo > h || hi < -h;
}

// TriangleIntersectAabb (maths.cpp:199-298): Akenine-Moller's triangle / box
// overlap with the box centred at `c`, half size `h`.  The nine edge axes in
// the reference's order (its early exits do not change the answer, only the
// rounding of each projection does, so each one is formed as the macro does:
// products, then one difference), then the box axes, then the plane.
TMPT_HD bool tri_overlaps_box(f3 c, f3 h, const f3* tri)
{
    const f3 v0 = tri[0] - c, v1 = tri[1] - c, v2 = tri[2] - c;
    const f3 e[3] = {v1 - v0, v2 - v1, v0 - v2};
    // vertex pairs per edge: x and y axes use (v0, v2) for edges 0 and 1 and
    // (v0, v1) for edge 2; the z axis (v1, v2), (v0, v1), (v1, v2), each pair
    // in the order its macro compares them
    const f3* xy_pair[3][2] = {{&v0, &v2}, {&v0, &v2}, {&v0, &v1}};
    const f3* z_pair[3][2] = {{&v2, &v1}, {&v0, &v1}, {&v2, &v1}};  // Z12 orders (p2, p1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f3 E = e[k];
        const float ax = fabsf(E.x), ay = fabsf(E.y), az = fabsf(E.z);
        const f3 &p = *xy_pair[k][0], &q = *xy_pair[k][1];
        // x: a = E.z, b = E.y -> a*v.y - b*v.z, rad = |E.z| h.y + |E.y| h.z
        if (axis_separates(E.z * p.y - E.y * p.z, E.z * q.y - E.y * q.z, az * h.y + ay * h.z)) return false;
        // y: -a*v.x + b*v.z with a = E.z, b = E.x, rad = |E.z| h.x + |E.x| h.z
        if (axis_separates(-E.z * p.x + E.x * p.z, -E.z * q.x + E.x * q.z, az * h.x + ax * h.z)) return false;
        // z: a*v.x - b*v.y with a = E.y, b = E.x, rad = |E.y| h.x + |E.x| h.y
        const f3 &r = *z_pair[k][0], &s = *z_pair[k][1];
        if (axis_separates(E.y * r.x - E.x * r.y, E.y * s.x - E.x * s.y, ay * h.x + ax * h.y)) return false;
    }
    if (extent_separates(v0.x, v1.x, v2.x, h.x)) return false;
    if (extent_separates(v0.y, v1.y, v2.y, h.y)) return false;
    if (extent_separates(v0.z, v1.z, v2.z, h.z)) return false;
    return plane_meets_box(cross(e[0], e[1]), v0, h);
}

// child k of [lo, hi] (scene.cpp:119-141): bit 0 of k offsets x, bit 1 z,
// bit 2 y by the parent's half size; child 0 keeps the parent's min
// without an addition (a -0 coordinate stays -0)
TMPT_HD void oct_child_box(f3 lo, f3 half, int k, f3& clo, f3& chi)
{
    clo = k == 0 ? lo : lo + mk((k & 1) ? half.x : 0.0f, (k & 4) ? half.y : 0.0f, (k & 2) ? half.z : 0.0f);
    chi = clo + half;
}

// does triangle `tri` overlap the child box [clo, chi] (scene.cpp:144-154:
// centre and half size from the child's own box)
TMPT_HD bool oct_child_keeps(f3 clo, f3 chi, const f3* tri)
{
    const f3 c = (clo + chi) * 0.5f, h = (chi - clo) * 0.5f;
    return tri_overlaps_box(c, h, tri);
}

constexpr int kOctSplitOver = 10, kOctMaxDepth = 10;  // scene.cpp:101

// The distance of coordinate x from the nearest plane r0 + j cell (octree_grid).
TMPT_HD double oct_plane_offset(double x, double r0, double cell)
{
    return ::fabs(x - (r0 + ::nearbyint((x - r0) / cell) * cell));
}

// ------------------------------------------------------- the level-order build
// One level's arrays (host vectors or device memory; the passes only index).
struct OctLevel {
    float* lo;         // [3 n] box min per node
    float* hi;         // [3 n] box max
    int32_t* start;    // [n] the node's list: ids[start .. start + cnt)
    int32_t* cnt;      // [n]
    uint32_t* split;   // [n + 1] flag, then its exclusive scan
    uint32_t* fstart;  // [n + 1] split ? cnt : 0, then its exclusive scan
    int32_t* subn;     // [n] nodes of the subtree
    int64_t* subr;     // [n] words of the subtree in refs
    int32_t* idx;      // [n] preorder index
    int64_t* roff;     // [n] offset of the subtree's first leaf list in refs
    int32_t* ids;      // [m] the lists, back to back in node order
    int32_t* owner;    // [m] the node of each list entry
    int32_t n;
    int32_t m;
};

TMPT_HD f3 oct_ld3(const float* p, int64_t i) { return mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
TMPT_HD void oct_st3(float* p, int64_t i, f3 v) { p[3 * i] = v.x, p[3 * i + 1] = v.y, p[3 * i + 2] = v.z; }
TMPT_HD bool oct_is_split(const OctLevel& L, int32_t i) { return L.split[i + 1] != L.split[i]; }  // after the scan

// pass "classify", i in [0, n]: the split rule; word n is the scans' total
TMPT_HD void oct_classify(const OctLevel& L, int32_t i, int depth)
{
    const bool sp = i < L.n && L.cnt[i] > kOctSplitOver && depth < kOctMaxDepth;
    L.split[i] = sp ? 1u : 0u;
    L.fstart[i] = sp ? (uint32_t)L.cnt[i] : 0u;
}

// pass "children", i in [0, P.n): the 8 child boxes of a split node
TMPT_HD void oct_children(const OctLevel& P, const OctLevel& C, int32_t i)
{
    if (!oct_is_split(P, i)) return;
    const int64_t c0 = 8 * (int64_t)P.split[i];
    const f3 lo = oct_ld3(P.lo, i), hi = oct_ld3(P.hi, i);
    const f3 half = (hi - lo) * 0.5f;  // dimensions() * 0.5f, scene.cpp:109
    for (int k = 0; k < 8; ++k) {
        f3 clo, chi;
        oct_child_box(lo, half, k, clo, chi);
        oct_st3(C.lo, c0 + k, clo);
        oct_st3(C.hi, c0 + k, chi);
    }
}

// pass "overlap", e in [0, P.m): list entry e against its node's 8 child
// boxes; tris + stride * id holds the triangle's 9 floats.  F has 8 x (list
// entries of split nodes) + 1 words, the last 0.
TMPT_HD void oct_overlap(const OctLevel& P, const OctLevel& C, const float* tris, int stride, uint32_t* F, int32_t e)
{
    const int32_t i = P.owner[e];
    if (!oct_is_split(P, i)) return;
    const int64_t c0 = 8 * (int64_t)P.split[i], cnt = P.cnt[i];
    const int64_t base = 8 * (int64_t)P.fstart[i] + (e - P.start[i]);
    const float* t = tris + (int64_t)stride * P.ids[e];
    const f3 tri[3] = {mk(t[0], t[1], t[2]), mk(t[3], t[4], t[5]), mk(t[6], t[7], t[8])};
    for (int k = 0; k < 8; ++k)
        F[base + k * cnt] = oct_child_keeps(oct_ld3(C.lo, c0 + k), oct_ld3(C.hi, c0 + k), tri) ? 1u : 0u;
}

// pass "child lists", i in [0, P.n), after F's exclusive scan: each child's
// start and count in level d + 1's lists
TMPT_HD void oct_child_lists(const OctLevel& P, const OctLevel& C, const uint32_t* F, int32_t i)
{
    if (!oct_is_split(P, i)) return;
    const int64_t c0 = 8 * (int64_t)P.split[i], cnt = P.cnt[i], base = 8 * (int64_t)P.fstart[i];
    for (int k = 0; k < 8; ++k) {
        const uint32_t a = F[base + k * cnt], b = F[base + (k + 1) * cnt];
        C.start[c0 + k] = (int32_t)a;
        C.cnt[c0 + k] = (int32_t)(b - a);
    }
}

// pass "scatter", e in [0, P.m), after F's exclusive scan: the kept entries to
// their places in level d + 1
TMPT_HD void oct_scatter(const OctLevel& P, const OctLevel& C, const uint32_t* F, int32_t e)
{
    const int32_t i = P.owner[e];
    if (!oct_is_split(P, i)) return;
    const int64_t c0 = 8 * (int64_t)P.split[i], cnt = P.cnt[i];
    const int64_t base = 8 * (int64_t)P.fstart[i] + (e - P.start[i]);
    const int32_t id = P.ids[e];
    for (int k = 0; k < 8; ++k) {
        const uint32_t a = F[base + k * cnt];
        if (F[base + k * cnt + 1] != a) {
            C.ids[a] = id;
            C.owner[a] = (int32_t)(c0 + k);
        }
    }
}

// pass "sizes", i in [0, P.n), levels bottom-up (C unused at a leaf)
TMPT_HD void oct_sizes(const OctLevel& P, const OctLevel& C, int32_t i)
{
    if (!oct_is_split(P, i)) {
        P.subn[i] = 1;
        P.subr[i] = 1 + (int64_t)P.cnt[i];
        return;
    }
    const int64_t c0 = 8 * (int64_t)P.split[i];
    int64_t nn = 1, nr = 0;  // nn: at most (8^11 - 1) / 7 < 2^31
    for (int k = 0; k < 8; ++k) {
        nn += C.subn[c0 + k];
        nr += C.subr[c0 + k];
    }
    P.subn[i] = (int32_t)nn;
    P.subr[i] = nr;
}

// pass "preorder", i in [0, P.n), levels top-down (the root: idx 0, roff 0)
TMPT_HD void oct_preorder(const OctLevel& P, const OctLevel& C, int32_t i)
{
    if (!oct_is_split(P, i)) return;
    const int64_t c0 = 8 * (int64_t)P.split[i];
    int32_t at = P.idx[i] + 1;
    int64_t r = P.roff[i];
    for (int k = 0; k < 8; ++k) {
        C.idx[c0 + k] = at;
        C.roff[c0 + k] = r;
        at += C.subn[c0 + k];
        r += C.subr[c0 + k];
    }
}

// pass "emit nodes", i in [0, L.n): the 8-word record (tmpt_internal.h
// OctNode: lo.xyz, skip, hi.xyz, ref) and a leaf's count word.  The totals
// are below INT32_MAX here (the caller refuses others before this pass).
TMPT_HD void oct_emit_node(const OctLevel& L, int32_t* nodes8, int32_t* refs, int32_t i)
{
    int32_t* o = nodes8 + 8 * (int64_t)L.idx[i];
    const bool leaf = !oct_is_split(L, i);
    for (int q = 0; q < 3; ++q) {
        o[q] = __builtin_bit_cast(int32_t, L.lo[3 * (int64_t)i + q]);
        o[4 + q] = __builtin_bit_cast(int32_t, L.hi[3 * (int64_t)i + q]);
    }
    o[3] = L.idx[i] + L.subn[i];
    o[7] = leaf ? (int32_t)L.roff[i] : -1;
    if (leaf) refs[L.roff[i]] = L.cnt[i];
}

// pass "emit lists", e in [0, L.m): a leaf's triangle ids behind its count
TMPT_HD void oct_emit_entry(const OctLevel& L, int32_t* refs, int32_t e)
{
    const int32_t i = L.owner[e];
    if (oct_is_split(L, i)) return;
    refs[L.roff[i] + 1 + (e - L.start[i])] = L.ids[e];
}

// pass "plane offsets", i in [0, n_nodes): the node's two planes of axis q
// against the grid, folded into w as octree_grid folds them (a NaN is skipped)
TMPT_HD double oct_node_offset(const int32_t* nodes8, int32_t i, int q, double r0, double cell, double w)
{
    const double v[2] = {(double)__builtin_bit_cast(float, nodes8[8 * (int64_t)i + q]),
                         (double)__builtin_bit_cast(float, nodes8[8 * (int64_t)i + 4 + q])};
    for (int b = 0; b < 2; ++b) {
        const double d = oct_plane_offset(v[b], r0, cell);
        w = w < d ? d : w;  // std::max(w, d)
    }
    return w;
}

}  // namespace tmpt
