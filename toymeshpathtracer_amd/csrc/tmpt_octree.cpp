// tmpt_octree.cpp -- the reference's octree, built on the host.
//
// The device answers HitScene from its BVH4Q, whose answer is the closest
// hit over all triangles.  The reference walks an 8-way octree instead
// (scene.cpp:21-52) and keeps the FIRST triangle of the smallest t in its
// depth-first visit order, and its root box test can drop a ray that only
// grazes the root.  The traversal flags the queries where that can matter --
// a tie on t; a closest hit near one of the octree's finest-level planes on a
// ray that runs almost within that plane, where the 1-2 ulp cracks between
// sibling boxes (min + half + half) can hide the hit (octree_grid); a hit on
// a triangle flat in such a plane, which may be in no leaf at all
// (octree_flat_triangles) -- and those, and only those, are answered again
// over this octree on the device (tmpt_traverse.h octree_closest, octree_flag).  So the octree has to be the
// reference's node for node: the same boxes (bmin/bmax halved in float,
// scene.cpp:109-141), the same triangle lists (the separating-axis overlap
// test of maths.cpp:165-298 in its own rounding order), the same limits
// (more than 10 triangles and depth below 10, scene.cpp:101).
//
// Layout (tmpt_internal.h OctNode): depth-first preorder, each node's skip
// link pointing past its subtree, so the device walks it without a stack.
// The 8 subtrees of the root are built on their own threads and spliced.
// Like the reference's BuildOctree (main.cpp:312, outside the timed region
// :319-333), this is scene set-up, not part of a render.
//
// The box and overlap rules live in tmpt_octree_build.h, shared with the device
// build (tmpt_octree_dev.hip, option octree_build=device), whose passes are
// restated here as host loops too (build_octree_levels).
#include <string.h>

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "tmpt_internal.h"
#include "tmpt_octree_build.h"  // comp, tri_overlaps_box, oct_child_box: shared with the device build

namespace tmpt {

namespace {

inline float int_bits(int32_t v)
{
    float f;
    memcpy(&f, &v, 4);
    return f;
}
inline int32_t bits_int(float f)
{
    int32_t v;
    memcpy(&v, &f, 4);
    return v;
}

struct Builder {
    const f3* tris;  // 3 vertices per triangle
    OctreeHost out;

    // child k of [lo, hi] (scene.cpp:119-141; tmpt_octree_build.h)
    static void child_box(f3 lo, f3 half, int k, f3& clo, f3& chi) { oct_child_box(lo, half, k, clo, chi); }

    // the triangles of `ids` that overlap child box [clo, chi], in order
    // (scene.cpp:144-154: centre and half size from the child's own box)
    void filter(f3 clo, f3 chi, const std::vector<int32_t>& ids, std::vector<int32_t>& sub) const
    {
        const f3 c = (clo + chi) * 0.5f, h = (chi - clo) * 0.5f;
        sub.clear();
        for (int32_t id : ids)
            if (tri_overlaps_box(c, h, tris + 3 * (size_t)id)) sub.push_back(id);
    }

    void node(f3 lo, f3 hi, const std::vector<int32_t>& ids, int depth)
    {
        const size_t me = out.nodes.size();
        out.nodes.push_back(OctNode{make_float4(lo.x, lo.y, lo.z, 0.0f), make_float4(hi.x, hi.y, hi.z, 0.0f)});
        out.depth = std::max(out.depth, depth);
        if (ids.size() > 10 && depth < 10) {  // scene.cpp:101
            out.nodes[me].hi.w = int_bits(-1);
            const f3 half = (hi - lo) * 0.5f;  // dimensions() * 0.5f, scene.cpp:109
            std::vector<int32_t> sub;
            sub.reserve(ids.size());
            for (int k = 0; k < 8; ++k) {
                f3 clo, chi;
                child_box(lo, half, k, clo, chi);
                filter(clo, chi, ids, sub);
                node(clo, chi, sub, depth + 1);
            }
        } else {
            out.nodes[me].hi.w = int_bits((int32_t)out.refs.size());
            out.refs.push_back((int32_t)ids.size());
            out.refs.insert(out.refs.end(), ids.begin(), ids.end());
            ++out.leaves;
        }
        out.nodes[me].lo.w = int_bits((int32_t)out.nodes.size());
    }
};

}  // namespace

void build_octree(const float* tris9, int32_t n, const float bmin[3], const float bmax[3], OctreeHost& out)
{
    std::vector<f3> v((size_t)n * 3);
    for (size_t i = 0; i < v.size(); ++i) v[i] = mk(tris9[3 * i], tris9[3 * i + 1], tris9[3 * i + 2]);
    const f3 lo = mk(bmin[0], bmin[1], bmin[2]), hi = mk(bmax[0], bmax[1], bmax[2]);
    std::vector<int32_t> all((size_t)n);
    for (int32_t i = 0; i < n; ++i) all[(size_t)i] = i;  // BuildOctree: the scene's triangle order
    out = OctreeHost();
    if (!(all.size() > 10)) {  // a leaf root
        Builder b{v.data(), {}};
        b.node(lo, hi, all, 0);
        out = std::move(b.out);
        return;
    }
    // the root's 8 subtrees on their own threads, spliced in child order
    const f3 half = (hi - lo) * 0.5f;
    Builder part[8];
    std::vector<std::thread> th;
    for (int k = 0; k < 8; ++k) {
        part[k].tris = v.data();
        th.emplace_back([&, k]() {
            f3 clo, chi;
            Builder::child_box(lo, half, k, clo, chi);
            std::vector<int32_t> sub;
            part[k].filter(clo, chi, all, sub);
            part[k].node(clo, chi, sub, 1);
        });
    }
    for (auto& t : th) t.join();
    size_t nn = 1, nr = 0;
    for (auto& p : part) {
        nn += p.out.nodes.size();
        nr += p.out.refs.size();
    }
    out.nodes.reserve(nn);
    out.refs.reserve(nr);
    out.nodes.push_back(OctNode{make_float4(lo.x, lo.y, lo.z, int_bits((int32_t)nn)),
                                make_float4(hi.x, hi.y, hi.z, int_bits(-1))});
    for (auto& p : part) {
        const int32_t on = (int32_t)out.nodes.size(), orf = (int32_t)out.refs.size();
        for (OctNode nd : p.out.nodes) {
            nd.lo.w = int_bits(bits_int(nd.lo.w) + on);
            const int32_t r = bits_int(nd.hi.w);
            if (r >= 0) nd.hi.w = int_bits(r + orf);
            out.nodes.push_back(nd);
        }
        out.refs.insert(out.refs.end(), p.out.refs.begin(), p.out.refs.end());
        out.leaves += p.out.leaves;
        out.depth = std::max(out.depth, p.out.depth);
    }
}

// The device build's passes (tmpt_octree_build.h) run on the host, one loop
// per kernel of tmpt_octree_dev.hip and in its order: the check hook
// tmpt_octree_arrays (method 1) compares its output with build_octree's word
// for word, so the level-order relayout is proved without a device.
namespace {
struct HostLevel {
    std::vector<float> lo, hi;
    std::vector<int32_t> start, cnt, subn, idx, ids, owner;
    std::vector<uint32_t> split, fstart;
    std::vector<int64_t> subr, roff;
    OctLevel v{};
    void nodes(size_t n)
    {
        lo.resize(3 * n), hi.resize(3 * n), start.resize(n), cnt.resize(n), subn.resize(n), idx.resize(n);
        split.resize(n + 1), fstart.resize(n + 1), subr.resize(n), roff.resize(n);
        v.n = (int32_t)n;
    }
    void lists(size_t m)
    {
        ids.resize(m), owner.resize(m);
        v.m = (int32_t)m;
    }
    const OctLevel& view()
    {
        v.lo = lo.data(), v.hi = hi.data(), v.start = start.data(), v.cnt = cnt.data(), v.split = split.data();
        v.fstart = fstart.data(), v.subn = subn.data(), v.subr = subr.data(), v.idx = idx.data(), v.roff = roff.data();
        v.ids = ids.data(), v.owner = owner.data();
        return v;
    }
};
void scan_exclusive(uint32_t* p, size_t n)
{
    uint32_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = p[i];
        p[i] = sum;
        sum += x;
    }
}
}  // namespace

int build_octree_levels(const float* tris9, int32_t n, const float bmin[3], const float bmax[3], OctreeHost& out)
{
    out = OctreeHost();
    std::vector<HostLevel> lv(1);
    lv[0].nodes(1);
    lv[0].lists((size_t)n);
    for (int q = 0; q < 3; ++q) lv[0].lo[(size_t)q] = bmin[q], lv[0].hi[(size_t)q] = bmax[q];
    lv[0].start[0] = 0, lv[0].cnt[0] = n;
    for (int32_t i = 0; i < n; ++i) lv[0].ids[(size_t)i] = i, lv[0].owner[(size_t)i] = 0;  // k_oct_root
    std::vector<uint32_t> F;
    for (int d = 0;; ++d) {
        const OctLevel P = lv[(size_t)d].view();
        for (int32_t i = 0; i <= P.n; ++i) oct_classify(P, i, d);
        scan_exclusive(P.split, (size_t)P.n + 1);
        scan_exclusive(P.fstart, (size_t)P.n + 1);
        const uint32_t n_split = P.split[P.n], m_split = P.fstart[P.n];
        if (!n_split) break;
        if (8 * (uint64_t)n_split >= (uint64_t)INT32_MAX || 8 * (uint64_t)m_split + 1 >= (uint64_t)INT32_MAX) return -1;
        lv.emplace_back();
        lv.back().nodes(8 * (size_t)n_split);
        const OctLevel P1 = lv[(size_t)d].view();  // (the vector moved)
        OctLevel C = lv.back().view();
        for (int32_t i = 0; i < P1.n; ++i) oct_children(P1, C, i);
        F.assign(8 * (size_t)m_split + 1, 0u);
        for (int32_t e = 0; e < P1.m; ++e) oct_overlap(P1, C, tris9, 9, F.data(), e);
        scan_exclusive(F.data(), F.size());
        for (int32_t i = 0; i < P1.n; ++i) oct_child_lists(P1, C, F.data(), i);
        lv.back().lists((size_t)F.back());
        C = lv.back().view();
        for (int32_t e = 0; e < P1.m; ++e) oct_scatter(P1, C, F.data(), e);
    }
    const int depth = (int)lv.size() - 1;
    for (int d = depth; d >= 0; --d) {
        const OctLevel P = lv[(size_t)d].view(), C = d < depth ? lv[(size_t)d + 1].view() : OctLevel{};
        for (int32_t i = 0; i < P.n; ++i) oct_sizes(P, C, i);
    }
    const int64_t nn = lv[0].subn[0], nr = lv[0].subr[0];
    if (nr >= (int64_t)INT32_MAX || nn >= (int64_t)INT32_MAX) return -1;
    lv[0].idx[0] = 0, lv[0].roff[0] = 0;
    for (int d = 0; d < depth; ++d) {
        const OctLevel P = lv[(size_t)d].view(), C = lv[(size_t)d + 1].view();
        for (int32_t i = 0; i < P.n; ++i) oct_preorder(P, C, i);
    }
    std::vector<int32_t> words(8 * (size_t)nn);
    out.refs.resize((size_t)nr);
    int32_t* nodes8 = words.data();
    for (int d = 0; d <= depth; ++d) {
        const OctLevel L = lv[(size_t)d].view();
        for (int32_t i = 0; i < L.n; ++i) oct_emit_node(L, nodes8, out.refs.data(), i);
        for (int32_t e = 0; e < L.m; ++e) oct_emit_entry(L, out.refs.data(), e);
        out.leaves += L.n - (int32_t)L.split[L.n];
    }
    out.depth = depth;
    static_assert(sizeof(OctNode) == 32, "8 words");
    out.nodes.resize((size_t)nn);
    memcpy(static_cast<void*>(out.nodes.data()), words.data(), 32 * (size_t)nn);
    return 0;
}

// The device build's plane-offset reduction on the host (k_oct_offsets).
void octree_offsets_levels(const OctreeHost& t, const float bmin[3], const float bmax[3], double w[3])
{
    std::vector<int32_t> words(8 * t.nodes.size());
    if (!words.empty()) memcpy(words.data(), static_cast<const void*>(t.nodes.data()), 4 * words.size());
    const int32_t* nodes8 = words.data();
    for (int k = 0; k < 3; ++k) {
        const double r0 = bmin[k], cell = octree_cell(t.depth, bmin, bmax, k);
        w[k] = 0.0;
        for (int32_t i = 0; i < (int32_t)t.nodes.size(); ++i) w[k] = oct_node_offset(nodes8, i, k, r0, cell, w[k]);
    }
}

// The crack grid (tmpt_internal.h OctGrid): every node box face lies on a plane
// r0 + j * cell of the finest level to within the largest offset found here
// (the rounding of min + half + half down the tree); the band adds margin for
// the device's float evaluation of the plane and of the hit point.
void octree_grid(const OctreeHost& t, const float bmin[3], const float bmax[3], OctGrid& g)
{
    double w[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        const double r0 = bmin[k], cell = octree_cell(t.depth, bmin, bmax, k);
        for (const OctNode& nd : t.nodes) {
            const double v[2] = {comp(mk(nd.lo.x, nd.lo.y, nd.lo.z), k), comp(mk(nd.hi.x, nd.hi.y, nd.hi.z), k)};
            for (double x : v) w[k] = std::max(w[k], oct_plane_offset(x, r0, cell));
        }
    }
    octree_grid_from_offsets(t.depth, w, bmin, bmax, g);
}

double octree_cell(int32_t depth, const float bmin[3], const float bmax[3], int k)
{
    const double scale = std::ldexp(1.0, depth);
    const double size = (double)bmax[k] - (double)bmin[k];
    return size > 0.0 ? size / scale : 1.0;
}

// The grid from the largest plane offset per axis (a max over all node boxes,
// exact in any order: the device build reduces it, tmpt_octree_dev.hip).
void octree_grid_from_offsets(int32_t depth, const double wmax[3], const float bmin[3], const float bmax[3], OctGrid& g)
{
    float cmin = INFINITY;
    for (int k = 0; k < 3; ++k) {
        const double cell = octree_cell(depth, bmin, bmax, k);
        const double w = wmax[k];
        const float ulp = std::nextafter(std::max(std::fabs(bmin[k]), std::fabs(bmax[k])), INFINITY) -
                          std::max(std::fabs(bmin[k]), std::fabs(bmax[k]));
        g.r0[k] = bmin[k];
        g.cell[k] = (float)cell;
        g.inv_cell[k] = (float)(1.0 / cell);
        g.band[k] = (float)(4.0 * w + 8.0 * (double)ulp);
        g.drift[k] = 2.0f * g.band[k];
        cmin = std::min(cmin, (float)cell);
    }
    g.reach = 0.5f * cmin;
}

// Distance of x to the nearest plane of axis k, as the device evaluates it
// (tmpt_traverse.h octree_crack), and that plane's number.
static float plane_dist(const OctGrid& g, int k, float x, float& j)
{
    const float rel = x - g.r0[k];
    j = rintf(rel * g.inv_cell[k]);
    return fabsf(fmaf(-j, g.cell[k], rel));
}

// Triangles the reference's octree may not hold where a ray hits them (DESIGN.md
// section 2, "the derived bound"): (F1) all three vertices within 2 band of one
// plane -- the triangle can lie in a crack, in no leaf at all; (F2) a triangle
// nearly parallel to a plane family that comes within band of one of its
// planes: its plane leaves the 2-band slab around that plane only beyond
// `reach` of a point inside it (sin(angle) * reach <= 2 band), so near such a
// point it may meet neither leaf either side of the crack robustly.
int32_t octree_flat_triangles(const float* tris9, int32_t n, const OctGrid& g, std::vector<uint8_t>& flat)
{
    flat.assign((size_t)n, 0);
    int32_t count = 0;
    for (int32_t i = 0; i < n; ++i) {
        const float* v = tris9 + 9 * (size_t)i;
        for (int k = 0; k < 3 && !flat[(size_t)i]; ++k) {  // F1
            float j0, j1, j2;
            const float d0 = plane_dist(g, k, v[k], j0), d1 = plane_dist(g, k, v[3 + k], j1),
                        d2 = plane_dist(g, k, v[6 + k], j2);
            const float lim = 2.0f * g.band[k];
            if (j0 == j1 && j1 == j2 && d0 <= lim && d1 <= lim && d2 <= lim) flat[(size_t)i] = 1;
        }
        if (!flat[(size_t)i]) {  // F2
            const double e1[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
            const double e2[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
            const double nr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                                  e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = std::sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
            for (int k = 0; k < 3 && len > 0.0 && !flat[(size_t)i]; ++k) {
                const double nk = std::fabs(nr[k]) / len, sin_a = std::sqrt(std::max(0.0, 1.0 - nk * nk));
                if (sin_a * (double)g.reach > 2.0 * (double)g.band[k]) continue;
                const double lo = std::min({(double)v[k], (double)v[3 + k], (double)v[6 + k]}) - g.band[k];
                const double hi = std::max({(double)v[k], (double)v[3 + k], (double)v[6 + k]}) + g.band[k];
                // a plane r0 + j cell inside [lo, hi]
                if (std::floor((hi - g.r0[k]) / g.cell[k]) >= std::ceil((lo - g.r0[k]) / g.cell[k])) flat[(size_t)i] = 1;
            }
        }
        count += flat[(size_t)i];
    }
    return count;
}

uint64_t octree_digest(const OctreeHost& t)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint32_t w) {
        for (int b = 0; b < 4; ++b) h = (h ^ ((w >> (8 * b)) & 255u)) * 1099511628211ull;
    };
    auto fbits = [](float f) {
        uint32_t u;
        memcpy(&u, &f, 4);
        return u;
    };
    for (const OctNode& nd : t.nodes) {
        mix(fbits(nd.lo.x)), mix(fbits(nd.lo.y)), mix(fbits(nd.lo.z));
        mix(fbits(nd.hi.x)), mix(fbits(nd.hi.y)), mix(fbits(nd.hi.z));
        const int32_t r = bits_int(nd.hi.w);
        mix(r < 0 ? 0u : 1u);
        if (r >= 0)
            for (int32_t k = 0; k <= t.refs[(size_t)r]; ++k) mix((uint32_t)t.refs[(size_t)r + (size_t)k]);
    }
    return h;
}

}  // namespace tmpt
