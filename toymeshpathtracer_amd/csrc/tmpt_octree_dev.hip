// tmpt_octree_dev.hip -- the reference's octree built on the device (option
// octree_build=device): the same nodes, skip links and leaf lists, word for
// word, as tmpt_octree.cpp's host recursion makes.
//
// A level-order build (tmpt_octree_build.h states the passes and their
// arrays; every kernel here is one of its pass functions called for the
// thread's index, and tmpt_octree.cpp build_octree_levels runs the same
// functions in host loops):
//   per level d:  k_oct_classify, two scans        split rule, children's numbers
//                 [host reads the split nodes and their list entries]
//                 k_oct_children                   child boxes (oct_child_box)
//                 k_oct_overlap, one scan          the 8 overlap flags of every list entry
//                 k_oct_child_lists                children's list starts and counts
//                 [host reads the next level's list size]
//                 k_oct_scatter                    the children's lists, stable
//   bottom-up:    k_oct_sizes per level            subtree nodes and reference words
//                 [host reads the root's totals]
//   top-down:     k_oct_preorder per level         preorder index, list offset
//   per level:    k_oct_emit_nodes, k_oct_emit_entries   the OctNode records and refs
//                 k_oct_offsets                    largest plane offset per axis (float64 max)
// The kernel boundary is the only synchronisation between workgroups; lists
// are placed by prefix sums, never by atomics, so two builds are equal raw.
// The one atomic is the float64 max of k_oct_offsets, exact in any order.
//
// Memory: the levels' arrays are bump-allocated from chunks the scene keeps
// (Scene::oct_scratch) and the flag array from one kept buffer
// (Scene::oct_flags), so a second build of a scene of like size allocates only
// its result.  Everything is charged against option octree_dev_max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "tmpt_internal.h"
#include "tmpt_octree_build.h"

namespace tmpt {

namespace {

constexpr int kOB = 256;  // threads per block of every pass
constexpr int kScanItems = 8, kScanTile = kOB * kScanItems;

inline unsigned oct_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ------------------------------------------------------------------ scan
// Exclusive scan of n words in place: each block scans its tile of kScanTile
// words and leaves the tile's total in sums; the totals are scanned the same
// way and added back.
__global__ void __launch_bounds__(kOB) k_oct_scan_tile(uint32_t* __restrict__ data, int64_t n, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t sh[kOB];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)t * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = base + j < n ? data[base + j] : 0u;
        sum += v[j];
    }
    sh[t] = sum;
    __syncthreads();
    for (int off = 1; off < kOB; off <<= 1) {
        const uint32_t x = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    uint32_t run = sh[t] - sum;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (base + j < n) data[base + j] = run;
        run += v[j];
    }
    if (t == kOB - 1) sums[blockIdx.x] = sh[kOB - 1];
}

__global__ void __launch_bounds__(kOB) k_oct_scan_add(uint32_t* __restrict__ data, int64_t n, const uint32_t* __restrict__ sums)
{
    const uint32_t add = sums[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) data[base + j] += add;
}

// ------------------------------------------------------------------ passes
__global__ void __launch_bounds__(kOB) k_oct_root(OctLevel L, float3 lo, float3 hi, int32_t n)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i == 0) {
        oct_st3(L.lo, 0, mk(lo.x, lo.y, lo.z));
        oct_st3(L.hi, 0, mk(hi.x, hi.y, hi.z));
        L.start[0] = 0;
        L.cnt[0] = n;
        L.idx[0] = 0;
        L.roff[0] = 0;
    }
    if (i < n) {
        L.ids[i] = i;  // BuildOctree: the scene's triangle order
        L.owner[i] = 0;
    }
}

__global__ void __launch_bounds__(kOB) k_oct_classify(OctLevel L, int depth)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i <= L.n) oct_classify(L, i, depth);
}

__global__ void __launch_bounds__(kOB) k_oct_children(OctLevel P, OctLevel C)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i < P.n) oct_children(P, C, i);
}

__global__ void __launch_bounds__(kOB) k_oct_overlap(OctLevel P, OctLevel C, const float* __restrict__ tris, int stride,
                                                     uint32_t* __restrict__ F, int64_t f_last)
{
    const int32_t e = blockIdx.x * kOB + threadIdx.x;
    if (e == 0) F[f_last] = 0u;
    if (e < P.m) oct_overlap(P, C, tris, stride, F, e);
}

__global__ void __launch_bounds__(kOB) k_oct_child_lists(OctLevel P, OctLevel C, const uint32_t* __restrict__ F)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i < P.n) oct_child_lists(P, C, F, i);
}

__global__ void __launch_bounds__(kOB) k_oct_scatter(OctLevel P, OctLevel C, const uint32_t* __restrict__ F)
{
    const int32_t e = blockIdx.x * kOB + threadIdx.x;
    if (e < P.m) oct_scatter(P, C, F, e);
}

__global__ void __launch_bounds__(kOB) k_oct_sizes(OctLevel P, OctLevel C)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i < P.n) oct_sizes(P, C, i);
}

__global__ void __launch_bounds__(kOB) k_oct_preorder(OctLevel P, OctLevel C)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i < P.n) oct_preorder(P, C, i);
}

__global__ void __launch_bounds__(kOB) k_oct_emit_nodes(OctLevel L, int32_t* __restrict__ nodes8, int32_t* __restrict__ refs)
{
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    if (i < L.n) oct_emit_node(L, nodes8, refs, i);
}

__global__ void __launch_bounds__(kOB) k_oct_emit_entries(OctLevel L, int32_t* __restrict__ refs)
{
    const int32_t e = blockIdx.x * kOB + threadIdx.x;
    if (e < L.m) oct_emit_entry(L, refs, e);
}

struct Grid3 {
    double r0[3], cell[3];
};

// The largest plane offset per axis over all node boxes: a block's max by an
// LDS tree, then one atomic max per block and axis on the float64 bit
// patterns (the offsets are >= +0 and never NaN, so the patterns order as the
// values do).  A max is exact in any order.
__global__ void __launch_bounds__(kOB) k_oct_offsets(const int32_t* __restrict__ nodes8, int32_t n, Grid3 g,
                                                     unsigned long long* __restrict__ out)
{
    __shared__ double sh[kOB];
    const int32_t i = blockIdx.x * kOB + threadIdx.x;
    for (int q = 0; q < 3; ++q) {
        sh[threadIdx.x] = i < n ? oct_node_offset(nodes8, i, q, g.r0[q], g.cell[q], 0.0) : 0.0;
        __syncthreads();
        for (int off = kOB / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) {
                const double a = sh[threadIdx.x], b = sh[threadIdx.x + off];
                sh[threadIdx.x] = a < b ? b : a;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) atomicMax(out + q, (unsigned long long)__double_as_longlong(sh[0]));
        __syncthreads();
    }
}

// ------------------------------------------------------------------ memory
// Bump allocation from the scene's kept chunks; a chunk that does not fit the
// request is left behind (its tail unused) and the next one tried or made.
struct Arena {
    Scene& s;
    size_t cap;          // bytes the build may hold in all (scratch, flags, result)
    size_t result = 0;   // bytes of the result, once known
    size_t chunk = 0, used = 0;
    bool over = false;   // the last failure was the cap, not the allocator

    size_t held() const
    {
        size_t b = s.oct_flags.bytes() + result;
        for (const auto& c : s.oct_scratch) b += c.bytes();
        return b;
    }
    void* take(size_t bytes)
    {
        bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        for (; chunk < s.oct_scratch.size(); ++chunk, used = 0)
            if (used + bytes <= s.oct_scratch[chunk].bytes()) {
                void* p = static_cast<char*>(s.oct_scratch[chunk].get()) + used;
                used += bytes;
                return p;
            }
        const size_t last = s.oct_scratch.empty() ? 0 : s.oct_scratch.back().bytes();
        size_t want = std::max(bytes, std::max<size_t>(2 * last, (size_t)1 << 20));
        const size_t have = held();
        if (have + want > cap) want = bytes;
        if (have + want > cap) return (over = true, nullptr);
        DeviceBuffer<> c;
        if (!c.alloc(want)) return (over = false, nullptr);
        s.oct_scratch.push_back(std::move(c));
        chunk = s.oct_scratch.size() - 1;
        used = bytes;
        return s.oct_scratch.back().get();
    }
    template <typename T>
    bool take(T*& p, size_t count)
    {
        p = static_cast<T*>(take(sizeof(T) * count));
        return p != nullptr;
    }
    bool flags(size_t bytes)
    {
        if (s.oct_flags.bytes() >= bytes) return true;
        if (held() - s.oct_flags.bytes() + bytes > cap) return (over = true, false);
        // the stream's earlier kernels may still read the old flags
        if (s.oct_flags && hipStreamSynchronize(s.stream) != hipSuccess) return (over = false, false);
        return s.oct_flags.alloc(bytes) ? true : (over = false, false);
    }
};

bool level_nodes(Arena& a, OctLevel& L, size_t n)
{
    L.n = (int32_t)n;
    return a.take(L.lo, 3 * n) && a.take(L.hi, 3 * n) && a.take(L.start, n) && a.take(L.cnt, n) &&
           a.take(L.split, n + 1) && a.take(L.fstart, n + 1) && a.take(L.subn, n) && a.take(L.subr, n) &&
           a.take(L.idx, n) && a.take(L.roff, n);
}
bool level_lists(Arena& a, OctLevel& L, size_t m)
{
    L.m = (int32_t)m;
    return a.take(L.ids, m) && a.take(L.owner, m);
}

bool scan_exclusive(Arena& a, uint32_t* data, int64_t n, hipStream_t st)
{
    const unsigned nb = oct_blocks(n, kScanTile);
    uint32_t* sums = nullptr;
    if (!a.take(sums, nb)) return false;
    k_oct_scan_tile<<<nb, kOB, 0, st>>>(data, n, sums);
    if (nb > 1) {
        if (!scan_exclusive(a, sums, (int64_t)nb, st)) return false;
        k_oct_scan_add<<<nb, kOB, 0, st>>>(data, n, sums);
    }
    return true;
}

}  // namespace

int build_octree_device(Scene& s, const float bmin[3], const float bmax[3], Octree& o, double wmax[3])
{
    const hipStream_t st = s.stream;
    const int32_t n = s.bvh.n;
    const size_t chunks_before = s.oct_scratch.size();
    const bool flags_before = (bool)s.oct_flags;
    size_t held = s.oct_flags.bytes();
    for (const auto& c : s.oct_scratch) held += c.bytes();
    Arena a{s, s.opt.octree_dev_max > 0.0 ? (size_t)s.opt.octree_dev_max : free_budget(1, 2, held)};
    // on any failure: what this call added to the kept scratch is released, the
    // stream drained first (its kernels may still use it)
    auto fail = [&](int rc, const std::string& msg) {
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        s.oct_scratch.resize(chunks_before);
        if (!flags_before) s.oct_flags.reset();
        o = Octree{};
        set_error(msg);
        return rc;
    };
    auto no_mem = [&]() {
        return fail(-12, a.over ? "tmpt_scene_build_octree: the device build needs more than octree_dev_max allows (" +
                                      std::to_string(a.cap) + " bytes); the scene keeps its octree"
                                : std::string("tmpt_scene_build_octree: out of device memory in the device build; the "
                                              "scene keeps its octree"));
    };
    auto hip_fail = [&](hipError_t e) { return fail(-1, std::string("tmpt_scene_build_octree: ") + hipGetErrorString(e)); };
#define OCT_HIP(call)                                  \
    do {                                               \
        const hipError_t e_ = (call);                  \
        if (e_ != hipSuccess) return hip_fail(e_);     \
    } while (0)

    // the triangles as the scene keeps them: TriOrig's first 9 floats are v0, v1, v2
    static_assert(sizeof(TriOrig) == 48, "12 floats per record");
    const float* tris = reinterpret_cast<const float*>(s.bvh.tri_orig.get());
    const int stride = (int)(sizeof(TriOrig) / sizeof(float));

    std::vector<OctLevel> lv(1);
    if (!level_nodes(a, lv[0], 1) || !level_lists(a, lv[0], (size_t)n)) return no_mem();
    k_oct_root<<<std::max(1u, oct_blocks(n, kOB)), kOB, 0, st>>>(lv[0], make_float3(bmin[0], bmin[1], bmin[2]),
                                                                 make_float3(bmax[0], bmax[1], bmax[2]), n);
    int32_t leaves = 0;
    for (int d = 0;; ++d) {
        const OctLevel P = lv[(size_t)d];
        k_oct_classify<<<oct_blocks((int64_t)P.n + 1, kOB), kOB, 0, st>>>(P, d);
        if (!scan_exclusive(a, P.split, (int64_t)P.n + 1, st) || !scan_exclusive(a, P.fstart, (int64_t)P.n + 1, st))
            return no_mem();
        uint32_t tot[2] = {0, 0};  // split nodes, their list entries
        OCT_HIP(hipGetLastError());
        OCT_HIP(hipMemcpyAsync(&tot[0], P.split + P.n, 4, hipMemcpyDeviceToHost, st));
        OCT_HIP(hipMemcpyAsync(&tot[1], P.fstart + P.n, 4, hipMemcpyDeviceToHost, st));
        OCT_HIP(hipStreamSynchronize(st));
        leaves += P.n - (int32_t)tot[0];
        if (!tot[0]) break;
        const uint64_t n_child = 8 * (uint64_t)tot[0], n_flag = 8 * (uint64_t)tot[1] + 1;
        if (n_child >= (uint64_t)INT32_MAX || n_flag >= (uint64_t)INT32_MAX)
            return fail(-22, "tmpt_scene_build_octree: octree too large");
        OctLevel C{};
        if (!level_nodes(a, C, (size_t)n_child) || !a.flags(4 * (size_t)n_flag)) return no_mem();
        uint32_t* F = s.oct_flags;
        k_oct_children<<<oct_blocks(P.n, kOB), kOB, 0, st>>>(P, C);
        k_oct_overlap<<<oct_blocks(P.m, kOB), kOB, 0, st>>>(P, C, tris, stride, F, (int64_t)n_flag - 1);
        if (!scan_exclusive(a, F, (int64_t)n_flag, st)) return no_mem();
        k_oct_child_lists<<<oct_blocks(P.n, kOB), kOB, 0, st>>>(P, C, F);
        uint32_t m_child = 0;
        OCT_HIP(hipGetLastError());
        OCT_HIP(hipMemcpyAsync(&m_child, F + (n_flag - 1), 4, hipMemcpyDeviceToHost, st));
        OCT_HIP(hipStreamSynchronize(st));
        if (!level_lists(a, C, (size_t)m_child)) return no_mem();
        k_oct_scatter<<<oct_blocks(P.m, kOB), kOB, 0, st>>>(P, C, F);
        lv.push_back(C);
    }
    const int depth = (int)lv.size() - 1;
    for (int d = depth; d >= 0; --d)
        k_oct_sizes<<<oct_blocks(lv[(size_t)d].n, kOB), kOB, 0, st>>>(lv[(size_t)d], d < depth ? lv[(size_t)d + 1] : OctLevel{});
    int32_t nn = 0;
    int64_t nr = 0;
    OCT_HIP(hipGetLastError());
    OCT_HIP(hipMemcpyAsync(&nn, lv[0].subn, 4, hipMemcpyDeviceToHost, st));
    OCT_HIP(hipMemcpyAsync(&nr, lv[0].subr, 8, hipMemcpyDeviceToHost, st));
    OCT_HIP(hipStreamSynchronize(st));
    if (nr >= (int64_t)INT32_MAX || nn >= INT32_MAX) return fail(-22, "tmpt_scene_build_octree: octree too large");
    const size_t nb = (size_t)nn * sizeof(OctNode), rb = std::max<size_t>(1, (size_t)nr) * sizeof(int32_t);
    a.result = nb + rb + sizeof(OctView) + 3 * sizeof(unsigned long long);
    if (a.held() > a.cap) return (a.over = true, no_mem());
    unsigned long long* d_w = nullptr;
    if (!a.take(d_w, 3)) return no_mem();
    if (!o.oct.alloc(nb) || !o.oct_refs.alloc(rb) || !o.oct_view.alloc(sizeof(OctView))) return (a.over = false, no_mem());
    int32_t* nodes8 = reinterpret_cast<int32_t*>(o.oct.get());
    for (int d = 0; d < depth; ++d)
        k_oct_preorder<<<oct_blocks(lv[(size_t)d].n, kOB), kOB, 0, st>>>(lv[(size_t)d], lv[(size_t)d + 1]);
    for (int d = 0; d <= depth; ++d) {
        const OctLevel& L = lv[(size_t)d];
        k_oct_emit_nodes<<<oct_blocks(L.n, kOB), kOB, 0, st>>>(L, nodes8, o.oct_refs);
        if (L.m > 0) k_oct_emit_entries<<<oct_blocks(L.m, kOB), kOB, 0, st>>>(L, o.oct_refs);
    }
    Grid3 g;
    for (int k = 0; k < 3; ++k) {
        g.r0[k] = bmin[k];
        g.cell[k] = octree_cell(depth, bmin, bmax, k);
    }
    OCT_HIP(hipMemsetAsync(d_w, 0, 3 * sizeof(unsigned long long), st));  // +0.0
    k_oct_offsets<<<oct_blocks(nn, kOB), kOB, 0, st>>>(nodes8, nn, g, d_w);
    unsigned long long w_bits[3] = {0, 0, 0};
    OCT_HIP(hipGetLastError());
    OCT_HIP(hipMemcpyAsync(w_bits, d_w, sizeof(w_bits), hipMemcpyDeviceToHost, st));
    OCT_HIP(hipStreamSynchronize(st));
#undef OCT_HIP
    for (int k = 0; k < 3; ++k) wmax[k] = __builtin_bit_cast(double, w_bits[k]);
    o.n_oct = nn;
    o.n_oct_refs = nr;
    o.oct_leaves = leaves;
    o.oct_depth = depth;
    return 0;
}

}  // namespace tmpt
