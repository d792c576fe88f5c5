// tmpt_api.cpp -- the C ABI of include/tmpt.h.  Status ints cross the
// boundary; no exception escapes (every entry point catches).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "tmpt.h"
#include "tmpt_internal.h"
#include "tmpt_traverse.h"
#include "tmpt_render.h"
#include "tmpt_query_key.h"

namespace tmpt {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
const char* last_error() { return g_last_error.c_str(); }

int load_obj(const char* path, std::vector<float>& tris, f3& bmin, f3& bmax);
void camera_init(tmpt_camera* cam, f3 lookFrom, f3 lookAt, f3 vup, float vfov, float aspect,
                 float aperture, float focusDist);
void camera_for_scene(tmpt_camera* cam, f3 sceneMin, f3 sceneMax, int w, int h, bool sponza);
int write_png(const char* path, const uint8_t* rgba, int w, int h);
int render(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* d_out,
           uint64_t* ray_count, float4* d_sums = nullptr);
// tmpt_render.hip: the camera pre-pass alone, its entries copied to host memory (tmpt_camera_rays)
int camera_rays(Scene& s, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* out);
int query_batch(Scene& s, const float* d_rays, int64_t n, float tmin, float tmax, bool any, bool ranged,
                int32_t* d_ids, float* d_hits, float* d_uv, bool wait, uint64_t wait_stream);
int query_wait(Scene& s, uint64_t wait_stream);
int intersect_batch(Scene& s, const float* d_rays, int64_t n, float tmin, float tmax, bool any, bool ranged,
                    float* d_hits, int32_t* d_ids);

// RandomUnitVector's (cos a, sin a) over a key range, as the renderers compute it
__global__ void k_unit_sincos(uint32_t key0, uint32_t n, float2* out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c, s;
    glibc_sincosf_unit(unit_angle((key0 + i) & 0xFFFFFFu), c, s);
    out[i] = make_float2(c, s);
}

// ---------------------------------------------------------------- multi-device gather
// Frame assembly on the root device: the gathered tiles are [rank][max_rows][W]
// (equal-size padded blocks, as ncclGather delivers them); frame row y belongs
// to rank y % nd as its tile row y / nd (1-row bands dealt round-robin).
__global__ void k_assemble_rows(const uint32_t* __restrict__ gathered, int32_t nd, int32_t max_rows, int32_t W,
                                int32_t H, uint32_t* __restrict__ frame)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const int32_t y = (int32_t)(i / W), x = (int32_t)(i - (int64_t)y * W);
    frame[i] = gathered[((int64_t)(y % nd) * max_rows + y / nd) * W + x];
}

// RCCL, resolved at run time (dlopen of librccl.so.1: in a process where torch
// already loaded its RCCL the same library is reused, so there is one RCCL and
// one HIP runtime; the library itself loads without RCCL).
struct Rccl {
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                           hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    bool ok = false;
};

const Rccl& rccl()
{
    static Rccl r = []() {
        Rccl x;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return x;
        x.comm_init_all = (decltype(x.comm_init_all))dlsym(h, "ncclCommInitAll");
        x.comm_destroy = (decltype(x.comm_destroy))dlsym(h, "ncclCommDestroy");
        x.gather = (decltype(x.gather))dlsym(h, "ncclGather");
        x.reduce = (decltype(x.reduce))dlsym(h, "ncclReduce");
        x.group_start = (decltype(x.group_start))dlsym(h, "ncclGroupStart");
        x.group_end = (decltype(x.group_end))dlsym(h, "ncclGroupEnd");
        x.error_string = (decltype(x.error_string))dlsym(h, "ncclGetErrorString");
        x.ok = x.comm_init_all && x.comm_destroy && x.gather && x.reduce && x.group_start && x.group_end &&
               x.error_string;
        return x;
    }();
    return r;
}

// ---------------------------------------------------------------- options
// The keys of include/tmpt.h "Scene options", in one table: name, build-time
// or not, range, and the member they set.
namespace {
struct OptionDef {
    const char* name;
    bool build;
    double lo, hi;
    int Options::*i;
    float Options::*f;
    double Options::*d;
};
const OptionDef kOptions[] = {
    {"builder", true, 0, 1, &Options::builder, nullptr, nullptr},
    {"layout", true, 0, 1, &Options::layout, nullptr, nullptr},
    {"leaf_max", true, 1, kLeafMaxTris, &Options::leaf_max, nullptr, nullptr},
    {"collapse", true, 0, 1, &Options::collapse, nullptr, nullptr},
    {"ploc_radius", true, 1, 256, &Options::ploc_radius, nullptr, nullptr},
    {"sah_c_leaf", true, 0, 1e6, nullptr, &Options::sah_c_leaf, nullptr},
    {"sah_c_tri", true, 0, 1e6, nullptr, &Options::sah_c_tri, nullptr},
    {"sample_base", false, 0, 64512, &Options::sample_base, nullptr, nullptr},
    {"sample_block", false, 0, 1024, &Options::sample_block, nullptr, nullptr},
    {"sample_tail", false, -1, 64, &Options::sample_tail, nullptr, nullptr},
    {"sbuf_max", false, 0, 1e18, nullptr, nullptr, &Options::sbuf_max},
    {"sbuf_pair", false, 0, 1, &Options::sbuf_pair, nullptr, nullptr},
    {"cam_pre", false, -1, 1, &Options::cam_pre, nullptr, nullptr},
    {"cam_pre_max", false, 0, 1e18, nullptr, nullptr, &Options::cam_pre_max},
    {"shadow_split", false, 0, 1, &Options::shadow_split, nullptr, nullptr},
    {"shadow_split_max", false, 0, 1e18, nullptr, nullptr, &Options::shadow_split_max},
    {"shadow_split_pass", false, 0, 1024, &Options::shadow_split_pass, nullptr, nullptr},
    {"pilot", false, -1, 512, &Options::pilot, nullptr, nullptr},
    {"help", false, -1, 1, &Options::help, nullptr, nullptr},
    {"pair", false, -1, 63, &Options::pair, nullptr, nullptr},
    {"balance", false, 0, 1, &Options::balance, nullptr, nullptr},
    {"dprio", false, 0, 1, &Options::dprio, nullptr, nullptr},
    {"wave_cap", false, 0, 64, &Options::wave_cap, nullptr, nullptr},
    {"pixel_chains", false, -1, 1024, &Options::pixel_chains, nullptr, nullptr},
    {"tie_defer", false, -1, 1, &Options::tie_defer, nullptr, nullptr},
    {"redo_cap", false, 0, 1 << 30, &Options::redo_cap, nullptr, nullptr},
    {"redo_inline", false, 0, 1, &Options::redo_inline, nullptr, nullptr},
    {"redo_lanes", false, 1, 64, &Options::redo_lanes, nullptr, nullptr},
    {"path_waves", false, 0, 6, &Options::path_waves, nullptr, nullptr},
    {"top_walk", false, -1, 8, &Options::top_walk, nullptr, nullptr},
    {"shadow_order", false, -1, 2, &Options::shadow_order, nullptr, nullptr},
    {"pop_cull", false, -1, 1, &Options::pop_cull, nullptr, nullptr},
    {"pop_key_cap", false, -1, kPopKeyMax, &Options::pop_key_cap, nullptr, nullptr},
    {"rowspec", false, 0, 1, &Options::rowspec, nullptr, nullptr},
    {"rowspec_wmax", false, 0, 16384, &Options::rowspec_wmax, nullptr, nullptr},
    {"rowspec_windows", false, 0, 32, &Options::rowspec_windows, nullptr, nullptr},
    {"rowspec_spread", false, -1, 100, nullptr, &Options::rowspec_spread, nullptr},
    {"rowspec_groups", false, 1, kRowSpecMaxGroups, &Options::rowspec_groups, nullptr, nullptr},
    {"rowspec_noshadow", false, 0, 1, &Options::rowspec_noshadow, nullptr, nullptr},
    {"rowspec_chase", false, 0, 1, &Options::rowspec_chase, nullptr, nullptr},
    {"rowspec_stream", false, 0, 1, &Options::rowspec_stream, nullptr, nullptr},
    {"rowstream_dynamic", false, 0, 1, &Options::rowstream_dynamic, nullptr, nullptr},
    {"row_flag_leaves", false, 0, 1, &Options::row_flag_leaves, nullptr, nullptr},
    {"row_occ", false, 0, 5, &Options::row_occ, nullptr, nullptr},
    {"wf_bins", false, 1, 8, &Options::wf_bins, nullptr, nullptr},
    {"rowstream_test_abort", false, 0, 1, &Options::rowstream_test_abort, nullptr, nullptr},
    {"tie_rule", false, 0, 1, &Options::tie_rule, nullptr, nullptr},
    {"aov_group", false, 0, 16, &Options::aov_group, nullptr, nullptr},
    {"octree_build", false, 0, 1, &Options::octree_build, nullptr, nullptr},
    {"octree_dev_max", false, 0, 1e18, nullptr, nullptr, &Options::octree_dev_max},
    {"denoise_lds", false, -1, 1, &Options::denoise_lds, nullptr, nullptr},
    {"query_sort", false, -1, 1, &Options::query_sort, nullptr, nullptr},
    {"query_top", false, -1, 1, &Options::query_top, nullptr, nullptr},
    {"query_max", false, 0, 1e18, nullptr, nullptr, &Options::query_max},
    {"query_chunk", false, 64, 1 << 22, &Options::query_chunk, nullptr, nullptr},
    {"query_grid", false, 0, 1 << 20, &Options::query_grid, nullptr, nullptr},
    {"query_legacy", false, 0, 1, &Options::query_legacy, nullptr, nullptr},
    {"motion_tile", false, -1, 1, &Options::motion_tile, nullptr, nullptr},
};

const OptionDef* find_option(const char* key)
{
    for (const OptionDef& d : kOptions)
        if (strcmp(d.name, key) == 0) return &d;
    return nullptr;
}
}  // namespace

int options_set(Options& o, const char* key, double v, bool allow_build)
{
    const OptionDef* d = key ? find_option(key) : nullptr;
    if (!d) {
        set_error(std::string("unknown option '") + (key ? key : "(null)") + "'");
        return -22;
    }
    if (d->build && !allow_build) {
        set_error(std::string("option '") + key + "' is a build option: give it to tmpt_scene_create_ex");
        return -22;
    }
    if (!(v >= d->lo && v <= d->hi)) {
        set_error(std::string("option '") + key + "' out of range [" + std::to_string(d->lo) + ", " +
                  std::to_string(d->hi) + "]");
        return -22;
    }
    if (d->i) {
        if (v != (double)(long long)v) {
            set_error(std::string("option '") + key + "' takes an integer");
            return -22;
        }
        if (strcmp(key, "row_occ") == 0 && v != 0 && v != 4 && v != 5) {
            set_error(std::string("option '") + key + "' takes 0 (auto), 4 or 5");  // waves per SIMD
            return -22;
        }
        if (strcmp(key, "path_waves") == 0 && v != 0 && v != 4 && v != 5 && v != 6) {
            set_error(std::string("option '") + key + "' takes 0 (auto), 4 or 5, or 6 (the shadow split's 6-wave kernels)");  // waves per SIMD
            return -22;
        }
        if (strcmp(key, "aov_group") == 0 && v > 0 && ((long long)v & ((long long)v - 1)) != 0) {
            set_error(std::string("option '") + key + "' out of range: 0 (auto), 1, 2, 4, 8 or 16");  // lanes per pixel
            return -22;
        }
        if ((strcmp(key, "sample_block") == 0 || strcmp(key, "wf_bins") == 0) && v > 0 &&
            ((long long)v & ((long long)v - 1)) != 0) {
            set_error(std::string("option '") + key + "' must be a power of two");
            return -22;
        }
        o.*(d->i) = (int)v;
    } else if (d->f) {
        o.*(d->f) = (float)v;
    } else {
        o.*(d->d) = v;
    }
    return 0;
}

int options_get(const Options& o, const char* key, double* v)
{
    const OptionDef* d = key ? find_option(key) : nullptr;
    if (!d) {
        set_error(std::string("unknown option '") + (key ? key : "(null)") + "'");
        return -22;
    }
    *v = d->i ? (double)(o.*(d->i)) : d->f ? (double)(o.*(d->f)) : o.*(d->d);
    return 0;
}

// "key=value,key=value" (spaces allowed); builder=ploc|lbvh and
// collapse=greedy|sah also take their names
int options_parse(Options& o, const char* text, bool allow_build)
{
    if (!text) return 0;
    std::string t(text);
    size_t pos = 0;
    while (pos <= t.size()) {
        size_t end = t.find(',', pos);
        if (end == std::string::npos) end = t.size();
        std::string item = t.substr(pos, end - pos);
        pos = end + 1;
        item.erase(0, item.find_first_not_of(" \t"));
        item.erase(item.find_last_not_of(" \t") + 1);
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) {
            set_error("option '" + item + "' has no value (key=value)");
            return -22;
        }
        std::string key = item.substr(0, eq), val = item.substr(eq + 1);
        key.erase(key.find_last_not_of(" \t") + 1);
        val.erase(0, val.find_first_not_of(" \t"));
        if (key == "builder" && (val == "ploc" || val == "lbvh")) val = val == "lbvh" ? "1" : "0";
        if (key == "collapse" && (val == "greedy" || val == "sah")) val = val == "sah" ? "1" : "0";
        if (key == "tie_rule" && (val == "visit" || val == "index")) val = val == "index" ? "1" : "0";
        if (key == "octree_build" && (val == "host" || val == "device")) val = val == "device" ? "1" : "0";
        if (key == "layout" && (val == "aos" || val == "soa")) val = val == "soa" ? "1" : "0";
        char* endp = nullptr;
        const double v = strtod(val.c_str(), &endp);
        if (val.empty() || !endp || *endp != '\0') {
            set_error("option '" + key + "': bad value '" + val + "'");
            return -22;
        }
        if (int rc = options_set(o, key.c_str(), v, allow_build)) return rc;
    }
    return 0;
}

}  // namespace tmpt

struct tmpt_scene {
    tmpt::Scene s;
};

using namespace tmpt;

#define TMPT_GUARD_BEGIN try {
#define TMPT_GUARD_END                                  \
    }                                                   \
    catch (const std::bad_alloc&) {                     \
        set_error("out of host memory");                \
        return -1;                                      \
    }                                                   \
    catch (...) {                                       \
        set_error("unexpected C++ exception");          \
        return -1;                                      \
    }

namespace {
int bad(const char* msg)
{
    set_error(msg);
    return -22;
}
}  // namespace

extern "C" {

int tmpt_abi_version(void) { return TMPT_ABI_VERSION; }
const char* tmpt_last_error(void) { return last_error(); }
void tmpt_free(void* p) { free(p); }

int tmpt_unit_sincos(int32_t device, uint32_t key0, uint32_t n, float* out)
{
    TMPT_GUARD_BEGIN
    if (!out && n) return bad("tmpt_unit_sincos: null argument");
    if (n == 0) return 0;
    if (device < 0) {
        for (uint32_t i = 0; i < n; ++i)
            glibc_sincosf_unit(unit_angle((key0 + i) & 0xFFFFFFu), out[2 * (size_t)i], out[2 * (size_t)i + 1]);
        return 0;
    }
    int ndev = 0;
    TMPT_HIP(hipGetDeviceCount(&ndev));
    if (device >= ndev) return bad("tmpt_unit_sincos: no such device");
    TMPT_HIP(hipSetDevice(device));
    DeviceBuffer<float2> d;
    TMPT_ALLOC(d.alloc(sizeof(float2) * (size_t)n), "tmpt_unit_sincos");
    k_unit_sincos<<<(n + 255u) / 256u, 256>>>(key0, n, d.get());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("tmpt_unit_sincos: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
    TMPT_GUARD_END
}

int tmpt_fastdiv(uint32_t divisor, const uint32_t* x, uint64_t n, uint32_t* out, uint32_t mul_shift[2])
{
    TMPT_GUARD_BEGIN
    if (divisor == 0u || divisor >= (1u << 31)) return bad("tmpt_fastdiv: divisor out of range (1 .. 2^31 - 1)");
    if ((!x || !out) && n) return bad("tmpt_fastdiv: null argument");
    const FastDiv f = fastdiv_make(divisor);
    if (mul_shift) {
        mul_shift[0] = f.mul;
        mul_shift[1] = f.shift;
    }
    for (uint64_t i = 0; i < n; ++i) {
        if (x[i] >= (1u << 31)) return bad("tmpt_fastdiv: dividend out of range (below 2^31)");
        out[i] = fastdiv(x[i], f);
    }
    return 0;
    TMPT_GUARD_END
}

int tmpt_load_obj(const char* path, float** out_tris, int32_t* out_n, float out_bmin[3],
                  float out_bmax[3])
{
    TMPT_GUARD_BEGIN
    if (!path || !out_tris || !out_n) return bad("tmpt_load_obj: null argument");
    std::vector<float> tris;
    f3 bmin, bmax;
    int rc = load_obj(path, tris, bmin, bmax);
    if (rc) return rc;
    float* p = (float*)malloc(tris.size() * sizeof(float));
    if (!p) return bad("tmpt_load_obj: out of memory");
    memcpy(p, tris.data(), tris.size() * sizeof(float));
    *out_tris = p;
    *out_n = (int32_t)(tris.size() / 9);
    if (out_bmin) { out_bmin[0] = bmin.x; out_bmin[1] = bmin.y; out_bmin[2] = bmin.z; }
    if (out_bmax) { out_bmax[0] = bmax.x; out_bmax[1] = bmax.y; out_bmax[2] = bmax.z; }
    return 0;
    TMPT_GUARD_END
}

int tmpt_camera_init(tmpt_camera* cam, const float lf[3], const float la[3], const float up[3],
                     float vfov, float aspect, float aperture, float focus_dist)
{
    if (!cam || !lf || !la || !up) return bad("tmpt_camera_init: null argument");
    camera_init(cam, mk(lf[0], lf[1], lf[2]), mk(la[0], la[1], la[2]), mk(up[0], up[1], up[2]),
                vfov, aspect, aperture, focus_dist);
    return 0;
}

int tmpt_camera_for_scene(tmpt_camera* cam, const float bmin[3], const float bmax[3],
                          int32_t width, int32_t height, int32_t is_sponza)
{
    if (!cam || !bmin || !bmax) return bad("tmpt_camera_for_scene: null argument");
    if (width < 1 || height < 1) return bad("tmpt_camera_for_scene: bad size");
    camera_for_scene(cam, mk(bmin[0], bmin[1], bmin[2]), mk(bmax[0], bmax[1], bmax[2]), width,
                     height, is_sponza != 0);
    return 0;
}

int tmpt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tmpt_scene_create(const float* tris, int32_t n, int32_t device, tmpt_scene** out)
{
    return tmpt_scene_create_ex(tris, n, device, nullptr, out);
}

int tmpt_scene_create_ex(const float* tris, int32_t n, int32_t device, const char* options, tmpt_scene** out)
{
    TMPT_GUARD_BEGIN
    if (!out || n < 0 || (n > 0 && !tris)) return bad("tmpt_scene_create: bad arguments");
    *out = nullptr;
    (void)hipGetLastError();  // a failed call before this one must not fail the build's checks
    Options opt;
    if (int rc = options_parse(opt, options, true)) {
        set_error(std::string("tmpt_scene_create: ") + last_error());
        return rc;
    }
    int ndev = 0;
    TMPT_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return bad("tmpt_scene_create: no such device");
    TMPT_HIP(hipSetDevice(device));
    tmpt_scene* h = new tmpt_scene();
    Scene& s = h->s;
    s.opt = opt;
    s.device = device;
    s.bvh.n = n;
    auto fail = [&](int rc) {
        tmpt_scene_destroy(h);
        return rc;
    };
    if (s.stream.ensure(hipStreamNonBlocking) != hipSuccess) return fail((set_error("tmpt_scene_create: no stream"), -1));
    DeviceBuffer<float> d_tris;
    if (n > 0) {
        if (!d_tris.alloc(sizeof(float) * 9 * (size_t)n))
            return fail((set_error("tmpt_scene_create: out of device memory"), -1));
        if (hipMemcpy(d_tris, tris, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
            return fail((set_error("tmpt_scene_create: upload failed"), -1));
    }
    // Scene::Scene's copy (scene.cpp:54-57): the octree's input, and the split references'
    s.tris_host.assign(tris, tris + 9 * (size_t)n);
    const int rc = build_lbvh(s.bvh, s.opt, s.stream, d_tris);
    d_tris.reset();
    if (rc) return fail(rc);
    *out = h;
    return 0;
    TMPT_GUARD_END
}

int tmpt_scene_destroy(tmpt_scene* h)
{
    if (!h) return 0;
    Scene& s = h->s;
    (void)hipSetDevice(s.device);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    for (auto& st : s.rs_stream)  // the speculative row engine's group streams
        if (st) (void)hipStreamSynchronize(st);
    delete h;
    return 0;
}

int tmpt_scene_build_octree(tmpt_scene* h, const float bmin[3], const float bmax[3])
{
    TMPT_GUARD_BEGIN
    if (!h || !bmin || !bmax) return bad("tmpt_scene_build_octree: null argument");
    Scene& s = h->s;
    if ((int64_t)s.tris_host.size() != 9 * (int64_t)s.bvh.n) return bad("tmpt_scene_build_octree: no triangle copy");
    TMPT_HIP(hipSetDevice(s.device));
    const auto t0 = std::chrono::steady_clock::now();
    OctreeHost t;
    Octree o;
    const bool on_device = s.opt.octree_build == 1;
    double wmax[3] = {0.0, 0.0, 0.0};
    if (on_device) {
        // the level-order build on the scene's stream, from the triangles the
        // scene keeps on the device; a failure leaves the scene as it was
        (void)hipGetLastError();
        if (int rc = build_octree_device(s, bmin, bmax, o, wmax)) return rc;
    } else {
        build_octree(s.tris_host.data(), s.bvh.n, bmin, bmax, t);
        if (t.refs.size() >= (size_t)INT32_MAX || t.nodes.size() >= (size_t)INT32_MAX)
            return bad("tmpt_scene_build_octree: octree too large");
        const size_t nb = t.nodes.size() * sizeof(OctNode), rb = std::max<size_t>(1, t.refs.size()) * sizeof(int32_t);
        if (!o.oct.alloc(nb) || !o.oct_refs.alloc(rb) || !o.oct_view.alloc(sizeof(OctView)) ||
            hipMemcpy(o.oct, t.nodes.data(), nb, hipMemcpyHostToDevice) != hipSuccess ||
            (t.refs.size() && hipMemcpy(o.oct_refs, t.refs.data(), t.refs.size() * sizeof(int32_t), hipMemcpyHostToDevice) !=
                                  hipSuccess))
            return (set_error("tmpt_scene_build_octree: out of device memory"), -1);
    }
    if (ensure_counters(s)) return -1;
    if (s.stream) (void)hipStreamSynchronize(s.stream);  // a render in flight may still read the old one
    // the crack grid and the flat triangles (tmpt_internal.h OctGrid), marked
    // in the BVH's triangle records so that a hit on one flags its query
    if (on_device)
        octree_grid_from_offsets(o.oct_depth, wmax, bmin, bmax, o.oct_grid);
    else
        octree_grid(t, bmin, bmax, o.oct_grid);
    std::vector<uint8_t> flat;
    o.oct_flat = octree_flat_triangles(s.tris_host.data(), s.bvh.n, o.oct_grid, flat);
    if (mark_flat_triangles(s, flat)) return -1;
    if (!on_device) {
        o.n_oct = (int32_t)t.nodes.size();
        o.n_oct_refs = (int64_t)t.refs.size();
        o.oct_leaves = t.leaves;
        o.oct_depth = t.depth;
    }
    const OctView ov{o.oct, o.oct_refs, o.n_oct, o.oct_flat, s.ties, o.oct_grid, o.n_oct_refs};
    if (hipMemcpy(o.oct_view, &ov, sizeof(ov), hipMemcpyHostToDevice) != hipSuccess) {
        // the previous octree (if any) stays in use: give the records back its
        // own flat marks (none without one), so marks and octree agree
        std::vector<uint8_t> old_flat((size_t)s.bvh.n, 0);
        if (s.octree.oct) (void)octree_flat_triangles(s.tris_host.data(), s.bvh.n, s.octree.oct_grid, old_flat);
        (void)mark_flat_triangles(s, old_flat);
        return (set_error("tmpt_scene_build_octree: upload failed"), -1);
    }
    for (int c = 0; c < 3; ++c) {
        o.oct_lo[c] = bmin[c];
        o.oct_hi[c] = bmax[c];
    }
    o.oct_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s.octree = std::move(o);
    return 0;
    TMPT_GUARD_END
}

int tmpt_scene_update(tmpt_scene* h, const float* tris, int32_t n, int32_t mode)
{
    TMPT_GUARD_BEGIN
    if (mode != TMPT_UPDATE_REFIT && mode != TMPT_UPDATE_REBUILD)
        return bad("tmpt_scene_update: mode is TMPT_UPDATE_REFIT (0) or TMPT_UPDATE_REBUILD (1)");
    if (n < 0) return bad("tmpt_scene_update: n < 0");
    if (n > 0 && !tris) return bad("tmpt_scene_update: null triangles with n > 0");
    if (!h) return bad("tmpt_scene_update: null scene");
    Scene& s = h->s;
    if (mode == TMPT_UPDATE_REFIT && n != s.bvh.n)
        return bad("tmpt_scene_update: a refit keeps the triangle count (n differs from the scene's); rebuild instead");
    TMPT_HIP(hipSetDevice(s.device));
    (void)hipGetLastError();  // a failed call before this one must not fail this one's checks
    TMPT_HIP(hipStreamSynchronize(s.stream));  // a render in flight may still read the tree
    for (auto& e : s.update_ev) TMPT_HIP(e.ensure());
    const size_t bytes = sizeof(float) * 9 * (size_t)n;
    DeviceBuffer<float> d_tris;
    if (n > 0 && !d_tris.alloc(bytes)) return (set_error("tmpt_scene_update: out of device memory"), -1);
    if (hipEventRecord(s.update_ev[0], s.stream) != hipSuccess) return (set_error("tmpt_scene_update: event failed"), -1);
    if (n > 0 && hipMemcpyAsync(d_tris, tris, bytes, hipMemcpyHostToDevice, s.stream) != hipSuccess)
        return (set_error("tmpt_scene_update: upload failed"), -1);
    if (mode == TMPT_UPDATE_REFIT) {
        // every record is written anew with its flat mark clear; a failure here is a
        // HIP error, after which the tree is whatever the launches left
        if (int rc = refit_bvh(s.bvh, s.stream, d_tris)) return rc;
    } else {
        // the full build into fresh allocations, on the scene's stream and with
        // its build options; swapped in only on success
        Bvh t;
        t.n = n;
        const int rc = build_lbvh(t, s.opt, s.stream, d_tris);
        if (rc) {
            const std::string why = last_error();
            (void)hipStreamSynchronize(s.stream);
            t = Bvh{};
            (void)hipGetLastError();
            set_error(why);
            return rc;
        }
        s.bvh = std::move(t);
    }
    hipError_t e = hipEventRecord(s.update_ev[1], s.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, s.update_ev[0], s.update_ev[1]);
    d_tris.reset();
    if (e != hipSuccess) {
        set_error(std::string("tmpt_scene_update: ") + hipGetErrorString(e));
        return -1;
    }
    s.tris_host.assign(tris, tris + 9 * (size_t)n);
    s.octree = Octree{};  // exactly as if none had been built; a refit and a rebuild both wrote every record's flat mark anew
    s.prog_key[6] = -1;  // the carried sums belong to the old triangles: spp_begin > 0 fails next
    s.update_kind = mode == TMPT_UPDATE_REFIT ? 1 : 2;
    s.update_ms = (double)ms;
    s.cost_known = false;
    return 0;
    TMPT_GUARD_END
}

int tmpt_octree_bounds(const float bmin[3], const float bmax[3], float box[6])
{
    if (!bmin || !bmax || !box) return bad("tmpt_octree_bounds: null argument");
    const f3 lo = mk(bmin[0], bmin[1], bmin[2]), hi = mk(bmax[0], bmax[1], bmax[2]);
    const f3 extra = (hi - lo) * 0.7f;  // main.cpp:296-297
    const f3 a = lo - extra, b = hi + extra;  // main.cpp:312
    box[0] = a.x, box[1] = a.y, box[2] = a.z, box[3] = b.x, box[4] = b.y, box[5] = b.z;
    return 0;
}

int tmpt_octree_digest(const float* tris, int32_t n, const float bmin[3], const float bmax[3], uint64_t out[5])
{
    TMPT_GUARD_BEGIN
    if (n < 0 || (n > 0 && !tris) || !bmin || !bmax || !out) return bad("tmpt_octree_digest: bad arguments");
    OctreeHost t;
    build_octree(tris, n, bmin, bmax, t);
    out[0] = t.nodes.size();
    out[1] = (uint64_t)t.leaves;
    out[2] = t.refs.size() - (uint64_t)t.leaves;  // triangle references (the count words excluded)
    out[3] = (uint64_t)t.depth;
    out[4] = octree_digest(t);
    return 0;
    TMPT_GUARD_END
}

namespace {
void grid_floats(const OctGrid& g, float out[16])
{
    static_assert(sizeof(OctGrid) == 16 * sizeof(float), "OctGrid is 16 floats");
    memcpy(out, &g, sizeof(OctGrid));
}
}  // namespace

int tmpt_scene_dump_octree(const tmpt_scene* hc, uint32_t* nodes, uint64_t node_words, uint32_t* refs,
                           uint64_t ref_words, int64_t info[5], float grid[16])
{
    TMPT_GUARD_BEGIN
    if (!hc) return bad("tmpt_scene_dump_octree: null scene");
    if (!info) return bad("tmpt_scene_dump_octree: null info");
    if ((nodes == nullptr) != (refs == nullptr)) return bad("tmpt_scene_dump_octree: nodes and refs go together");
    Scene& s = const_cast<tmpt_scene*>(hc)->s;
    const Octree& o = s.octree;
    const bool have = (bool)o.oct;
    const uint64_t nw = have ? 8 * (uint64_t)o.n_oct : 0, rw = have ? (uint64_t)o.n_oct_refs : 0;
    if (nodes && node_words < nw) return bad("tmpt_scene_dump_octree: node buffer too small");
    if (nodes && ref_words < rw) return bad("tmpt_scene_dump_octree: reference buffer too small");
    info[0] = have ? o.n_oct : 0;
    info[1] = have ? o.oct_leaves : 0;
    info[2] = (int64_t)rw;
    info[3] = have ? o.oct_depth : 0;
    info[4] = have ? o.oct_flat : 0;
    if (grid) grid_floats(have ? o.oct_grid : OctGrid{}, grid);
    if (!nodes || !have) return 0;
    TMPT_HIP(hipSetDevice(s.device));
    TMPT_HIP(hipStreamSynchronize(s.stream));
    if (nw) TMPT_HIP(hipMemcpy(nodes, o.oct, 4 * nw, hipMemcpyDeviceToHost));
    if (rw) TMPT_HIP(hipMemcpy(refs, o.oct_refs, 4 * rw, hipMemcpyDeviceToHost));
    return 0;
    TMPT_GUARD_END
}

int tmpt_octree_arrays(const float* tris, int32_t n, const float bmin[3], const float bmax[3], int32_t method,
                       uint32_t* nodes, uint64_t node_words, uint32_t* refs, uint64_t ref_words, int64_t info[5],
                       float grid[16])
{
    TMPT_GUARD_BEGIN
    if (n < 0) return bad("tmpt_octree_arrays: n < 0");
    if (n > 0 && !tris) return bad("tmpt_octree_arrays: null triangles with n > 0");
    if (!bmin || !bmax) return bad("tmpt_octree_arrays: null bounds");
    if (method != 0 && method != 1) return bad("tmpt_octree_arrays: method is 0 (recursion) or 1 (level-order passes)");
    if (!info) return bad("tmpt_octree_arrays: null info");
    if ((nodes == nullptr) != (refs == nullptr)) return bad("tmpt_octree_arrays: nodes and refs go together");
    OctreeHost t;
    OctGrid g;
    if (method == 0) {
        build_octree(tris, n, bmin, bmax, t);
        if (t.refs.size() >= (size_t)INT32_MAX || t.nodes.size() >= (size_t)INT32_MAX)
            return bad("tmpt_octree_arrays: octree too large");
        octree_grid(t, bmin, bmax, g);
    } else {
        if (build_octree_levels(tris, n, bmin, bmax, t)) return bad("tmpt_octree_arrays: octree too large");
        double w[3];
        octree_offsets_levels(t, bmin, bmax, w);
        octree_grid_from_offsets(t.depth, w, bmin, bmax, g);
    }
    const uint64_t nw = 8 * (uint64_t)t.nodes.size(), rw = t.refs.size();
    if (nodes && node_words < nw) return bad("tmpt_octree_arrays: node buffer too small");
    if (nodes && ref_words < rw) return bad("tmpt_octree_arrays: reference buffer too small");
    std::vector<uint8_t> flat;
    info[0] = (int64_t)t.nodes.size();
    info[1] = t.leaves;
    info[2] = (int64_t)rw;
    info[3] = t.depth;
    info[4] = octree_flat_triangles(tris, n, g, flat);
    if (grid) grid_floats(g, grid);
    if (nodes) {
        memcpy(nodes, static_cast<const void*>(t.nodes.data()), 4 * nw);
        if (rw) memcpy(refs, t.refs.data(), 4 * rw);
    }
    return 0;
    TMPT_GUARD_END
}

int tmpt_octree_flags(const float* tris, int32_t n, const float bmin[3], const float bmax[3], const float* rays,
                      const float* t, const int32_t* ids, int64_t n_rays, uint8_t* flags, float grid[13])
{
    TMPT_GUARD_BEGIN
    if (n < 0 || (n > 0 && !tris) || !bmin || !bmax || n_rays < 0 || (n_rays > 0 && (!rays || !t || !ids || !flags)))
        return bad("tmpt_octree_flags: bad arguments");
    OctreeHost oh;
    build_octree(tris, n, bmin, bmax, oh);
    OctGrid g;
    octree_grid(oh, bmin, bmax, g);
    std::vector<uint8_t> flat;
    octree_flat_triangles(tris, n, g, flat);
    for (int64_t i = 0; i < n_rays; ++i) {
        const float* r = rays + 6 * i;
        const int32_t id = ids[i];
        uint8_t f = 0;
        if (id >= 0 && id < n)
            f = (uint8_t)(flat[(size_t)id] | (octree_crack(g, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), t[i]) ? 2 : 0));
        flags[i] = f;
    }
    if (grid) {
        for (int k = 0; k < 3; ++k) {
            grid[k] = g.r0[k];
            grid[3 + k] = g.inv_cell[k];
            grid[6 + k] = g.cell[k];
            grid[9 + k] = g.band[k];
        }
        grid[12] = g.reach;
    }
    return 0;
    TMPT_GUARD_END
}

int tmpt_scene_set_option(tmpt_scene* h, const char* key, double value)
{
    TMPT_GUARD_BEGIN
    if (!h) return bad("tmpt_scene_set_option: null scene");
    Scene& s = h->s;
    const int base = s.opt.sample_base;
    const int rc = options_set(s.opt, key, value, false);
    if (s.opt.sample_base != base) {
        // another window of every pixel's stream: the jump tables are rebuilt by the
        // next sample-seeded call, and carried sums belong to the old window, as
        // they would to another camera (spp_begin > 0 fails next)
        s.jt_spp = 0;
        s.prog_key[6] = -1;
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_scene_get_option(const tmpt_scene* h, const char* key, double* value)
{
    TMPT_GUARD_BEGIN
    if (!h || !value) return bad("tmpt_scene_get_option: null argument");
    if (key && strcmp(key, "pop_key_bits") == 0) {  // read-only: the scene's layout under pop_key_cap
        *value = (double)pop_key_bits(h->s.bvh.link_bits, h->s.opt.pop_key_cap);
        return 0;
    }
    if (key && strcmp(key, "cam_rays_used") == 0) {  // read-only: the last render ran the camera pre-pass
        *value = (double)h->s.cam_rays_used;
        return 0;
    }
    if (key && strcmp(key, "shadow_split_used") == 0) {  // read-only: passes of the last render the shadow split ran
        *value = (double)h->s.split_used;
        return 0;
    }
    if (key && strcmp(key, "path_waves_used") == 0) {  // read-only: waves per SIMD of the last render's path kernel
        *value = (double)h->s.path_waves_used;
        return 0;
    }
    if (key && strcmp(key, "shadow_split_resolve_ms") == 0) {  // read-only: k_split_resolve's time in that render
        *value = h->s.split_resolve_ms;
        return 0;
    }
    if (key && strcmp(key, "update_kind") == 0) {  // read-only: 0 none since creation, 1 refit, 2 rebuild
        *value = (double)h->s.update_kind;
        return 0;
    }
    if (key && strcmp(key, "update_ms") == 0) {  // read-only: device time of the last tmpt_scene_update
        *value = h->s.update_ms;
        return 0;
    }
    if (key && strcmp(key, "live_device_objects") == 0) {  // read-only: the process's live tmpt_device.h owners
        *value = (double)g_live_device_objects.load();
        return 0;
    }
    // read-only, of the last tmpt_scene_hit_device: device time, the keys + sort share, chunks, whether it sorted
    if (key && strcmp(key, "query_ms") == 0) return (*value = h->s.query_ms, 0);
    if (key && strcmp(key, "query_sort_ms") == 0) return (*value = h->s.query_sort_ms, 0);
    if (key && strcmp(key, "query_chunks") == 0) return (*value = (double)h->s.query_chunks, 0);
    if (key && strcmp(key, "query_sorted") == 0) return (*value = (double)h->s.query_sorted, 0);
    if (key && strcmp(key, "bvh_cost") == 0) {  // read-only: the tree's surface-area cost, cached until an update
        Scene& s = const_cast<tmpt_scene*>(h)->s;
        if (!s.cost_known) {
            TMPT_HIP(hipSetDevice(s.device));
            if (int rc = bvh_cost(s, &s.cost)) return rc;
            s.cost_known = true;
        }
        *value = s.cost;
        return 0;
    }
    return options_get(h->s.opt, key, value);
    TMPT_GUARD_END
}

namespace {
// the batched HitScene: stride 6 (one range) or 8 (per-ray tmin, tmax)
int scene_hit(const tmpt_scene* hc, const float* rays, int64_t n, float tmin, float tmax, bool ranged,
              int32_t any_hit, float* hits, int32_t* ids)
{
    if (!hc || n < 0 || (n > 0 && (!rays || !hits || !ids))) return bad("tmpt_scene_hit: bad arguments");
    if (n == 0) return 0;
    const size_t rs = ranged ? 32 : 24;
    Scene& s = const_cast<tmpt_scene*>(hc)->s;
    TMPT_HIP(hipSetDevice(s.device));
    DeviceBuffer<float> d_rays, d_hits;
    DeviceBuffer<int32_t> d_ids;
    if (!d_rays.alloc(rs * (size_t)n) || !d_hits.alloc(28 * (size_t)n) || !d_ids.alloc(4 * (size_t)n))
        return bad("tmpt_scene_hit: out of device memory");
    int rc = 0;
    if (hipMemcpy(d_rays, rays, rs * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_hits, hits, 28 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
        rc = (set_error("tmpt_scene_hit: upload failed"), -1);
    if (!rc) rc = intersect_batch(s, d_rays, n, tmin, tmax, any_hit != 0, ranged, d_hits, d_ids);
    if (!rc && (hipStreamSynchronize(s.stream) != hipSuccess ||
                hipMemcpy(hits, d_hits, 28 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(ids, d_ids, 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess))
        rc = (set_error("tmpt_scene_hit: kernel or readback failed"), -1);
    if (!rc) {
        s.tie_queries = s.counters_host[kTieCounter];
        s.root_misses = s.counters_host[kTieCounter + 1];
        s.crack_queries = s.counters_host[kCrackCounter];
    }
    if (!rc) rc = check_report(s, "tmpt_scene_hit");
    return rc;
}
}  // namespace

int tmpt_scene_hit(const tmpt_scene* hc, const float* rays, int64_t n, float tmin, float tmax,
                   int32_t any_hit, float* hits, int32_t* ids)
{
    TMPT_GUARD_BEGIN
    return scene_hit(hc, rays, n, tmin, tmax, false, any_hit, hits, ids);
    TMPT_GUARD_END
}

int tmpt_scene_hit_ranged(const tmpt_scene* hc, const float* rays8, int64_t n, int32_t any_hit, float* hits,
                          int32_t* ids)
{
    TMPT_GUARD_BEGIN
    return scene_hit(hc, rays8, n, 0.0f, 0.0f, true, any_hit, hits, ids);
    TMPT_GUARD_END
}

int tmpt_scene_hit_device(tmpt_scene* h, const tmpt_hit_desc* d, const float* d_rays, int32_t* d_ids, float* d_hits,
                          float* d_uv)
{
    TMPT_GUARD_BEGIN
    if (!h) return bad("tmpt_scene_hit_device: null scene");
    if (!d) return bad("tmpt_scene_hit_device: null descriptor");
    if (d->n < 0) return bad("tmpt_scene_hit_device: n < 0");
    if (d->n > 0 && (!d_rays || !d_ids)) return bad("tmpt_scene_hit_device: null d_rays or d_ids");
    if (d->flags & ~TMPT_FLAG_WAIT_STREAM) return bad("tmpt_scene_hit_device: unknown flag (TMPT_FLAG_WAIT_STREAM only)");
    if ((d->ranged != 0 && d->ranged != 1) || (d->any_hit != 0 && d->any_hit != 1))
        return bad("tmpt_scene_hit_device: ranged and any_hit are 0 or 1");
    // (a non-finite tmin / tmax is accepted, as tmpt_scene_hit accepts it)
    if (d->n == 0) return 0;
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const bool wait = (d->flags & TMPT_FLAG_WAIT_STREAM) != 0;  // order after the caller's stream
    int rc;
    if (s.opt.query_legacy) {  // k_intersect on the caller's data (tools/hit_device_time.py)
        if (!d_hits || d_uv) return bad("tmpt_scene_hit_device: query_legacy takes d_hits and no d_uv");
        if (wait && query_wait(s, d->wait_stream)) return -1;
        for (auto& e : s.query_ev) TMPT_HIP(e.ensure());
        TMPT_HIP(hipEventRecord(s.query_ev[0], s.stream));
        rc = intersect_batch(s, d_rays, d->n, d->tmin, d->tmax, d->any_hit != 0, d->ranged != 0, d_hits, d_ids);
        if (!rc) TMPT_HIP(hipEventRecord(s.query_ev[1], s.stream));
        if (!rc && hipStreamSynchronize(s.stream) != hipSuccess) rc = (set_error("tmpt_scene_hit_device: kernel failed"), -1);
        if (!rc) {
            float ms = 0.0f;
            TMPT_HIP(hipEventElapsedTime(&ms, s.query_ev[0], s.query_ev[1]));
            s.query_ms = ms, s.query_sort_ms = 0.0, s.query_chunks = 1, s.query_sorted = 0;
            s.tie_queries = s.counters_host[kTieCounter];
            s.root_misses = s.counters_host[kTieCounter + 1];
            s.crack_queries = s.counters_host[kCrackCounter];
        }
    } else {
        rc = query_batch(s, d_rays, d->n, d->tmin, d->tmax, d->any_hit != 0, d->ranged != 0, d_ids, d_hits, d_uv, wait,
                         d->wait_stream);
    }
    if (!rc) rc = check_report(s, "tmpt_scene_hit_device");
    return rc;
    TMPT_GUARD_END
}

int tmpt_query_keys(const float* rays, int64_t n, int32_t stride, const float box[6], uint32_t* keys)
{
    TMPT_GUARD_BEGIN
    if (n < 0) return bad("tmpt_query_keys: n < 0");
    if (n > 0 && (!rays || !keys)) return bad("tmpt_query_keys: null rays or keys");
    if (stride != 6 && stride != 8) return bad("tmpt_query_keys: stride is 6 or 8");
    if (!box) return bad("tmpt_query_keys: null box");
    for (int64_t i = 0; i < n; ++i) {
        const float* r = rays + (int64_t)stride * i;
        keys[i] = query_key(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), box);
    }
    return 0;
    TMPT_GUARD_END
}

int tmpt_query_plan(int64_t n, int32_t sorted, int64_t chunk, int64_t grid_cap, int64_t resident, int64_t out[6])
{
    TMPT_GUARD_BEGIN
    if (n < 0) return bad("tmpt_query_plan: n < 0");
    if (sorted != 0 && sorted != 1) return bad("tmpt_query_plan: sorted is 0 or 1");
    if (chunk < 64 || chunk > kQueryChunkMax) return bad("tmpt_query_plan: chunk outside 64 .. 2^22");
    if (grid_cap < 0) return bad("tmpt_query_plan: grid_cap < 0");
    if (resident < 1) return bad("tmpt_query_plan: resident < 1");
    if (!out) return bad("tmpt_query_plan: null out");
    const QueryPlan p = query_plan(n, sorted != 0, chunk, grid_cap, resident, kStackTotal - kSL, radix_sort_hist_words);
    out[0] = p.chunks, out[1] = p.chunk_n, out[2] = p.last_n, out[3] = p.grid;
    out[4] = (int64_t)p.ovf_bytes, out[5] = (int64_t)p.sort_bytes;
    return 0;
    TMPT_GUARD_END
}

int32_t tmpt_tile_rows(const tmpt_render_desc* d)
{
    if (!d || d->height < 1) return 0;
    int band = d->band_rows > 0 ? d->band_rows : d->height;
    int ns = d->num_shards > 1 ? d->num_shards : 1;
    int sh = ns > 1 ? d->shard : 0;
    int nbands = (d->height + band - 1) / band;
    int rows = 0;
    for (int b = sh; b < nbands; b += ns) rows += std::min(band, d->height - b * band);
    return rows;
}

int32_t tmpt_tile_row_to_y(const tmpt_render_desc* d, int32_t r)
{
    int band = d->band_rows > 0 ? d->band_rows : d->height;
    int ns = d->num_shards > 1 ? d->num_shards : 1;
    int sh = ns > 1 ? d->shard : 0;
    int lb = r / band;
    return (lb * ns + sh) * band + (r - lb * band);
}

int tmpt_render(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d,
                uint8_t* rgba_out, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    if (!h || !cam || !d || !rgba_out) return bad("tmpt_render: null argument");
    // main.cpp:258-280 argument ranges
    if (d->width < 1 || d->width > 10000) return bad("tmpt_render: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_render: invalid height");
    if (d->spp < 1 || d->spp > 1024) return bad("tmpt_render: invalid samplesPerPixel");
    if (d->seed_mode != TMPT_SEED_ROW && d->seed_mode != TMPT_SEED_PIXEL && d->seed_mode != TMPT_SEED_SAMPLE)
        return bad("tmpt_render: invalid seed_mode");
    if (d->engine != TMPT_ENGINE_WAVEFRONT && d->engine != TMPT_ENGINE_MEGAKERNEL &&
        d->engine != TMPT_ENGINE_PERSISTENT)
        return bad("tmpt_render: invalid engine");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards))
        return bad("tmpt_render: invalid shard");
    if (d->spp_begin < 0 || d->spp_begin >= d->spp || d->spp_count < 0 ||
        d->spp_count > d->spp - d->spp_begin)
        return bad("tmpt_render: invalid spp_begin / spp_count");
    const bool progressive = d->spp_begin > 0 || (d->spp_count > 0 && d->spp_count < d->spp);
    if (progressive && (d->engine != TMPT_ENGINE_PERSISTENT || d->seed_mode == TMPT_SEED_ROW))
        return bad("tmpt_render: progressive spp needs the persistent engine and pixel or sample seeding");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const int32_t rows = tmpt_tile_rows(d);
    const size_t bytes = (size_t)rows * (size_t)d->width * 4;
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    DeviceBuffer<uint32_t> own;
    if (!dev_out && bytes && !own.alloc(bytes)) return bad("tmpt_render: out of device memory");
    uint32_t* d_out = dev_out ? (uint32_t*)rgba_out : own.get();
    int rc = render(s, cam, d, d_out, ray_count);
    if (!rc) rc = check_report(s, "tmpt_render");
    if (!rc && !dev_out && bytes) {
        if (hipMemcpy(rgba_out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = (set_error("tmpt_render: readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_render_aov(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, tmpt_aov_pixel* out,
                    uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    if (!h || !cam || !d || !out) return bad("tmpt_render_aov: null argument");
    if (d->width < 1 || d->width > 10000) return bad("tmpt_render_aov: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_render_aov: invalid height");
    if (d->spp < 1 || d->spp > 1024) return bad("tmpt_render_aov: invalid samplesPerPixel");
    if (d->seed_mode != TMPT_SEED_SAMPLE)
        return bad("tmpt_render_aov: seed_mode must be TMPT_SEED_SAMPLE (the only seeding where a camera ray is a "
                   "function of pixel and sample)");
    if (d->spp_begin != 0 || d->spp_count != 0)
        return bad("tmpt_render_aov: spp_begin / spp_count must be 0 (the pass is not progressive)");
    if (d->flags & TMPT_FLAG_COUNT_VISITS) return bad("tmpt_render_aov: TMPT_FLAG_COUNT_VISITS is not supported");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards))
        return bad("tmpt_render_aov: invalid shard");
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
        return bad("tmpt_render_aov: a device output must be 16-byte aligned");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const size_t bytes = (size_t)tmpt_tile_rows(d) * (size_t)d->width * sizeof(tmpt_aov_pixel);
    DeviceBuffer<tmpt_aov_pixel> own;
    if (!dev_out && bytes && !own.alloc(bytes)) return bad("tmpt_render_aov: out of device memory");
    tmpt_aov_pixel* d_out = dev_out ? out : own.get();
    int rc = render_aov(s, cam, d, d_out, ray_count);
    if (!rc) rc = check_report(s, "tmpt_render_aov");
    if (!rc && !dev_out && bytes) {
        if (hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = (set_error("tmpt_render_aov: readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_camera_rays(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* out)
{
    TMPT_GUARD_BEGIN
    if (!h || !cam || !d || !out) return bad("tmpt_camera_rays: null argument");
    if (d->width < 1 || d->width > 10000) return bad("tmpt_camera_rays: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_camera_rays: invalid height");
    if (d->spp < 1 || d->spp > 1024) return bad("tmpt_camera_rays: invalid samplesPerPixel");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards))
        return bad("tmpt_camera_rays: invalid shard");
    if (d->spp_begin < 0 || d->spp_begin >= d->spp || d->spp_count < 0 || d->spp_count > d->spp - d->spp_begin)
        return bad("tmpt_camera_rays: invalid spp_begin / spp_count");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    return camera_rays(s, cam, d, out);
    TMPT_GUARD_END
}

int tmpt_render_radiance(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, float* rgba32f_out,
                         uint8_t* rgba8_out, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    if (!h || !cam || !d || !rgba32f_out) return bad("tmpt_render_radiance: null argument");
    if (d->width < 1 || d->width > 10000) return bad("tmpt_render_radiance: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_render_radiance: invalid height");
    if (d->spp < 1 || d->spp > 1024) return bad("tmpt_render_radiance: invalid samplesPerPixel");
    if (d->seed_mode != TMPT_SEED_PIXEL && d->seed_mode != TMPT_SEED_SAMPLE)
        return bad("tmpt_render_radiance: seed_mode must be TMPT_SEED_PIXEL or TMPT_SEED_SAMPLE (row seeding keeps no "
                   "float sum per pixel)");
    if (d->engine != TMPT_ENGINE_PERSISTENT)
        return bad("tmpt_render_radiance: engine must be TMPT_ENGINE_PERSISTENT");
    if (d->spp_begin != 0 || d->spp_count != 0)
        return bad("tmpt_render_radiance: spp_begin / spp_count must be 0 (whole renders only)");
    if (d->flags & TMPT_FLAG_COUNT_VISITS)
        return bad("tmpt_render_radiance: TMPT_FLAG_COUNT_VISITS is not supported");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards))
        return bad("tmpt_render_radiance: invalid shard");
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && (reinterpret_cast<uintptr_t>(rgba32f_out) & 15u) != 0)
        return bad("tmpt_render_radiance: a device rgba32f_out must be 16-byte aligned");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const size_t px = (size_t)tmpt_tile_rows(d) * (size_t)d->width;
    // the kernels write both tiles: device buffers of the library's own stand in
    // for host outputs and for an rgba8_out the caller does not want
    float4* d_f = dev_out ? reinterpret_cast<float4*>(rgba32f_out) : nullptr;
    uint32_t* d_8 = dev_out ? reinterpret_cast<uint32_t*>(rgba8_out) : nullptr;
    DeviceBuffer<float4> own_f;
    DeviceBuffer<uint32_t> own_8;
    if (px && ((!d_f && !own_f.alloc(px * sizeof(float4))) || (!d_8 && !own_8.alloc(px * 4))))
        return bad("tmpt_render_radiance: out of device memory");
    if (own_f) d_f = own_f;
    if (own_8) d_8 = own_8;
    int rc = render(s, cam, d, d_8, ray_count, d_f);
    if (!rc) rc = check_report(s, "tmpt_render_radiance");
    if (!rc && !dev_out && px) {
        if (hipMemcpy(rgba32f_out, d_f, px * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess ||
            (rgba8_out && hipMemcpy(rgba8_out, d_8, px * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = (set_error("tmpt_render_radiance: readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

// tmpt_render_adaptive, tmpt_render_moments and tmpt_render_guided: one body.
// `name` is the call's name in errors; with_mom: ad NULL means the uniform
// schedule spp_min = desc->spp, not the adaptive defaults, and moments_out is
// required -- unless guided, where any one of the four outputs will do and
// `prior` (the tile's float4, following the outputs' flag; may be null) enters
// the test.
static int adaptive_call(const char* name, bool with_mom, tmpt_scene* h, const tmpt_camera* cam,
                         const tmpt_render_desc* d, const tmpt_adaptive_desc* ad, float* rgba32f_out, float* moments_out,
                         uint8_t* rgba8_out, int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count,
                         bool guided = false, const float* prior = nullptr)
{
    const auto no = [name](const char* msg) { return bad((std::string(name) + ": " + msg).c_str()); };
    if (!h || !cam || !d) return no("null argument");
    if (d->width < 1 || d->width > 10000) return no("invalid width");
    if (d->height < 1 || d->height > 10000) return no("invalid height");
    if (d->spp < 1 || d->spp > 1024) return no("invalid samplesPerPixel");
    if (d->seed_mode != TMPT_SEED_SAMPLE)
        return no("seed_mode must be TMPT_SEED_SAMPLE (the only seeding where a sample is a "
                  "function of pixel and sample)");
    if (d->engine != TMPT_ENGINE_PERSISTENT) return no("engine must be TMPT_ENGINE_PERSISTENT");
    if (d->spp_begin != 0 || d->spp_count != 0)
        return no("spp_begin / spp_count must be 0 (the call makes its own passes)");
    if (d->flags & TMPT_FLAG_COUNT_VISITS) return no("TMPT_FLAG_COUNT_VISITS is not supported");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards)) return no("invalid shard");
    tmpt_adaptive_desc r;  // the defaults, in one place ("Adaptive sampling")
    memset(&r, 0, sizeof(r));
    if (ad) r = *ad;
    else r.threshold = -1.0f;
    if (!ad && with_mom) r.spp_min = d->spp;  // uniform: one pass, every pixel at desc->spp
    if (r.spp_min == 0) r.spp_min = std::min(24, d->spp);
    if (r.spp_step == 0) r.spp_step = 8;
    if (!(r.threshold >= -3.0e38f) || !(r.threshold <= 3.0e38f))
        return no("threshold must be finite (negative = default)");
    if (r.threshold < 0.0f) r.threshold = 0.015f;
    if (r.spp_min < 2 || r.spp_min > d->spp) return no("spp_min outside 2 .. spp (0 = default)");
    if (r.spp_step < 1) return no("spp_step must not be negative (0 = default)");
    if (r.radius < 0 || r.radius > 8) return no("radius outside 0 .. 8 (0 = no neighbourhood rule)");
    if (1 + (d->spp - r.spp_min + r.spp_step - 1) / r.spp_step > 64)
        return no("spp_min / spp_step give a schedule of more than 64 passes");
    if (guided) {
        if (!rgba32f_out && !moments_out && !rgba8_out && !spp_out)
            return no("no output (rgba32f_out, moments_out, rgba8_out and spp_out are all null)");
    } else if (with_mom) {
        if (!moments_out) return no("moments_out is required");
    } else if (!rgba32f_out && !rgba8_out && !spp_out) {
        return no("no output (rgba32f_out, rgba8_out and spp_out are all null)");
    }
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && (((reinterpret_cast<uintptr_t>(rgba32f_out) | reinterpret_cast<uintptr_t>(moments_out)) & 15u) != 0 ||
                    ((reinterpret_cast<uintptr_t>(rgba8_out) | reinterpret_cast<uintptr_t>(spp_out)) & 3u) != 0))
        return no(with_mom ? "device outputs must be aligned (rgba32f_out and moments_out 16 bytes, rgba8_out and "
                             "spp_out 4)"
                           : "device outputs must be aligned (rgba32f_out 16 bytes, rgba8_out and "
                             "spp_out 4)");
    if (dev_out && (reinterpret_cast<uintptr_t>(prior) & 15u) != 0) return no("a device prior must be 16-byte aligned");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const size_t px = (size_t)tmpt_tile_rows(d) * (size_t)d->width;
    // host outputs are staged in device tiles of the library's own
    float4* d_f = dev_out ? reinterpret_cast<float4*>(rgba32f_out) : nullptr;
    float4* d_m = dev_out ? reinterpret_cast<float4*>(moments_out) : nullptr;
    uint32_t* d_8 = dev_out ? reinterpret_cast<uint32_t*>(rgba8_out) : nullptr;
    int32_t* d_n = dev_out ? spp_out : nullptr;
    DeviceBuffer<float4> own_f, own_m;
    DeviceBuffer<uint32_t> own_8;
    DeviceBuffer<int32_t> own_n;
    if (!dev_out && px &&
        ((rgba32f_out && !own_f.alloc(px * sizeof(float4))) || (moments_out && !own_m.alloc(px * sizeof(float4))) ||
         (rgba8_out && !own_8.alloc(px * 4)) || (spp_out && !own_n.alloc(px * 4))))
        return no("out of device memory");
    if (own_f) d_f = own_f;
    if (own_m) d_m = own_m;
    if (own_8) d_8 = own_8;
    if (own_n) d_n = own_n;
    const float4* d_p = reinterpret_cast<const float4*>(prior);
    DeviceBuffer<float4> own_p;
    if (prior && !dev_out && px) {  // a host prior: staged beside the outputs' tiles
        if (!own_p.alloc(px * sizeof(float4))) return no("out of device memory");
        if (hipMemcpy(own_p, prior, px * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess)
            return (set_error(std::string(name) + ": upload failed"), -1);
        d_p = own_p;
    }
    int rc = render_adaptive(s, cam, d, &r, d_f, d_8, d_n, info, ray_count, d_m, name, d_p);
    if (!rc) rc = check_report(s, name);
    if (!rc && !dev_out && px) {
        if ((rgba32f_out && hipMemcpy(rgba32f_out, d_f, px * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) ||
            (moments_out && hipMemcpy(moments_out, d_m, px * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) ||
            (rgba8_out && hipMemcpy(rgba8_out, d_8, px * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
            (spp_out && hipMemcpy(spp_out, d_n, px * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = (set_error(std::string(name) + ": readback failed"), -1);
    }
    return rc;
}

int tmpt_render_adaptive(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d,
                         const tmpt_adaptive_desc* ad, float* rgba32f_out, uint8_t* rgba8_out, int32_t* spp_out,
                         tmpt_adaptive_info* info, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    return adaptive_call("tmpt_render_adaptive", false, h, cam, d, ad, rgba32f_out, nullptr, rgba8_out, spp_out, info,
                         ray_count);
    TMPT_GUARD_END
}

int tmpt_render_moments(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d,
                        const tmpt_adaptive_desc* ad, float* rgba32f_out, float* moments_out, uint8_t* rgba8_out,
                        int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    return adaptive_call("tmpt_render_moments", true, h, cam, d, ad, rgba32f_out, moments_out, rgba8_out, spp_out, info,
                         ray_count);
    TMPT_GUARD_END
}

int tmpt_render_guided(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, const tmpt_adaptive_desc* ad,
                       const float* prior, float* rgba32f_out, float* moments_out, uint8_t* rgba8_out,
                       int32_t* spp_out, tmpt_adaptive_info* info, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    return adaptive_call("tmpt_render_guided", true, h, cam, d, ad, rgba32f_out, moments_out, rgba8_out, spp_out, info,
                         ray_count, true, prior);
    TMPT_GUARD_END
}

// tmpt_denoise_moments' default shrink: the grid point tools/noise_aware_sweep.py's rule
// picks ("Noise-aware filter")
constexpr float kShrinkDefault = 2.0f;

// tmpt_denoise and tmpt_denoise_moments: one body.  `name` is the call's name in
// errors; with_mom: the moments frame is required and shrink is read.
static int denoise_call(const char* name, bool with_mom, tmpt_scene* h, const tmpt_denoise_desc* d, float shrink,
                        const float* rgba32f_in, const tmpt_aov_pixel* aov, const float* moments, float* rgba32f_out,
                        uint8_t* rgba8_out)
{
    const auto no = [name](const char* msg) { return bad((std::string(name) + ": " + msg).c_str()); };
    // the descriptor first, before anything that needs a scene or a device
    if (!d) return no("null descriptor");
    if (d->width < 1 || d->width > 10000) return no("invalid width");
    if (d->height < 1 || d->height > 10000) return no("invalid height");
    if (d->spp < 1 || d->spp > 1024) return no("invalid samplesPerPixel");
    if (d->levels < 0 || d->levels > 6) return no("levels out of range (1..6, 0 = 5)");
    if (d->normal_exp < -1 || d->normal_exp > 8) return no("normal_exp out of range (0..8, -1 = 5)");
    if (!(d->sigma_depth >= 0.0f) || !(d->sigma_depth <= 3.0e38f))
        return no("sigma_depth must be finite and not negative (0 = auto)");
    if (!(d->sigma_direct >= 0.0f) || !(d->sigma_direct <= 3.0e38f))
        return no("sigma_direct must be finite and not negative (0 = default)");
    if (with_mom && (!(shrink >= 0.0f) || !(shrink <= 3.4028235e38f)))
        return no("shrink must be finite and not negative (0 = default)");
    if (d->flags & ~(TMPT_FLAG_OUT_DEVICE | TMPT_FLAG_WAIT_STREAM)) return no("unknown flag");
    if (!rgba32f_out && !rgba8_out) return no("no output (rgba32f_out and rgba8_out are both null)");
    if (!h || !rgba32f_in || !aov || (with_mom && !moments)) return no("null argument");
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && (((reinterpret_cast<uintptr_t>(rgba32f_in) | reinterpret_cast<uintptr_t>(aov) |
                  reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(rgba32f_out)) & 15u) != 0 ||
                (reinterpret_cast<uintptr_t>(rgba8_out) & 3u) != 0))
        return no("device pointers must be 16-byte aligned (rgba8_out: 4)");
    if (shrink == 0.0f) shrink = kShrinkDefault;
    tmpt_denoise_desc r = *d;  // the defaults, in one place
    if (r.levels == 0) r.levels = 5;
    if (r.normal_exp < 0) r.normal_exp = 5;
    if (r.sigma_depth == 0.0f) r.sigma_depth = 1.0f / (float)r.height;
    if (r.sigma_direct == 0.0f) r.sigma_direct = 0.05f;
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const size_t n = (size_t)r.width * (size_t)r.height;
    const float4* d_in = reinterpret_cast<const float4*>(rgba32f_in);
    const tmpt_aov_pixel* d_aov = aov;
    float4* d_o32 = reinterpret_cast<float4*>(rgba32f_out);
    uint32_t* d_o8 = reinterpret_cast<uint32_t*>(rgba8_out);
    DeviceBuffer<float4> own_in;
    DeviceBuffer<tmpt_aov_pixel> own_aov;
    DeviceBuffer<uint32_t> own_8;
    const float4* d_mom = reinterpret_cast<const float4*>(moments);
    DeviceBuffer<float4> own_mom;
    if (!dev) {  // host pointers: staged on the device; the float result is filtered in place there
        if (!own_in.alloc(n * sizeof(float4)) || !own_aov.alloc(n * sizeof(tmpt_aov_pixel)) ||
            (rgba8_out && !own_8.alloc(n * 4)) || (with_mom && !own_mom.alloc(n * sizeof(float4))))
            return no("out of device memory");
        if (hipMemcpy(own_in, rgba32f_in, n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(own_aov, aov, n * sizeof(tmpt_aov_pixel), hipMemcpyHostToDevice) != hipSuccess ||
            (with_mom && hipMemcpy(own_mom, moments, n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess))
            return (set_error(std::string(name) + ": upload failed"), -1);
        d_in = own_in;
        d_aov = own_aov;
        d_mom = own_mom;
        d_o32 = rgba32f_out ? own_in.get() : nullptr;
        d_o8 = own_8;
    }
    int rc = with_mom ? denoise_moments(s, &r, shrink, d_in, d_aov, d_mom, d_o32, d_o8)
                      : denoise(s, &r, d_in, d_aov, d_o32, d_o8);
    if (!rc && !dev) {
        if ((rgba32f_out && hipMemcpy(rgba32f_out, d_o32, n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) ||
            (rgba8_out && hipMemcpy(rgba8_out, d_o8, n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = (set_error(std::string(name) + ": readback failed"), -1);
    }
    return rc;
}

int tmpt_denoise(tmpt_scene* h, const tmpt_denoise_desc* d, const float* rgba32f_in, const tmpt_aov_pixel* aov,
                 float* rgba32f_out, uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    return denoise_call("tmpt_denoise", false, h, d, 0.0f, rgba32f_in, aov, nullptr, rgba32f_out, rgba8_out);
    TMPT_GUARD_END
}

int tmpt_denoise_moments(tmpt_scene* h, const tmpt_denoise_desc* d, float shrink, const float* rgba32f_in,
                         const tmpt_aov_pixel* aov, const float* moments, float* rgba32f_out, uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    return denoise_call("tmpt_denoise_moments", true, h, d, shrink, rgba32f_in, aov, moments, rgba32f_out, rgba8_out);
    TMPT_GUARD_END
}

int tmpt_render_motion(tmpt_scene* h, const tmpt_camera* cam, const tmpt_camera* prev_cam, const float* prev_tris,
                       int32_t prev_n, const tmpt_render_desc* d, tmpt_motion_pixel* out, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    // everything that needs no scene first, so that it is refused without a device
    if (!cam || !prev_cam || !d || !out) return bad("tmpt_render_motion: null argument");
    if (d->width < 1 || d->width > 10000) return bad("tmpt_render_motion: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_render_motion: invalid height");
    if (d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards))
        return bad("tmpt_render_motion: invalid shard");
    if (d->flags & TMPT_FLAG_COUNT_VISITS) return bad("tmpt_render_motion: TMPT_FLAG_COUNT_VISITS is not supported");
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
        return bad("tmpt_render_motion: a device output must be 16-byte aligned");
    if (!h) return bad("tmpt_render_motion: null scene");
    Scene& s = h->s;
    if (prev_tris && prev_n != s.bvh.n)
        return bad("tmpt_render_motion: prev_n differs from the scene's triangle count (the previous pose has the "
                   "scene's triangles, slot for slot)");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    TMPT_HIP(hipSetDevice(s.device));
    const float* d_prev = prev_tris;
    if (prev_tris && !dev_out) {  // a host pose: into the scene's kept buffer
        const size_t pb = sizeof(float) * 9 * (size_t)prev_n;
        TMPT_HIP(hipStreamSynchronize(s.stream));
        if (pb && !s.motion_prev.reserve(pb)) return bad("tmpt_render_motion: out of device memory");
        if (pb && hipMemcpy(s.motion_prev, prev_tris, pb, hipMemcpyHostToDevice) != hipSuccess)
            return (set_error("tmpt_render_motion: upload failed"), -1);
        d_prev = s.motion_prev;
    }
    const size_t bytes = (size_t)tmpt_tile_rows(d) * (size_t)d->width * sizeof(tmpt_motion_pixel);
    DeviceBuffer<tmpt_motion_pixel> own;
    if (!dev_out && bytes && !own.alloc(bytes)) return bad("tmpt_render_motion: out of device memory");
    tmpt_motion_pixel* d_out = dev_out ? out : own.get();
    int rc = render_motion(s, cam, prev_cam, d_prev, d, d_out, ray_count);
    if (!rc) rc = check_report(s, "tmpt_render_motion");
    if (!rc && !dev_out && bytes) {
        if (hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = (set_error("tmpt_render_motion: readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_temporal(tmpt_scene* h, const tmpt_temporal_desc* d, const float* rgba32f_cur, const tmpt_motion_pixel* motion,
                  const tmpt_motion_pixel* prev_motion, const float* rgba32f_history, float* rgba32f_out,
                  uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    // the descriptor first, before anything that needs a scene or a device
    if (!d) return bad("tmpt_temporal: null descriptor");
    if (d->width < 1 || d->width > 10000) return bad("tmpt_temporal: invalid width");
    if (d->height < 1 || d->height > 10000) return bad("tmpt_temporal: invalid height");
    if (!rgba32f_cur || !motion || !prev_motion || !rgba32f_history) return bad("tmpt_temporal: null argument");
    if (!rgba32f_out && !rgba8_out) return bad("tmpt_temporal: no output (rgba32f_out and rgba8_out are both null)");
    tmpt_temporal_desc r = *d;  // the defaults, in one place ("Temporal accumulation")
    if (r.n_max == 0.0f) r.n_max = 3.0f;
    if (r.sigma_depth == 0.0f) r.sigma_depth = 0.05f;
    if (!(r.n_max >= 1.0f) || !(r.n_max <= 3.0e38f))
        return bad("tmpt_temporal: n_max must be finite and at least 1 (0 = default)");
    if (!(r.sigma_depth >= 0.0f) || !(r.sigma_depth <= 3.0e38f))
        return bad("tmpt_temporal: sigma_depth must be finite and not negative (0 = default)");
    if (d->flags & ~(TMPT_FLAG_OUT_DEVICE | TMPT_FLAG_WAIT_STREAM)) return bad("tmpt_temporal: unknown flag");
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && (((reinterpret_cast<uintptr_t>(rgba32f_cur) | reinterpret_cast<uintptr_t>(motion) |
                  reinterpret_cast<uintptr_t>(prev_motion) | reinterpret_cast<uintptr_t>(rgba32f_history) |
                  reinterpret_cast<uintptr_t>(rgba32f_out)) & 15u) != 0 ||
                (reinterpret_cast<uintptr_t>(rgba8_out) & 3u) != 0))
        return bad("tmpt_temporal: device pointers must be 16-byte aligned (rgba8_out: 4)");
    const size_t n = (size_t)r.width * (size_t)r.height;
    if (rgba32f_out) {
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(rgba32f_out), h0 = reinterpret_cast<uintptr_t>(rgba32f_history);
        if (o0 < h0 + n * sizeof(float4) && h0 < o0 + n * sizeof(float4))
            return bad("tmpt_temporal: rgba32f_out overlaps rgba32f_history (its neighbours are read)");
    }
    if (!h) return bad("tmpt_temporal: null scene");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const float4* d_cur = reinterpret_cast<const float4*>(rgba32f_cur);
    const float4* d_hist = reinterpret_cast<const float4*>(rgba32f_history);
    const tmpt_motion_pixel *d_m = motion, *d_pm = prev_motion;
    float4* d_o32 = reinterpret_cast<float4*>(rgba32f_out);
    uint32_t* d_o8 = reinterpret_cast<uint32_t*>(rgba8_out);
    DeviceBuffer<float4> own_cur, own_hist;
    DeviceBuffer<tmpt_motion_pixel> own_m, own_pm;
    DeviceBuffer<uint32_t> own_8;
    if (!dev) {  // host pointers: staged on the device; the float result is blended in place there
        if (!own_cur.alloc(n * sizeof(float4)) || !own_hist.alloc(n * sizeof(float4)) ||
            !own_m.alloc(n * sizeof(tmpt_motion_pixel)) || !own_pm.alloc(n * sizeof(tmpt_motion_pixel)) ||
            (rgba8_out && !own_8.alloc(n * 4)))
            return bad("tmpt_temporal: out of device memory");
        if (hipMemcpy(own_cur, rgba32f_cur, n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(own_hist, rgba32f_history, n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(own_m, motion, n * sizeof(tmpt_motion_pixel), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(own_pm, prev_motion, n * sizeof(tmpt_motion_pixel), hipMemcpyHostToDevice) != hipSuccess)
            return (set_error("tmpt_temporal: upload failed"), -1);
        d_cur = own_cur;
        d_hist = own_hist;
        d_m = own_m;
        d_pm = own_pm;
        d_o32 = rgba32f_out ? own_cur.get() : nullptr;
        d_o8 = own_8;
    }
    int rc = temporal(s, &r, d_cur, d_m, d_pm, d_hist, d_o32, d_o8);
    if (!rc && !dev) {
        if ((rgba32f_out && hipMemcpy(rgba32f_out, d_o32, n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) ||
            (rgba8_out && hipMemcpy(rgba8_out, d_o8, n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = (set_error("tmpt_temporal: readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_sample_plan(tmpt_scene* h, const tmpt_temporal_desc* d, const tmpt_motion_pixel* motion,
                     const tmpt_motion_pixel* prev_motion, const float* moments_history, float* prior_out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_sample_plan: ";
    auto no = [&](const char* what) { return bad((std::string(fn) + what).c_str()); };
    // tmpt_temporal's checks in its order, its colour frames left out
    if (!d) return no("null descriptor");
    if (d->width < 1 || d->width > 10000) return no("invalid width");
    if (d->height < 1 || d->height > 10000) return no("invalid height");
    if (!motion || !prev_motion || !moments_history || !prior_out) return no("null argument");
    tmpt_temporal_desc r = *d;  // the defaults, in one place: tmpt_temporal's
    if (r.n_max == 0.0f) r.n_max = 3.0f;
    if (r.sigma_depth == 0.0f) r.sigma_depth = 0.05f;
    if (!(r.n_max >= 1.0f) || !(r.n_max <= 3.0e38f)) return no("n_max must be finite and at least 1 (0 = default)");
    if (!(r.sigma_depth >= 0.0f) || !(r.sigma_depth <= 3.0e38f))
        return no("sigma_depth must be finite and not negative (0 = default)");
    if (d->flags & ~(TMPT_FLAG_OUT_DEVICE | TMPT_FLAG_WAIT_STREAM)) return no("unknown flag");
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (dev && ((at(motion) | at(prev_motion) | at(moments_history) | at(prior_out)) & 15u) != 0)
        return no("device pointers must be 16-byte aligned");
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4);
    if (at(prior_out) < at(moments_history) + fb && at(moments_history) < at(prior_out) + fb)
        return no("prior_out overlaps moments_history (its neighbours are read)");
    if (!h) return no("null scene");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const float4* d_hist = reinterpret_cast<const float4*>(moments_history);
    const tmpt_motion_pixel *d_m = motion, *d_pm = prev_motion;
    float4* d_out = reinterpret_cast<float4*>(prior_out);
    if (!dev) {  // host pointers: staged in the scene's kept buffer, as tmpt_temporal_clip stages its own
        const size_t mb = n * sizeof(tmpt_motion_pixel);
        TMPT_HIP(hipStreamSynchronize(s.stream));
        if (!s.clip_stage.reserve(2 * fb + 2 * mb)) return no("out of device memory");
        char* at_dev = s.clip_stage.as<char>();
        auto take = [&](size_t bytes) { char* p = at_dev; at_dev += bytes; return p; };
        auto up = [&](const void* src, size_t bytes) -> char* {
            char* p = take(bytes);
            return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? p : nullptr;
        };
        d_hist = reinterpret_cast<const float4*>(up(moments_history, fb));
        d_m = reinterpret_cast<const tmpt_motion_pixel*>(up(motion, mb));
        d_pm = reinterpret_cast<const tmpt_motion_pixel*>(up(prev_motion, mb));
        if (!d_hist || !d_m || !d_pm) return (set_error(std::string(fn) + "upload failed"), -1);
        d_out = reinterpret_cast<float4*>(take(fb));
    }
    int rc = sample_plan(s, &r, d_m, d_pm, d_hist, d_out);
    if (!rc && !dev && hipMemcpy(prior_out, d_out, fb, hipMemcpyDeviceToHost) != hipSuccess)
        rc = (set_error(std::string(fn) + "readback failed"), -1);
    return rc;
    TMPT_GUARD_END
}

// tmpt_temporal_clip's defaults: the grid point tools/temporal_clip_sweep.py's rule
// chose (profiles/temporal_clip_sweep.log, DESIGN.md section 4, "History clipping")
constexpr float kClipNMax = 3.0f, kClipGamma = 0.5f;
constexpr int32_t kClipRadius = 1;

int tmpt_temporal_clip(tmpt_scene* h, const tmpt_temporal_clip_desc* d, const float* rgba32f_cur,
                       const float* rgba32f_stat, const tmpt_motion_pixel* motion, const tmpt_motion_pixel* prev_motion,
                       const float* rgba32f_history, const float* aux_cur, const float* aux_history, float* aux_out,
                       float* rgba32f_out, uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_temporal_clip: ";
    auto no = [&](const char* what) { return bad((std::string(fn) + what).c_str()); };
    // tmpt_temporal's checks in its order, the new ones where the header puts them
    if (!d) return no("null descriptor");
    if (d->width < 1 || d->width > 10000) return no("invalid width");
    if (d->height < 1 || d->height > 10000) return no("invalid height");
    if (!rgba32f_cur || !motion || !prev_motion || !rgba32f_history) return no("null argument");
    const bool aux = aux_cur || aux_history || aux_out;
    if (aux && (!aux_cur || !aux_history || !aux_out))
        return no("null argument (aux_cur, aux_history and aux_out: all three or none)");
    if (!rgba32f_out && !rgba8_out) return no("no output (rgba32f_out and rgba8_out are both null)");
    tmpt_temporal_clip_desc r = *d;  // the defaults, in one place
    if (r.n_max == 0.0f) r.n_max = kClipNMax;
    if (r.sigma_depth == 0.0f) r.sigma_depth = 0.05f;
    if (r.gamma == 0.0f) r.gamma = kClipGamma;
    if (r.radius == 0) r.radius = kClipRadius;
    if (!(r.n_max >= 1.0f) || !(r.n_max <= 3.0e38f)) return no("n_max must be finite and at least 1 (0 = default)");
    if (!(r.sigma_depth >= 0.0f) || !(r.sigma_depth <= 3.0e38f))
        return no("sigma_depth must be finite and not negative (0 = default)");
    if (!(r.gamma >= 0.0f) || !(r.gamma <= 3.0e38f)) return no("gamma must be finite and not negative (0 = default)");
    if (r.radius < 1 || r.radius > 3) return no("radius must be 1, 2 or 3 (0 = default)");
    if (d->flags & ~(TMPT_FLAG_OUT_DEVICE | TMPT_FLAG_WAIT_STREAM)) return no("unknown flag");
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (dev && (((at(rgba32f_cur) | at(rgba32f_stat) | at(motion) | at(prev_motion) | at(rgba32f_history) | at(aux_cur) |
                  at(aux_history) | at(aux_out) | at(rgba32f_out)) & 15u) != 0 || (at(rgba8_out) & 3u) != 0))
        return no("device pointers must be 16-byte aligned (rgba8_out: 4)");
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4);
    {
        const struct { const void* p; const char* name; } outs[] = {{rgba32f_out, "rgba32f_out"}, {aux_out, "aux_out"}},
            ins[] = {{rgba32f_history, "rgba32f_history"}, {aux_history, "aux_history"}, {rgba32f_cur, "rgba32f_cur"},
                     {rgba32f_stat, "rgba32f_stat"}};
        for (const auto& o : outs)
            for (const auto& i : ins)
                if (o.p && i.p && at(o.p) < at(i.p) + fb && at(i.p) < at(o.p) + fb)
                    return no((std::string(o.name) + " overlaps " + i.name + " (its neighbours are read)").c_str());
    }
    if (!h) return no("null scene");
    (void)hipGetLastError();  // clear a stale error of an earlier failed call (launch checks read it)
    Scene& s = h->s;
    TMPT_HIP(hipSetDevice(s.device));
    const float4* d_cur = reinterpret_cast<const float4*>(rgba32f_cur);
    const float4* d_stat = reinterpret_cast<const float4*>(rgba32f_stat);
    const float4* d_hist = reinterpret_cast<const float4*>(rgba32f_history);
    const float4* d_ac = reinterpret_cast<const float4*>(aux_cur);
    const float4* d_ah = reinterpret_cast<const float4*>(aux_history);
    const tmpt_motion_pixel *d_m = motion, *d_pm = prev_motion;
    float4* d_ao = reinterpret_cast<float4*>(aux_out);
    float4* d_o32 = reinterpret_cast<float4*>(rgba32f_out);
    uint32_t* d_o8 = reinterpret_cast<uint32_t*>(rgba8_out);
    if (!dev) {  // host pointers: staged in the scene's kept buffer, frame after frame
        const size_t mb = n * sizeof(tmpt_motion_pixel);
        const size_t total = fb * (3 + (rgba32f_stat ? 1 : 0) + (aux ? 3 : 0)) + 2 * mb + n * 4;
        TMPT_HIP(hipStreamSynchronize(s.stream));
        if (!s.clip_stage.reserve(total)) return no("out of device memory");
        char* at_dev = s.clip_stage.as<char>();
        auto take = [&](size_t bytes) { char* p = at_dev; at_dev += bytes; return p; };
        auto up = [&](const void* src, size_t bytes) -> char* {
            char* p = take(bytes);
            return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? p : nullptr;
        };
        d_cur = reinterpret_cast<const float4*>(up(rgba32f_cur, fb));
        d_hist = reinterpret_cast<const float4*>(up(rgba32f_history, fb));
        d_m = reinterpret_cast<const tmpt_motion_pixel*>(up(motion, mb));
        d_pm = reinterpret_cast<const tmpt_motion_pixel*>(up(prev_motion, mb));
        bool ok = d_cur && d_hist && d_m && d_pm;
        if (rgba32f_stat) ok = (d_stat = reinterpret_cast<const float4*>(up(rgba32f_stat, fb))) && ok;
        if (aux) {
            ok = (d_ac = reinterpret_cast<const float4*>(up(aux_cur, fb))) && ok;
            ok = (d_ah = reinterpret_cast<const float4*>(up(aux_history, fb))) && ok;
            d_ao = reinterpret_cast<float4*>(take(fb));
        }
        if (!ok) return (set_error(std::string(fn) + "upload failed"), -1);
        d_o32 = rgba32f_out ? reinterpret_cast<float4*>(take(fb)) : nullptr;
        d_o8 = rgba8_out ? reinterpret_cast<uint32_t*>(take(n * 4)) : nullptr;
    }
    if (!d_stat) d_stat = d_cur;
    int rc = temporal_clip(s, &r, d_cur, d_stat, d_m, d_pm, d_hist, d_ac, d_ah, d_ao, d_o32, d_o8);
    if (!rc && !dev) {
        if ((rgba32f_out && hipMemcpy(rgba32f_out, d_o32, fb, hipMemcpyDeviceToHost) != hipSuccess) ||
            (aux && hipMemcpy(aux_out, d_ao, fb, hipMemcpyDeviceToHost) != hipSuccess) ||
            (rgba8_out && hipMemcpy(rgba8_out, d_o8, n * 4, hipMemcpyDeviceToHost) != hipSuccess))
            rc = (set_error(std::string(fn) + "readback failed"), -1);
    }
    return rc;
    TMPT_GUARD_END
}

int tmpt_render_multi(const float* tris, int32_t n, const float* octree_box, const tmpt_camera* cam,
                      const tmpt_render_desc* desc, const int32_t* devices, int32_t ndevices, uint8_t* rgba_full,
                      uint64_t* ray_count, double* seconds)
{
    TMPT_GUARD_BEGIN
    if (!cam || !desc || !devices || ndevices < 1 || !rgba_full || (n > 0 && !tris))
        return bad("tmpt_render_multi: bad arguments");
    if (desc->width < 1 || desc->width > 10000 || desc->height < 1 || desc->height > 10000)
        return bad("tmpt_render_multi: invalid width / height");
    const int nd = ndevices;
    const int W = desc->width, H = desc->height;
    bool unique = true;
    for (int g = 0; g < nd; ++g)
        for (int k = 0; k < g; ++k) unique = unique && devices[g] != devices[k];
    const bool use_rccl = unique && rccl().ok;
    if ((desc->flags & TMPT_FLAG_REQUIRE_RCCL) && !use_rccl)
        return bad(unique ? "tmpt_render_multi: RCCL (librccl.so.1) not available"
                          : "tmpt_render_multi: RCCL needs distinct devices (a device is listed twice)");
    std::vector<tmpt_scene*> scenes((size_t)nd, nullptr);
    std::vector<int> rcs((size_t)nd, 0);
    std::vector<std::string> errs((size_t)nd);
    // per rank: its padded tile and ray count on its device; on rank 0 also the
    // gathered tiles, the frame and the summed count
    const int max_rows = (H + nd - 1) / nd;
    const size_t tile_bytes = (size_t)max_rows * (size_t)W * 4;
    std::vector<DeviceBuffer<uint8_t>> d_tile((size_t)nd);
    std::vector<DeviceBuffer<uint64_t>> d_rays((size_t)nd);
    std::vector<Stream> streams((size_t)nd);
    DeviceBuffer<uint8_t> d_gather;
    DeviceBuffer<uint32_t> d_frame;
    DeviceBuffer<uint64_t> d_total;
    std::vector<ncclComm_t> comms;
    auto cleanup = [&]() {  // touches only devices whose resources exist (a bad ordinal is never set)
        for (int g = 0; g < nd; ++g)
            if (streams[(size_t)g]) {
                (void)hipSetDevice(devices[g]);
                (void)hipStreamSynchronize(streams[(size_t)g]);
            }
        for (ncclComm_t c : comms)
            if (c) (void)rccl().comm_destroy(c);
        for (int g = 0; g < nd; ++g) {
            if (!streams[(size_t)g] && !d_tile[(size_t)g] && !d_rays[(size_t)g]) continue;
            (void)hipSetDevice(devices[g]);
            d_tile[(size_t)g].reset();
            d_rays[(size_t)g].reset();
            streams[(size_t)g].reset();
        }
        if (d_gather || d_frame || d_total) {
            (void)hipSetDevice(devices[0]);
            d_gather.reset();
            d_frame.reset();
            d_total.reset();
        }
        for (auto*& sc : scenes) {
            tmpt_scene_destroy(sc);
            sc = nullptr;
        }
        (void)hipGetLastError();  // leave no sticky error behind for this thread's next call
    };
    auto fail = [&](const std::string& msg, int rc) {
        cleanup();
        set_error("tmpt_render_multi: " + msg);
        return rc;
    };
    {  // scene per device, concurrently (error text is thread-local: keep each thread's)
        std::vector<std::thread> th;
        for (int g = 0; g < nd; ++g)
            th.emplace_back([&, g]() {
                rcs[(size_t)g] = tmpt_scene_create(tris, n, devices[g], &scenes[(size_t)g]);
                if (!rcs[(size_t)g] && octree_box && (desc->flags & TMPT_FLAG_OCTREE_DEVICE))
                    rcs[(size_t)g] = tmpt_scene_set_option(scenes[(size_t)g], "octree_build", 1.0);
                if (!rcs[(size_t)g] && octree_box)  // main.cpp:312
                    rcs[(size_t)g] = tmpt_scene_build_octree(scenes[(size_t)g], octree_box, octree_box + 3);
                if (rcs[(size_t)g]) errs[(size_t)g] = tmpt_last_error();
            });
        for (auto& t : th) t.join();
    }
    for (int g = 0; g < nd; ++g)
        if (rcs[(size_t)g]) return fail(errs[(size_t)g], rcs[(size_t)g]);
    for (int g = 0; g < nd; ++g) {
        if (hipSetDevice(devices[g]) != hipSuccess || streams[(size_t)g].ensure(hipStreamNonBlocking) != hipSuccess ||
            !d_tile[(size_t)g].alloc(tile_bytes) || !d_rays[(size_t)g].alloc(sizeof(uint64_t)) ||
            hipMemsetAsync(d_tile[(size_t)g], 0, tile_bytes, streams[(size_t)g]) != hipSuccess)
            return fail("out of device memory", -1);
    }
    if (hipSetDevice(devices[0]) != hipSuccess || !d_gather.alloc(tile_bytes * (size_t)nd) ||
        !d_frame.alloc((size_t)W * H * 4) || !d_total.alloc(sizeof(uint64_t)))
        return fail("out of device memory (root)", -1);
    if (use_rccl) {  // single-process form of SURVEY.md §8e: one communicator per device
        comms.assign((size_t)nd, nullptr);
        const ncclResult_t r = rccl().comm_init_all(comms.data(), nd, devices);
        if (r != ncclSuccess) {
            comms.clear();
            return fail(std::string("ncclCommInitAll: ") + rccl().error_string(r), -1);
        }
    }
    for (int g = 0; g < nd; ++g) (void)hipStreamSynchronize(streams[(size_t)g]);
    std::vector<tmpt_render_desc> ds((size_t)nd, *desc);
    std::vector<uint64_t> rays((size_t)nd, 0);
    const auto t0 = std::chrono::steady_clock::now();
    {  // every device renders its rows into its device tile, one host thread each
        std::vector<std::thread> th;
        for (int g = 0; g < nd; ++g)
            th.emplace_back([&, g]() {
                tmpt_render_desc& d = ds[(size_t)g];
                d.band_rows = 1;  // rows dealt round-robin: statistically equal shards
                d.shard = g;
                d.num_shards = nd;
                d.flags = TMPT_FLAG_OUT_DEVICE;
                rcs[(size_t)g] = tmpt_render(scenes[(size_t)g], cam, &d, d_tile[(size_t)g], &rays[(size_t)g]);
                if (rcs[(size_t)g]) errs[(size_t)g] = tmpt_last_error();
                else if (hipSetDevice(devices[g]) != hipSuccess ||
                         hipMemcpyAsync(d_rays[(size_t)g], &rays[(size_t)g], sizeof(uint64_t), hipMemcpyHostToDevice,
                                        streams[(size_t)g]) != hipSuccess ||
                         hipStreamSynchronize(streams[(size_t)g]) != hipSuccess)
                    rcs[(size_t)g] = -1, errs[(size_t)g] = "ray count upload failed";
            });
        for (auto& t : th) t.join();
    }
    for (int g = 0; g < nd; ++g)
        if (rcs[(size_t)g]) return fail(errs[(size_t)g], rcs[(size_t)g]);
    uint64_t total = 0;
    if (use_rccl) {
        // ONE gather of the equal-size padded tiles to device 0 over xGMI and a
        // uint64 sum of the ray counts, grouped (one thread drives every device)
        ncclResult_t r = rccl().group_start();
        for (int g = 0; g < nd && r == ncclSuccess; ++g) {
            r = rccl().gather(d_tile[(size_t)g], g == 0 ? d_gather : nullptr, tile_bytes, ncclUint8, 0,
                              comms[(size_t)g], streams[(size_t)g]);
            if (r == ncclSuccess)
                r = rccl().reduce(d_rays[(size_t)g], g == 0 ? d_total : nullptr, 1, ncclUint64, ncclSum, 0,
                                  comms[(size_t)g], streams[(size_t)g]);
        }
        const ncclResult_t re = rccl().group_end();
        if (r == ncclSuccess) r = re;
        if (r != ncclSuccess) return fail(std::string("RCCL gather: ") + rccl().error_string(r), -1);
        for (int g = 0; g < nd; ++g)
            if (hipSetDevice(devices[g]) != hipSuccess || hipStreamSynchronize(streams[(size_t)g]) != hipSuccess)
                return fail("gather failed", -1);
        (void)hipSetDevice(devices[0]);
        if (hipMemcpy(&total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
            return fail("ray count readback failed", -1);
    } else {
        // a device listed more than once (RCCL ranks need distinct devices):
        // the same gather as device-to-device copies into the root's buffer
        (void)hipSetDevice(devices[0]);
        for (int g = 0; g < nd; ++g) {
            if (hipMemcpyPeerAsync(d_gather + (size_t)g * tile_bytes, devices[0], d_tile[(size_t)g], devices[g],
                                   tile_bytes, streams[0]) != hipSuccess)
                return fail("device-to-device gather failed", -1);
            total += rays[(size_t)g];
        }
    }
    (void)hipSetDevice(devices[0]);
    k_assemble_rows<<<(unsigned)(((int64_t)W * H + 255) / 256), 256, 0, streams[0]>>>(
        reinterpret_cast<const uint32_t*>(d_gather.get()), nd, max_rows, W, H, d_frame);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(streams[0]) != hipSuccess)
        return fail("frame assembly failed", -1);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (hipMemcpy(rgba_full, d_frame, (size_t)W * H * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail("frame readback failed", -1);
    cleanup();
    if (ray_count) *ray_count = total;
    if (seconds) *seconds = dt;
    return 0;
    TMPT_GUARD_END
}

int tmpt_get_stats(const tmpt_scene* h, tmpt_stats* o)
{
    if (!h || !o) return bad("tmpt_get_stats: null argument");
    const Scene& s = h->s;
    memset(o, 0, sizeof(*o));
    o->render_ms = s.render_ms;
    o->extend_ms = s.extend_ms;
    o->shadow_ms = s.shadow_ms;
    o->extend_rays = s.extend_rays;
    o->shadow_rays = s.shadow_rays;
    o->extend_launches = s.extend_launches;
    o->shadow_launches = s.shadow_launches;
    o->iterations = s.iterations;
    o->node_visits = s.node_visits;
    o->tri_tests = s.tri_tests;
    o->shadow_node_visits = s.shadow_node_visits;
    o->shadow_tri_tests = s.shadow_tri_tests;
    o->build_ms = s.bvh.build_ms;
    o->bvh_nodes = s.bvh.n_nodes;
    o->bvh_depth = s.bvh.max_depth;
    o->n_tris = s.bvh.n;
    o->device = s.device;
    o->bvh4_nodes = s.bvh.n_nodes4;
    o->bvh4_depth = s.bvh.depth4;
    o->leaf_max = s.bvh.leaf_max;
    o->builder_iters = s.bvh.ploc_iters;
    o->octree_nodes = s.octree.n_oct;
    o->octree_leaves = s.octree.oct_leaves;
    o->octree_refs = s.octree.n_oct ? s.octree.n_oct_refs - s.octree.oct_leaves : 0;
    o->octree_build_ms = s.octree.oct_build_ms;
    o->tie_queries = s.tie_queries;
    o->root_misses = s.root_misses;
    o->row_engine = s.row_engine;
    o->stream_fallbacks = s.stream_fallbacks;
    o->octree_depth = s.octree.oct_depth;
    o->tie_rule = s.octree.oct && s.opt.tie_rule == 0 ? 0 : 1;
    o->chain_pixels = s.chain_pixels;
    o->redo_samples = s.redo_samples;
    o->redo_late = s.redo_late;
    o->crack_queries = s.crack_queries;
    o->octree_flat = s.octree.oct ? s.octree.oct_flat : 0;
    o->redo_launches = s.redo_launches;
    o->redo_ms = s.redo_ms;
    o->redo_rays = s.redo_rays;
    o->tie_path = s.tie_path;
    o->reserved_stats = 0;
    return 0;
}

int tmpt_scene_dump_bvh(const tmpt_scene* hc, int32_t layout, uint32_t* nodes, uint64_t node_words, uint32_t* tris,
                        uint64_t tri_words, int32_t info[8])
{
    TMPT_GUARD_BEGIN
    if (!hc || !info) return bad("tmpt_scene_dump_bvh: null argument");
    if (layout != 0 && layout != 1) return bad("tmpt_scene_dump_bvh: layout is 0 (aos) or 1 (soa)");
    if ((nodes == nullptr) != (tris == nullptr)) return bad("tmpt_scene_dump_bvh: give both buffers, or neither");
    Scene& s = const_cast<tmpt_scene*>(hc)->s;
    const bool has_soa = s.bvh.soa_buf != nullptr;
    if (layout == 1 && !has_soa) return bad("tmpt_scene_dump_bvh: the scene was built without layout=soa");
    const int32_t out[8] = {s.bvh.n, s.bvh.n_nodes4, s.bvh.depth4, s.bvh.leaf_max, s.bvh.count_shift, s.bvh.link_bits, s.bvh.ploc_iters,
                            has_soa ? 1 : 0};
    if (nodes && (node_words < 16u * (uint64_t)s.bvh.n_nodes4 || tri_words < 12u * ((uint64_t)s.bvh.n + 1u)))
        return bad("tmpt_scene_dump_bvh: short buffer (16 words per node, 12 per triangle record and one more)");
    memcpy(info, out, sizeof(out));
    if (!nodes) return 0;
    TMPT_HIP(hipSetDevice(s.device));
    return dump_bvh(s, layout == 1, nodes, tris);
    TMPT_GUARD_END
}

int tmpt_radix_sort(const tmpt_scene* hc, uint32_t* keys, uint32_t* vals, int64_t n, int32_t bits)
{
    TMPT_GUARD_BEGIN
    if (bits < 1 || bits > 32) return bad("tmpt_radix_sort: bits out of range (1 .. 32)");
    if (n < 0 || n > (int64_t)kRadixSortHookMax) return bad("tmpt_radix_sort: n out of range (0 .. 2^22)");
    if (n > 0 && (!keys || !vals)) return bad("tmpt_radix_sort: null argument");
    if (!hc) return bad("tmpt_radix_sort: null scene");
    if (n == 0) return 0;
    Scene& s = const_cast<tmpt_scene*>(hc)->s;
    TMPT_HIP(hipSetDevice(s.device));
    return radix_sort_host(s, keys, vals, (int32_t)n, bits);
    TMPT_GUARD_END
}

int tmpt_write_png(const char* path, const uint8_t* rgba, int32_t w, int32_t h)
{
    TMPT_GUARD_BEGIN
    if (!path || !rgba || w < 1 || h < 1) return bad("tmpt_write_png: bad arguments");
    return write_png(path, rgba, w, h);
    TMPT_GUARD_END
}

}  // extern "C"
