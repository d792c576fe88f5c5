// tmpt_api.cpp -- the C ABI of include/tmpt.h.  Status ints cross the
// boundary; no exception escapes (every entry point catches).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <stdexcept>
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

// The read-only keys of tmpt_scene_get_option, looked up before kOptions
// (bvh_cost, computed on first use, is the call's own case).
struct ReadOnlyKey {
    const char* name;
    double (*get)(const Scene&);
};
const ReadOnlyKey kReadOnly[] = {
    // the scene's layout under pop_key_cap
    {"pop_key_bits", [](const Scene& s) { return (double)pop_key_bits(s.bvh.link_bits, s.opt.pop_key_cap); }},
    // of the last render: it ran the camera pre-pass, the passes the shadow split ran, the path
    // kernel's waves per SIMD, k_split_resolve's time
    {"cam_rays_used", [](const Scene& s) { return (double)s.cam_rays_used; }},
    {"shadow_split_used", [](const Scene& s) { return (double)s.split_used; }},
    {"path_waves_used", [](const Scene& s) { return (double)s.path_waves_used; }},
    {"shadow_split_resolve_ms", [](const Scene& s) { return (double)s.split_resolve_ms; }},
    // of the last tmpt_scene_update: 0 none since creation, 1 refit, 2 rebuild; its device time
    {"update_kind", [](const Scene& s) { return (double)s.update_kind; }},
    {"update_ms", [](const Scene& s) { return (double)s.update_ms; }},
    // the process's live tmpt_device.h owners
    {"live_device_objects", [](const Scene&) { return (double)g_live_device_objects.load(); }},
    // of the last tmpt_scene_hit_device: device time, the keys + sort share, chunks, whether it sorted
    {"query_ms", [](const Scene& s) { return (double)s.query_ms; }},
    {"query_sort_ms", [](const Scene& s) { return (double)s.query_sort_ms; }},
    {"query_chunks", [](const Scene& s) { return (double)s.query_chunks; }},
    {"query_sorted", [](const Scene& s) { return (double)s.query_sorted; }},
};
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

// "<call>: <what>": an argument refused (-22), a device operation failed (-1)
int no(const char* name, const std::string& what) { return bad((std::string(name) + ": " + what).c_str()); }
int failed(const char* name, const char* what) { return (set_error(std::string(name) + ": " + what), -1); }

// ---------------------------------------------------------------- descriptor checks
// main.cpp:258-280 argument ranges: a frame's sides, and its spp where the call reads one
bool bad_side(int32_t v) { return v < 1 || v > 10000; }
int check_frame(const char* name, int32_t width, int32_t height, const int32_t* spp)
{
    if (bad_side(width)) return no(name, "invalid width");
    if (bad_side(height)) return no(name, "invalid height");
    if (spp && (*spp < 1 || *spp > 1024)) return no(name, "invalid samplesPerPixel");
    return 0;
}

// What one frame call asks of its tmpt_render_desc.  A null message: the field is not looked at.
enum SppRule {
    kSppUnread,       // spp_begin / spp_count are not looked at
    kSppRange,        // any pass inside 0 .. spp
    kSppProgressive,  // that, and a partial pass needs the persistent engine and pixel or sample seeding
    kSppZero,         // both 0: `spp_msg` says why
};
struct DescRules {
    bool spp;                // spp is read
    unsigned seeds;          // bit TMPT_SEED_* set: allowed
    const char* seed_msg;    // the refusal, with the call's own reason
    unsigned engines;        // bit TMPT_ENGINE_* set: allowed
    const char* engine_msg;
    SppRule spp_rule;
    const char* spp_msg;
    bool no_visits;          // TMPT_FLAG_COUNT_VISITS is refused
};
constexpr unsigned kSeedAny = 1u << TMPT_SEED_ROW | 1u << TMPT_SEED_PIXEL | 1u << TMPT_SEED_SAMPLE;
constexpr unsigned kSeedSample = 1u << TMPT_SEED_SAMPLE;
constexpr unsigned kEngineAny = 1u << TMPT_ENGINE_WAVEFRONT | 1u << TMPT_ENGINE_MEGAKERNEL | 1u << TMPT_ENGINE_PERSISTENT;
constexpr unsigned kEnginePersistent = 1u << TMPT_ENGINE_PERSISTENT;
constexpr const char* kMustPersist = "engine must be TMPT_ENGINE_PERSISTENT";

// The checks of a render descriptor, in the order every call has had them: sizes,
// seeding, engine, the sample range, the visit flag.  The shard comes before the
// sample range where a pass is allowed and last where it is not.
int check_render_desc(const char* name, const tmpt_render_desc* d, const DescRules& r)
{
    if (int rc = check_frame(name, d->width, d->height, r.spp ? &d->spp : nullptr)) return rc;
    const auto allowed = [](unsigned mask, int32_t v) { return v >= 0 && v < 32 && (mask >> v & 1u) != 0; };
    if (r.seed_msg && !allowed(r.seeds, d->seed_mode)) return no(name, r.seed_msg);
    if (r.engine_msg && !allowed(r.engines, d->engine)) return no(name, r.engine_msg);
    const bool bad_shard = d->num_shards > 1 && (d->shard < 0 || d->shard >= d->num_shards);
    if (r.spp_rule != kSppZero && bad_shard) return no(name, "invalid shard");
    if (r.spp_rule == kSppZero) {
        if (d->spp_begin != 0 || d->spp_count != 0) return no(name, r.spp_msg);
    } else if (r.spp_rule != kSppUnread) {
        if (d->spp_begin < 0 || d->spp_begin >= d->spp || d->spp_count < 0 || d->spp_count > d->spp - d->spp_begin)
            return no(name, "invalid spp_begin / spp_count");
        const bool progressive = d->spp_begin > 0 || (d->spp_count > 0 && d->spp_count < d->spp);
        if (r.spp_rule == kSppProgressive && progressive &&
            (d->engine != TMPT_ENGINE_PERSISTENT || d->seed_mode == TMPT_SEED_ROW))
            return no(name, "progressive spp needs the persistent engine and pixel or sample seeding");
    }
    if (r.no_visits && (d->flags & TMPT_FLAG_COUNT_VISITS)) return no(name, "TMPT_FLAG_COUNT_VISITS is not supported");
    if (bad_shard) return no(name, "invalid shard");
    return 0;
}

// Device pointers: each of `quads` on 16 bytes, each of `words` on 4 (a null pointer passes)
bool aligned(std::initializer_list<const void*> quads, std::initializer_list<const void*> words = {})
{
    uintptr_t q = 0, w = 0;
    for (const void* p : quads) q |= reinterpret_cast<uintptr_t>(p);
    for (const void* p : words) w |= reinterpret_cast<uintptr_t>(p);
    return (q & 15u) == 0 && (w & 3u) == 0;
}

// The whole-frame descriptors (tmpt_denoise, tmpt_temporal, tmpt_sample_plan, tmpt_temporal_clip)
int check_frame_flags(const char* name, int32_t flags)
{
    return flags & ~(TMPT_FLAG_OUT_DEVICE | TMPT_FLAG_WAIT_STREAM) ? no(name, "unknown flag") : 0;
}

// tmpt_temporal's defaults ("Temporal accumulation"), tmpt_sample_plan's too;
// tmpt_denoise_moments' default shrink and tmpt_temporal_clip's defaults: the grid points the rules of
// tools/noise_aware_sweep.py and tools/temporal_clip_sweep.py chose (profiles/temporal_clip_sweep.log,
// DESIGN.md section 4, "Noise-aware filter" and "History clipping")
constexpr float kTemporalNMax = 3.0f, kTemporalSigmaDepth = 0.05f;
constexpr float kShrinkDefault = 2.0f;
constexpr float kClipNMax = 3.0f, kClipGamma = 0.5f;
constexpr int32_t kClipRadius = 1;

// n_max and sigma_depth of a temporal descriptor: 0 takes the default, then the ranges
int temporal_defaults(const char* name, float n_max_default, float* n_max, float* sigma_depth)
{
    if (*n_max == 0.0f) *n_max = n_max_default;
    if (*sigma_depth == 0.0f) *sigma_depth = kTemporalSigmaDepth;
    if (!(*n_max >= 1.0f) || !(*n_max <= 3.0e38f)) return no(name, "n_max must be finite and at least 1 (0 = default)");
    if (!(*sigma_depth >= 0.0f) || !(*sigma_depth <= 3.0e38f))
        return no(name, "sigma_depth must be finite and not negative (0 = default)");
    return 0;
}

// No output frame may overlap an input frame whose neighbours the kernel reads (frames of
// `bytes` each; a null frame is absent)
struct NamedFrame {
    const void* p;
    const char* name;
};
int check_overlap(const char* name, size_t bytes, std::initializer_list<NamedFrame> outs,
                  std::initializer_list<NamedFrame> ins)
{
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    for (const NamedFrame& o : outs)
        for (const NamedFrame& i : ins)
            if (o.p && i.p && at(o.p) < at(i.p) + bytes && at(i.p) < at(o.p) + bytes)
                return no(name, std::string(o.name) + " overlaps " + i.name + " (its neighbours are read)");
    return 0;
}

// ---------------------------------------------------------------- staging
// A frame call's pointers are the caller's device memory (TMPT_FLAG_OUT_DEVICE: they
// pass through, nothing is copied) or host memory: then every frame gets a slot of
// one device buffer -- the call's own, freed on return, or one the scene keeps and
// grows -- inputs are copied in, the kernels run on the slots, and fetch() copies
// the outputs back.  The caller reserves room for the frames it will name (a null
// one is absent and takes none) before it names them; slots start on 16 bytes.
class Staging {
public:
    struct Frame {
        const void* p;
        size_t bytes;
    };
    explicit Staging(bool device) : device_(device) {}
    // false: out of device memory.  `kept`: the scene's buffer (synchronise its stream
    // first); `scratch_bytes`: room for a scratch() slot, in either form
    template <typename T>
    bool reserve(std::initializer_list<Frame> frames, DeviceBuffer<T>& kept, size_t scratch_bytes = 0)
    {
        size_t total = slot(scratch_bytes);
        for (const Frame& f : frames)
            if (!device_ && f.p) total += slot(f.bytes);
        if (!kept.reserve(total)) return false;
        base_ = reinterpret_cast<char*>(kept.get());
        cap_ = kept.bytes();
        return true;
    }
    bool reserve(std::initializer_list<Frame> frames, size_t scratch_bytes = 0)
    {
        return reserve(frames, own_, scratch_bytes);
    }
    // a slot nobody copies (a tile the kernels write and the caller did not ask for), in either form
    template <typename T>
    T* scratch(size_t bytes)
    {
        if (used_ + slot(bytes) > cap_) throw std::length_error("Staging: more slots than reserved");
        char* p = base_ + used_;
        used_ += slot(bytes);
        return reinterpret_cast<T*>(p);
    }
    // an input frame: copied into its slot (null stays null)
    template <typename T>
    const T* in(const void* p, size_t bytes)
    {
        if (device_ || !p || !bytes) return static_cast<const T*>(p);
        T* d = scratch<T>(bytes);
        if (ok_) ok_ = hipMemcpy(d, p, bytes, hipMemcpyHostToDevice) == hipSuccess;
        return d;
    }
    bool uploaded() const { return ok_; }
    // an output frame: a slot that fetch() copies to `p` (null stays null) ...
    template <typename T>
    T* out(void* p, size_t bytes)
    {
        return device_ || !p ? static_cast<T*>(p) : out_at<T>(p, scratch<T>(bytes), bytes);
    }
    // ... or the slot of a staged input, for a kernel that filters in place
    template <typename T>
    T* out_at(void* p, const T* staged, size_t bytes)
    {
        if (device_ || !p) return static_cast<T*>(p);
        back_.push_back({p, staged, bytes});
        return const_cast<T*>(staged);
    }
    bool fetch() const
    {
        for (const Back& b : back_)
            if (b.bytes && hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
        return true;
    }

private:
    struct Back {
        void* host;
        const void* dev;
        size_t bytes;
    };
    static size_t slot(size_t bytes) { return (bytes + 15) & ~(size_t)15; }  // slots start on 16 bytes
    const bool device_;
    DeviceBuffer<> own_;
    char* base_ = nullptr;
    size_t cap_ = 0, used_ = 0;
    bool ok_ = true;
    std::vector<Back> back_;
};

// Before a frame call's device work: a stale error of an earlier failed call cleared
// (launch checks read it), the scene's device made current
int enter(const Scene& s)
{
    (void)hipGetLastError();
    TMPT_HIP(hipSetDevice(s.device));
    return 0;
}

// After a frame call's run: the checked build's report (the render calls make one, the
// whole-frame filters none), then the staged outputs
int finish(int rc, Scene& s, const char* name, const Staging& st, bool report)
{
    if (!rc && report) rc = check_report(s, name);
    if (!rc && !st.fetch()) rc = failed(name, "readback failed");
    return rc;
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
    for (const ReadOnlyKey& k : kReadOnly)
        if (key && strcmp(key, k.name) == 0) return (*value = k.get(h->s), 0);
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
    const char* const fn = "tmpt_render";
    if (!h || !cam || !d || !rgba_out) return no(fn, "null argument");
    if (int rc = check_render_desc(fn, d, {true, kSeedAny, "invalid seed_mode", kEngineAny, "invalid engine",
                                           kSppProgressive, nullptr, false}))
        return rc;
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    const size_t bytes = (size_t)tmpt_tile_rows(d) * (size_t)d->width * 4;
    Staging st((d->flags & TMPT_FLAG_OUT_DEVICE) != 0);
    if (!st.reserve({{rgba_out, bytes}})) return no(fn, "out of device memory");
    const int rc = render(s, cam, d, st.out<uint32_t>(rgba_out, bytes), ray_count);
    return finish(rc, s, fn, st, true);
    TMPT_GUARD_END
}

int tmpt_render_aov(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, tmpt_aov_pixel* out,
                    uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_render_aov";
    if (!h || !cam || !d || !out) return no(fn, "null argument");
    if (int rc = check_render_desc(fn, d, {true, kSeedSample,
                                           "seed_mode must be TMPT_SEED_SAMPLE (the only seeding where a camera ray is a "
                                           "function of pixel and sample)",
                                           0, nullptr, kSppZero,
                                           "spp_begin / spp_count must be 0 (the pass is not progressive)", true}))
        return rc;
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && !aligned({out})) return no(fn, "a device output must be 16-byte aligned");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    const size_t bytes = (size_t)tmpt_tile_rows(d) * (size_t)d->width * sizeof(tmpt_aov_pixel);
    Staging st(dev_out);
    if (!st.reserve({{out, bytes}})) return no(fn, "out of device memory");
    const int rc = render_aov(s, cam, d, st.out<tmpt_aov_pixel>(out, bytes), ray_count);
    return finish(rc, s, fn, st, true);
    TMPT_GUARD_END
}

int tmpt_camera_rays(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, uint32_t* out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_camera_rays";
    if (!h || !cam || !d || !out) return no(fn, "null argument");
    if (int rc = check_render_desc(fn, d, {true, 0, nullptr, 0, nullptr, kSppRange, nullptr, false})) return rc;
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    return camera_rays(s, cam, d, out);
    TMPT_GUARD_END
}

int tmpt_render_radiance(tmpt_scene* h, const tmpt_camera* cam, const tmpt_render_desc* d, float* rgba32f_out,
                         uint8_t* rgba8_out, uint64_t* ray_count)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_render_radiance";
    if (!h || !cam || !d || !rgba32f_out) return no(fn, "null argument");
    if (int rc = check_render_desc(fn, d, {true, 1u << TMPT_SEED_PIXEL | kSeedSample,
                                           "seed_mode must be TMPT_SEED_PIXEL or TMPT_SEED_SAMPLE (row seeding keeps no "
                                           "float sum per pixel)",
                                           kEnginePersistent, kMustPersist, kSppZero,
                                           "spp_begin / spp_count must be 0 (whole renders only)", true}))
        return rc;
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && !aligned({rgba32f_out})) return no(fn, "a device rgba32f_out must be 16-byte aligned");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    const size_t px = (size_t)tmpt_tile_rows(d) * (size_t)d->width, fb = px * sizeof(float4), wb = px * 4;
    // the kernels write both tiles: a slot of the library's own stands in for an
    // rgba8_out the caller does not want, in the device form too
    Staging st(dev_out);
    if (!st.reserve({{rgba32f_out, fb}, {rgba8_out, wb}}, rgba8_out ? 0 : wb)) return no(fn, "out of device memory");
    float4* d_f = st.out<float4>(rgba32f_out, fb);
    uint32_t* d_8 = rgba8_out ? st.out<uint32_t>(rgba8_out, wb) : st.scratch<uint32_t>(wb);
    const int rc = render(s, cam, d, d_8, ray_count, d_f);
    return finish(rc, s, fn, st, true);
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
    if (!h || !cam || !d) return no(name, "null argument");
    if (int rc = check_render_desc(name, d, {true, kSeedSample,
                                             "seed_mode must be TMPT_SEED_SAMPLE (the only seeding where a sample is a "
                                             "function of pixel and sample)",
                                             kEnginePersistent, kMustPersist, kSppZero,
                                             "spp_begin / spp_count must be 0 (the call makes its own passes)", true}))
        return rc;
    tmpt_adaptive_desc r;  // the defaults, in one place ("Adaptive sampling")
    memset(&r, 0, sizeof(r));
    if (ad) r = *ad;
    else r.threshold = -1.0f;
    if (!ad && with_mom) r.spp_min = d->spp;  // uniform: one pass, every pixel at desc->spp
    if (r.spp_min == 0) r.spp_min = std::min(24, d->spp);
    if (r.spp_step == 0) r.spp_step = 8;
    if (!(r.threshold >= -3.0e38f) || !(r.threshold <= 3.0e38f))
        return no(name, "threshold must be finite (negative = default)");
    if (r.threshold < 0.0f) r.threshold = 0.015f;
    if (r.spp_min < 2 || r.spp_min > d->spp) return no(name, "spp_min outside 2 .. spp (0 = default)");
    if (r.spp_step < 1) return no(name, "spp_step must not be negative (0 = default)");
    if (r.radius < 0 || r.radius > 8) return no(name, "radius outside 0 .. 8 (0 = no neighbourhood rule)");
    if (1 + (d->spp - r.spp_min + r.spp_step - 1) / r.spp_step > 64)
        return no(name, "spp_min / spp_step give a schedule of more than 64 passes");
    if (guided) {
        if (!rgba32f_out && !moments_out && !rgba8_out && !spp_out)
            return no(name, "no output (rgba32f_out, moments_out, rgba8_out and spp_out are all null)");
    } else if (with_mom) {
        if (!moments_out) return no(name, "moments_out is required");
    } else if (!rgba32f_out && !rgba8_out && !spp_out) {
        return no(name, "no output (rgba32f_out, rgba8_out and spp_out are all null)");
    }
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && !aligned({rgba32f_out, moments_out}, {rgba8_out, spp_out}))
        return no(name, with_mom ? "device outputs must be aligned (rgba32f_out and moments_out 16 bytes, rgba8_out and "
                                   "spp_out 4)"
                                 : "device outputs must be aligned (rgba32f_out 16 bytes, rgba8_out and "
                                   "spp_out 4)");
    if (dev_out && !aligned({prior})) return no(name, "a device prior must be 16-byte aligned");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    const size_t px = (size_t)tmpt_tile_rows(d) * (size_t)d->width, fb = px * sizeof(float4), wb = px * 4;
    // host form: the outputs the caller asked for, and its prior beside them
    Staging st(dev_out);
    if (!st.reserve({{rgba32f_out, fb}, {moments_out, fb}, {rgba8_out, wb}, {spp_out, wb}, {prior, fb}}))
        return no(name, "out of device memory");
    const float4* d_p = st.in<float4>(prior, fb);
    if (!st.uploaded()) return failed(name, "upload failed");
    float4* d_f = st.out<float4>(rgba32f_out, fb);
    float4* d_m = st.out<float4>(moments_out, fb);
    uint32_t* d_8 = st.out<uint32_t>(rgba8_out, wb);
    int32_t* d_n = st.out<int32_t>(spp_out, wb);
    const int rc = render_adaptive(s, cam, d, &r, d_f, d_8, d_n, info, ray_count, d_m, name, d_p);
    return finish(rc, s, name, st, true);
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

// tmpt_denoise and tmpt_denoise_moments: one body.  `name` is the call's name in
// errors; with_mom: the moments frame is required and shrink is read.
static int denoise_call(const char* name, bool with_mom, tmpt_scene* h, const tmpt_denoise_desc* d, float shrink,
                        const float* rgba32f_in, const tmpt_aov_pixel* aov, const float* moments, float* rgba32f_out,
                        uint8_t* rgba8_out)
{
    // the descriptor first, before anything that needs a scene or a device
    if (!d) return no(name, "null descriptor");
    if (int rc = check_frame(name, d->width, d->height, &d->spp)) return rc;
    if (d->levels < 0 || d->levels > 6) return no(name, "levels out of range (1..6, 0 = 5)");
    if (d->normal_exp < -1 || d->normal_exp > 8) return no(name, "normal_exp out of range (0..8, -1 = 5)");
    if (!(d->sigma_depth >= 0.0f) || !(d->sigma_depth <= 3.0e38f))
        return no(name, "sigma_depth must be finite and not negative (0 = auto)");
    if (!(d->sigma_direct >= 0.0f) || !(d->sigma_direct <= 3.0e38f))
        return no(name, "sigma_direct must be finite and not negative (0 = default)");
    if (with_mom && (!(shrink >= 0.0f) || !(shrink <= 3.4028235e38f)))
        return no(name, "shrink must be finite and not negative (0 = default)");
    if (int rc = check_frame_flags(name, d->flags)) return rc;
    if (!rgba32f_out && !rgba8_out) return no(name, "no output (rgba32f_out and rgba8_out are both null)");
    if (!h || !rgba32f_in || !aov || (with_mom && !moments)) return no(name, "null argument");
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && !aligned({rgba32f_in, aov, moments, rgba32f_out}, {rgba8_out}))
        return no(name, "device pointers must be 16-byte aligned (rgba8_out: 4)");
    if (shrink == 0.0f) shrink = kShrinkDefault;
    tmpt_denoise_desc r = *d;  // the defaults, in one place
    if (r.levels == 0) r.levels = 5;
    if (r.normal_exp < 0) r.normal_exp = 5;
    if (r.sigma_depth == 0.0f) r.sigma_depth = 1.0f / (float)r.height;
    if (r.sigma_direct == 0.0f) r.sigma_direct = 0.05f;
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4), ab = n * sizeof(tmpt_aov_pixel);
    Staging st(dev);
    if (!st.reserve({{rgba32f_in, fb}, {aov, ab}, {moments, fb}, {rgba8_out, n * 4}}))
        return no(name, "out of device memory");
    const float4* d_in = st.in<float4>(rgba32f_in, fb);
    const tmpt_aov_pixel* d_aov = st.in<tmpt_aov_pixel>(aov, ab);
    const float4* d_mom = st.in<float4>(moments, fb);
    if (!st.uploaded()) return failed(name, "upload failed");
    float4* d_o32 = st.out_at<float4>(rgba32f_out, d_in, fb);  // host form: filtered in place in the staged input
    uint32_t* d_o8 = st.out<uint32_t>(rgba8_out, n * 4);
    const int rc = with_mom ? denoise_moments(s, &r, shrink, d_in, d_aov, d_mom, d_o32, d_o8)
                            : denoise(s, &r, d_in, d_aov, d_o32, d_o8);
    return finish(rc, s, name, st, false);
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
    const char* const fn = "tmpt_render_motion";
    // everything that needs no scene first, so that it is refused without a device
    if (!cam || !prev_cam || !d || !out) return no(fn, "null argument");
    if (int rc = check_render_desc(fn, d, {false, 0, nullptr, 0, nullptr, kSppUnread, nullptr, true})) return rc;
    const bool dev_out = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev_out && !aligned({out})) return no(fn, "a device output must be 16-byte aligned");
    if (!h) return no(fn, "null scene");
    Scene& s = h->s;
    if (prev_tris && prev_n != s.bvh.n)
        return no(fn, "prev_n differs from the scene's triangle count (the previous pose has the "
                      "scene's triangles, slot for slot)");
    if (int rc = enter(s)) return rc;
    Staging pose(dev_out), st(dev_out);
    const size_t pb = prev_tris ? sizeof(float) * 9 * (size_t)prev_n : 0;
    if (prev_tris && !dev_out) {  // a host pose: into the scene's kept buffer
        TMPT_HIP(hipStreamSynchronize(s.stream));
        if (!pose.reserve({{prev_tris, pb}}, s.motion_prev)) return no(fn, "out of device memory");
    }
    const float* d_prev = pose.in<float>(prev_tris, pb);
    if (!pose.uploaded()) return failed(fn, "upload failed");
    const size_t bytes = (size_t)tmpt_tile_rows(d) * (size_t)d->width * sizeof(tmpt_motion_pixel);
    if (!st.reserve({{out, bytes}})) return no(fn, "out of device memory");
    const int rc = render_motion(s, cam, prev_cam, d_prev, d, st.out<tmpt_motion_pixel>(out, bytes), ray_count);
    return finish(rc, s, fn, st, true);
    TMPT_GUARD_END
}

int tmpt_temporal(tmpt_scene* h, const tmpt_temporal_desc* d, const float* rgba32f_cur, const tmpt_motion_pixel* motion,
                  const tmpt_motion_pixel* prev_motion, const float* rgba32f_history, float* rgba32f_out,
                  uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_temporal";
    // the descriptor first, before anything that needs a scene or a device
    if (!d) return no(fn, "null descriptor");
    if (int rc = check_frame(fn, d->width, d->height, nullptr)) return rc;
    if (!rgba32f_cur || !motion || !prev_motion || !rgba32f_history) return no(fn, "null argument");
    if (!rgba32f_out && !rgba8_out) return no(fn, "no output (rgba32f_out and rgba8_out are both null)");
    tmpt_temporal_desc r = *d;
    if (int rc = temporal_defaults(fn, kTemporalNMax, &r.n_max, &r.sigma_depth)) return rc;
    if (int rc = check_frame_flags(fn, d->flags)) return rc;
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && !aligned({rgba32f_cur, motion, prev_motion, rgba32f_history, rgba32f_out}, {rgba8_out}))
        return no(fn, "device pointers must be 16-byte aligned (rgba8_out: 4)");
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4), mb = n * sizeof(tmpt_motion_pixel);
    if (int rc = check_overlap(fn, fb, {{rgba32f_out, "rgba32f_out"}}, {{rgba32f_history, "rgba32f_history"}})) return rc;
    if (!h) return no(fn, "null scene");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    Staging st(dev);
    if (!st.reserve({{rgba32f_cur, fb}, {rgba32f_history, fb}, {motion, mb}, {prev_motion, mb}, {rgba8_out, n * 4}}))
        return no(fn, "out of device memory");
    const float4* d_cur = st.in<float4>(rgba32f_cur, fb);
    const float4* d_hist = st.in<float4>(rgba32f_history, fb);
    const tmpt_motion_pixel* d_m = st.in<tmpt_motion_pixel>(motion, mb);
    const tmpt_motion_pixel* d_pm = st.in<tmpt_motion_pixel>(prev_motion, mb);
    if (!st.uploaded()) return failed(fn, "upload failed");
    float4* d_o32 = st.out_at<float4>(rgba32f_out, d_cur, fb);  // host form: blended in place in the staged frame
    uint32_t* d_o8 = st.out<uint32_t>(rgba8_out, n * 4);
    const int rc = temporal(s, &r, d_cur, d_m, d_pm, d_hist, d_o32, d_o8);
    return finish(rc, s, fn, st, false);
    TMPT_GUARD_END
}

int tmpt_sample_plan(tmpt_scene* h, const tmpt_temporal_desc* d, const tmpt_motion_pixel* motion,
                     const tmpt_motion_pixel* prev_motion, const float* moments_history, float* prior_out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_sample_plan";
    // tmpt_temporal's checks in its order, its colour frames left out
    if (!d) return no(fn, "null descriptor");
    if (int rc = check_frame(fn, d->width, d->height, nullptr)) return rc;
    if (!motion || !prev_motion || !moments_history || !prior_out) return no(fn, "null argument");
    tmpt_temporal_desc r = *d;
    if (int rc = temporal_defaults(fn, kTemporalNMax, &r.n_max, &r.sigma_depth)) return rc;
    if (int rc = check_frame_flags(fn, d->flags)) return rc;
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && !aligned({motion, prev_motion, moments_history, prior_out}))
        return no(fn, "device pointers must be 16-byte aligned");
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4), mb = n * sizeof(tmpt_motion_pixel);
    if (int rc = check_overlap(fn, fb, {{prior_out, "prior_out"}}, {{moments_history, "moments_history"}})) return rc;
    if (!h) return no(fn, "null scene");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    Staging st(dev);  // host form: in the scene's kept buffer, as tmpt_temporal_clip stages its own
    if (!dev) TMPT_HIP(hipStreamSynchronize(s.stream));
    if (!st.reserve({{moments_history, fb}, {motion, mb}, {prev_motion, mb}, {prior_out, fb}}, s.clip_stage))
        return no(fn, "out of device memory");
    const float4* d_hist = st.in<float4>(moments_history, fb);
    const tmpt_motion_pixel* d_m = st.in<tmpt_motion_pixel>(motion, mb);
    const tmpt_motion_pixel* d_pm = st.in<tmpt_motion_pixel>(prev_motion, mb);
    if (!st.uploaded()) return failed(fn, "upload failed");
    const int rc = sample_plan(s, &r, d_m, d_pm, d_hist, st.out<float4>(prior_out, fb));
    return finish(rc, s, fn, st, false);
    TMPT_GUARD_END
}

int tmpt_temporal_clip(tmpt_scene* h, const tmpt_temporal_clip_desc* d, const float* rgba32f_cur,
                       const float* rgba32f_stat, const tmpt_motion_pixel* motion, const tmpt_motion_pixel* prev_motion,
                       const float* rgba32f_history, const float* aux_cur, const float* aux_history, float* aux_out,
                       float* rgba32f_out, uint8_t* rgba8_out)
{
    TMPT_GUARD_BEGIN
    const char* const fn = "tmpt_temporal_clip";
    // tmpt_temporal's checks in its order, the new ones where the header puts them
    if (!d) return no(fn, "null descriptor");
    if (int rc = check_frame(fn, d->width, d->height, nullptr)) return rc;
    if (!rgba32f_cur || !motion || !prev_motion || !rgba32f_history) return no(fn, "null argument");
    if ((aux_cur || aux_history || aux_out) && (!aux_cur || !aux_history || !aux_out))
        return no(fn, "null argument (aux_cur, aux_history and aux_out: all three or none)");
    if (!rgba32f_out && !rgba8_out) return no(fn, "no output (rgba32f_out and rgba8_out are both null)");
    tmpt_temporal_clip_desc r = *d;  // the defaults, in one place
    if (r.gamma == 0.0f) r.gamma = kClipGamma;
    if (r.radius == 0) r.radius = kClipRadius;
    if (int rc = temporal_defaults(fn, kClipNMax, &r.n_max, &r.sigma_depth)) return rc;
    if (!(r.gamma >= 0.0f) || !(r.gamma <= 3.0e38f)) return no(fn, "gamma must be finite and not negative (0 = default)");
    if (r.radius < 1 || r.radius > 3) return no(fn, "radius must be 1, 2 or 3 (0 = default)");
    if (int rc = check_frame_flags(fn, d->flags)) return rc;
    const bool dev = (d->flags & TMPT_FLAG_OUT_DEVICE) != 0;
    if (dev && !aligned({rgba32f_cur, rgba32f_stat, motion, prev_motion, rgba32f_history, aux_cur, aux_history, aux_out,
                         rgba32f_out},
                        {rgba8_out}))
        return no(fn, "device pointers must be 16-byte aligned (rgba8_out: 4)");
    const size_t n = (size_t)r.width * (size_t)r.height, fb = n * sizeof(float4), mb = n * sizeof(tmpt_motion_pixel);
    if (int rc = check_overlap(fn, fb, {{rgba32f_out, "rgba32f_out"}, {aux_out, "aux_out"}},
                               {{rgba32f_history, "rgba32f_history"}, {aux_history, "aux_history"},
                                {rgba32f_cur, "rgba32f_cur"}, {rgba32f_stat, "rgba32f_stat"}}))
        return rc;
    if (!h) return no(fn, "null scene");
    Scene& s = h->s;
    if (int rc = enter(s)) return rc;
    Staging st(dev);  // host form: in the scene's kept buffer, frame after frame
    if (!dev) TMPT_HIP(hipStreamSynchronize(s.stream));
    if (!st.reserve({{rgba32f_cur, fb}, {rgba32f_history, fb}, {motion, mb}, {prev_motion, mb}, {rgba32f_stat, fb},
                     {aux_cur, fb}, {aux_history, fb}, {aux_out, fb}, {rgba32f_out, fb}, {rgba8_out, n * 4}},
                    s.clip_stage))
        return no(fn, "out of device memory");
    const float4* d_cur = st.in<float4>(rgba32f_cur, fb);
    const float4* d_hist = st.in<float4>(rgba32f_history, fb);
    const tmpt_motion_pixel* d_m = st.in<tmpt_motion_pixel>(motion, mb);
    const tmpt_motion_pixel* d_pm = st.in<tmpt_motion_pixel>(prev_motion, mb);
    const float4* d_stat = st.in<float4>(rgba32f_stat, fb);
    const float4* d_ac = st.in<float4>(aux_cur, fb);
    const float4* d_ah = st.in<float4>(aux_history, fb);
    if (!st.uploaded()) return failed(fn, "upload failed");
    float4* d_o32 = st.out<float4>(rgba32f_out, fb);
    float4* d_ao = st.out<float4>(aux_out, fb);
    uint32_t* d_o8 = st.out<uint32_t>(rgba8_out, n * 4);
    const int rc = temporal_clip(s, &r, d_cur, d_stat ? d_stat : d_cur, d_m, d_pm, d_hist, d_ac, d_ah, d_ao, d_o32, d_o8);
    return finish(rc, s, fn, st, false);
    TMPT_GUARD_END
}

int tmpt_render_multi(const float* tris, int32_t n, const float* octree_box, const tmpt_camera* cam,
                      const tmpt_render_desc* desc, const int32_t* devices, int32_t ndevices, uint8_t* rgba_full,
                      uint64_t* ray_count, double* seconds)
{
    TMPT_GUARD_BEGIN
    if (!cam || !desc || !devices || ndevices < 1 || !rgba_full || (n > 0 && !tris))
        return bad("tmpt_render_multi: bad arguments");
    if (bad_side(desc->width) || bad_side(desc->height))
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
