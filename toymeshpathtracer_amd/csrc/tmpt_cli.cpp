// tmpt_cli.cpp -- the reference's command line (main.cpp:248-345) over the C ABI:
//   tmpt <width> <height> <spp> <objFile> [--seed row|pixel|sample] [--engine persistent|wavefront|mega]
//        [--gpus N] [--device D] [--out output.png] [--aov PREFIX] [--denoise OUT.png [--shrink K]]
//        [--adaptive TAU[,MIN[,STEP[,RADIUS]]]] [--spp-map OUT.png]
//        [--twist DEG,FRAMES [--rebuild] [--temporal [--clip [GAMMA[,RADIUS[,NMAX]]]] [--guided [MIN[,STEP[,TAU[,CAP]]]]]]]
//        [--octree host|device]
// Defaults reproduce the reference: row seeding (main.cpp:204) and output.png.
// Row seeding runs the speculative row engine on the persistent engine (every even RNG offset
// of a window traced, the chain walked through it) and one lane per row with
// --engine mega; pixel or sample seeding make every pixel or sample independent
// work.  With --gpus N (tmpt_render_multi) the rows
// are dealt round-robin one at a time (row y to device y % N), one host thread
// per device, and the tiles are assembled into the frame.
// --aov PREFIX (one device only): after the frame, the AOV pass (tmpt_render_aov) at the same
// size and spp on the same device, written as PREFIX_normal.png, PREFIX_direct.png and
// PREFIX_depth.png.
// --denoise OUT.png (one device, --seed sample): beside the usual output, the frame's float
// radiance (tmpt_render_radiance) filtered by tmpt_denoise with the AOV records as guides.
// --shrink K (with --denoise): the noise-aware filter instead -- the radiance comes with its luminance
// moments (tmpt_render_moments: uniform at spp, which must then be at least 2, or the --adaptive
// schedule) and tmpt_denoise_moments filters it with shrink K (0 = the default).  Without --shrink
// nothing changes.
// --adaptive TAU[,MIN[,STEP[,RADIUS]]] (one device, --seed sample): the frame comes from tmpt_render_adaptive
// with spp as the cap (MIN, STEP: spp_min, spp_step; left out or 0 = the defaults, a negative TAU
// too; RADIUS 0..8, left out = 0: the neighbourhood rule -- a pixel goes on while the test holds for
// any pixel within RADIUS columns and rows of it, the whole frame being one band); --spp-map OUT.png writes the samples each pixel got, n_p / spp, as grey.  With --denoise
// the filter takes the adaptive radiance; the AOV pass stays at spp.
// --twist DEG,FRAMES [--rebuild] (one device): an animation on one scene handle.  Frame f renders the
// mesh, floor included, twisted about the vertical (y) axis through the centre of its bounds by
// DEG * f / (FRAMES - 1) at the top and nothing at the bottom; each frame is one tmpt_scene_update
// (a refit; --rebuild: the full build) and the octree built again over the twisted mesh's bounds, the
// camera staying frame 0's.  The frames go to OUT_000.png, OUT_001.png, ... (OUT: --out less its
// .png); per frame the update's device time and the tree's bvh_cost are printed.
// --temporal (with --twist, --seed sample, the persistent engine, a refit): temporal accumulation over the
// sequence.  Frame f sets the option sample_base to f * spp, so no frame repeats another's random
// numbers, renders its radiance (tmpt_render_radiance; its packed pixels are the plain frame), runs
// the motion pass (tmpt_render_motion) against frame f-1's triangles and the same camera, and blends
// (tmpt_temporal, its defaults) with the accumulation kept from frame f-1; frame 0's accumulation is
// frame 0 itself.  The accumulated frames go to OUT_temporal_000.png, ... beside the plain ones.
// --clip [GAMMA[,RADIUS[,NMAX]]] (with --temporal): the blend is tmpt_temporal_clip instead -- the history
// clipped to GAMMA standard deviations of the frame's own (2 RADIUS + 1)^2 window, capped at NMAX (left out
// or 0 = that call's defaults) -- into the same files.  Without --clip nothing changes.
// --guided [MIN[,STEP[,TAU[,CAP]]]] (with --temporal): history-guided sampling.  Frame f sets sample_base to
// f * CAP and runs the motion pass first, then the sample plan (tmpt_sample_plan) over the accumulated moments
// of frame f-1 with the blend's n_max, then the guided render (tmpt_render_guided: spp_min MIN, left out or 0 = 2;
// spp_step STEP and threshold TAU, left out or 0 / negative = the adaptive defaults; the cap CAP, left out or
// 0 = spp) with its moments, then the blend: tmpt_temporal_clip with the moments frame as aux, or without --clip
// tmpt_temporal twice, once on the colour frame and once on the moments frame.  The accumulated colour and
// moments are the next frame's history; frame 0 has no prior.  --spp-map OUT.png then writes one map per frame,
// OUT_000.png, ... (n_p / CAP as grey).  Without --guided nothing changes.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "tmpt.h"

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static float saturate(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// --octree host|device: where every scene of this run builds its octree (option octree_build)
static int g_octree_device = 0;
static int build_octree(tmpt_scene* scene, const float box[6])
{
    if (g_octree_device)
        if (int rc = tmpt_scene_set_option(scene, "octree_build", 1.0)) return rc;
    return tmpt_scene_build_octree(scene, box, box + 3);
}

// The AOV pass on `device` (its own scene, the octree built as for the frame) and its three
// images, all float32 maps, alpha 255:
//   PREFIX_normal.png  uint8(saturate(n * 0.5 + 0.5) * 255) per channel
//   PREFIX_direct.png  grey uint8(saturate(sqrtf(direct)) * 255)
//   PREFIX_depth.png   grey over the pixels with hits > 0 of d = depth * spp / hits:
//                      uint8((1 - (d - dmin) / (dmax - dmin)) * 255), dmin / dmax over those
//                      pixels (dmax == dmin: 255); a pixel without a hit is 0
static int write_aovs(const char* prefix, const float* tris, int32_t n, const float box[6], const tmpt_camera* cam,
                      int w, int h, int spp, int device)
{
    tmpt_scene* scene = nullptr;
    if (tmpt_scene_create(tris, n, device, &scene)) return 1;
    std::vector<tmpt_aov_pixel> rec((size_t)w * h);
    tmpt_render_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.width = w; desc.height = h; desc.spp = spp; desc.seed_mode = TMPT_SEED_SAMPLE;
    uint64_t rays = 0;
    int rc = build_octree(scene, box);
    if (!rc) rc = tmpt_render_aov(scene, cam, &desc, rec.data(), &rays);
    tmpt_stats st;
    if (!rc) rc = tmpt_get_stats(scene, &st);
    // (a failed call's message survives the destroy: only failures set it)
    if (tmpt_scene_destroy(scene) && !rc) rc = 1;
    if (rc) return rc;
    printf("AOV pass: %.1f K Rays in %.3f ms\n", rays / 1000.0, st.render_ms);
    const size_t P = rec.size();
    std::vector<float> depth(P, 0.0f);
    float dmin = INFINITY, dmax = -INFINITY;
    for (size_t i = 0; i < P; ++i) {
        if (rec[i].hits == 0) continue;
        const float d = rec[i].depth * (float)spp / (float)rec[i].hits;
        depth[i] = d;
        dmin = d < dmin ? d : dmin;
        dmax = d > dmax ? d : dmax;
    }
    std::vector<uint8_t> img[3];
    for (auto& v : img) v.assign(P * 4, 255);
    for (size_t i = 0; i < P; ++i) {
        for (int c = 0; c < 3; ++c) {
            const float m = rec[i].normal[c] * 0.5f;
            img[0][4 * i + c] = (uint8_t)(saturate(m + 0.5f) * 255.0f);
        }
        const uint8_t g = (uint8_t)(saturate(sqrtf(rec[i].direct)) * 255.0f);
        uint8_t z = 0;
        if (rec[i].hits != 0) {
            const float num = depth[i] - dmin, den = dmax - dmin;
            const float q = num / den;
            z = dmax == dmin ? (uint8_t)255 : (uint8_t)((1.0f - q) * 255.0f);
        }
        for (int c = 0; c < 3; ++c) img[1][4 * i + c] = g, img[2][4 * i + c] = z;
    }
    const char* names[3] = {"_normal.png", "_direct.png", "_depth.png"};
    for (int k = 0; k < 3; ++k)
        if (tmpt_write_png((std::string(prefix) + names[k]).c_str(), img[k].data(), w, h)) return 1;
    return 0;
}

// --denoise OUT.png on `device` (its own scene, the octree built as for the frame): the
// sample-seeded radiance render (tmpt_render_radiance), the AOV pass at the same size and spp
// (tmpt_render_aov) and the filter with its defaults (tmpt_denoise); the filtered frame's
// packed pixels are written to `path`.  shrink (--shrink; null without): the radiance comes from
// tmpt_render_moments instead, uniform at spp, and tmpt_denoise_moments filters it.
static int write_denoised(const char* path, const float* tris, int32_t n, const float box[6], const tmpt_camera* cam,
                          int w, int h, int spp, int device, const float* shrink)
{
    tmpt_scene* scene = nullptr;
    if (tmpt_scene_create(tris, n, device, &scene)) return 1;
    const size_t P = (size_t)w * h;
    std::vector<float> rad(P * 4), mom(shrink ? P * 4 : 0);
    std::vector<tmpt_aov_pixel> rec(P);
    std::vector<uint8_t> img(P * 4);
    tmpt_render_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.width = w; desc.height = h; desc.spp = spp; desc.seed_mode = TMPT_SEED_SAMPLE;
    desc.engine = TMPT_ENGINE_PERSISTENT;
    tmpt_denoise_desc dn;
    memset(&dn, 0, sizeof(dn));
    dn.width = w; dn.height = h; dn.spp = spp; dn.normal_exp = -1;
    uint64_t rays = 0, aov_rays = 0;
    tmpt_stats st;
    int rc = build_octree(scene, box);
    if (!rc && shrink)
        rc = tmpt_render_moments(scene, cam, &desc, nullptr, rad.data(), mom.data(), nullptr, nullptr, nullptr, &rays);
    else if (!rc)
        rc = tmpt_render_radiance(scene, cam, &desc, rad.data(), nullptr, &rays);
    if (!rc) rc = tmpt_render_aov(scene, cam, &desc, rec.data(), &aov_rays);
    if (!rc && shrink)
        rc = tmpt_denoise_moments(scene, &dn, *shrink, rad.data(), rec.data(), mom.data(), nullptr, img.data());
    else if (!rc)
        rc = tmpt_denoise(scene, &dn, rad.data(), rec.data(), nullptr, img.data());
    if (!rc) rc = tmpt_get_stats(scene, &st);
    if (tmpt_scene_destroy(scene) && !rc) rc = 1;
    if (rc) return rc;
    printf("Denoised frame%s: %.1f K Rays + %.1f K AOV Rays, filter %.3f ms\n", shrink ? " (noise-aware)" : "",
           rays / 1000.0, aov_rays / 1000.0, st.render_ms);
    return tmpt_write_png(path, img.data(), w, h);
}

// --adaptive on `device` (its own scene, the octree built as for a frame): the adaptive render
// into `image` (what --out writes), the spp map as grey uint8(n_p / spp * 255) and, with
// `denoised`, the filter over the adaptive radiance guided by the AOV pass at spp.  shrink (--shrink
// with --denoise; null without): the call is tmpt_render_moments and the filter tmpt_denoise_moments.
static int render_adaptive_frame(const float* tris, int32_t n, const float box[6], const tmpt_camera* cam, int w, int h,
                                 int spp, int device, const tmpt_adaptive_desc* ad, std::vector<uint8_t>& image,
                                 const char* spp_map, const char* denoised, const float* shrink)
{
    tmpt_scene* scene = nullptr;
    if (tmpt_scene_create(tris, n, device, &scene)) return 1;
    const size_t P = (size_t)w * h;
    std::vector<float> rad(P * 4), mom(shrink ? P * 4 : 0);
    std::vector<int32_t> cnt(P);
    tmpt_render_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.width = w; desc.height = h; desc.spp = spp; desc.seed_mode = TMPT_SEED_SAMPLE;
    desc.engine = TMPT_ENGINE_PERSISTENT;
    tmpt_adaptive_info info;
    tmpt_stats st;
    uint64_t rays = 0;
    int rc = build_octree(scene, box);
    if (!rc && shrink)
        rc = tmpt_render_moments(scene, cam, &desc, ad, rad.data(), mom.data(), image.data(), cnt.data(), &info, &rays);
    else if (!rc)
        rc = tmpt_render_adaptive(scene, cam, &desc, ad, rad.data(), image.data(), cnt.data(), &info, &rays);
    if (!rc) rc = tmpt_get_stats(scene, &st);
    if (!rc) {
        printf("Rendered scene at %ix%i, up to %ispp, adaptively in %.3f s (%d passes)\n", w, h, spp,
               st.render_ms / 1000.0, info.passes);
        printf("- %llu of %llu samples traced (%.1f%%), %.1f K Rays, %.1f K Rays/s\n",
               (unsigned long long)info.samples, (unsigned long long)P * spp, 100.0 * info.samples / ((double)P * spp),
               rays / 1000.0, rays / 1000.0 / (st.render_ms / 1000.0));
        if (spp_map) {
            std::vector<uint8_t> grey(P * 4, 255);
            for (size_t i = 0; i < P; ++i)
                for (int c = 0; c < 3; ++c) grey[4 * i + c] = (uint8_t)((float)cnt[i] / (float)spp * 255.0f);
            rc = tmpt_write_png(spp_map, grey.data(), w, h);
        }
    }
    if (!rc && denoised) {
        std::vector<tmpt_aov_pixel> rec(P);
        std::vector<uint8_t> img(P * 4);
        tmpt_denoise_desc dn;
        memset(&dn, 0, sizeof(dn));
        dn.width = w; dn.height = h; dn.spp = spp; dn.normal_exp = -1;
        uint64_t aov_rays = 0;
        rc = tmpt_render_aov(scene, cam, &desc, rec.data(), &aov_rays);
        if (!rc && shrink)
            rc = tmpt_denoise_moments(scene, &dn, *shrink, rad.data(), rec.data(), mom.data(), nullptr, img.data());
        else if (!rc)
            rc = tmpt_denoise(scene, &dn, rad.data(), rec.data(), nullptr, img.data());
        if (!rc) rc = tmpt_get_stats(scene, &st);
        if (!rc) {
            printf("Denoised adaptive frame%s: %.1f K AOV Rays, filter %.3f ms\n", shrink ? " (noise-aware)" : "",
                   aov_rays / 1000.0, st.render_ms);
            rc = tmpt_write_png(denoised, img.data(), w, h);
        }
    }
    if (tmpt_scene_destroy(scene) && !rc) rc = 1;
    return rc;
}

// --twist: see the head of this file.  tris: the n triangles of tmpt_load_obj (the last two are the floor).
static int render_twist(const float* tris, int32_t n, const tmpt_camera* cam, const tmpt_render_desc* desc, int device,
                        double degrees, int frames, bool rebuild, bool temporal, const tmpt_temporal_clip_desc* clip,
                        const char* out, const tmpt_adaptive_desc* guided = nullptr, int cap = 0,
                        const char* spp_map = nullptr)
{
    tmpt_scene* scene = nullptr;
    if (tmpt_scene_create(tris, n, device, &scene)) return 1;
    const int w = desc->width, h = desc->height;
    std::vector<uint8_t> image((size_t)w * h * 4, 0);
    std::vector<float> cur((size_t)n * 9);
    // --temporal: the previous pose, this frame's radiance, the accumulation, both frames' motion records
    std::vector<float> prev, rad, acc, clipped;
    std::vector<tmpt_motion_pixel> mot, pmot;
    std::vector<uint8_t> timage;
    // --guided: this frame's moments, their accumulation, the prior, the counts
    std::vector<float> mom, macc, mout, prior;
    std::vector<int32_t> cnt;
    tmpt_render_desc gdesc = *desc;
    if (guided) {
        gdesc.spp = cap;
        mom.resize((size_t)w * h * 4);
        mout.resize((size_t)w * h * 4);
        prior.resize((size_t)w * h * 4);
        cnt.resize((size_t)w * h);
    }
    std::string map_stem(spp_map ? spp_map : "");
    if (map_stem.size() > 4 && map_stem.compare(map_stem.size() - 4, 4, ".png") == 0) map_stem.resize(map_stem.size() - 4);
    if (temporal) {
        rad.resize((size_t)w * h * 4);
        mot.resize((size_t)w * h);
        timage.resize((size_t)w * h * 4);
    }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < (size_t)n * 3; ++i)
        for (int c = 0; c < 3; ++c) {
            lo[c] = fmin(lo[c], (double)tris[3 * i + c]);
            hi[c] = fmax(hi[c], (double)tris[3 * i + c]);
        }
    const double cx = 0.5 * (lo[0] + hi[0]), cz = 0.5 * (lo[2] + hi[2]), height = hi[1] - lo[1];
    std::string stem(out);
    if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".png") == 0) stem.resize(stem.size() - 4);
    int rc = 0;
    for (int f = 0; f < frames && !rc; ++f) {
        const double full = degrees * (frames > 1 ? (double)f / (frames - 1) : 1.0) * 3.14159265358979323846 / 180.0;
        float bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = 0; i < (size_t)n * 3; ++i) {
            const double x = tris[3 * i] - cx, y = tris[3 * i + 1], z = tris[3 * i + 2] - cz;
            const double a = height > 0.0 ? full * (y - lo[1]) / height : 0.0;
            cur[3 * i] = (float)(cx + cos(a) * x + sin(a) * z);
            cur[3 * i + 1] = tris[3 * i + 1];
            cur[3 * i + 2] = (float)(cz - sin(a) * x + cos(a) * z);
            if (i + 6 < (size_t)n * 3 || n <= 2)  // the mesh's bounds: the two floor triangles come last
                for (int c = 0; c < 3; ++c) {
                    bmin[c] = fminf(bmin[c], cur[3 * i + c]);
                    bmax[c] = fmaxf(bmax[c], cur[3 * i + c]);
                }
        }
        float box[6];
        double ms = 0.0, cost = 0.0;
        uint64_t rays = 0;
        tmpt_stats st;
        if (temporal) rc = tmpt_scene_set_option(scene, "sample_base", (double)f * (guided ? cap : desc->spp));
        if (!rc) rc = tmpt_scene_update(scene, cur.data(), n, rebuild ? TMPT_UPDATE_REBUILD : TMPT_UPDATE_REFIT);
        if (!rc) rc = tmpt_octree_bounds(bmin, bmax, box);
        if (!rc) rc = build_octree(scene, box);
        if (!rc) rc = tmpt_scene_get_option(scene, "update_ms", &ms);
        if (!rc) rc = tmpt_scene_get_option(scene, "bvh_cost", &cost);
        tmpt_adaptive_info ginfo;
        memset(&ginfo, 0, sizeof(ginfo));
        if (!rc && guided) {  // motion, then the plan, then the guided render with its moments
            tmpt_temporal_desc pd;
            memset(&pd, 0, sizeof(pd));
            pd.width = w;
            pd.height = h;
            pd.n_max = clip ? clip->n_max : 0.0f;
            pd.sigma_depth = clip ? clip->sigma_depth : 0.0f;
            rc = tmpt_render_motion(scene, cam, cam, f ? prev.data() : nullptr, n, desc, mot.data(), nullptr);
            if (!rc && f) rc = tmpt_sample_plan(scene, &pd, mot.data(), pmot.data(), macc.data(), prior.data());
            if (!rc)
                rc = tmpt_render_guided(scene, cam, &gdesc, guided, f ? prior.data() : nullptr, rad.data(), mom.data(),
                                        image.data(), cnt.data(), &ginfo, &rays);
        }
        if (!rc && !temporal) rc = tmpt_render(scene, cam, desc, image.data(), &rays);
        if (!rc && temporal && !guided) rc = tmpt_render_radiance(scene, cam, desc, rad.data(), image.data(), &rays);
        if (!rc) rc = tmpt_get_stats(scene, &st);
        if (!rc && guided) {  // the blend carries the moments along
            if (f == 0) {
                acc = rad;
                macc = mom;
                timage = image;
            } else if (clip) {
                tmpt_temporal_clip_desc cd = *clip;
                cd.width = w;
                cd.height = h;
                clipped.resize(rad.size());
                rc = tmpt_temporal_clip(scene, &cd, rad.data(), nullptr, mot.data(), pmot.data(), acc.data(), mom.data(),
                                        macc.data(), mout.data(), clipped.data(), timage.data());
                if (!rc) acc.swap(clipped), macc.swap(mout);
            } else {
                tmpt_temporal_desc td;
                memset(&td, 0, sizeof(td));
                td.width = w;
                td.height = h;
                rc = tmpt_temporal(scene, &td, rad.data(), mot.data(), pmot.data(), acc.data(), rad.data(), timage.data());
                if (!rc) rc = tmpt_temporal(scene, &td, mom.data(), mot.data(), pmot.data(), macc.data(), mom.data(), nullptr);
                if (!rc) acc.swap(rad), macc.swap(mom);
            }
            pmot = mot;
            prev = cur;
            if (!rc) {
                printf("frame %d: guided, %d passes, %llu of %llu samples traced (%.1f%%)\n", f, ginfo.passes,
                       (unsigned long long)ginfo.samples, (unsigned long long)w * h * cap,
                       100.0 * ginfo.samples / ((double)w * h * cap));
                if (spp_map) {
                    std::vector<uint8_t> grey((size_t)w * h * 4, 255);
                    for (size_t i = 0; i < (size_t)w * h; ++i)
                        for (int c = 0; c < 3; ++c) grey[4 * i + c] = (uint8_t)((float)cnt[i] / (float)cap * 255.0f);
                    char mname[32];
                    snprintf(mname, sizeof(mname), "_%03d.png", f);
                    rc = tmpt_write_png((map_stem + mname).c_str(), grey.data(), w, h);
                }
            }
        } else if (!rc && temporal) {
            rc = tmpt_render_motion(scene, cam, cam, f ? prev.data() : nullptr, n, desc, mot.data(), nullptr);
            if (!rc && f == 0) {  // a history of length one
                acc = rad;
                timage = image;
            } else if (!rc && clip) {  // (its output may not be the frame itself)
                tmpt_temporal_clip_desc cd = *clip;
                cd.width = w;
                cd.height = h;
                clipped.resize(rad.size());
                rc = tmpt_temporal_clip(scene, &cd, rad.data(), nullptr, mot.data(), pmot.data(), acc.data(), nullptr,
                                        nullptr, nullptr, clipped.data(), timage.data());
                if (!rc) acc.swap(clipped);
            } else if (!rc) {
                tmpt_temporal_desc td;
                memset(&td, 0, sizeof(td));
                td.width = w;
                td.height = h;
                rc = tmpt_temporal(scene, &td, rad.data(), mot.data(), pmot.data(), acc.data(), rad.data(), timage.data());
                if (!rc) acc.swap(rad);
            }
            pmot = mot;
            prev = cur;
        }
        if (rc) break;
        if (temporal) {
            char tname[32];
            snprintf(tname, sizeof(tname), "_temporal_%03d.png", f);
            rc = tmpt_write_png((stem + tname).c_str(), timage.data(), w, h);
            if (rc) break;
        }
        char name[32];
        snprintf(name, sizeof(name), "_%03d.png", f);
        printf("frame %d: twist %.2f deg, %s %.3f ms, bvh_cost %.3f, %.1f K Rays in %.3f ms\n", f,
               full * 180.0 / 3.14159265358979323846, rebuild ? "rebuild" : "refit", ms, cost, rays / 1000.0, st.render_ms);
        rc = tmpt_write_png((stem + name).c_str(), image.data(), w, h);
    }
    if (tmpt_scene_destroy(scene) && !rc) rc = 1;
    return rc;
}

int main(int argc, const char** argv)
{
    if (argc < 5) {
        printf("Usage: tmpt [width] [height] [samplesPerPixel] [objFile] [--seed row|pixel|sample] "
               "[--engine persistent|wavefront|mega] [--gpus N] [--device D] [--out file.png] [--aov prefix] "
               "[--denoise file.png [--shrink k]] [--adaptive tau[,min[,step[,radius]]]] [--spp-map file.png] "
               "[--twist deg,frames [--rebuild] [--temporal [--clip [gamma[,radius[,nmax]]]] [--guided [min[,step[,tau[,cap]]]]]]] "
               "[--octree host|device]\n"
               "  --octree: where the reference's octree is built, every time this run builds one (each frame of "
               "--twist too): host (default) or device (option octree_build)\n"
               "  --adaptive: radius 0..8 (default 0) keeps a pixel sampling while the variance test holds for "
               "any pixel within radius columns and rows of it\n"
               "  --shrink (with --denoise): the noise-aware filter (tmpt_denoise_moments) over the frame and its "
               "luminance moments, k > 0 scaling the noise estimate (0 = the default); spp >= 2\n"
               "  --twist: frames of the mesh twisted about y by up to deg on one scene, each a tmpt_scene_update "
               "(a refit; --rebuild: a full build), to <out>_000.png ...\n"
               "  --temporal (with --twist, --seed sample): each frame draws its own samples (sample_base) and is "
               "blended with the reprojected accumulation of the frames before it, to <out>_temporal_000.png ...\n"
               "  --clip (with --temporal): the history is clipped to gamma standard deviations of the frame's own "
               "(2 radius + 1)^2 window first (tmpt_temporal_clip; left out or 0 = its defaults)\n"
               "  --guided (with --temporal): history-guided sampling -- per frame the motion pass, the sample plan "
               "(tmpt_sample_plan) over the accumulated moments, the guided adaptive render (tmpt_render_guided: "
               "spp_min min, default 2; step and tau, default the adaptive ones; cap samples at most, default spp) and "
               "the blend with the moments carried along; --spp-map then writes one map per frame\n");
        return 1;
    }
    int w = atoi(argv[1]);
    if (w < 1 || w > 10000) { printf("ERROR: invalid width argument '%s'\n", argv[1]); return 1; }
    int h = atoi(argv[2]);
    if (h < 1 || h > 10000) { printf("ERROR: invalid height argument '%s'\n", argv[2]); return 1; }
    int spp = atoi(argv[3]);
    if (spp < 1 || spp > 1024) { printf("ERROR: invalid samplesPerPixel argument '%s'\n", argv[3]); return 1; }
    const char* obj = argv[4];
    int seed = TMPT_SEED_ROW, engine = TMPT_ENGINE_PERSISTENT, gpus = 1, device = 0;
    const char* out = "output.png";
    const char* aov = nullptr;
    const char* denoised = nullptr;
    const char* spp_map = nullptr;
    bool adaptive = false, twist = false, rebuild = false, temporal = false, have_shrink = false, clip = false;
    bool guided = false;
    int guided_cap = 0;
    tmpt_adaptive_desc gd;
    memset(&gd, 0, sizeof(gd));
    gd.threshold = -1.0f;
    tmpt_temporal_clip_desc cd;
    memset(&cd, 0, sizeof(cd));
    float shrink = 0.0f;
    double twist_deg = 0.0;
    int twist_frames = 0;
    tmpt_adaptive_desc ad;
    memset(&ad, 0, sizeof(ad));
    for (int i = 5; i < argc; ++i) {
        if (!strcmp(argv[i], "--seed") && i + 1 < argc) {
            ++i;
            seed = !strcmp(argv[i], "pixel") ? TMPT_SEED_PIXEL
                                             : (!strcmp(argv[i], "sample") ? TMPT_SEED_SAMPLE : TMPT_SEED_ROW);
        }
        else if (!strcmp(argv[i], "--engine") && i + 1 < argc) {
            ++i;
            engine = !strcmp(argv[i], "mega") ? TMPT_ENGINE_MEGAKERNEL
                     : (!strcmp(argv[i], "wavefront") ? TMPT_ENGINE_WAVEFRONT : TMPT_ENGINE_PERSISTENT);
        }
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
        else if (!strcmp(argv[i], "--aov") && i + 1 < argc) aov = argv[++i];
        else if (!strcmp(argv[i], "--denoise") && i + 1 < argc) denoised = argv[++i];
        else if (!strcmp(argv[i], "--spp-map") && i + 1 < argc) spp_map = argv[++i];
        else if (!strcmp(argv[i], "--shrink") && i + 1 < argc) {
            if (sscanf(argv[++i], "%f", &shrink) != 1 || !(shrink >= 0.0f) || !(shrink <= 3.4028235e38f)) {
                printf("ERROR: invalid --shrink argument '%s' (finite, not negative; 0 = the default)\n", argv[i]);
                return 1;
            }
            have_shrink = true;
        }
        else if (!strcmp(argv[i], "--adaptive") && i + 1 < argc) {
            int mn = 0, stp = 0, rad = 0;
            float tau = -1.0f;
            if (sscanf(argv[++i], "%f,%d,%d,%d", &tau, &mn, &stp, &rad) < 1) {
                printf("ERROR: invalid --adaptive argument '%s'\n", argv[i]);
                return 1;
            }
            adaptive = true;
            ad.threshold = tau;
            ad.spp_min = mn;
            ad.spp_step = stp;
            ad.radius = rad;
        }
        else if (!strcmp(argv[i], "--twist") && i + 1 < argc) {
            if (sscanf(argv[++i], "%lf,%d", &twist_deg, &twist_frames) != 2 || twist_frames < 1 || twist_frames > 1000) {
                printf("ERROR: invalid --twist argument '%s' (DEG,FRAMES with 1 <= FRAMES <= 1000)\n", argv[i]);
                return 1;
            }
            twist = true;
        }
        else if (!strcmp(argv[i], "--octree") && i + 1 < argc) {
            ++i;
            if (strcmp(argv[i], "host") != 0 && strcmp(argv[i], "device") != 0) {
                printf("ERROR: invalid --octree argument '%s' (host or device)\n", argv[i]);
                return 1;
            }
            g_octree_device = !strcmp(argv[i], "device");
        }
        else if (!strcmp(argv[i], "--rebuild")) rebuild = true;
        else if (!strcmp(argv[i], "--temporal")) temporal = true;
        else if (!strcmp(argv[i], "--clip")) {
            clip = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0 &&
                sscanf(argv[++i], "%f,%d,%f", &cd.gamma, &cd.radius, &cd.n_max) < 1) {
                printf("ERROR: invalid --clip argument '%s' (GAMMA[,RADIUS[,NMAX]])\n", argv[i]);
                return 1;
            }
        }
        else if (!strcmp(argv[i], "--guided")) {
            guided = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0 &&
                sscanf(argv[++i], "%d,%d,%f,%d", &gd.spp_min, &gd.spp_step, &gd.threshold, &guided_cap) < 1) {
                printf("ERROR: invalid --guided argument '%s' (MIN[,STEP[,TAU[,CAP]]])\n", argv[i]);
                return 1;
            }
        }
        else { printf("ERROR: unknown option '%s'\n", argv[i]); return 1; }
    }
    float* tris = nullptr;
    int32_t n = 0;
    float bmin[3], bmax[3];
    if (tmpt_load_obj(obj, &tris, &n, bmin, bmax)) {
        printf("ERROR: failed to load .obj file\n");
        return 1;
    }
    if (gpus < 1) gpus = 1;
    if (aov && gpus > 1) { printf("ERROR: --aov runs on one device (--gpus 1)\n"); return 1; }
    if (denoised && gpus > 1) { printf("ERROR: --denoise runs on one device (--gpus 1)\n"); return 1; }
    if (have_shrink && (!denoised || seed != TMPT_SEED_SAMPLE)) {
        printf("ERROR: --shrink needs --denoise and --seed sample\n");
        return 1;
    }
    if (denoised && seed != TMPT_SEED_SAMPLE) {
        printf("ERROR: --denoise needs --seed sample (the AOV records are a sample-seeded frame's)\n");
        return 1;
    }
    if (adaptive && (gpus > 1 || seed != TMPT_SEED_SAMPLE || engine != TMPT_ENGINE_PERSISTENT)) {
        printf("ERROR: --adaptive needs --seed sample, the persistent engine and one device (--gpus 1)\n");
        return 1;
    }
    if (guided && !temporal) { printf("ERROR: --guided needs --temporal\n"); return 1; }
    if (guided) {
        if (gd.spp_min == 0) gd.spp_min = 2;
        if (gd.threshold == 0.0f) gd.threshold = -1.0f;
        if (guided_cap == 0) guided_cap = spp;
        if (guided_cap < 2 || guided_cap > 1024) { printf("ERROR: --guided: CAP outside 2 .. 1024\n"); return 1; }
    }
    if (spp_map && !adaptive && !guided) { printf("ERROR: --spp-map needs --adaptive\n"); return 1; }
    if (rebuild && !twist) { printf("ERROR: --rebuild needs --twist\n"); return 1; }
    if (temporal && (!twist || rebuild || seed != TMPT_SEED_SAMPLE || engine != TMPT_ENGINE_PERSISTENT)) {
        printf("ERROR: --temporal needs --twist without --rebuild, --seed sample and the persistent engine\n");
        return 1;
    }
    if (clip && !temporal) { printf("ERROR: --clip needs --temporal\n"); return 1; }
    if (temporal && (long long)(twist_frames - 1) * (guided ? guided_cap : spp) > 64512) {
        printf("ERROR: --temporal: (FRAMES - 1) * spp must not exceed 64512 (option sample_base)\n");
        return 1;
    }
    if (twist && (gpus > 1 || adaptive || aov || denoised)) {
        printf("ERROR: --twist runs on one device (--gpus 1), without --adaptive, --aov and --denoise\n");
        return 1;
    }
    int ndev = tmpt_device_count();
    if (device + gpus > ndev) {
        printf("ERROR: %d GPU(s) requested from device %d, %d present\n", gpus, device, ndev);
        return 1;
    }
    tmpt_camera cam;
    tmpt_camera_for_scene(&cam, bmin, bmax, w, h, strstr(obj, "sponza.obj") != nullptr);

    std::vector<uint8_t> image((size_t)w * h * 4, 0);
    tmpt_render_desc desc;
    memset(&desc, 0, sizeof(desc));
    desc.width = w; desc.height = h; desc.spp = spp; desc.seed_mode = seed; desc.engine = engine;
    if (g_octree_device) desc.flags |= TMPT_FLAG_OCTREE_DEVICE;  // read by tmpt_render_multi, which builds its own scenes
    std::vector<int32_t> devs(gpus);
    for (int g = 0; g < gpus; ++g) devs[g] = device + g;
    uint64_t total = 0;
    double dt = 0.0;
    const double t0 = now_s();
    // scene builds + renders; tmpt_render_multi times the renders alone (main.cpp:319-333)
    // BuildOctree(sceneMin - extra, sceneMax + extra), main.cpp:296-297, 312
    float box[6];
    tmpt_octree_bounds(bmin, bmax, box);
    if (twist) {  // the frames of one scene handle, each written by render_twist
        if (render_twist(tris, n, &cam, &desc, device, twist_deg, twist_frames, rebuild, temporal, clip ? &cd : nullptr, out,
                         guided ? &gd : nullptr, guided_cap, spp_map)) {
            printf("ERROR: %s\n", tmpt_last_error());
            return 1;
        }
        tmpt_free(tris);
        return 0;
    }
    if (adaptive) {  // the frame, the spp map and the denoised frame from one adaptive call
        if (render_adaptive_frame(tris, n, box, &cam, w, h, spp, device, &ad, image, spp_map, denoised,
                                  have_shrink ? &shrink : nullptr)) {
            printf("ERROR: %s\n", tmpt_last_error());
            return 1;
        }
        denoised = nullptr;
    } else {
        if (tmpt_render_multi(tris, n, box, &cam, &desc, devs.data(), gpus, image.data(), &total, &dt)) {
            printf("ERROR: %s\n", tmpt_last_error());
            return 1;
        }
        printf("Initialized scene '%s' (%i tris) in %.3fs\n", obj, n, now_s() - t0 - dt);
        printf("Rendered scene at %ix%i,%ispp in %.3f s\n", w, h, spp, dt);
        printf("- %.1f K Rays, %.1f K Rays/s\n", total / 1000.0, total / 1000.0 / dt);
    }
    if (tmpt_write_png(out, image.data(), w, h)) { printf("ERROR: %s\n", tmpt_last_error()); return 1; }
    if (aov && write_aovs(aov, tris, n, box, &cam, w, h, spp, device)) {
        printf("ERROR: %s\n", tmpt_last_error());
        return 1;
    }
    if (denoised && write_denoised(denoised, tris, n, box, &cam, w, h, spp, device, have_shrink ? &shrink : nullptr)) {
        printf("ERROR: %s\n", tmpt_last_error());
        return 1;
    }
    tmpt_free(tris);
    return 0;
}
