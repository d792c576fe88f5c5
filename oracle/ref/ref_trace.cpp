// ref_trace: the reference's own Camera::GetRay, Scene::HitScene and Trace() on
// chains of samples from a file (test infrastructure; compiled against the
// reference's sources by oracle/ref/Makefile into oracle/_ref/, never committed
// in built form).  Trace() is static in the reference's main.cpp, so that file is
// included whole with its main renamed; nothing of it is restated here.
//
//   ref_trace IN OUT
//
// IN   int32 n_tris, n_chains, width, height; float box_min[3], box_max[3] (the
//      octree's root box as BuildOctree takes it); float cam[13] {look_from,
//      look_at, vup, vfov, aspect, aperture, focus_dist} (Camera::Camera's
//      arguments); float tris[n_tris][9]; uint32 chains[n_chains][4] {x, y, state,
//      count}
// OUT  per sample, chain after chain, 17 words: float ray[6] {origin, direction},
//      uint32 state after GetRay, int32 first hit (1: HitScene returned != -1),
//      float {t, normal} of it (zeros on a miss), float colour[3] (Trace's),
//      uint32 state after Trace, int32 ray count of Trace
//
// A chain runs `count` samples of pixel (x, y), the RNG state threaded from one
// sample to the next; each sample is the body of the reference's sample loop
// (main.cpp:212-218): the two jitter draws (x's first, as the compiled reference
// draws them), GetRay, Trace.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define main tmpt_reference_main
#include "main.cpp"
#undef main

static bool read_all(FILE* f, void* p, size_t bytes)
{
    return bytes == 0 || fread(p, 1, bytes, f) == bytes;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: ref_trace IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) {
        perror(argv[1]);
        return 1;
    }
    int32_t n[4];
    float box[6], cam[13];
    if (!read_all(in, n, sizeof n) || !read_all(in, box, sizeof box) || !read_all(in, cam, sizeof cam) ||
        n[0] < 0 || n[1] < 0 || n[2] < 1 || n[3] < 1) {
        fprintf(stderr, "ref_trace: bad header\n");
        return 1;
    }
    static_assert(sizeof(Triangle) == 9 * sizeof(float), "Triangle is nine packed floats");
    std::vector<Triangle> tris(n[0]);
    std::vector<uint32_t> chains(size_t(n[1]) * 4);
    if (!read_all(in, tris.data(), tris.size() * sizeof(Triangle)) ||
        !read_all(in, chains.data(), chains.size() * sizeof(uint32_t))) {
        fprintf(stderr, "ref_trace: short input\n");
        return 1;
    }
    fclose(in);

    Scene scene(tris.data(), n[0]);
    scene.BuildOctree(glm::vec3(box[0], box[1], box[2]), glm::vec3(box[3], box[4], box[5]));
    const Camera camera(glm::vec3(cam[0], cam[1], cam[2]), glm::vec3(cam[3], cam[4], cam[5]),
                        glm::vec3(cam[6], cam[7], cam[8]), cam[9], cam[10], cam[11], cam[12]);
    const float inv_w = 1.0f / n[2];
    const float inv_h = 1.0f / n[3];

    std::vector<uint32_t> out;
    for (int32_t c = 0; c < n[1]; ++c) {
        const uint32_t* ch = &chains[size_t(c) * 4];
        const float x = static_cast<float>(ch[0]);
        const float y = static_cast<float>(ch[1]);
        uint32_t state = ch[2];
        for (uint32_t k = 0; k < ch[3]; ++k) {
            const float s = (x + RandomFloat01(state)) * inv_w;
            const float t = (y + RandomFloat01(state)) * inv_h;
            const Ray ray = camera.GetRay(s, t, state);
            const uint32_t after_ray = state;
            Hit first;
            memset(&first, 0, sizeof first);
            const int32_t hit = scene.HitScene(ray, kMinT, kMaxT, first) != -1;
            int rays = 0;
            const glm::vec3 col = Trace(ray, scene, state, rays);
            const float f[13] = {ray.orig.x, ray.orig.y, ray.orig.z, ray.dir.x, ray.dir.y, ray.dir.z,
                                 hit ? first.t : 0.0f, hit ? first.normal.x : 0.0f, hit ? first.normal.y : 0.0f,
                                 hit ? first.normal.z : 0.0f, col.x, col.y, col.z};
            uint32_t w[17];
            memcpy(&w[0], &f[0], 6 * sizeof(float));
            w[6] = after_ray;
            w[7] = uint32_t(hit);
            memcpy(&w[8], &f[6], 7 * sizeof(float));
            w[15] = state;
            w[16] = uint32_t(rays);
            out.insert(out.end(), w, w + 17);
        }
    }

    FILE* outf = fopen(argv[2], "wb");
    if (!outf) {
        perror(argv[2]);
        return 1;
    }
    bool ok = fwrite(out.data(), sizeof(uint32_t), out.size(), outf) == out.size();
    ok = fclose(outf) == 0 && ok;
    return ok ? 0 : 1;
}
