// ref_hits: the reference's own Scene::HitScene on rays from a file (test
// infrastructure; compiled against the reference's scene.h by oracle/ref/Makefile
// into oracle/_ref/, never committed in built form).
//
//   ref_hits IN OUT
//
// IN   int32 n_tris, int32 n_rays, float box_min[3], box_max[3] (the octree's root
//      box as BuildOctree takes it), float tris[n_tris][9],
//      float rays[n_rays][8] {origin, direction, t_min, t_max}
// OUT  int8 hit[n_rays] (1: HitScene returned != -1), float rec[n_rays][7]
//      {pos, normal, t} (zeros on a miss)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "scene.h"

static bool read_all(FILE* f, void* p, size_t bytes)
{
    return bytes == 0 || fread(p, 1, bytes, f) == bytes;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: ref_hits IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) {
        perror(argv[1]);
        return 1;
    }
    int32_t n[2];
    float head[6];
    if (!read_all(in, n, sizeof n) || !read_all(in, head, sizeof head) || n[0] < 0 || n[1] < 0) {
        fprintf(stderr, "ref_hits: bad header\n");
        return 1;
    }
    static_assert(sizeof(Triangle) == 9 * sizeof(float), "Triangle is nine packed floats");
    std::vector<Triangle> tris(n[0]);
    std::vector<float> rays(size_t(n[1]) * 8);
    if (!read_all(in, tris.data(), tris.size() * sizeof(Triangle)) ||
        !read_all(in, rays.data(), rays.size() * sizeof(float))) {
        fprintf(stderr, "ref_hits: short input\n");
        return 1;
    }
    fclose(in);

    Scene scene(tris.data(), n[0]);
    scene.BuildOctree(glm::vec3(head[0], head[1], head[2]), glm::vec3(head[3], head[4], head[5]));

    std::vector<int8_t> hit(n[1]);
    std::vector<float> rec(size_t(n[1]) * 7, 0.0f);
    for (int32_t i = 0; i < n[1]; ++i) {
        const float* r = &rays[size_t(i) * 8];
        Ray ray;  // the members directly: the constructor only asserts a unit direction
        ray.orig = glm::vec3(r[0], r[1], r[2]);
        ray.dir = glm::vec3(r[3], r[4], r[5]);
        Hit h;
        memset(&h, 0, sizeof h);
        hit[i] = scene.HitScene(ray, r[6], r[7], h) != -1;
        if (hit[i]) {
            const float out[7] = {h.pos.x, h.pos.y, h.pos.z, h.normal.x, h.normal.y, h.normal.z, h.t};
            memcpy(&rec[size_t(i) * 7], out, sizeof out);
        }
    }

    FILE* outf = fopen(argv[2], "wb");
    if (!outf) {
        perror(argv[2]);
        return 1;
    }
    bool ok = fwrite(hit.data(), 1, hit.size(), outf) == hit.size() &&
              fwrite(rec.data(), sizeof(float), rec.size(), outf) == rec.size();
    ok = fclose(outf) == 0 && ok;
    return ok ? 0 : 1;
}
