// Host side of the device-resident queries under ASan + UBSan, as a program of its own
// (tools/san_query.sh builds it against the SAN=1 library; no device is touched): the
// argument checks of tmpt_scene_hit_device that come before any device call, the key hook
// tmpt_query_keys on heap arrays of exactly the stated sizes (both strides, NaN and
// infinite components, a box with a zero extent), and the sizes of the call's chunk loop
// (tmpt_query_plan) for n up to 2^40.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tmpt.h"

static int fails = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("san_query: FAILED %s (line %d): %s\n", #c, __LINE__, tmpt_last_error()); \
            ++fails;                                                    \
        }                                                               \
    } while (0)

int main()
{
    // ---- tmpt_scene_hit_device: refused before any device call
    tmpt_hit_desc d;
    memset(&d, 0, sizeof d);
    d.n = 4;
    float rays4[4 * 8] = {0};
    int32_t ids4[4];
    EXPECT(sizeof(tmpt_hit_desc) == 56);
    EXPECT(tmpt_scene_hit_device(nullptr, &d, rays4, ids4, nullptr, nullptr) == -22 && strstr(tmpt_last_error(), "null scene"));
    EXPECT(tmpt_scene_hit_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == -22);

    // ---- tmpt_query_keys on exactly-sized heap arrays
    const float box[6] = {-1.0f, 0.0f, -2.0f, 3.0f, 0.0f, 5.0f};  // extent 0 on y: the 1e-30 floor
    for (int stride = 6; stride <= 8; stride += 2) {
        const int64_t n = 4099;
        std::vector<float> rays((size_t)(n * stride));
        std::vector<uint32_t> keys((size_t)n, 0xdeadbeefu);
        uint32_t x = 12345u;
        for (size_t k = 0; k < rays.size(); ++k) {
            x = x * 1664525u + 1013904223u;
            rays[k] = ((float)(x >> 8) / 16777216.0f) * 12.0f - 6.0f;
        }
        const float odd[] = {NAN, INFINITY, -INFINITY, -0.0f, 1e38f, -1e38f, 1e-45f};
        for (int k = 0; k < 7 * 6; ++k) rays[(size_t)((k + 1) * 17 * stride + k % 6)] = odd[k / 6];
        EXPECT(tmpt_query_keys(rays.data(), n, stride, box, keys.data()) == 0);
        int nan_keys = 0;
        for (int64_t i = 0; i < n; ++i) {
            EXPECT(keys[(size_t)i] <= 0xFFFFFFu);
            nan_keys += keys[(size_t)i] == 0xFFFFFFu;
        }
        EXPECT(nan_keys >= 6);
        EXPECT(tmpt_query_keys(rays.data(), -1, stride, box, keys.data()) == -22);
        EXPECT(tmpt_query_keys(nullptr, n, stride, box, keys.data()) == -22);
        EXPECT(tmpt_query_keys(rays.data(), n, stride, nullptr, keys.data()) == -22);
        EXPECT(tmpt_query_keys(rays.data(), n, 7, box, keys.data()) == -22);
        EXPECT(tmpt_query_keys(nullptr, 0, stride, box, nullptr) == 0);
    }

    // ---- the chunk loop's sizes, n up to 2^40
    const int64_t ns[] = {0, 1, 63, 64, 65, 1000, (1ll << 22) - 1, 1ll << 22, (1ll << 22) + 1, (1ll << 31) - 1, 1ll << 31,
                          (1ll << 32) + 7, (1ll << 40) - 1, 1ll << 40};
    const int64_t chunks[] = {64, 100, 128, 4096, 1ll << 22};
    for (int64_t n : ns)
        for (int64_t chunk : chunks)
            for (int sorted = 0; sorted < 2; ++sorted)
                for (int64_t cap : {0ll, 1ll, 7ll}) {
                    int64_t o[6];
                    EXPECT(tmpt_query_plan(n, sorted, chunk, cap, 1280, o) == 0);
                    if (n == 0) {
                        EXPECT(o[0] == 0 && o[3] == 0 && o[4] == 0 && o[5] == 0);
                        continue;
                    }
                    EXPECT(o[0] >= 1 && o[1] >= 1 && o[2] >= 1 && o[2] <= o[1]);
                    EXPECT((o[0] - 1) * o[1] + o[2] == n);
                    EXPECT(sorted ? (o[1] <= chunk && o[1] <= (1ll << 22)) : (o[0] == 1 && o[5] == 0));
                    EXPECT(o[3] >= 1 && o[3] <= 1280 && (cap == 0 || o[3] <= cap) && o[3] <= (o[1] + 255) / 256);
                    EXPECT(o[4] == o[3] * 256 * 112 * 4);
                    EXPECT(!sorted || o[5] >= 16 * o[1]);
                }
    int64_t o[6];
    EXPECT(tmpt_query_plan(-1, 0, 64, 0, 1, o) == -22);
    EXPECT(tmpt_query_plan(1, 2, 64, 0, 1, o) == -22);
    EXPECT(tmpt_query_plan(1, 1, 63, 0, 1, o) == -22);
    EXPECT(tmpt_query_plan(1, 1, (1ll << 22) + 1, 0, 1, o) == -22);
    EXPECT(tmpt_query_plan(1, 1, 64, -1, 1, o) == -22);
    EXPECT(tmpt_query_plan(1, 1, 64, 0, 0, o) == -22);
    EXPECT(tmpt_query_plan(1, 1, 64, 0, 1, nullptr) == -22);
    printf(fails ? "san_query: %d checks failed\n" : "san_query: clean\n", fails);
    return fails ? 1 : 0;
}
