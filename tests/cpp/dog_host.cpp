// tests/cpp/dog_host.cpp -- a host build of sfm-gms_amd/csrc/dog_core.h for the CPU tests (tests/test_dog_ref.py). The product library
// only runs dog_core.h on the GPU; this exposes its tables and its candidate plane to ctypes. With -DDOG_HOST_MAIN it is a stand-alone
// program (its own main) for a sanitizer build: the test's small cases, candidates counted.
#include "dog_core.h"

#include <vector>

namespace dog = gms::dog;

extern "C" {

int dog_host_radius(int j) { return dog::radius(j); }
void dog_host_table(int j, int32_t* out) { for (int i = 0; i <= 2 * dog::radius(j); ++i) out[i] = dog::tap(j, i); }
int dog_host_score(int c) { return dog::score_of(c); }

// B_j of an image (uint16 [h][w]; 0 where a tap would leave the image)
void dog_host_blur(const uint8_t* img, int w, int h, int j, uint16_t* B)
{
    std::vector<uint16_t> H((size_t)w * h);
    switch (j) {
    case 0: dog::blur_plane<0>(img, w, h, H.data(), B); break;
    case 1: dog::blur_plane<1>(img, w, h, H.data(), B); break;
    case 2: dog::blur_plane<2>(img, w, h, H.data(), B); break;
    default: dog::blur_plane<3>(img, w, h, H.data(), B); break;
    }
}

// the candidate plane (uint8 [h][w]); returns the number of candidates, -1 for arguments the detector refuses
int dog_host_candidates(const uint8_t* img, int w, int h, int contrast, uint8_t* cand)
{
    if (w <= 2 * dog::kBorder || h <= 2 * dog::kBorder || contrast < 0 || contrast > dog::kMaxContrast) return -1;
    std::vector<uint16_t> planes[dog::kBlurs];
    const uint16_t* B[dog::kBlurs];
    for (int j = 0; j < dog::kBlurs; ++j) {
        planes[j].resize((size_t)w * h);
        dog_host_blur(img, w, h, j, planes[j].data());
        B[j] = planes[j].data();
    }
    dog::candidate_plane(B, w, h, contrast, cand);
    int n = 0;
    for (size_t i = 0; i < (size_t)w * h; ++i) n += cand[i] != 0;
    return n;
}
}

#ifdef DOG_HOST_MAIN
#include <math.h>
#include <stdio.h>

static int run_case(const std::vector<uint8_t>& img, int w, int h, int contrast)
{
    std::vector<uint8_t> cand((size_t)w * h);
    return dog_host_candidates(img.data(), w, h, contrast, cand.data());
}

int main()
{
    // noise at the smallest size and at one that is no multiple of anything, 4 x 4 blocks of 20 / 220 (scores of 255), a flat image and
    // a bright Gaussian blob
    uint32_t state = 12345u;
    auto next = [&state]() { state = state * 1664525u + 1013904223u; return state >> 24; };
    std::vector<uint8_t> tiny(33 * 33), noise(97 * 65), blocks(97 * 65), flat(97 * 65, 77), blob(120 * 120);
    for (auto& v : tiny) v = (uint8_t)next();
    for (auto& v : noise) v = (uint8_t)next();
    std::vector<uint8_t> cells(25 * 17);
    for (auto& v : cells) v = (next() & 1) ? 220 : 20;
    for (int y = 0; y < 65; ++y)
        for (int x = 0; x < 97; ++x) blocks[(size_t)y * 97 + x] = cells[(size_t)(y / 4) * 25 + x / 4];
    for (int y = 0; y < 120; ++y)
        for (int x = 0; x < 120; ++x)
            blob[(size_t)y * 120 + x] = (uint8_t)lrint(110.0 + 100.0 * exp(-((x - 60) * (x - 60) + (y - 60) * (y - 60)) / (2.0 * 1.5 * 1.5)));
    const int a = run_case(tiny, 33, 33, 0), b = run_case(noise, 97, 65, 0), c = run_case(blocks, 97, 65, 128), d = run_case(flat, 97, 65, 0),
              e = run_case(blob, 120, 120, 128), f = run_case(noise, 97, 65, 65535), g = run_case(noise, 32, 65, 0);
    printf("dog_host: tiny %d noise %d blocks %d flat %d blob %d top %d refused %d\n", a, b, c, d, e, f, g);
    return a >= 0 && b > 0 && c > 0 && d == 0 && e > 0 && f == 0 && g == -1 ? 0 : 1;
}
#endif
