// tests/cpp/dog_refine_host.cpp -- a host build of the refinement in sfm-gms_amd/csrc/dog_core.h for the CPU tests
// (tests/test_dog_refine_ref.py): the code plane of an image, the scale constants and the record's arithmetic, exposed to ctypes. With
// -DDOG_REFINE_HOST_MAIN it is a stand-alone program (its own main) for a sanitizer build: small cases, candidates and offsets counted.
#include "dog_core.h"

#include <vector>

namespace dog = gms::dog;

extern "C" {

float dog_refine_host_scale(int os) { return dog::scale_of(os); }
float dog_refine_host_coord(int v, int o, float f) { return dog::refined_coord(v, o, f); }
float dog_refine_host_size(int os, float fx) { return dog::refined_size(os, fx); }
int dog_refine_host_sixteenths(int64_t n, int64_t q) { return dog::sixteenths(n, q); }
int dog_refine_host_floor_div_clamped(int64_t a, int64_t b, int lim) { return dog::floor_div_clamped(a, b, lim); }
int dog_refine_host_pack(int ox, int oy, int os) { return dog::Offsets{ox, oy, os}.code(); }
void dog_refine_host_unpack(int code, int32_t* out)
{
    const dog::Offsets o = dog::offsets_of(code);
    out[0] = o.ox; out[1] = o.oy; out[2] = o.os;
}

// candidate plane (uint8 [h][w]) and code plane (uint16 [h][w]); returns the number of candidates, -1 for arguments the detector refuses
int dog_refine_host_offsets(const uint8_t* img, int w, int h, int contrast, uint8_t* cand, uint16_t* codes)
{
    if (w <= 2 * dog::kBorder || h <= 2 * dog::kBorder || contrast < 0 || contrast > dog::kMaxContrast) return -1;
    std::vector<uint16_t> H((size_t)w * h), planes[dog::kBlurs];
    const uint16_t* B[dog::kBlurs];
    for (int j = 0; j < dog::kBlurs; ++j) planes[j].resize((size_t)w * h);
    dog::blur_plane<0>(img, w, h, H.data(), planes[0].data());
    dog::blur_plane<1>(img, w, h, H.data(), planes[1].data());
    dog::blur_plane<2>(img, w, h, H.data(), planes[2].data());
    dog::blur_plane<3>(img, w, h, H.data(), planes[3].data());
    for (int j = 0; j < dog::kBlurs; ++j) B[j] = planes[j].data();
    dog::candidate_and_code_plane(B, w, h, contrast, cand, codes);
    int n = 0;
    for (size_t i = 0; i < (size_t)w * h; ++i) n += cand[i] != 0;
    return n;
}
}

#ifdef DOG_REFINE_HOST_MAIN
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

// candidates of a case; adds the moved ones (a non-zero offset) and the clamped ones (|ox| or |oy| = 8) to the counters; -2: a bad code
static int run_case(const std::vector<uint8_t>& img, int w, int h, int contrast, int* moved, int* edge)
{
    std::vector<uint8_t> cand((size_t)w * h);
    std::vector<uint16_t> codes((size_t)w * h);
    const int n = dog_refine_host_offsets(img.data(), w, h, contrast, cand.data(), codes.data());
    for (size_t i = 0; i < codes.size() && n >= 0; ++i) {
        if ((codes[i] != 0) != (cand[i] != 0) || codes[i] > dog::kMaxCode) return -2;
        if (codes[i] == 0) continue;
        const dog::Offsets o = dog::offsets_of(codes[i]);
        if (o.code() != codes[i] || abs(o.ox) > 8 || abs(o.oy) > 8 || abs(o.os) > 8) return -2;
        *moved += o.ox != 0 || o.oy != 0 || o.os != 0;
        *edge += abs(o.ox) == 8 || abs(o.oy) == 8;
    }
    return n;
}

int main()
{
    // noise at the smallest size and at one that is no multiple of anything, 4 x 4 blocks of 20 / 220, a flat image and a bright
    // Gaussian blob centred between pixels
    uint32_t state = 12345u;
    auto next = [&state]() { state = state * 1664525u + 1013904223u; return state >> 24; };
    std::vector<uint8_t> tiny(33 * 33), noise(97 * 65), blocks(97 * 65), flat(97 * 65, 77), blob(65 * 65);
    for (auto& v : tiny) v = (uint8_t)next();
    for (auto& v : noise) v = (uint8_t)next();
    std::vector<uint8_t> cells(25 * 17);
    for (auto& v : cells) v = (next() & 1) ? 220 : 20;
    for (int y = 0; y < 65; ++y)
        for (int x = 0; x < 97; ++x) blocks[(size_t)y * 97 + x] = cells[(size_t)(y / 4) * 25 + x / 4];
    const double cx = 32.25, cy = 31.625;
    for (int y = 0; y < 65; ++y)
        for (int x = 0; x < 65; ++x)
            blob[(size_t)y * 65 + x] = (uint8_t)lrint(110.0 + 100.0 * exp(-((x - cx) * (x - cx) + (y - cy) * (y - cy)) / (2.0 * 1.5 * 1.5)));
    int moved = 0, edge = 0, blob_moved = 0, blob_edge = 0;
    const int a = run_case(tiny, 33, 33, 0, &moved, &edge), b = run_case(noise, 97, 65, 0, &moved, &edge), c = run_case(blocks, 97, 65, 128, &moved, &edge),
              d = run_case(flat, 97, 65, 0, &moved, &edge), e = run_case(blob, 65, 65, 128, &blob_moved, &blob_edge),
              f = run_case(noise, 97, 65, 65535, &moved, &edge), g = run_case(noise, 32, 65, 0, &moved, &edge);
    // the extremes of the divisions: the floor of a negative quotient, and the record's arithmetic at both ends of the table
    const int64_t big = (int64_t)1 << 39;
    const bool div_ok = dog::sixteenths(-1, 1) == -8 && dog::sixteenths(-1, 32) == 0 && dog::sixteenths(-1, 3) == -5 && dog::sixteenths(3, 32) == 2 &&
                        dog::sixteenths(-big, big) == -8 && dog::sixteenths(big - 1, big) == 8 && dog::sixteenths(-big, 1) == -8 &&
                        dog::floor_div_clamped(-7, 2, 100) == -4 && dog::floor_div_clamped(7, 2, 100) == 3 && dog::floor_div_clamped(-7, 2, 3) == -3 &&
                        dog::floor_div_clamped(64 * big - 1, 64 * big, 8) == 0 && dog::floor_div_clamped(-1, 64 * big, 8) == -1;
    const bool rec_ok = dog::scale_of(0) == 1.0f && dog::scale_of(-8) < dog::scale_of(8) && dog::refined_coord(5, -8, 1.0f) == 4.5f &&
                        dog::refined_size(0, 2.0f) == 62.0f;
    printf("dog_refine_host: tiny %d noise %d blocks %d flat %d blob %d top %d refused %d moved %d clamped %d blob moved %d divisions %d record %d\n", a,
           b, c, d, e, f, g, moved, edge, blob_moved, (int)div_ok, (int)rec_ok);
    return a >= 0 && b > 0 && c > 0 && d == 0 && e > 0 && f == 0 && g == -1 && moved > 0 && blob_moved > 0 && div_ok && rec_ok ? 0 : 1;
}
#endif
