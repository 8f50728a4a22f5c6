// block_layout_check.cpp -- CPU check of gms::BlockLayout (sfm-gms_amd/csrc/block_layout.h), the offset arithmetic of the one-shot
// host entry points' device block. tests/test_block_layout.py builds it with g++ (plain and under the address / undefined-behaviour
// sanitizers) and runs it.
//
// Seeded sequences of add(bytes, slack): 1 .. 12 regions whose sizes are drawn from the edge values 0, 1, 255, 256, 257, sizes just
// below, at and above 4 GiB, and random ones up to 64 GiB; slack 0, 16 or random. After every sequence:
//   every offset is a multiple of 256, offsets never decrease, offset[i] + bytes[i] + slack[i] <= offset[i + 1] (total() behind the
//   last), and total() exceeds the sum of bytes + slack by less than 256 * (regions + 1).
//
//   block_layout_check [sequences] [seed]      exit 0: every sequence holds; 1: one did not (it is printed)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "block_layout.h"

static_assert(sizeof(size_t) == 8, "the block's offsets are 64-bit");

int main(int argc, char** argv)
{
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    const size_t gib4 = (size_t)1 << 32;
    const size_t edge[] = {0, 1, 255, 256, 257, 4095, 65536, gib4 - 1, gib4, gib4 + 1, gib4 + 257, 5 * gib4 + 255};
    const size_t n_edge = sizeof(edge) / sizeof(edge[0]);
    int bad = 0;
    size_t largest = 0;
    for (int s = 0; s < sequences; ++s) {
        const int regions = 1 + (int)(rng() % 12);
        std::vector<size_t> bytes(regions), slack(regions), off(regions);
        gms::BlockLayout lay;
        size_t sum = 0;
        for (int i = 0; i < regions; ++i) {
            const unsigned pick = (unsigned)(rng() % 16);
            bytes[i] = pick < n_edge ? edge[pick] : pick == 15 ? rng() % (16 * gib4) : rng() % 100000;
            const unsigned sp = (unsigned)(rng() % 4);
            slack[i] = sp == 0 ? 16 : sp == 1 ? rng() % 600 : 0;
            off[i] = lay.add(bytes[i], slack[i]);
            sum += bytes[i] + slack[i];
        }
        bool ok = lay.total() >= sum && lay.total() - sum < 256 * ((size_t)regions + 1);
        for (int i = 0; i < regions; ++i) {
            const size_t next = i + 1 < regions ? off[i + 1] : lay.total();
            ok = ok && off[i] % 256 == 0 && off[i] <= next && off[i] + bytes[i] + slack[i] <= next;
        }
        if (lay.total() > largest) largest = lay.total();
        if (!ok) {
            ++bad;
            std::printf("sequence %d does not hold: total %zu, sum %zu\n", s, lay.total(), sum);
            for (int i = 0; i < regions; ++i) std::printf("  region %d: offset %zu, bytes %zu, slack %zu\n", i, off[i], bytes[i], slack[i]);
        }
    }
    // an empty layout is an empty block, and an empty region shares its offset with its successor
    gms::BlockLayout lay;
    const bool empty_ok = lay.total() == 0 && lay.add(0) == 0 && lay.add(0) == 0 && lay.total() == 0 && lay.add(1) == 0 && lay.add(0) == 256 &&
                          lay.total() == 256;
    if (!empty_ok) {
        ++bad;
        std::printf("empty regions are not free\n");
    }
    std::printf("block_layout_check: %d sequences, largest block %zu bytes: %d bad\n", sequences, largest, bad);
    return bad ? 1 : 0;
}
