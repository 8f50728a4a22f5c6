// tests/test_match_unique_ref.py: a host build of match_unique_core.h (the key, the live test and the sequential statement of the
// one-to-one rule) on the arrays of an input file. The test holds the result to the numpy statement
// tests/match_unique_ref.py, byte for byte. Built with g++ alone, plain and under the address / undefined-behaviour sanitizers.
//
//   match_unique_host IN.bin OUT.bin
//   IN:  int64 n_frames, n_pairs, total_m, flags (1: a mask follows, 2: two-view records follow); int64 frame_off [n_frames + 1];
//        gms_pair [n_pairs]; gms_dmatch [total_m]; uint8 mask [total_m]; gms_two_view [n_pairs]
//   OUT: uint8 keep [total_m] (slots of no fitting pair: 0), int32 counts [n_pairs][2]
// Every array is copied into a vector of exactly its length, so that a read or write outside shows under the address sanitizer.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "match_unique_core.h"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: match_unique_host IN.bin OUT.bin\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    int64_t head[4];
    if (!f || std::fread(head, 8, 4, f) != 4 || head[0] < 1 || head[1] < 0 || head[2] < 0) return 2;
    const int n_frames = (int)head[0], n_pairs = (int)head[1];
    const int64_t total_m = head[2];
    std::vector<int64_t> frame_off;
    std::vector<gms_pair> pairs;
    std::vector<gms_dmatch> matches;
    std::vector<uint8_t> mask;
    std::vector<gms_two_view> tv;
    bool ok = read_n(f, frame_off, (size_t)n_frames + 1) && read_n(f, pairs, (size_t)n_pairs) && read_n(f, matches, (size_t)total_m);
    if (ok && (head[3] & 1)) ok = read_n(f, mask, (size_t)total_m);
    if (ok && (head[3] & 2)) ok = read_n(f, tv, (size_t)n_pairs);
    std::fclose(f);
    if (!ok) return 2;

    // the key's order, stated once more in plain words
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    const bool order = mu::key(0.0f, 5) == mu::key(-0.0f, 5) && mu::key(-0.0f, 1) < mu::key(0.0f, 2) && mu::key(1e-45f, 0) > mu::key(0.0f, 9) &&
                       mu::key(3.0e38f, 9) < mu::key(inf, 0) && mu::key(nan, 3) < mu::key(-1.0f, 4) && mu::key(-inf, 4) < mu::key(inf, 5) &&
                       mu::key(1.0f, 7) < mu::key(1.5f, 0) && (mu::key(nan, 6) >> 32) == 0xFFFFFFFFu && mu::key(2.0f, 1) != mu::kEmpty;
    if (!order) {
        std::fprintf(stderr, "match_unique_host: the key's order does not hold\n");
        return 1;
    }

    std::vector<uint8_t> keep((size_t)total_m, 0);
    std::vector<int32_t> counts(2 * (size_t)n_pairs, -1);
    mu::unique_sequential(frame_off.data(), n_frames, frame_off[n_frames], pairs.data(), n_pairs, total_m, matches.data(),
                          (head[3] & 1) ? mask.data() : nullptr, (head[3] & 2) ? tv.data() : nullptr, keep.data(), counts.data());
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    if (total_m) std::fwrite(keep.data(), 1, keep.size(), o);
    if (n_pairs) std::fwrite(counts.data(), 4, counts.size(), o);
    std::fclose(o);
    std::printf("match_unique_host: %d pairs, %lld slots\n", n_pairs, (long long)total_m);
    return 0;
}
