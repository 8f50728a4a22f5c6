// sfm_register_layout_check.cpp -- CPU check of the registration workspace's layout (SfmRegisterLayout in sfm-gms_amd/csrc/ws_layout.h).
// tests/test_sfm_register_ref.py builds it with g++ (plain and under the address / undefined-behaviour sanitizers) and runs it.
//
// Swept over pairs in {0, 1, 2, 63, 257, 1000}, keypoints in {0, 1, 31, 4095, 4096, 4097, 10^7, 2^31 - 2} and match slots in {0, 1, 255,
// 4097, 3 * 10^6, 2^33 + 5}: the regions lie in declaration order without overlap, each at least as long as what its kernels index (the
// element counts of the struct's comments, restated here), each starts on a 256-byte boundary, the gaps are smaller than the rounding,
// and the last one ends at `total`; the table of (root, frame) keys is a power of two of at least twice the keypoints; the tile
// counts hold one word per kSfrScanTile keypoints and one more.
//
//   sfm_register_layout_check      exit 0: everything holds; 1: something did not (it is printed)
#include <cstdio>
#include <string>
#include <vector>

#include "ws_layout.h"

static_assert(sizeof(size_t) == 8, "the offsets are 64-bit");
using namespace gms;

namespace {

struct Region {
    const char* name;
    size_t offset, bytes;
};

int g_bad = 0;
long g_cases = 0;

void fail(const std::string& what, const char* detail)
{
    if (++g_bad <= 20) std::printf("%s: %s\n", what.c_str(), detail);
}

void check(int P, long long K, long long M)
{
    const SfmRegisterLayout L = sfm_register_layout(P, K, M);
    const size_t k = (size_t)K, m = (size_t)M, p = (size_t)P, slots = sfr_hash_slots(k), tiles = (k + kSfrScanTile - 1) / kSfrScanTile + 1;
    char what[120];
    std::snprintf(what, sizeof what, "register %d pairs, %lld keypoints, %lld match slots", P, K, M);
    ++g_cases;
    if (slots < 2 * k || slots < 64 || (slots & (slots - 1)) != 0 || (slots > 64 && slots / 2 >= 2 * k)) fail(what, "the key table is not the least power of two of at least 2 K (64 at least)");
    if ((tiles - 1) * kSfrScanTile < k) fail(what, "the tiles do not cover the keypoints");
    const std::vector<Region> r = {{"rank", L.rank, 4 * m},     {"rho", L.rho, 8 * m},       {"slot", L.slot, 4 * k},   {"parent", L.parent, 4 * k},
                                   {"member", L.member, 4 * k}, {"obs", L.obs, 4 * k},       {"est", L.est, 4 * k},     {"multi", L.multi, 4 * k},
                                   {"repkey", L.repkey, 8 * k}, {"spread", L.spread, 8 * k}, {"hash", L.hash, 8 * slots}, {"tiles", L.tiles, 4 * tiles},
                                   {"npts", L.npts, 4 * p},     {"ok", L.ok, 4 * p}};
    for (size_t i = 0; i < r.size(); ++i) {
        const size_t next = i + 1 < r.size() ? r[i + 1].offset : L.total;
        char msg[200];
        std::snprintf(msg, sizeof msg, "region %s at %zu, %zu bytes, next at %zu", r[i].name, r[i].offset, r[i].bytes, next);
        if (r[i].offset % 256 != 0) fail(std::string(what) + " is misaligned", msg);
        if (r[i].offset > next || r[i].bytes > next - r[i].offset) fail(std::string(what) + " overlaps", msg);
        else if (next - r[i].offset - r[i].bytes >= 256) fail(std::string(what) + " leaves a gap", msg);
    }
    if (r[0].offset != 0) fail(what, "the first region does not start the workspace");
}

}  // namespace

int main()
{
    for (int P : {0, 1, 2, 63, 257, 1000})
        for (long long K : {0ll, 1ll, 31ll, 4095ll, 4096ll, 4097ll, 10000000ll, (1ll << 31) - 2})
            for (long long M : {0ll, 1ll, 255ll, 4097ll, 3000000ll, (1ll << 33) + 5}) check(P, K, M);
    std::printf("sfm_register_layout_check: %ld cases: %d bad\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
