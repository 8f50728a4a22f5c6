// ws_layout_check.cpp -- CPU check of nine workspace layouts of sfm-gms_amd/csrc/ws_layout.h (all but SGM's and the chessboard's; the pyramid's in both its forms). tests/test_ws_layout.py builds it
// with g++ (plain and under the address / undefined-behaviour sanitizers) and runs it.
//
// Every layout is swept over n in {1, 2, 3, 63, 64, 255, 257} and its other arguments' awkward values (below). For each case:
//   1. the regions lie in declaration order without overlap, each at least as long as what its kernel indexes (the element counts of
//      the struct comments, restated here), and the last one ends inside `total`; a gap is smaller than the rounding that made it;
//   2. each region starts on the alignment its readers need: 256 where the layout rounds to 256, 16 for rotmask and every region of
//      the two streamed layouts, natural alignment for the rest;
//   3. the spans the launchers clear are the regions they are meant to cover, byte for byte;
//   4. for the four per-slice layouts, total(n) <= n * bytes per pair: what plan_workspace reserves holds what the launcher walks.
// Then every line of the fixture (tests/golden/ws_layout_sizes.txt: sizes recorded from the library before the layouts existed) is
// compared with the layout's total or per-pair figure for the same arguments; a recorded 0 is a refusal of the C ABI, which
// tests/test_ws_layout.py checks against the library itself.
//
//   ws_layout_check <fixture> [seed]      exit 0: everything holds; 1: something did not (it is printed)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ws_layout.h"

static_assert(sizeof(size_t) == 8, "the offsets are 64-bit");
using namespace gms;

namespace {

struct Region {
    const char* name;
    size_t offset, bytes, align;
};

int g_bad = 0;
long g_cases = 0;

void fail(const std::string& what, const char* detail)
{
    if (++g_bad <= 20) std::printf("%s: %s\n", what.c_str(), detail);
}

// properties 1 and 2; max_gap = the largest rounding of the layout
void check_regions(const std::string& what, const std::vector<Region>& r, size_t total, size_t max_gap)
{
    ++g_cases;
    for (size_t i = 0; i < r.size(); ++i) {
        const size_t next = i + 1 < r.size() ? r[i + 1].offset : total;
        char msg[200];
        std::snprintf(msg, sizeof msg, "region %s at %zu, %zu bytes, next at %zu, alignment %zu", r[i].name, r[i].offset, r[i].bytes, next, r[i].align);
        if (r[i].offset % r[i].align != 0) fail(what + " is misaligned", msg);
        if (r[i].offset > next || r[i].bytes > next - r[i].offset) fail(what + " overlaps", msg);
        else if (next - r[i].offset - r[i].bytes >= max_gap) fail(what + " leaves a gap", msg);
    }
}

void expect(const std::string& what, const char* name, size_t got, size_t want)
{
    if (got == want) return;
    char msg[120];
    std::snprintf(msg, sizeof msg, "%s is %zu, expected %zu", name, got, want);
    fail(what, msg);
}

std::string fmt(const char* f, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0)
{
    char s[160];
    std::snprintf(s, sizeof s, f, a, b, c, d, e);
    return s;
}

// the level images' bytes, stated independently of the header: w' = (5 w + 3) / 6 while both sides exceed 32
size_t level_bytes(int w, int h, int n, int n_levels)
{
    size_t b = 0;
    for (int l = 0; l < n_levels && l < 16 && w > 32 && h > 32 && w <= 65535 && h <= 65535; ++l) {
        if (l > 0) b += (size_t)w * h * n;
        w = (5 * w + 3) / 6;
        h = (5 * h + 3) / 6;
    }
    return b;
}

void check_detect(int w, int h, int n, int maxkp, int levels)
{
    const size_t N = n, px = (size_t)w * h * N;
    const DetectLayout d = detect_layout(w, h, n, maxkp);
    std::string what = fmt("detect %lld x %lld, %lld images, %lld keypoints", w, h, n, maxkp);
    check_regions(what, {{"score", d.score, px, 256}, {"cand", d.cand, px, 256}, {"box", d.box, 2 * px, 256}, {"hist", d.hist, N * 256 * 4, 256},
                         {"cut", d.cut, N * 16, 256}, {"rows", d.rows, N * h * 8, 16}, {"list", d.list, N * maxkp * 8, 16}}, d.total, 256);
    expect(what, "the cleared histogram", d.cut - d.hist, N * 256 * 4);
    const PyramidLayout p = pyramid_layout(w, h, n, maxkp, levels, false);
    what = fmt("pyramid %lld x %lld, %lld images, %lld keypoints, %lld levels", w, h, n, maxkp, levels);
    check_regions(what, {{"levels", p.levels, level_bytes(w, h, n, levels), 256}, {"counts", p.counts, 16 * N * 4, 256},
                         {"hists", p.hists, 16 * N * 256 * 4, 256}, {"detect", p.detect, d.total, 256}, {"codes", p.codes, 0, 1}}, p.total, 256);
    expect(what, "the cleared span", p.detect - p.counts, round_up(16 * N * 4, 256) + 16 * N * 256 * 4);
    expect(what, "the total", p.total, p.detect + d.total);   // what it was before the refined form shared the struct
    expect(what, "the empty code plane", p.codes, p.total);
    // the refined form: the same regions at the same offsets, then the plane of refinement codes (2 w h n bytes) on a 256-byte boundary
    const PyramidLayout r = pyramid_layout(w, h, n, maxkp, levels, true);
    what = fmt("refined pyramid %lld x %lld, %lld images, %lld keypoints, %lld levels", w, h, n, maxkp, levels);
    check_regions(what, {{"levels", r.levels, level_bytes(w, h, n, levels), 256}, {"counts", r.counts, 16 * N * 4, 256},
                         {"hists", r.hists, 16 * N * 256 * 4, 256}, {"detect", r.detect, d.total, 256}, {"codes", r.codes, 2 * px, 256}}, r.total, 256);
    expect(what, "the cleared span", r.detect - r.counts, round_up(16 * N * 4, 256) + 16 * N * 256 * 4);
    expect(what, "the unrefined regions", (size_t)(r.levels == p.levels && r.counts == p.counts && r.hists == p.hists && r.detect == p.detect), 1);
    expect(what, "the code plane", r.codes, round_up(p.total, 256));
    expect(what, "the total", r.total, round_up(p.total, 256) + round_up(2 * px, 256));
}

void check_images(int w, int h, int n)
{
    const size_t N = n, px = (size_t)w * h * N;
    const StereoBmLayout s = stereo_bm_layout(n, w, h);
    check_regions(fmt("stereo %lld x %lld, %lld pairs", w, h, n), {{"pre", s.pre, 2 * px, 256}, {"cost", s.cost, 4 * px, 256}}, s.total, 256);
    const PortraitLayout p = portrait_layout(n, w, h);
    check_regions(fmt("portrait %lld x %lld, %lld images", w, h, n),
                  {{"mask", p.mask, px, 256}, {"nb", p.nb, px, 256}, {"flag", p.flag, px, 256}, {"sel", p.sel, px, 256}, {"label", p.label, 4 * px, 256},
                   {"tog", p.tog, 8 * px, 256}, {"keys", p.keys, 8 * N * h * ((w + 1) / 2), 256}, {"chosen", p.chosen, N * 66 * 4, 256}}, p.total, 256);
}

void check_bf_select(int n, long long rows, long long back)
{
    const size_t R = (size_t)n * rows;
    const BfSelectLayout b = bf_select_layout(n, rows, back);
    check_regions(fmt("bf_select %lld pairs, %lld rows, %lld backward rows", n, rows, back),
                  {{"pairs2", b.pairs2, sizeof(gms_pair) * n, 256}, {"back", b.back, sizeof(gms_dmatch) * back, 256}, {"qt", b.qt, 8 * R, 256},
                   {"cd", b.cd, 4 * R, 256}, {"cix", b.cix, 4 * R, 256}}, b.total, 256);
}

void check_slices(size_t n, size_t mcap, bool mask, size_t tiles, size_t scales)
{
    const size_t m = mask ? n * mcap : 0;
    const BandLayout b = band_layout(n, mcap, mask);
    std::string what = fmt("band %lld pairs, mcap %lld, mask %lld", n, mcap, mask);
    check_regions(what, {{"lists", b.lists, n * 3 * mcap * 8, 8}, {"nfine", b.nfine, n * 1600 * 4, 4}, {"list_len", b.list_len, n * 3 * 4, 4},
                         {"flags", b.flags, n * 4, 4}, {"mask", b.mask, m, 1}}, b.total, 1);
    expect(what, "the cleared span", b.mask - b.nfine, (n * 1600 + n * 4) * 4);
    if (b.total > n * band_bytes_per_pair(mcap, mask)) fail(what, "the slice is larger than n times the bytes per pair");

    const TileLayout t = tile_layout(n, tiles, mcap, mask);
    what = fmt("tile %lld pairs, %lld tiles, mcap %lld, mask %lld", n, tiles, mcap, mask);
    check_regions(what, {{"lists", t.lists, n * tiles * mcap * 8, 8}, {"nfine", t.nfine, n * 1600 * 4, 4}, {"list_len", t.list_len, n * 32 * 4, 4},
                         {"cnt", t.cnt, n * 8 * 4, 4}, {"flags", t.flags, n * 4, 4}, {"state", t.state, 2 * n * 4 * 4, 4},
                         {"rotmask", t.rotmask, n * mcap, 16}, {"bestmask", t.bestmask, m, 1}}, t.total, 16);
    expect(what, "the span cleared per scale", t.flags - t.nfine, (n * 1600 + n * 32 + n * 8) * 4);
    expect(what, "the span cleared per launch", t.state_end - t.flags, n * 9 * 4);
    if (t.total > n * tile_bytes_per_pair(tiles, mcap, mask)) fail(what, "the slice is larger than n times the bytes per pair");

    const StreamLayout s = stream_layout(n, mcap, scales);
    what = fmt("stream %lld pairs, mcap %lld, %lld scales", n, mcap, scales);
    check_regions(what, {{"entries", s.entries, n * mcap * 8, 16}, {"codes", s.codes, n * mcap * 8, 16}, {"nfine", s.nfine, n * 1600 * 4, 16},
                         {"row_cnt", s.row_cnt, n * 192 * 4, 16}, {"counts", s.counts, n * 5 * 8 * 4, 16}, {"flags", s.flags, n * 4, 16},
                         {"tile_cnt", s.tile_cnt, n * 8 * 5 * 8 * 4, 16}, {"tables", s.tables, n * scales * 4 * 400 * 4, 16},
                         {"nleft", s.nleft, n * 4 * 400 * 2, 16}}, s.total, 16);
    expect(what, "the cleared span", s.tile_cnt - s.nfine, n * (1600 + 192 + 40) * 4 + round_up(n * 4, 16));
    if (s.total > n * stream_bytes_per_pair(mcap, scales)) fail(what, "the slice is larger than n times the bytes per pair");

    const StreamDenseLayout d = stream_dense_layout(n, mcap);
    what = fmt("stream-dense %lld pairs, mcap %lld", n, mcap);
    check_regions(what, {{"codes", d.codes, n * mcap * 4, 16}, {"nleft", d.nleft, n * 4 * 400 * 2, 16}, {"flags", d.flags, n * 4, 16}}, d.total, 16);
    expect(what, "the cleared span", d.total - d.flags, n * 4);
    if (d.total > n * stream_dense_bytes_per_pair(mcap)) fail(what, "the slice is larger than n times the bytes per pair");
}

// property: the fixture's sizes. Returns the number of lines compared.
int check_fixture(const char* path)
{
    std::FILE* f = std::fopen(path, "r");
    if (!f) {
        fail(path, "cannot be opened");
        return 0;
    }
    // the most tiles of a scale's TileGeom under the product's right grids: 3 x 1 tiles at scale 0 (20 x 20), 5 x 4 at scale 4 (40 x 40)
    const size_t tiles_of[2] = {3, 20};
    char line[256], name[32];
    int lines = 0;
    while (std::fgets(line, sizeof line, f)) {
        long long a[6] = {0, 0, 0, 0, 0, 0};
        const int k = std::sscanf(line, "%31s %lld %lld %lld %lld %lld %lld", name, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) - 1;
        if (k < 2) {
            fail(line, "is no fixture line");
            continue;
        }
        const size_t want = (size_t)a[k - 1];
        const std::string id = name;
        size_t got = 0;
        if (id == "detect" && k == 5) got = detect_layout((int)a[0], (int)a[1], (int)a[2], (int)a[3]).total;
        else if (id == "pyramid" && k == 6) got = pyramid_layout((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], false).total;
        else if (id == "refined" && k == 6) got = pyramid_layout((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], true).total;
        else if (id == "stereo" && k == 4) got = stereo_bm_layout((int)a[2], (int)a[0], (int)a[1]).total;
        else if (id == "portrait" && k == 4) got = portrait_layout((int)a[2], (int)a[0], (int)a[1]).total;
        else if (id == "bfsel" && k == 4) got = bf_select_layout((int)a[0], a[1], a[2]).total;
        else if (id == "band" && k == 3) got = band_bytes_per_pair((size_t)a[0], a[1] != 0);
        else if (id == "tile" && k == 4) got = tile_bytes_per_pair(tiles_of[a[0] != 0], (size_t)a[1], a[2] != 0);
        else if (id == "stream" && k == 3) got = stream_bytes_per_pair((size_t)a[1], a[0] ? 5 : 1);
        else if (id == "dense" && k == 2) got = stream_dense_bytes_per_pair((size_t)a[0]);
        else {
            fail(line, "is no fixture line");
            continue;
        }
        ++lines;
        if (want != 0) expect(line, "the layout's figure", got, want);
    }
    std::fclose(f);
    return lines;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::printf("usage: ws_layout_check <fixture> [seed]\n");
        return 2;
    }
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 1);
    const int ns[] = {1, 2, 3, 63, 64, 255, 257};
    const int sides[][2] = {{33, 33}, {35, 33}, {97, 65}, {1921, 1081}, {8192, 8192}, {65535, 65535}, {0, 0}};
    for (int n : ns) {
        for (const auto& s0 : sides) {
            const bool random = s0[0] == 0;
            const int w = random ? 33 + (int)(rng() % 4000) : s0[0], h = random ? 33 + (int)(rng() % 4000) : s0[1];
            for (int maxkp : {0, 1, 7, 5000})
                for (int levels : {1, 2, 16}) check_detect(w, h, n, maxkp, levels);
            check_images(w, h, n);  // (n w h passes 4 GiB from 8192 x 8192 x 64 on)
        }
        for (long long rows : {0ll, 1ll, 37ll, 4095ll, 4096ll, 4097ll, 1ll << 22})
            for (long long back : {0ll, 1ll, 17ll, n * rows, (1ll << 33) + 5}) check_bf_select(n, rows, back);
        // mcap: the least and the most big_mcap gives, around multiples of 4096, values no multiple of 16, a random one
        for (size_t mcap : {(size_t)16448, (size_t)4194304, (size_t)20416, (size_t)20480, (size_t)20544, (size_t)4095, (size_t)4097, (size_t)16385,
                            (size_t)1 + rng() % 4194304})
            for (int mask = 0; mask < 2; ++mask)
                for (size_t tiles : {1, 3, 20, 32})  // (257 pairs x 32 tiles x 4 194 304 x 8 bytes passes 4 GiB many times)
                    check_slices((size_t)n, mcap, mask != 0, tiles, tiles == 1 ? 1 : 5);
    }
    const int lines = check_fixture(argv[1]);
    std::printf("ws_layout_check: %ld cases, %d fixture lines: %d bad\n", g_cases, lines, g_bad);
    return g_bad ? 1 : 0;
}
