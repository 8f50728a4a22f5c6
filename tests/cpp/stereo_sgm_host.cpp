// tests/test_stereo_sgm_ref.py: a host build of stereo_sgm_core.h (the parameter rule, the lines of a direction, the path step) and of
// stereo_bm_core.h's subpixel step, as the kernels use them: the path costs of a cost volume line by line, their sum, and the decision
// on it. The test holds the result to the numpy statement tests/stereo_sgm_ref.py.
//   sgm_host_params_ok(params as 14 int32, W, H) -> 0 / 1
//   sgm_host_aggregate(C uint16 [ny][wx][nd], ny, wx, nd, p1, p2, n_paths, S uint16 out, Lmax int32 [n_paths] out) -> 0, or -1 when a
//       pixel is on no line or on two, or a value leaves 16 bits
//   sgm_host_decide(S uint16 [n][nd], tex int32 [n], n, params, disp int32 out, cost int32 out)
//   sgm_host_layout(n, W, H, ny, wx, nd, out uint64 [5]): stereo_sgm_layout's StereoBM total, tex, C, S and total (ws_layout.h)
// -DSGM_HOST_MAIN: a stand-alone program (for a sanitizer run) that aggregates a small random volume and prints a checksum.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "stereo_sgm_core.h"
#include "ws_layout.h"

extern "C" {

int sgm_host_params_ok(const int32_t* params, int W, int H)
{
    gms_stereo_sgm_params p;
    std::memcpy(&p, params, sizeof p);
    return sgm::params_ok(p, W, H) ? 1 : 0;
}

int sgm_host_aggregate(const uint16_t* C, int ny, int wx, int nd, int p1, int p2, int n_paths, uint16_t* S, int32_t* Lmax)
{
    const size_t px = (size_t)ny * wx;
    std::vector<int> sum(px * nd, 0), lp(nd), l(nd);
    std::vector<uint8_t> seen(px);
    for (int r = 0; r < n_paths; r++) {
        const int dy = sgm::path_dy(r), dx = sgm::path_dx(r);
        std::fill(seen.begin(), seen.end(), 0);
        Lmax[r] = 0;
        for (int i = 0; i < sgm::line_count(dy, dx, ny, wx); i++) {
            const sgm::Line ln = sgm::line(dy, dx, i, ny, wx);
            if (ln.len < 1) return -1;
            for (int s = 0; s < ln.len; s++) {
                const int y = ln.y0 + s * dy, x = ln.x0 + s * dx;
                if (y < 0 || y >= ny || x < 0 || x >= wx || seen[(size_t)y * wx + x]++) return -1;
                const uint16_t* c = C + ((size_t)y * wx + x) * nd;
                if (s == 0) {
                    for (int k = 0; k < nd; k++) l[k] = c[k];
                } else {
                    int m = lp[0];
                    for (int k = 1; k < nd; k++) m = lp[k] < m ? lp[k] : m;
                    for (int k = 0; k < nd; k++)
                        l[k] = sgm::step(c[k], lp[k], k > 0 ? lp[k - 1] : sgm::kBig, k + 1 < nd ? lp[k + 1] : sgm::kBig, m, p1, p2);
                }
                for (int k = 0; k < nd; k++) {
                    if (l[k] < 0 || l[k] > c[k] + p2) return -1;  // 0 <= L <= C + p2
                    Lmax[r] = l[k] > Lmax[r] ? l[k] : Lmax[r];
                    sum[((size_t)y * wx + x) * nd + k] += l[k];
                }
                lp = l;
            }
        }
        for (size_t q = 0; q < px; q++)
            if (seen[q] != 1) return -1;
    }
    for (size_t q = 0; q < px * nd; q++) {
        if (sum[q] > 65535) return -1;
        S[q] = (uint16_t)sum[q];
    }
    return 0;
}

void sgm_host_decide(const uint16_t* S, const int32_t* tex, int n, const int32_t* params, int32_t* disp, int32_t* cost)
{
    gms_stereo_sgm_params p;
    std::memcpy(&p, params, sizeof p);
    const int nd = p.bm.num_disparities, md = p.bm.min_disparity;
    for (int q = 0; q < n; q++) {
        const uint16_t* s = S + (size_t)q * nd;
        int mind = 0;
        for (int k = 1; k < nd; k++)
            if (s[k] < s[mind]) mind = k;
        const int mins = s[mind];
        bool ok = tex[q] >= p.bm.texture_threshold;
        if (ok && p.bm.uniqueness_ratio > 0) {
            const int thresh = mins + mins * p.bm.uniqueness_ratio / 100;
            for (int k = 0; k < nd; k++) ok = ok && !((k < mind - 1 || k > mind + 1) && s[k] <= thresh);
        }
        disp[q] = ok ? sbm::subpixel(nd, md, mind, s[mind + 1 < nd ? mind + 1 : nd - 2], s[mind >= 1 ? mind - 1 : 1], mins) : (md - 1) * 16;
        cost[q] = ok ? mins : -1;
    }
}

void sgm_host_layout(int n, int W, int H, int ny, int wx, int nd, uint64_t* out)
{
    const gms::StereoSgmLayout L = gms::stereo_sgm_layout(n, W, H, ny, wx, nd);
    out[0] = L.bm.total; out[1] = L.tex; out[2] = L.C; out[3] = L.S; out[4] = L.total;
}

}  // extern "C"

#ifdef SGM_HOST_MAIN
int main()
{
    const int ny = 7, wx = 9, nd = 16;
    std::vector<uint16_t> C((size_t)ny * wx * nd), S(C.size());
    uint32_t v = 12345;
    for (auto& c : C) {
        v = v * 1664525u + 1013904223u;
        c = (uint16_t)((v >> 16) % 3000);
    }
    int32_t lmax[sgm::kMaxPaths];
    if (sgm_host_aggregate(C.data(), ny, wx, nd, 200, 800, 8, S.data(), lmax) != 0) return 1;
    unsigned long long sum = 0;
    for (auto s : S) sum = sum * 31 + s;
    std::printf("sgm_host: tiny %llu\n", sum);
    return 0;
}
#endif
