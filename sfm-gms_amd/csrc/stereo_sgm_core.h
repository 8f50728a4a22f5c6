// stereo_sgm_core.h -- semi-global matching on StereoBM's costs: the parameter check, the eight path directions, the
// lines a direction cuts the computed region into, and one step of the path recurrence. What the C ABI (capi_stereo.cpp, capi_dense.cpp), the kernels
// (stereo_sgm_kernels.hip) and the host build (tests/cpp/stereo_sgm_host.cpp) share; tests/stereo_sgm_ref.py states the same in numpy.
// This is the library's own definition, not cv::StereoSGBM: the matching cost is StereoBM's window SAD, not Birchfield-Tomasi.
#pragma once
#include <stdint.h>

#include "gms.h"
#include "stereo_bm_core.h"

namespace sgm {

constexpr int kMaxPaths = 8;
// (dy, dx) of path r: a pixel's predecessor on the path is (y - dy, x - dx). n_paths = 4 uses the first four.
SBM_HD int path_dy(int r)
{
    constexpr int t[kMaxPaths] = {0, 0, 1, -1, 1, 1, -1, -1};
    return t[r];
}
SBM_HD int path_dx(int r)
{
    constexpr int t[kMaxPaths] = {1, -1, 0, 0, 1, -1, 1, -1};
    return t[r];
}
// above every path cost, and still far from overflow with a penalty added
constexpr int kBig = 1 << 28;

// The parameter sets stated here (the others are GMS_ERR_BAD_ARG): StereoBM's, 0 <= p1 <= p2, four or eight paths, and every path
// cost and their sum within 16 unsigned bits: 0 <= L <= C + p2 by induction over the path, C <= block_size^2 * 2 * pre_filter_cap.
SBM_HD bool params_ok(const gms_stereo_sgm_params& p, int W, int H)
{
    if (!sbm::params_ok(p.bm, W, H)) return false;
    if (p.p1 < 0 || p.p2 < p.p1 || (p.n_paths != 4 && p.n_paths != 8)) return false;
    const int64_t cmax = (int64_t)p.bm.block_size * p.bm.block_size * 2 * p.bm.pre_filter_cap;
    return (int64_t)p.n_paths * (cmax + (int64_t)p.p2) <= 65535;
}

// The region paths run in: rows [w2, H - w2) and output columns lofs + [0, wx), as (ny, wx); a path never leaves it.
// The lines of direction (dy, dx): every pixel of the region lies on exactly one. Line i starts at the pixel whose predecessor is outside.
SBM_HD int line_count(int dy, int dx, int ny, int wx)
{
    return dy == 0 ? ny : dx == 0 ? wx : wx + ny - 1;
}

struct Line {
    int y0, x0, len;
};

SBM_HD Line line(int dy, int dx, int i, int ny, int wx)
{
    const int ey = dy > 0 ? 0 : ny - 1, ex = dx > 0 ? 0 : wx - 1;  // the entry row and column
    Line l;
    if (dy == 0) {
        l.y0 = i; l.x0 = ex; l.len = wx;
    } else if (dx == 0) {
        l.y0 = ey; l.x0 = i; l.len = ny;
    } else {
        // the entry row's pixels first, then the entry column's other pixels, away from the entry row
        l.y0 = i < wx ? ey : (dy > 0 ? i - wx + 1 : ny - 1 - (i - wx + 1));
        l.x0 = i < wx ? i : ex;
        const int ly = dy > 0 ? ny - l.y0 : l.y0 + 1, lx = dx > 0 ? wx - l.x0 : l.x0 + 1;
        l.len = ly < lx ? ly : lx;
    }
    return l;
}

// L[k] = C[k] + min(Lp[k], Lp[k - 1] + p1, Lp[k + 1] + p1, m + p2) - m with m = min over k of Lp[k]; a neighbour outside [0, nd) is
// passed as kBig
SBM_HD int step(int c, int lp, int lp_below, int lp_above, int m, int p1, int p2)
{
    int t = lp < m + p2 ? lp : m + p2;
    t = lp_below + p1 < t ? lp_below + p1 : t;
    t = lp_above + p1 < t ? lp_above + p1 : t;
    return c + t - m;
}

}  // namespace sgm
