// stereo_bm_core.h -- StereoBM's geometry, parameter check and subpixel step: what the C ABI (capi_stereo.cpp) and the
// kernels (stereo_bm_kernels.hip) share. tests/stereo_bm_ref.py states the same in numpy.
#pragma once
#include <stdint.h>

#include "gms.h"

#if defined(__HIPCC__)
#define SBM_HD __host__ __device__ inline
#else
#define SBM_HD inline
#endif

namespace sbm {

// Where findStereoCorrespondenceBM computes: output column lofs + x for x in [0, wx); disparity index k reads right column x + k (+ rofs)
// and means disparity nd - 1 + md - k. wx = min(width1, W - lofs): with md > 0 OpenCV's loop runs md columns past the row's end.
struct Geometry {
    int lofs, rofs, width1, wx;
    int none;            // width1 < 1, lofs >= W or rofs >= W: the whole map is FILTERED
    int w2;
    int filtered;        // (md - 1) * 16
    int roi_x0, roi_x1;  // getValidDisparityROI of two full-image ROIs: columns [lofs + w2, W - w2) (rows [w2, H - w2))
    int minX1, maxX1;    // validateDisparity's column range
};

SBM_HD Geometry geometry(const gms_stereo_bm_params& p, int W)
{
    Geometry g;
    const int nd = p.num_disparities, md = p.min_disparity;
    g.lofs = nd - 1 + md > 0 ? nd - 1 + md : 0;
    g.rofs = nd - 1 + md < 0 ? -(nd - 1 + md) : 0;
    g.width1 = W - g.rofs - nd + 1;
    g.wx = g.width1 < W - g.lofs ? g.width1 : W - g.lofs;
    g.none = g.width1 < 1 || g.lofs >= W || g.rofs >= W;
    g.w2 = p.block_size / 2;
    g.filtered = (md - 1) * 16;
    g.roi_x0 = g.lofs + g.w2;
    g.roi_x1 = W - g.w2;
    g.minX1 = md + nd > 0 ? md + nd : 0;
    g.maxX1 = W + (md < 0 ? md : 0);
    return g;
}

// the parameter sets stated here (the others are GMS_ERR_BAD_ARG)
SBM_HD bool params_ok(const gms_stereo_bm_params& p, int W, int H)
{
    const int bs = p.block_size, nd = p.num_disparities, md = p.min_disparity;
    return p.pre_filter_type == GMS_STEREO_BM_PREFILTER_XSOBEL && p.pre_filter_size >= 5 && p.pre_filter_size <= 255 &&
           (p.pre_filter_size & 1) && p.pre_filter_cap >= 1 && p.pre_filter_cap <= 63 && bs >= 5 && bs <= 51 && (bs & 1) && nd > 0 &&
           nd <= 512 && nd % 16 == 0 && md >= -2047 && md <= 2048 - nd && p.texture_threshold >= 0 && p.uniqueness_ratio >= 0 &&
           p.uniqueness_ratio <= 1000 && p.speckle_window_size == 0 && W > 0 && W <= GMS_STEREO_BM_MAX_WIDTH && H > 0 &&
           bs < (W < H ? W : H);
}

// the 4-fractional-bit disparity of winner mind (cost c) from its neighbours' costs p = sad[mind + 1], n = sad[mind - 1]; C's
// truncating division, arithmetic shift
SBM_HD int subpixel(int nd, int md, int mind, int p, int n, int c)
{
    const int den = p + n - 2 * c + (p > n ? p - n : n - p);
    return ((nd - mind - 1 + md) * 256 + (den != 0 ? (p - n) * 256 / den : 0) + 15) >> 4;
}

}  // namespace sbm
