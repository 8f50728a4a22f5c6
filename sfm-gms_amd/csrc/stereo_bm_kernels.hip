// stereo_bm_kernels.hip -- the reference's block-matching baseline (DisparityUtil.cpp:22-49): OpenCV 4.5.2's
// StereoBM::compute on its integer path for a batch of n equally sized 8-bit pairs, and the reference's 8-bit map.
//
// Three stream-ordered launches per batch, no allocation, no synchronisation (graph-capturable):
//   sbm_prefilter_kernel   XSOBEL pre-filter of both images of every pair: a 64 x 16 tile plus a one-pixel halo through LDS.
//   sbm_match_kernel<KPL>  cost volume and winner-take-all. A workgroup owns kTileX output columns and a band of kBandY rows, and holds
//                          the band's pre-filtered rows in LDS (left: the tile plus the window, right: the tile plus the window plus
//                          nd - 1). Each wave walks one column at a time down the band with running vertical window sums per
//                          disparity; lane l holds disparities l, l + 64, ... (KPL of them). Costs and winners stay in registers: no
//                          cost volume goes to HBM. The raw map goes to d_disp16, the costs to the workspace.
//   sbm_validate_kernel    one workgroup per row: validateDisparity (a 64-bit LDS atomicMin of cost << 32 | x per target column), the
//                          ROI fill, the final int16 row and the cost row.
// launch_stereo_bm_prefilter and launch_stereo_bm_validate launch the first and the last alone: stereo_sgm_kernels.hip runs them
// around its own kernels.
// gms_stereo_bm_normalize_device: sbm_normalize_kernel, one workgroup per map (min / max, then NORM_MINMAX to 8 bits, 0 -> 255).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "stereo_bm_core.h"

namespace gms {
namespace {

constexpr int kPfX = 64, kPfY = 16, kPfBlock = 256;
constexpr int kTileX = 64, kBandY = 32, kMatchBlock = 256, kMatchWaves = kMatchBlock / 64;
constexpr int kValBlock = 256;
constexpr int kNormBlock = 1024;
constexpr int kMaxW = GMS_STEREO_BM_MAX_WIDTH;

__global__ void __launch_bounds__(kPfBlock)
sbm_prefilter_kernel(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right, int64_t pair_stride, int pitch, int W, int H,
                     int cap, uint8_t* __restrict__ pre)
{
    __shared__ uint8_t t[kPfY + 2][kPfX + 2];  // image rows y0 - 1 .. y0 + kPfY, columns x0 - 1 .. x0 + kPfX
    const int img = blockIdx.z, tid = threadIdx.x;
    const uint8_t* __restrict__ src = ((img & 1) ? right : left) + (int64_t)(img >> 1) * pair_stride;
    const int x0 = blockIdx.x * kPfX, y0 = blockIdx.y * kPfY;
    for (int i = tid; i < (kPfY + 2) * (kPfX + 2); i += kPfBlock) {
        const int r = i / (kPfX + 2), c = i - r * (kPfX + 2);
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        t[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(int64_t)y * pitch + x] : 0;
    }
    __syncthreads();
    uint8_t* __restrict__ dst = pre + (int64_t)img * H * W;
    for (int i = tid; i < kPfY * kPfX; i += kPfBlock) {
        const int ty = i / kPfX, tx = i - ty * kPfX;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        int v = cap;
        // OpenCV works rows in pairs (y, y + 1): an odd height's last row is left over, all cap. Within a pair the rows above and below
        // are reflect-101 (row 1 above row 0, row H - 2 below row H - 1). Columns 0 and W - 1 are cap.
        if (!((H & 1) && y == H - 1) && x > 0 && x < W - 1) {
            const int yu = y > 0 ? y - 1 : 1, yd = y + 1 < H ? y + 1 : y - 1;
            const int ru = yu - y0 + 1, rc = ty + 1, rd = yd - y0 + 1, c = tx + 1;
            const int d = (t[ru][c + 1] - t[ru][c - 1]) + 2 * (t[rc][c + 1] - t[rc][c - 1]) + (t[rd][c + 1] - t[rd][c - 1]);
            v = (d < -cap ? -cap : d > cap ? cap : d) + cap;
        }
        dst[(int64_t)y * W + x] = (uint8_t)v;
    }
}

struct MatchArgs {
    const uint8_t* pre;
    int16_t* disp;
    int32_t* cost;
    int W, H, nd, md, w2, cap, tex_thresh, uniq, lofs, rofs, wx, filtered;
};

// one LDS row pair's horizontal sums at output column x: hs[i] for disparity lane + 64 i; returns the texture term (wave-uniform)
template <int KPL>
__device__ __forceinline__ int row_sums(const uint8_t* __restrict__ rl, const uint8_t* __restrict__ rr, const MatchArgs& a, int x, int bL,
                                        int bR, const int (&kread)[KPL], int (&hs)[KPL])
{
    int tex = 0;
#pragma unroll
    for (int i = 0; i < KPL; i++) hs[i] = 0;
    for (int j = -a.w2; j <= a.w2; j++) {
        const int xl = a.lofs + min(max(x + j, -a.lofs), a.W - 1 - a.lofs) - bL;
        const int xr = a.rofs + min(max(x + j, -a.rofs), a.W - a.nd - a.rofs) - bR;
        const int lv = rl[xl];
        tex += abs(lv - a.cap);
        const uint8_t* __restrict__ rp = rr + xr;
#pragma unroll
        for (int i = 0; i < KPL; i++) hs[i] += abs(lv - (int)rp[kread[i]]);
    }
    return tex;
}

// the cost of disparity kq (wave-uniform) from the lane that holds it
template <int KPL>
__device__ __forceinline__ int sad_at(const int (&vs)[KPL], int kq)
{
    const int slot = kq >> 6;
    int v = vs[0];
#pragma unroll
    for (int i = 1; i < KPL; i++)
        if (slot == i) v = vs[i];
    return __shfl(v, kq & 63);
}

template <int KPL>
__global__ void __launch_bounds__(kMatchBlock)
sbm_match_kernel(MatchArgs a)
{
    extern __shared__ uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.z;
    const int x0 = blockIdx.x * kTileX;                  // output columns [x0, x0 + kTileX) of [0, wx)
    const int ya = a.w2 + blockIdx.y * kBandY;           // image rows [ya, ye) of [w2, H - w2)
    const int ye = min(ya + kBandY, a.H - a.w2);
    const int bs = 2 * a.w2 + 1;
    const int nR = ye - ya + 2 * a.w2;                   // LDS row r = image row ya - w2 + r
    const int cL = kTileX + 2 * a.w2, cR = kTileX + 2 * a.w2 + a.nd - 1;
    const int bL = a.lofs + x0 - a.w2, bR = a.rofs + x0 - a.w2;  // image column of LDS column 0
    uint8_t* sL = smem;
    uint8_t* sR = smem + nR * cL;
    const uint8_t* __restrict__ gL = a.pre + (int64_t)(2 * pair) * a.H * a.W;
    const uint8_t* __restrict__ gR = gL + (int64_t)a.H * a.W;
    const int64_t row0 = (int64_t)(ya - a.w2) * a.W;
    for (int i = tid; i < nR * cL; i += kMatchBlock) {
        const int r = i / cL, x = bL + (i - r * cL);
        sL[i] = (x >= 0 && x < a.W) ? gL[row0 + (int64_t)r * a.W + x] : 0;
    }
    for (int i = tid; i < nR * cR; i += kMatchBlock) {
        const int r = i / cR, x = bR + (i - r * cR);
        sR[i] = (x >= 0 && x < a.W) ? gR[row0 + (int64_t)r * a.W + x] : 0;
    }
    __syncthreads();

    int kread[KPL];  // the right-row offset of each slot; slots past nd read disparity nd - 1 and take no part
#pragma unroll
    for (int i = 0; i < KPL; i++) kread[i] = min(lane + 64 * i, a.nd - 1);

    for (int c = wave; c < kTileX; c += kMatchWaves) {
        const int x = x0 + c;
        if (x >= a.wx) break;  // wave-uniform
        int vs[KPL], hs[KPL], ho[KPL];
#pragma unroll
        for (int i = 0; i < KPL; i++) vs[i] = 0;
        int ts = 0;
        for (int r = 0; r < bs; r++) {
            ts += row_sums<KPL>(sL + r * cL, sR + r * cR, a, x, bL, bR, kread, hs);
#pragma unroll
            for (int i = 0; i < KPL; i++) vs[i] += hs[i];
        }
        for (int y = ya; y < ye; y++) {
            if (y > ya) {  // slide: row y + w2 enters, row y - w2 - 1 leaves
                const int rn = y - ya + 2 * a.w2, ro = rn - bs;
                ts += row_sums<KPL>(sL + rn * cL, sR + rn * cR, a, x, bL, bR, kread, hs);
                ts -= row_sums<KPL>(sL + ro * cL, sR + ro * cR, a, x, bL, bR, kread, ho);
#pragma unroll
                for (int i = 0; i < KPL; i++) vs[i] += hs[i] - ho[i];
            }
            // the winner: the lowest (sad, k); sad <= 51 * 51 * 126 < 2^19 and k < 512, so (sad << 9 | k) orders both in 28 bits
            int key = INT_MAX;
#pragma unroll
            for (int i = 0; i < KPL; i++)
                if (lane + 64 * i < a.nd) key = min(key, (vs[i] << 9) | (lane + 64 * i));
            for (int s = 32; s > 0; s >>= 1) key = min(key, __shfl_xor(key, s));
            const int mind = key & 511, minsad = key >> 9;
            bool ok = ts >= a.tex_thresh;
            if (ok && a.uniq > 0) {
                const int thresh = minsad + minsad * a.uniq / 100;
                bool other = false;
#pragma unroll
                for (int i = 0; i < KPL; i++) {
                    const int k = lane + 64 * i;
                    other |= k < a.nd && (k < mind - 1 || k > mind + 1) && vs[i] <= thresh;
                }
                ok = __ballot(other) == 0ull;
            }
            int d = a.filtered, cst = -1;
            if (ok) {  // wave-uniform
                const int p = sad_at<KPL>(vs, mind + 1 < a.nd ? mind + 1 : a.nd - 2);
                const int n = sad_at<KPL>(vs, mind >= 1 ? mind - 1 : 1);
                d = sbm::subpixel(a.nd, a.md, mind, p, n, minsad);
                cst = minsad;
            }
            if (lane == 0) {
                const int64_t o = ((int64_t)pair * a.H + y) * a.W + a.lofs + x;
                a.disp[o] = (int16_t)d;
                a.cost[o] = cst;
            }
        }
    }
}

struct ValArgs {
    int16_t* disp;
    const int32_t* wcost;
    int32_t* cost_out;
    int W, H, w2, lofs, wx, none, filtered, maxdiff, minX1, maxX1, roi_x0, roi_x1;
};

__global__ void __launch_bounds__(kValBlock)
sbm_validate_kernel(ValArgs a)
{
    __shared__ unsigned long long s_key[kMaxW];  // per target column x2: cost << 32 | x of the strictly cheapest x, lowest x on ties
    __shared__ int16_t s_d[kMaxW];               // the raw row
    const int y = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x;
    const int64_t row = ((int64_t)pair * a.H + y) * a.W;
    const bool rows_in = !a.none && y >= a.w2 && y < a.H - a.w2;  // workgroup-uniform
    const int F = a.filtered;
    const bool check = rows_in && a.maxdiff >= 0;
    for (int x = tid; x < a.W; x += kValBlock) {
        const bool computed = rows_in && x >= a.lofs && x < a.lofs + a.wx;
        s_d[x] = computed ? a.disp[row + x] : (int16_t)F;
        s_key[x] = ~0ull;
    }
    __syncthreads();
    if (check) {
        for (int x = a.minX1 + tid; x < a.maxX1; x += kValBlock) {
            const int d = s_d[x];
            if (d == F) continue;
            const int x2 = x - ((d + 8) >> 4);
            if ((unsigned)x2 < (unsigned)a.W)
                atomicMin(&s_key[x2], ((unsigned long long)(uint32_t)a.wcost[row + x] << 32) | (unsigned long long)(uint32_t)x);
        }
        __syncthreads();
    }
    const int maxdiff16 = min(a.maxdiff, 1 << 20) * 16;  // beyond any difference of two 16-bit values either way
    for (int x = tid; x < a.W; x += kValBlock) {
        int d = s_d[x];
        if (check && d != F && x >= a.minX1 && x < a.maxX1) {
            const int xa = x - (d >> 4), xb = x - ((d + 15) >> 4);
            bool off_a = false, off_b = false;
            if ((unsigned)xa < (unsigned)a.W && s_key[xa] != ~0ull) {
                const int d2 = s_d[(uint32_t)s_key[xa]];
                off_a = d2 > F && abs(d2 - d) > maxdiff16;
            }
            if ((unsigned)xb < (unsigned)a.W && s_key[xb] != ~0ull) {
                const int d2 = s_d[(uint32_t)s_key[xb]];
                off_b = d2 > F && abs(d2 - d) > maxdiff16;
            }
            if (off_a && off_b) d = F;
        }
        const bool in_roi = rows_in && x >= a.roi_x0 && x < a.roi_x1;
        a.disp[row + x] = (int16_t)(in_roi ? d : F);
        if (a.cost_out) a.cost_out[row + x] = (rows_in && x >= a.lofs && x < a.lofs + a.wx) ? a.wcost[row + x] : -1;
    }
}

__global__ void __launch_bounds__(kNormBlock)
sbm_normalize_kernel(const int16_t* __restrict__ disp, int64_t px, uint8_t* __restrict__ out)
{
    __shared__ int s_mn[kNormBlock / 64], s_mx[kNormBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int16_t* __restrict__ src = disp + (int64_t)blockIdx.x * px;
    uint8_t* __restrict__ dst = out + (int64_t)blockIdx.x * px;
    int mn = INT_MAX, mx = INT_MIN;
    for (int64_t i = tid; i < px; i += kNormBlock) {
        const int v = src[i];
        mn = min(mn, v);
        mx = max(mx, v);
    }
    for (int s = 32; s > 0; s >>= 1) {
        mn = min(mn, __shfl_xor(mn, s));
        mx = max(mx, __shfl_xor(mx, s));
    }
    if (lane == 0) {
        s_mn[wave] = mn;
        s_mx[wave] = mx;
    }
    __syncthreads();
    mn = s_mn[0];
    mx = s_mx[0];
    for (int w = 1; w < kNormBlock / 64; w++) {
        mn = min(mn, s_mn[w]);
        mx = max(mx, s_mx[w]);
    }
    // cv::normalize(NORM_MINMAX, 0, 255): scale = (dmax - dmin) * (1 / (smax - smin)), shift = dmin - smin * scale, in double; the
    // conversion to 8 bits takes both as float, v * scale + shift unfused, cvRound (half to even), saturation
    const double range = (double)mx - (double)mn;
    const double scale = 255.0 * (range > 2.220446049250313e-16 ? 1.0 / range : 0.0);
    const double shift = 0.0 - (double)mn * scale;
    const float fs = (float)scale, fb = (float)shift;
    for (int64_t i = tid; i < px; i += kNormBlock) {
        const float v = __fadd_rn(__fmul_rn((float)src[i], fs), fb);
        int r = (int)rintf(v);
        r = r < 0 ? 0 : r > 255 ? 255 : r;
        dst[i] = (uint8_t)(r == 0 ? 255 : r);
    }
}

template <int KPL>
hipError_t launch_match(const MatchArgs& a, int n, hipStream_t stream)
{
    const dim3 grid((uint32_t)((a.wx + kTileX - 1) / kTileX), (uint32_t)((a.H - 2 * a.w2 + kBandY - 1) / kBandY), (uint32_t)n);
    const size_t lds = (size_t)(kBandY + 2 * a.w2) * (size_t)(2 * kTileX + 4 * a.w2 + a.nd - 1);  // < 64 KiB at w2 = 25, nd = 512
    hipLaunchKernelGGL(sbm_match_kernel<KPL>, grid, dim3(kMatchBlock), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

size_t stereo_bm_ws_bytes(int n, int W, int H) { return stereo_bm_layout(n, W, H).total; }

hipError_t launch_stereo_bm_prefilter(const gms_stereo_bm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H,
                                      int pitch, uint8_t* pre, hipStream_t stream)
{
    hipLaunchKernelGGL(sbm_prefilter_kernel, dim3((uint32_t)((W + kPfX - 1) / kPfX), (uint32_t)((H + kPfY - 1) / kPfY), (uint32_t)(2 * n)),
                       dim3(kPfBlock), 0, stream, d_left, d_right, (int64_t)pitch * H, pitch, W, H, p.pre_filter_cap, pre);
    return hipGetLastError();
}

hipError_t launch_stereo_bm_validate(const gms_stereo_bm_params& p, int n, int W, int H, int16_t* d_disp, const int32_t* wcost,
                                     int32_t* d_cost, hipStream_t stream)
{
    const sbm::Geometry g = sbm::geometry(p, W);
    ValArgs v{d_disp, wcost, d_cost, W, H, g.w2, g.lofs, g.wx, g.none, g.filtered, p.disp12_max_diff, g.minX1, g.maxX1, g.roi_x0, g.roi_x1};
    hipLaunchKernelGGL(sbm_validate_kernel, dim3((uint32_t)H, (uint32_t)n), dim3(kValBlock), 0, stream, v);
    return hipGetLastError();
}

hipError_t launch_stereo_bm(const gms_stereo_bm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H, int pitch,
                            void* d_ws, int16_t* d_disp, int32_t* d_cost, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const sbm::Geometry g = sbm::geometry(p, W);
    const StereoBmLayout L = stereo_bm_layout(n, W, H);
    uint8_t* pre = ws_ptr<uint8_t>(d_ws, L.pre);
    int32_t* cost = ws_ptr<int32_t>(d_ws, L.cost);
    if (!g.none) {
        hipError_t e = launch_stereo_bm_prefilter(p, d_left, d_right, n, W, H, pitch, pre, stream);
        if (e != hipSuccess) return e;
        MatchArgs a{pre, d_disp, cost, W, H, p.num_disparities, p.min_disparity, g.w2, p.pre_filter_cap, p.texture_threshold,
                    p.uniqueness_ratio, g.lofs, g.rofs, g.wx, g.filtered};
        const int nd = p.num_disparities;
        e = nd <= 64 ? launch_match<1>(a, n, stream) : nd <= 128 ? launch_match<2>(a, n, stream)
            : nd <= 256 ? launch_match<4>(a, n, stream) : launch_match<8>(a, n, stream);
        if (e != hipSuccess) return e;
    }
    return launch_stereo_bm_validate(p, n, W, H, d_disp, cost, d_cost, stream);
}

hipError_t launch_stereo_bm_normalize(const int16_t* d_disp, int n, int W, int H, uint8_t* d_out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sbm_normalize_kernel, dim3((uint32_t)n), dim3(kNormBlock), 0, stream, d_disp, (int64_t)W * H, d_out);
    return hipGetLastError();
}

}  // namespace gms
