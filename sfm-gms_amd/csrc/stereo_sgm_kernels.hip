// stereo_sgm_kernels.hip -- semi-global matching on StereoBM's costs (stereo_sgm_core.h; tests/stereo_sgm_ref.py) for a
// batch of n equally sized 8-bit pairs. The library's own definition, not cv::StereoSGBM.
//
// Stream-ordered launches, no allocation, no synchronisation (graph-capturable):
//   sbm_prefilter_kernel    StereoBM's, unchanged (launch_stereo_bm_prefilter).
//   sgm_cost_kernel<KPL>    the front half of sbm_match_kernel -- the same tile, band and LDS rows, running vertical window sums per
//                           disparity, lane l holding disparities l, l + 64, ... -- with the costs written to the volume
//                           C[pair][y][x][k] (uint16, k fastest) and the texture sum to its plane, in place of the winner.
//   sgm_path_kernel<R, FIRST> one launch per direction: one wave per path line, a loop along the line. Lane l holds the R consecutive
//                           disparities l R ..: one load of 2 R bytes fetches their costs, the k +- 1 neighbours are in the lane but
//                           for its two ends (one wave shift each), m is a wave minimum; both are DPP moves, no LDS traffic. The
//                           costs and the S values of the next kPathDepth pixels are in flight while a pixel is worked: neither
//                           depends on L, so a step costs its arithmetic, not a trip to memory. A pixel lies on one line of a
//                           direction, so S is written (the first direction) or read, added to and written (the others) by one
//                           lane per value: no atomics.
//   sgm_decide_kernel<R>    one wave per pixel, a few pixels in turn: sbm_match_kernel's tail on S in the same lane layout. The raw map
//                           goes to d_disp16, the winner's S to StereoBM's cost plane of the workspace.
//   sbm_validate_kernel     StereoBM's, unchanged (launch_stereo_bm_validate): left-right check, ROI fill, the cost map.
// Every value of C, L and S is below 2^16 (sgm::params_ok) and is held in 32-bit registers; in memory two share a 32-bit word, and S
// is added to two values at a time: no carry leaves the low half because the sum over all paths fits 16 bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "stereo_sgm_core.h"

namespace gms {
namespace {

constexpr int kTileX = 64, kBandY = 32, kCostBlock = 256, kCostWaves = kCostBlock / 64;
constexpr int kPathBlock = 256, kPathWaves = kPathBlock / 64;
constexpr int kPathDepth = 8;                                            // pixels ahead whose C and S a path wave has in flight
constexpr int kDecBlock = 256, kDecWaves = kDecBlock / 64, kDecPix = 8;  // pixels a wave of the decision kernel takes in turn

// A DPP move of v (every lane enabled): a lane whose source lane does not exist keeps `old`. Called with all 64 lanes active.
template <int CTRL>
__device__ __forceinline__ int dpp(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false);
}
constexpr int kQuadSwap1 = 0xB1, kQuadSwap2 = 0x4E;      // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1]
constexpr int kRowHalfMirror = 0x141, kRowMirror = 0x140;  // lane i of 8 <- 7 - i; lane i of a row of 16 <- 15 - i
constexpr int kWaveShl1 = 0x130, kWaveShr1 = 0x138;      // lane i <- lane i + 1 (lane 63 keeps old); lane i <- lane i - 1 (lane 0 keeps old)

// the minimum over the wave's 64 lanes, in every lane (wave-uniform): four exchanges inside each row of 16, then the four rows
__device__ __forceinline__ int wave_min(int v)
{
    v = min(v, dpp<kQuadSwap1>(v, v));
    v = min(v, dpp<kQuadSwap2>(v, v));
    v = min(v, dpp<kRowHalfMirror>(v, v));
    v = min(v, dpp<kRowMirror>(v, v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

struct CostArgs {
    const uint8_t* pre;
    uint16_t* C;
    int32_t* tex;
    int W, H, nd, w2, cap, lofs, rofs, wx;
};

// one LDS row pair's horizontal sums at output column x: hs[i] for disparity lane + 64 i; returns the texture term (wave-uniform)
template <int KPL>
__device__ __forceinline__ int row_sums(const uint8_t* __restrict__ rl, const uint8_t* __restrict__ rr, const CostArgs& a, int x, int bL,
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

template <int KPL>
__global__ void __launch_bounds__(kCostBlock)
sgm_cost_kernel(CostArgs a)
{
    extern __shared__ uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.z;
    const int x0 = blockIdx.x * kTileX;                  // output columns [x0, x0 + kTileX) of [0, wx)
    const int ya = a.w2 + blockIdx.y * kBandY;           // image rows [ya, ye) of [w2, H - w2)
    const int ye = min(ya + kBandY, a.H - a.w2);
    const int bs = 2 * a.w2 + 1, ny = a.H - 2 * a.w2;
    const int nR = ye - ya + 2 * a.w2;                   // LDS row r = image row ya - w2 + r
    const int cL = kTileX + 2 * a.w2, cR = kTileX + 2 * a.w2 + a.nd - 1;
    const int bL = a.lofs + x0 - a.w2, bR = a.rofs + x0 - a.w2;  // image column of LDS column 0
    uint8_t* sL = smem;
    uint8_t* sR = smem + nR * cL;
    const uint8_t* __restrict__ gL = a.pre + (int64_t)(2 * pair) * a.H * a.W;
    const uint8_t* __restrict__ gR = gL + (int64_t)a.H * a.W;
    const int64_t row0 = (int64_t)(ya - a.w2) * a.W;
    for (int i = tid; i < nR * cL; i += kCostBlock) {
        const int r = i / cL, x = bL + (i - r * cL);
        sL[i] = (x >= 0 && x < a.W) ? gL[row0 + (int64_t)r * a.W + x] : 0;
    }
    for (int i = tid; i < nR * cR; i += kCostBlock) {
        const int r = i / cR, x = bR + (i - r * cR);
        sR[i] = (x >= 0 && x < a.W) ? gR[row0 + (int64_t)r * a.W + x] : 0;
    }
    __syncthreads();

    int kread[KPL];  // the right-row offset of each slot; slots past nd read disparity nd - 1 and write nothing
#pragma unroll
    for (int i = 0; i < KPL; i++) kread[i] = min(lane + 64 * i, a.nd - 1);

    for (int c = wave; c < kTileX; c += kCostWaves) {
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
            const int64_t px = ((int64_t)pair * ny + (y - a.w2)) * a.wx + x;
            uint16_t* __restrict__ dst = a.C + px * a.nd;
#pragma unroll
            for (int i = 0; i < KPL; i++)
                if (lane + 64 * i < a.nd) dst[lane + 64 * i] = (uint16_t)vs[i];
            if (lane == 0) a.tex[px] = ts;
        }
    }
}

// R consecutive 16-bit values of one lane, as R / 2 words: value j is the low (j even) or high half of word j / 2
template <int R>
struct alignas(2 * R) Run {
    uint32_t w[R / 2];
};

template <int R>
__device__ __forceinline__ void unpack(const Run<R>& v, int (&o)[R])
{
#pragma unroll
    for (int j = 0; j < R / 2; j++) {
        o[2 * j] = (int)(v.w[j] & 0xffffu);
        o[2 * j + 1] = (int)(v.w[j] >> 16);
    }
}

template <int R>
__device__ __forceinline__ Run<R> pack(const int (&v)[R])
{
    Run<R> o;
#pragma unroll
    for (int j = 0; j < R / 2; j++) o.w[j] = (uint32_t)v[2 * j] | ((uint32_t)v[2 * j + 1] << 16);
    return o;
}

struct PathArgs {
    const uint16_t* C;
    uint16_t* S;
    int ny, wx, nd, dy, dx, p1, p2, n_lines;
};

template <int R, bool FIRST>
__global__ void __launch_bounds__(kPathBlock)
sgm_path_kernel(PathArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kPathWaves + (threadIdx.x >> 6);
    if (i >= a.n_lines) return;  // wave-uniform
    const sgm::Line ln = sgm::line(a.dy, a.dx, i, a.ny, a.wx);
    const bool active = lane * R < a.nd;  // nd is a multiple of 16: a lane's run is inside [0, nd) or outside
    // Every lane loads at every step, so that the loads in flight can be counted: a lane outside the range reads lane 0's run (the
    // same bytes, no further traffic) and drops it, and past the line's end the last pixel is read again and dropped.
    const int64_t first = (((int64_t)blockIdx.y * a.ny + ln.y0) * a.wx + ln.x0) * a.nd + (active ? lane * R : 0);
    const int64_t delta = ((int64_t)a.dy * a.wx + a.dx) * a.nd;
    const uint16_t* __restrict__ cp = a.C + first;
    uint16_t* sp = a.S + first;
    Run<R> cb[kPathDepth], sb[kPathDepth];  // the pixels in flight: slot j holds pixel s with s % kPathDepth == j (registers)
#pragma unroll
    for (int j = 0; j < kPathDepth; j++) {
        const int64_t at = (int64_t)min(j, ln.len - 1) * delta;
        cb[j] = *reinterpret_cast<const Run<R>*>(cp + at);
        sb[j] = {};
        if (!FIRST) sb[j] = *reinterpret_cast<const Run<R>*>(sp + at);
    }
    int lp[R];
#pragma unroll
    for (int k = 0; k < R; k++) lp[k] = sgm::kBig;
    // pixel s of the line from its costs cc and the S it found there
    auto work = [&](int s, const Run<R>& cc, const Run<R>& sv) {
        int c[R], l[R];
        unpack<R>(cc, c);
        if (s == 0) {
#pragma unroll
            for (int k = 0; k < R; k++) l[k] = c[k];
        } else {
            int m = lp[0];
#pragma unroll
            for (int k = 1; k < R; k++) m = min(m, lp[k]);
            m = wave_min(m);
            // the neighbours across the lane's ends; lanes outside [0, nd) hold kBig, and so do the wave's ends
            const int below = dpp<kWaveShr1>(sgm::kBig, lp[R - 1]), above = dpp<kWaveShl1>(sgm::kBig, lp[0]);
#pragma unroll
            for (int k = 0; k < R; k++)
                l[k] = sgm::step(c[k], lp[k], k > 0 ? lp[k - 1] : below, k < R - 1 ? lp[k + 1] : above, m, a.p1, a.p2);
        }
        Run<R> o = pack<R>(l);
        if (!FIRST) {
#pragma unroll
            for (int k = 0; k < R / 2; k++) o.w[k] += sv.w[k];  // both halves stay below 2^16: no carry between them
        }
        Run<R>* dst = reinterpret_cast<Run<R>*>(sp + (int64_t)s * delta);
        if (active) *dst = o;
#pragma unroll
        for (int k = 0; k < R; k++) lp[k] = active ? l[k] : sgm::kBig;
    };
    // whole groups of kPathDepth pixels: no branch around a load, so that the loads in flight can be counted
    const int whole = ln.len & ~(kPathDepth - 1);
    for (int s0 = 0; s0 < whole; s0 += kPathDepth) {
#pragma unroll
        for (int j = 0; j < kPathDepth; j++) {
            work(s0 + j, cb[j], sb[j]);
            // the slot is free: pixel s + kPathDepth into it (this wave alone touches the line's S in this launch, and reads a pixel's
            // S before it writes it)
            const int64_t ahead = (int64_t)min(s0 + j + kPathDepth, ln.len - 1) * delta;
            cb[j] = *reinterpret_cast<const Run<R>*>(cp + ahead);
            if (!FIRST) sb[j] = *reinterpret_cast<const Run<R>*>(sp + ahead);
        }
    }
#pragma unroll
    for (int j = 0; j < kPathDepth; j++)  // the rest of the line: its pixels are in their slots
        if (whole + j < ln.len) work(whole + j, cb[j], sb[j]);
}

struct DecideArgs {
    const uint16_t* S;
    const int32_t* tex;
    int16_t* disp;
    int32_t* cost;
    int64_t n_px;  // ny * wx
    int W, H, wx, nd, md, w2, lofs, tex_thresh, uniq, filtered;
};

// the value of disparity index kq (wave-uniform) from the lane that holds it
template <int R>
__device__ __forceinline__ int value_at(const int (&v)[R], int kq)
{
    const int slot = kq % R;
    int t = v[0];
#pragma unroll
    for (int j = 1; j < R; j++)
        if (slot == j) t = v[j];
    return __shfl(t, kq / R);
}

template <int R>
__global__ void __launch_bounds__(kDecBlock)
sgm_decide_kernel(DecideArgs a)
{
    const int lane = threadIdx.x & 63, pair = blockIdx.y;
    const bool active = lane * R < a.nd;
    const int64_t q0 = ((int64_t)blockIdx.x * kDecWaves + (threadIdx.x >> 6)) * kDecPix;
    Run<R> sv[kDecPix];  // every pixel's values are requested before the first is worked
#pragma unroll
    for (int t = 0; t < kDecPix; t++) {
        sv[t] = {};
        if (active && q0 + t < a.n_px) sv[t] = *reinterpret_cast<const Run<R>*>(a.S + ((int64_t)pair * a.n_px + q0 + t) * a.nd + lane * R);
    }
#pragma unroll
    for (int t = 0; t < kDecPix; t++) {
        const int64_t q = q0 + t;
        if (q >= a.n_px) break;  // wave-uniform
        const int64_t px = (int64_t)pair * a.n_px + q;
        int s[R];
        unpack<R>(sv[t], s);
        // the winner: the lowest (S, k); S < 2^16 and k < 512, so (S << 9 | k) orders both in 25 bits
        int key = INT_MAX;
        if (active) {
#pragma unroll
            for (int j = 0; j < R; j++) key = min(key, (s[j] << 9) | (lane * R + j));
        }
        key = wave_min(key);
        const int mind = key & 511, mins = key >> 9;
        bool ok = a.tex[px] >= a.tex_thresh;
        if (ok && a.uniq > 0) {
            const int thresh = mins + mins * a.uniq / 100;
            bool other = false;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int k = lane * R + j;
                other |= active && (k < mind - 1 || k > mind + 1) && s[j] <= thresh;
            }
            ok = __ballot(other) == 0ull;
        }
        int d = a.filtered, cst = -1;
        if (ok) {  // wave-uniform
            const int p = value_at<R>(s, mind + 1 < a.nd ? mind + 1 : a.nd - 2);
            const int n = value_at<R>(s, mind >= 1 ? mind - 1 : 1);
            d = sbm::subpixel(a.nd, a.md, mind, p, n, mins);
            cst = mins;
        }
        if (lane == 0) {
            const int y = (int)(q / a.wx), x = (int)(q - (int64_t)y * a.wx);
            const int64_t o = ((int64_t)pair * a.H + a.w2 + y) * a.W + a.lofs + x;
            a.disp[o] = (int16_t)d;
            a.cost[o] = cst;
        }
    }
}

template <int KPL>
hipError_t launch_cost(const CostArgs& a, int n, hipStream_t stream)
{
    const dim3 grid((uint32_t)((a.wx + kTileX - 1) / kTileX), (uint32_t)((a.H - 2 * a.w2 + kBandY - 1) / kBandY), (uint32_t)n);
    const size_t lds = (size_t)(kBandY + 2 * a.w2) * (size_t)(2 * kTileX + 4 * a.w2 + a.nd - 1);  // < 64 KiB at w2 = 25, nd = 512
    hipLaunchKernelGGL(sgm_cost_kernel<KPL>, grid, dim3(kCostBlock), lds, stream, a);
    return hipGetLastError();
}

template <int R>
hipError_t launch_paths_and_decision(const gms_stereo_sgm_params& p, const sbm::Geometry& g, const StereoSgmLayout& L, int n, int W, int H,
                                     void* d_ws, int16_t* d_disp, hipStream_t stream)
{
    const int ny = H - 2 * g.w2, nd = p.bm.num_disparities;
    uint16_t* S = ws_ptr<uint16_t>(d_ws, L.S);
    for (int r = 0; r < p.n_paths; r++) {
        const int dy = sgm::path_dy(r), dx = sgm::path_dx(r), n_lines = sgm::line_count(dy, dx, ny, g.wx);
        const PathArgs a{ws_ptr<uint16_t>(d_ws, L.C), S, ny, g.wx, nd, dy, dx, p.p1, p.p2, n_lines};
        const dim3 grid((uint32_t)((n_lines + kPathWaves - 1) / kPathWaves), (uint32_t)n);
        if (r == 0)  // the first direction writes S, the others add to it
            hipLaunchKernelGGL((sgm_path_kernel<R, true>), grid, dim3(kPathBlock), 0, stream, a);
        else
            hipLaunchKernelGGL((sgm_path_kernel<R, false>), grid, dim3(kPathBlock), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int64_t n_px = (int64_t)ny * g.wx, per_block = (int64_t)kDecWaves * kDecPix;
    const int64_t blocks = (n_px + per_block - 1) / per_block;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    const DecideArgs a{S, ws_ptr<int32_t>(d_ws, L.tex), d_disp, ws_ptr<int32_t>(d_ws, L.bm.cost), n_px, W, H, g.wx, nd,
                       p.bm.min_disparity, g.w2, g.lofs, p.bm.texture_threshold, p.bm.uniqueness_ratio, g.filtered};
    hipLaunchKernelGGL(sgm_decide_kernel<R>, dim3((uint32_t)blocks, (uint32_t)n), dim3(kDecBlock), 0, stream, a);
    return hipGetLastError();
}

StereoSgmLayout layout_of(const gms_stereo_sgm_params& p, int n, int W, int H)
{
    const sbm::Geometry g = sbm::geometry(p.bm, W);
    return stereo_sgm_layout(n, W, H, g.none ? 0 : H - 2 * g.w2, g.none ? 0 : g.wx, p.bm.num_disparities);
}

}  // namespace

size_t stereo_sgm_ws_bytes(const gms_stereo_sgm_params& p, int n, int W, int H) { return layout_of(p, n, W, H).total; }

hipError_t launch_stereo_sgm(const gms_stereo_sgm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H, int pitch,
                             void* d_ws, int16_t* d_disp, int32_t* d_cost, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const sbm::Geometry g = sbm::geometry(p.bm, W);
    const StereoSgmLayout L = layout_of(p, n, W, H);
    if (!g.none) {
        uint8_t* pre = ws_ptr<uint8_t>(d_ws, L.bm.pre);
        hipError_t e = launch_stereo_bm_prefilter(p.bm, d_left, d_right, n, W, H, pitch, pre, stream);
        if (e != hipSuccess) return e;
        const int nd = p.bm.num_disparities;
        const CostArgs a{pre, ws_ptr<uint16_t>(d_ws, L.C), ws_ptr<int32_t>(d_ws, L.tex), W, H, nd, g.w2, p.bm.pre_filter_cap, g.lofs, g.rofs,
                         g.wx};
        e = nd <= 64 ? launch_cost<1>(a, n, stream) : nd <= 128 ? launch_cost<2>(a, n, stream)
            : nd <= 256 ? launch_cost<4>(a, n, stream) : launch_cost<8>(a, n, stream);
        if (e != hipSuccess) return e;
        // a lane's run: the shortest that covers nd with 64 lanes (nd is a multiple of 16, so of every run length)
        e = nd <= 128 ? launch_paths_and_decision<2>(p, g, L, n, W, H, d_ws, d_disp, stream)
            : nd <= 256 ? launch_paths_and_decision<4>(p, g, L, n, W, H, d_ws, d_disp, stream)
                        : launch_paths_and_decision<8>(p, g, L, n, W, H, d_ws, d_disp, stream);
        if (e != hipSuccess) return e;
    }
    return launch_stereo_bm_validate(p.bm, n, W, H, d_disp, ws_ptr<int32_t>(d_ws, L.bm.cost), d_cost, stream);
}

}  // namespace gms
