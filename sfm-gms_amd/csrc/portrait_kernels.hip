// portrait_kernels.hip -- portrait mode, the image tail of the reference's createPortraitMode (DisparityUtil.cpp:317-412; DESIGN.md
// §4.9) for a batch of n equally sized images: disparity map -> foreground mask -> the largest borders, filled -> the photograph with
// everything else median-blurred. tests/portrait_ref.py states every step; each array here equals it byte for byte.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback (graph-capturable):
//   pm_mask_kernel      255 -> 0, threshold, and the (2 it + 1)^2 maximum inside the image: a 64 x 16 tile plus an it-pixel halo in LDS.
//   pm_init_kernel      per pixel: its neighbour code (which of the 8 neighbours are set), label = own index, and the planes zeroed.
//   pm_merge_kernel     union-find over the whole image (atomicMin on the roots): set pixels 8-connected, zero pixels 4-connected.
//   pm_flatten_kernel   label = root = the component's first pixel in raster order; zero components that touch the image edge are
//                       flagged (the virtual frame). Every set root is an outer border, every unflagged zero root a hole border.
//   pm_area_kernel      the thread of a root pixel walks its border (pm::walk_border, the literal Suzuki-Abe walk on the neighbour
//                       codes: one byte load per step) and appends the border's rank key (area, start pixel, kind) to the image's list.
//   pm_select_kernel    one workgroup per image: num_contours rounds of a 64-bit maximum over that list.
//   pm_trace_kernel     one lane per chosen border walks it again: the chain's pixels are marked, and every step between two rows
//                       toggles bit k of the upper row's pixel (even-odd crossings).
//   pm_fill_kernel      one wave per row: the exclusive prefix XOR of the toggles = inside, per chosen border; `selected`.
//   pm_median_kernel<C> median + composite, the hot kernel: a 64 x 16 tile plus the window's halo in LDS, one plane per channel; a
//                       thread finds each median by 8 steps of a binary search on the value (count the samples below the candidate).
//                       Selected pixels take the photograph's bytes and skip the search unless the blurred image is asked for.
// The two walks are one lane per border and one dependent byte load per step: their time grows with the longest chain, which for a
// ragged mask that is one component can be of the order of the pixel count (DESIGN.md §4.9 has measured figures).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "portrait_core.h"

namespace gms {
namespace {

constexpr int kTX = 64, kTY = 16, kBlock = 256;
constexpr int kSelBlock = 1024;

// the workspace's typed pointers (its regions: PortraitLayout in ws_layout.h)
struct PmWs {
    uint8_t *mask, *nb, *flag, *sel;
    int32_t* label;
    unsigned long long *tog, *keys;
    int32_t* chosen;
};

__global__ void __launch_bounds__(kBlock)
pm_mask_kernel(const uint8_t* __restrict__ disp, int64_t img_stride, int pitch, int W, int H, int threshold, int it,
               uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_out)
{
    __shared__ uint8_t t[kTY + 16][kTX + 16];  // image rows y0 - it .. y0 + kTY + it - 1, columns x0 - it ..; 1 = above the threshold
    const int img = blockIdx.z, tid = threadIdx.x;
    const uint8_t* __restrict__ src = disp + (int64_t)img * img_stride;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const int rows = kTY + 2 * it, cols = kTX + 2 * it;
    for (int i = tid; i < rows * cols; i += kBlock) {
        const int r = i / cols, c = i - r * cols;
        const int y = y0 - it + r, x = x0 - it + c;
        int v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int d = src[(int64_t)y * pitch + x];
            v = d != 255 && d > threshold;
        }
        t[r][c] = (uint8_t)v;
    }
    __syncthreads();
    for (int i = tid; i < kTY * kTX; i += kBlock) {
        const int ty = i / kTX, tx = i - ty * kTX;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        int v = 0;
        for (int r = 0; r <= 2 * it && !v; r++)
            for (int c = 0; c <= 2 * it; c++) v |= t[ty + r][tx + c];
        const int64_t o = ((int64_t)img * H + y) * W + x;
        mask[o] = v ? 255 : 0;
        if (mask_out) mask_out[o] = v ? 255 : 0;
    }
}

__global__ void __launch_bounds__(kBlock)
pm_init_kernel(const uint8_t* __restrict__ mask, int W, int H, uint8_t* __restrict__ nb, uint8_t* __restrict__ flag,
               uint8_t* __restrict__ sel, int32_t* __restrict__ label, unsigned long long* __restrict__ tog, int32_t* __restrict__ chosen)
{
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= px) return;
    if (p == 0) chosen[(int64_t)blockIdx.y * kChosenStride + 1 + pm::kMaxContours] = 0;  // the image's border count
    const int64_t base = (int64_t)blockIdx.y * px;
    const uint8_t* __restrict__ m = mask + base;
    const int y = p / W, x = p - y * W;
    unsigned code = 0;
    if (m[p]) {
        for (int s = 0; s < 8; s++) {
            const int xn = x + pm::dx(s), yn = y + pm::dy(s);
            if (xn >= 0 && xn < W && yn >= 0 && yn < H && m[yn * W + xn]) code |= 1u << s;
        }
    }
    nb[base + p] = (uint8_t)code;
    flag[base + p] = 0;
    sel[base + p] = 0;
    label[base + p] = p;
    tog[base + p] = 0ull;
}

__device__ __forceinline__ int uf_find(const int32_t* L, int a)
{
    int p = L[a];
    while (p != a) {
        a = p;
        p = L[a];
    }
    return a;
}

// the roots only ever decrease: a root is its component's lowest pixel index so far
__device__ __forceinline__ void uf_union(int32_t* L, int a, int b)
{
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);  // a > b: hang root a under b, unless a stopped being a root meanwhile
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kBlock)
pm_merge_kernel(const uint8_t* __restrict__ mask, int W, int H, int32_t* __restrict__ label)
{
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= px) return;
    const uint8_t* __restrict__ m = mask + (int64_t)blockIdx.y * px;
    int32_t* L = label + (int64_t)blockIdx.y * px;
    const int y = p / W, x = p - y * W;
    const uint8_t v = m[p];
    if (x > 0 && m[p - 1] == v) uf_union(L, p, p - 1);
    if (y > 0 && m[p - W] == v) uf_union(L, p, p - W);
    if (v && y > 0) {  // set pixels are 8-connected
        if (x > 0 && m[p - W - 1]) uf_union(L, p, p - W - 1);
        if (x + 1 < W && m[p - W + 1]) uf_union(L, p, p - W + 1);
    }
}

__global__ void __launch_bounds__(kBlock)
pm_flatten_kernel(const uint8_t* __restrict__ mask, int W, int H, int32_t* __restrict__ label, uint8_t* __restrict__ flag)
{
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= px) return;
    const int64_t base = (int64_t)blockIdx.y * px;
    int32_t* L = label + base;
    const int root = uf_find(L, p);
    L[p] = root;  // a shorter path to the same root: finds that run beside this one stay right
    const int y = p / W, x = p - y * W;
    if (!mask[base + p] && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) flag[base + root] = 1;
}

// rank key of the border rooted at pixel p: doubled area, then the earlier start pixel, then outer before hole; larger = better
__device__ __forceinline__ unsigned long long pm_key(int a2, int p, bool hole)
{
    const unsigned code = (unsigned)(p - (hole ? 1 : 0)) * 2u + (hole ? 1u : 0u);
    return ((unsigned long long)(unsigned)a2 << 32) | (unsigned long long)(0xFFFFFFFFu - code);
}

__global__ void __launch_bounds__(kBlock)
pm_area_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ nb, const uint8_t* __restrict__ flag,
               const int32_t* __restrict__ label, int W, int H, int cap, unsigned long long* __restrict__ keys,
               int32_t* __restrict__ chosen)
{
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= px) return;
    const int64_t base = (int64_t)blockIdx.y * px;
    if (label[base + p] != p) return;
    const bool hole = mask[base + p] == 0;
    if (hole && flag[base + p]) return;
    const int s = p - (hole ? 1 : 0);  // a hole border starts at the set pixel left of the hole's first pixel
    const int y0 = s / W, x0 = s - y0 * W;
    const long long a2 = pm::walk_border(nb + base, W, x0, y0, hole, [](int, int, int, int) {});
    const int i = atomicAdd(&chosen[(int64_t)blockIdx.y * kChosenStride + 1 + pm::kMaxContours], 1);
    if (i < cap)  // always (pm_key_cap); the doubled area is at most 2 (W - 1)(H - 1) < 2^31
        keys[(int64_t)blockIdx.y * cap + i] = pm_key((int)(a2 < 0 ? -a2 : a2), p, hole);
}

__global__ void __launch_bounds__(kSelBlock)
pm_select_kernel(const unsigned long long* __restrict__ keys, int cap, int num, int32_t* __restrict__ chosen)
{
    __shared__ unsigned long long s_best[kSelBlock / 64];
    __shared__ unsigned long long s_bound;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long* __restrict__ a = keys + (int64_t)blockIdx.x * cap;
    int32_t* out = chosen + (int64_t)blockIdx.x * kChosenStride;
    const int nb = min(out[1 + pm::kMaxContours], cap);
    unsigned long long bound = ~0ull;  // above every key: areas stay below 2^31
    int count = 0;
    for (int k = 0; k < num; k++) {
        unsigned long long best = 0ull;  // below every key: the low word of a key is never 0
        for (int i = tid; i < nb; i += kSelBlock) {
            const unsigned long long key = a[i];
            if (key < bound && key > best) best = key;
        }
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o = __shfl_xor(best, s);
            best = o > best ? o : best;
        }
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long b = s_best[0];
            for (int w = 1; w < kSelBlock / 64; w++) b = s_best[w] > b ? s_best[w] : b;
            s_bound = b;
        }
        __syncthreads();
        bound = s_bound;
        if (bound == 0ull) break;  // workgroup-uniform: no border left
        if (tid == 0) {
            const unsigned code = 0xFFFFFFFFu - (unsigned)bound;
            out[1 + k] = (int32_t)((code >> 1) + (code & 1u));  // the root pixel
        }
        count = k + 1;
        __syncthreads();
    }
    if (tid == 0) out[0] = count;
}

__global__ void __launch_bounds__(64)
pm_trace_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ nb, const int32_t* __restrict__ chosen, int W, int H,
                uint8_t* __restrict__ sel, unsigned long long* __restrict__ tog)
{
    const int k = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * W * H;
    const int32_t* __restrict__ c = chosen + (int64_t)blockIdx.x * kChosenStride;
    if (k >= c[0]) return;
    const int p = c[1 + k];
    const bool hole = mask[base + p] == 0;
    const int s = p - (hole ? 1 : 0);
    const int y0 = s / W, x0 = s - y0 * W;
    uint8_t* __restrict__ on = sel + base;
    unsigned long long* __restrict__ t = tog + base;
    const unsigned long long bit = 1ull << k;
    pm::walk_border(nb + base, W, x0, y0, hole, [=](int x, int y, int xn, int yn) {
        on[y * W + x] = 1;  // several borders may share a pixel: they all store 1
        if (y != yn) atomicXor(&t[(y < yn ? y : yn) * W + (y < yn ? x : xn)], bit);
    });
}

__global__ void __launch_bounds__(kBlock)
pm_fill_kernel(const unsigned long long* __restrict__ tog, int W, int H, uint8_t* __restrict__ sel, uint8_t* __restrict__ sel_out)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (y >= H) return;  // wave-uniform
    const int64_t row = ((int64_t)blockIdx.y * H + y) * W;
    unsigned long long carry = 0ull;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const unsigned long long own = x < W ? tog[row + x] : 0ull;
        unsigned long long inc = own;
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long o = __shfl_up(inc, s);
            if (lane >= s) inc ^= o;
        }
        const unsigned long long left = carry ^ inc ^ own;  // the crossings at columns below x, one bit per chosen border
        if (x < W) {
            const uint8_t v = (left != 0ull || sel[row + x]) ? 255 : 0;
            sel[row + x] = v;
            if (sel_out) sel_out[row + x] = v;
        }
        carry ^= __shfl(inc, 63);
    }
}

struct MedianArgs {
    const uint8_t* src;
    const uint8_t* sel;   // NULL: no composite (every pixel is the median)
    uint8_t* out;         // the composite (or the plain median), pitch out_pitch
    uint8_t* blurred;     // optional: the plain median beside the composite, dense rows
    int64_t src_stride, out_stride;
    int W, H, pitch, out_pitch, k;
};

template <int C>
__global__ void __launch_bounds__(kBlock)
pm_median_kernel(MedianArgs a)
{
    extern __shared__ uint8_t smem[];  // [C][kTY + k - 1][stride]: image rows y0 - r .., columns x0 - r .., the border replicated
    const int tid = threadIdx.x, img = blockIdx.z;
    const int k = a.k, r = k >> 1;
    const int rows = kTY + k - 1, cols = kTX + k - 1, stride = (cols + 3) & ~3, plane = rows * stride;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const uint8_t* __restrict__ src = a.src + (int64_t)img * a.src_stride;
    for (int i = tid; i < rows * cols; i += kBlock) {
        const int ry = i / cols, cx = i - ry * cols;
        const int y = min(max(y0 - r + ry, 0), a.H - 1), x = min(max(x0 - r + cx, 0), a.W - 1);
        const uint8_t* __restrict__ s = src + (int64_t)y * a.pitch + x * C;
#pragma unroll
        for (int c = 0; c < C; c++) smem[c * plane + ry * stride + cx] = s[c];
    }
    __syncthreads();
    const int tx = tid & 63, x = x0 + tx;
    if (x >= a.W) return;
    const int rank = (k * k) >> 1;
    for (int ty = tid >> 6; ty < kTY; ty += kBlock / 64) {
        const int y = y0 + ty;
        if (y >= a.H) break;
        const bool keep = a.sel && y < a.H - 3 && x < a.W - 3 && a.sel[((int64_t)img * a.H + y) * a.W + x];
        uint8_t* __restrict__ o = a.out + (int64_t)img * a.out_stride + (int64_t)y * a.out_pitch + x * C;
        uint8_t* __restrict__ b = a.blurred ? a.blurred + (((int64_t)img * a.H + y) * a.W + x) * C : nullptr;
        if (keep && !b) {
#pragma unroll
            for (int c = 0; c < C; c++) o[c] = smem[c * plane + (ty + r) * stride + tx + r];
            continue;
        }
#pragma unroll
        for (int c = 0; c < C; c++) {
            const uint8_t* __restrict__ w = smem + c * plane + ty * stride + tx;
            int med = 0;  // the largest value v with (samples below v) <= rank, bit by bit: the rank-th smallest sample
            for (int bit = 128; bit > 0; bit >>= 1) {
                const int cand = med | bit;
                int below = 0;
                for (int wy = 0; wy < k; wy++) {
                    const uint8_t* __restrict__ wr = w + wy * stride;
                    for (int wx = 0; wx < k; wx++) below += (int)wr[wx] < cand;
                }
                if (below <= rank) med = cand;
            }
            if (b) b[c] = (uint8_t)med;
            o[c] = keep ? smem[c * plane + (ty + r) * stride + tx + r] : (uint8_t)med;
        }
    }
}

hipError_t launch_median(const MedianArgs& a, int n, int channels, hipStream_t stream)
{
    const dim3 grid((uint32_t)((a.W + kTX - 1) / kTX), (uint32_t)((a.H + kTY - 1) / kTY), (uint32_t)n);
    const size_t lds = (size_t)channels * (size_t)(kTY + a.k - 1) * (size_t)((kTX + a.k - 1 + 3) & ~3);  // < 14 KiB at k = 31, C = 3
    if (channels == 3)
        hipLaunchKernelGGL(pm_median_kernel<3>, grid, dim3(kBlock), lds, stream, a);
    else
        hipLaunchKernelGGL(pm_median_kernel<1>, grid, dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

size_t portrait_ws_bytes(int n, int W, int H) { return portrait_layout(n, W, H).total; }

hipError_t launch_median_blur(const uint8_t* d_src, int n, int W, int H, int channels, int pitch, int ksize, uint8_t* d_dst,
                              hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const MedianArgs a{d_src, nullptr, d_dst, nullptr, (int64_t)pitch * H, (int64_t)pitch * H, W, H, pitch, pitch, ksize};
    return launch_median(a, n, channels, stream);
}

hipError_t launch_portrait(const gms_portrait_params& p, const uint8_t* d_bgr, const uint8_t* d_disp, int n, int W, int H, int pitch_bgr,
                           int pitch_disp, void* d_ws, uint8_t* d_out, uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred,
                           hipStream_t stream, hipEvent_t* ev)
{
    if (n <= 0) return hipSuccess;
    const PortraitLayout L = portrait_layout(n, W, H);
    const PmWs ws = {ws_ptr<uint8_t>(d_ws, L.mask), ws_ptr<uint8_t>(d_ws, L.nb), ws_ptr<uint8_t>(d_ws, L.flag), ws_ptr<uint8_t>(d_ws, L.sel),
                     ws_ptr<int32_t>(d_ws, L.label), ws_ptr<unsigned long long>(d_ws, L.tog), ws_ptr<unsigned long long>(d_ws, L.keys),
                     ws_ptr<int32_t>(d_ws, L.chosen)};
    const int cap = (int)pm_key_cap(W, H);
    int stage = 0;
    // ev (diagnostic, NULL in production): GMS_PORTRAIT_STAGES + 1 events, one before the first launch and one after each
    auto mark = [&]() { return ev ? hipEventRecord(ev[stage++], stream) : hipSuccess; };
    const int px = W * H;
    const dim3 tiles((uint32_t)((W + kTX - 1) / kTX), (uint32_t)((H + kTY - 1) / kTY), (uint32_t)n);
    const dim3 flat((uint32_t)((px + kBlock - 1) / kBlock), (uint32_t)n);
    hipError_t e = mark();
    if (e != hipSuccess) return e;
#define PM_STAGE(...)                            \
    do {                                         \
        hipLaunchKernelGGL(__VA_ARGS__);         \
        e = hipGetLastError();                   \
        if (e == hipSuccess) e = mark();         \
        if (e != hipSuccess) return e;           \
    } while (0)
    PM_STAGE(pm_mask_kernel, tiles, dim3(kBlock), 0, stream, d_disp, (int64_t)pitch_disp * H, pitch_disp, W, H, p.threshold,
             p.dilate_iterations, ws.mask, d_mask);
    PM_STAGE(pm_init_kernel, flat, dim3(kBlock), 0, stream, ws.mask, W, H, ws.nb, ws.flag, ws.sel, ws.label, ws.tog, ws.chosen);
    PM_STAGE(pm_merge_kernel, flat, dim3(kBlock), 0, stream, ws.mask, W, H, ws.label);
    PM_STAGE(pm_flatten_kernel, flat, dim3(kBlock), 0, stream, ws.mask, W, H, ws.label, ws.flag);
    PM_STAGE(pm_area_kernel, flat, dim3(kBlock), 0, stream, ws.mask, ws.nb, ws.flag, ws.label, W, H, cap, ws.keys, ws.chosen);
    PM_STAGE(pm_select_kernel, dim3((uint32_t)n), dim3(kSelBlock), 0, stream, ws.keys, cap, p.num_contours, ws.chosen);
    PM_STAGE(pm_trace_kernel, dim3((uint32_t)n), dim3(64), 0, stream, ws.mask, ws.nb, ws.chosen, W, H, ws.sel, ws.tog);
    PM_STAGE(pm_fill_kernel, dim3((uint32_t)((H + kBlock / 64 - 1) / (kBlock / 64)), (uint32_t)n), dim3(kBlock), 0, stream, ws.tog, W, H,
             ws.sel, d_selected);
#undef PM_STAGE
    const MedianArgs a{d_bgr, ws.sel, d_out, d_blurred, (int64_t)pitch_bgr * H, (int64_t)3 * px, W, H, pitch_bgr, 3 * W, p.median_ksize};
    e = launch_median(a, n, 3, stream);
    return e == hipSuccess ? mark() : e;
}

}  // namespace gms
