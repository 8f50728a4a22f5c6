// speckle_kernels.hip -- filterSpeckles on int16 disparity maps (the definition, the link predicate and the tile
// constants are in speckle_core.h; tests/speckle_ref.py states the filter twice in numpy): connected components under a difference
// predicate, for a batch of n equally sized maps, in place.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback (graph-capturable):
//   spk_tile_kernel     one workgroup per 64 x 32 tile of one map: values and labels in LDS, a union-find over the links inside the
//                       tile with LDS atomics only; then label = the global index of the pixel's tile-local root (-1: new_val) and,
//                       at the tile-local roots, the tile-local component's size. Also zeroes the map's `removed`.
//   spk_seam_kernel     only the pixels on a tile's left column or top row: a global atomicMin union with the pixel across the seam.
//   spk_flatten_kernel  every pixel finds its global root; a tile-local root that is not the global root adds its tile-local size
//                       to the root's: one integer atomic per (tile, component), so the sums are the same on every run.
//   spk_apply_kernel    new_val where the root's size is at most max_speckle_size; `removed` by a block reduction and one integer
//                       atomic per block.
// Labels are pixel indices within the map (y * W + x < 2^26). A label only ever points at a lower index or at itself, in LDS and in
// global memory: every find walks a strictly decreasing chain and ends at a root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "speckle_core.h"
#include "ws_layout.h"

namespace gms {
namespace {

using spk::kBlock;
using spk::kTileH;
using spk::kTilePx;
using spk::kTileW;

// Ends: a non-root's label is below its index, so `a` strictly decreases until L[a] == a. Labels change only by atomicMin to a lower
// value, so a chain read while others union is still decreasing.
__device__ __forceinline__ int spk_find(const int32_t* L, int a)
{
    int p = L[a];
    while (p != a) {
        a = p;
        p = L[a];
    }
    return a;
}

// Ends: each round either returns, or its atomicMin found that `a` had stopped being a root (old < a), which means another lane's
// atomicMin on the same word succeeded since the find; the round then continues from old < a, so (a, b) decreases and is bounded
// below by 0. Roots only ever decrease: a root is its component's lowest index so far. The same routine serves LDS and global labels.
__device__ __forceinline__ void spk_union(int32_t* L, int a, int b)
{
    for (;;) {
        a = spk_find(L, a);
        b = spk_find(L, b);
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
spk_tile_kernel(const int16_t* __restrict__ disp, int W, int H, int new_val, int max_diff, int32_t* __restrict__ label,
                int32_t* __restrict__ size, int32_t* __restrict__ removed)
{
    __shared__ int16_t s_v[kTilePx];    // pixels outside the map hold new_val: never linked
    __shared__ int32_t s_lab[kTilePx];  // tile-local union-find over tile-local indices ty * kTileW + tx
    __shared__ int32_t s_cnt[kTilePx];
    const int tid = threadIdx.x, img = blockIdx.z;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int64_t base = (int64_t)img * W * H;
    const int16_t* __restrict__ src = disp + base;
    if (removed && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) removed[img] = 0;
    for (int i = tid; i < kTilePx; i += kBlock) {
        const int y = y0 + i / kTileW, x = x0 + (i & (kTileW - 1));
        s_v[i] = (y < H && x < W) ? src[(int64_t)y * W + x] : (int16_t)new_val;
        s_lab[i] = i;
        s_cnt[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < kTilePx; i += kBlock) {
        const int v = s_v[i];
        if (v == new_val) continue;
        if ((i & (kTileW - 1)) && spk::linked(v, s_v[i - 1], new_val, max_diff)) spk_union(s_lab, i, i - 1);
        if (i >= kTileW && spk::linked(v, s_v[i - kTileW], new_val, max_diff)) spk_union(s_lab, i, i - kTileW);
    }
    __syncthreads();  // no union after this: the roots are final
    int root[kTilePx / kBlock];
#pragma unroll
    for (int k = 0; k < kTilePx / kBlock; k++) {
        const int i = tid + k * kBlock;
        root[k] = -1;
        if (s_v[i] != new_val) {
            root[k] = spk_find(s_lab, i);
            atomicAdd(&s_cnt[root[k]], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTilePx / kBlock; k++) {
        const int i = tid + k * kBlock;
        const int y = y0 + i / kTileW, x = x0 + (i & (kTileW - 1));
        if (y >= H || x >= W) continue;
        const int r = root[k];
        const int64_t o = base + (int64_t)y * W + x;
        label[o] = r < 0 ? -1 : (y0 + r / kTileW) * W + x0 + (r & (kTileW - 1));  // the root is a pixel of the map: it is not new_val
        size[o] = r == i ? s_cnt[i] : 0;
    }
}

// Thread t < n_vert: pixel (x, y) on the t / H-th vertical seam with its left neighbour; the others: a pixel on a horizontal seam
// with the pixel above. Both pixels' labels lead to their tile-local roots, whose labels are themselves.
__global__ void __launch_bounds__(kBlock)
spk_seam_kernel(const int16_t* __restrict__ disp, int W, int H, int new_val, int max_diff, int n_vert, int n_all, int32_t* __restrict__ label)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_all) return;
    const int64_t base = (int64_t)blockIdx.y * W * H;
    int p, q;
    if (t < n_vert) {
        const int s = t / H, y = t - s * H;
        p = y * W + (s + 1) * kTileW;
        q = p - 1;
    } else {
        const int u = t - n_vert, s = u / W, x = u - s * W;
        p = (s + 1) * kTileH * W + x;
        q = p - W;
    }
    if (spk::linked(disp[base + p], disp[base + q], new_val, max_diff)) spk_union(label + base, p, q);
}

__global__ void __launch_bounds__(kBlock)
spk_flatten_kernel(int W, int H, int32_t* __restrict__ label, int32_t* __restrict__ size)
{
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= px) return;
    const int64_t base = (int64_t)blockIdx.y * px;
    int32_t* L = label + base;
    if (L[p] < 0) return;
    const int root = spk_find(L, p);
    L[p] = root;  // a shorter path to the same root: finds that run beside this one stay right
    // size[p] != 0: p was a tile-local root. Nobody adds to it unless it is a global root, and then it is not read here.
    if (root != p) {
        const int own = size[base + p];
        if (own) atomicAdd(&size[base + root], own);
    }
}

__global__ void __launch_bounds__(kBlock)
spk_apply_kernel(int16_t* __restrict__ disp, int W, int H, int new_val, int max_speckle_size, const int32_t* __restrict__ label,
                 const int32_t* __restrict__ size, int32_t* __restrict__ removed)
{
    __shared__ int s_part[kBlock / 64];
    const int px = W * H;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * px;
    int hit = 0;
    if (p < px) {
        const int root = label[base + p];
        if (root >= 0 && size[base + root] <= max_speckle_size) {
            disp[base + p] = (int16_t)new_val;
            hit = 1;
        }
    }
    if (!removed) return;
    for (int s = 32; s > 0; s >>= 1) hit += __shfl_down(hit, s);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = hit;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < kBlock / 64; w++) sum += s_part[w];
        if (sum) atomicAdd(&removed[blockIdx.y], sum);
    }
}

}  // namespace

size_t speckle_ws_bytes(int n, int W, int H) { return speckle_layout(n, W, H).total; }

hipError_t launch_filter_speckles(int16_t* d_disp16, int n, int W, int H, int new_val, int max_speckle_size, int max_diff, void* d_ws,
                                  int32_t* d_removed, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (max_speckle_size == 0)  // nothing can be removed: the maps stay as they are
        return d_removed ? hipMemsetAsync(d_removed, 0, sizeof(int32_t) * (size_t)n, stream) : hipSuccess;
    const SpeckleLayout L = speckle_layout(n, W, H);
    int32_t *label = ws_ptr<int32_t>(d_ws, L.label), *size = ws_ptr<int32_t>(d_ws, L.size);
    const int tx = (W + kTileW - 1) / kTileW, ty = (H + kTileH - 1) / kTileH;
    const int px = W * H;
    const dim3 flat((uint32_t)((px + kBlock - 1) / kBlock), (uint32_t)n);
    hipLaunchKernelGGL(spk_tile_kernel, dim3((uint32_t)tx, (uint32_t)ty, (uint32_t)n), dim3(kBlock), 0, stream, d_disp16, W, H, new_val, max_diff,
                       label, size, d_removed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_vert = (tx - 1) * H, n_all = n_vert + (ty - 1) * W;  // at most 127 * 8192 + 255 * 8192 < 2^22
    if (n_all > 0) {
        hipLaunchKernelGGL(spk_seam_kernel, dim3((uint32_t)((n_all + kBlock - 1) / kBlock), (uint32_t)n), dim3(kBlock), 0, stream, d_disp16, W, H,
                           new_val, max_diff, n_vert, n_all, label);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(spk_flatten_kernel, flat, dim3(kBlock), 0, stream, W, H, label, size);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(spk_apply_kernel, flat, dim3(kBlock), 0, stream, d_disp16, W, H, new_val, max_speckle_size, label, size, d_removed);
    return hipGetLastError();
}

}  // namespace gms
