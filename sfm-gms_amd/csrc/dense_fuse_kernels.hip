// dense_fuse_kernels.hip -- the clouds of several posed pairs fused into one by depth consistency. The arithmetic is
// dense_fuse_core.h's; tests/dense_fuse_ref.py states it in numpy, and every output byte equals it.
//
// Stream-ordered launches, no allocation, no synchronisation, no readback (graph-capturable). The sources are a table of records in
// device memory whose pointers the kernels follow when they run (a captured graph follows new maps, poses and counts).
//   fuse_mark_kernel   the hot path. A workgroup of 256 lanes takes 1024 consecutive points of one source, 4 adjacent points per lane.
//                      Wave 0 stages the source's live neighbours in LDS, one lane per slot, packed in slot order by a ballot. Per
//                      neighbour a lane aims its 4 points (fp64), then issues the 4 + 4 gathers from the neighbour's valid plane and
//                      disparity map together (a point that is UNSEEN before any load aims at pixel 0, so the loads need no branch),
//                      then gives the verdicts. It writes two decision bytes per point and the block's kept count.
//   fuse_scan_kernel   one workgroup: the exclusive prefix of the kept counts over all blocks in source-major order, 256 blocks per
//                      pass with the carry into the next; then d_counts.
//   fuse_write_kernel  a block ranks its kept points by an LDS scan and copies the records of those below fused_cap.
// No atomic decides a position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_fuse_core.h"
#include "gms_kernels.h"
#include "ws_layout.h"

namespace gms {
namespace {

constexpr int kBlock = 256, kPerLane = fuse::kBlockPoints / kBlock;
static_assert(fuse::kBlockPoints == kFuseBlockPoints && kPerLane == 4, "the layout and the kernels cut the same blocks; a lane's marks are one 8-byte word");

struct FuseArgs {
    const gms_dense_fuse_src* src;
    const int32_t* neighbors;
    int32_t* blocks;  // workspace: [n_src][nbs]
    uint8_t* marks;   // workspace: [n_src][nbs * 1024][2]
    float* xyz;
    uint8_t* color;
    int32_t *source, *index;
    uint8_t *support, *conflict;
    int32_t* counts;
    int n_src, max_cap, nbs, n_nb, channels, tol16, min_support, fused_cap;
};

__device__ __forceinline__ int64_t first_mark(const FuseArgs& a, int src, int first) { return ((int64_t)src * a.nbs * fuse::kBlockPoints + first) * 2; }

__global__ void __launch_bounds__(kBlock)
fuse_mark_kernel(FuseArgs a)
{
    __shared__ fuse::View s_nb[fuse::kMaxNeighbors];
    __shared__ int s_kept[kBlock / 64], s_live;
    const int i = blockIdx.y, tid = threadIdx.x, first = (int)blockIdx.x * fuse::kBlockPoints + tid * kPerLane;
    const gms_dense_fuse_src& me = a.src[i];
    const int n = fuse::n_points(me, fuse::is_live(me, a.max_cap));
    uint2* __restrict__ mark = reinterpret_cast<uint2*>(a.marks + first_mark(a, i, first));
    if ((int)blockIdx.x * fuse::kBlockPoints >= n) {  // (uniform) nothing here: the write kernel still reads the marks
        *mark = make_uint2(0u, 0u);
        if (tid == 0) a.blocks[(int64_t)i * a.nbs + blockIdx.x] = 0;
        return;
    }
    if (tid < 64) {
        const int j = tid < a.n_nb ? a.neighbors[(int64_t)i * a.n_nb + tid] : -1;
        const bool ok = j >= 0 && j < a.n_src && j != i && fuse::is_live(a.src[j], a.max_cap);
        const uint64_t m = __ballot(ok);
        if (ok) fuse::make_view(a.src[j], j < i, s_nb[__popcll(m & ((1ull << tid) - 1ull))]);
        if (tid == 0) s_live = __popcll(m);
    }
    __syncthreads();
    const int n_live = s_live;
    double P[kPerLane][3];
    int support[kPerLane], conflict[kPerLane], dup[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const int k = min(first + j, n - 1);  // (points past the source's last are computed from its last and marked 0)
        const float* f = me.d_xyz + 3 * (int64_t)k;
        P[j][0] = (double)f[0];
        P[j][1] = (double)f[1];
        P[j][2] = (double)f[2];
        support[j] = 1, conflict[j] = 0, dup[j] = 0;
    }
    for (int q = 0; q < n_live; q++) {
        const fuse::View& s = s_nb[q];
        fuse::Aim aim[kPerLane];
        int ok[kPerLane], d16[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; j++) aim[j] = fuse::aim(s, P[j]);
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            ok[j] = s.valid[aim[j].at];
            d16[j] = s.disp[aim[j].at];
        }
#pragma unroll
        for (int j = 0; j < kPerLane; j++) fuse::tally(fuse::verdict(s, aim[j], ok[j], d16[j], a.tol16), s.lower, support[j], conflict[j], dup[j]);
    }
    uint32_t w[2] = {0u, 0u};
    int kept = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        if (first + j >= n) continue;
        const int sb = fuse::support_byte(support[j], dup[j], a.min_support);
        kept += (sb & fuse::kKept) != 0;
        w[j >> 1] |= ((uint32_t)sb | ((uint32_t)conflict[j] << 8)) << (16 * (j & 1));
    }
    *mark = make_uint2(w[0], w[1]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o, 64);
    if ((tid & 63) == 0) s_kept[tid >> 6] = kept;
    __syncthreads();
    if (tid == 0) a.blocks[(int64_t)i * a.nbs + blockIdx.x] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
}

// exclusive prefix sum of kBlock values, one per lane, through LDS; returns the lane's prefix, total: the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* s, int& total)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const int add = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const int incl = s[tid];
    total = s[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kBlock)
fuse_scan_kernel(FuseArgs a)
{
    __shared__ int s[kBlock];
    const int tid = threadIdx.x, n_blocks = a.n_src * a.nbs;
    int32_t* b = a.blocks;
    int carry = 0;
    for (int base = 0; base < n_blocks; base += kBlock) {
        const int i = base + tid;
        const int v = i < n_blocks ? b[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, s, total);
        if (i < n_blocks) b[i] = carry + ex;
        carry += total;
    }
    __syncthreads();  // the prefixes written above are read below by other lanes
    for (int src = tid; src < a.n_src; src += kBlock)
        a.counts[src] = (src + 1 < a.n_src ? b[(int64_t)(src + 1) * a.nbs] : carry) - b[(int64_t)src * a.nbs];
    if (tid == 0) a.counts[a.n_src] = carry;
}

__global__ void __launch_bounds__(kBlock)
fuse_write_kernel(FuseArgs a)
{
    __shared__ int s[kBlock];
    const int i = blockIdx.y, tid = threadIdx.x, first = (int)blockIdx.x * fuse::kBlockPoints + tid * kPerLane;
    const int start = a.blocks[(int64_t)i * a.nbs + blockIdx.x];
    if (start >= a.fused_cap) return;  // (uniform) every point of the block is beyond the cap
    const uint2 m = *reinterpret_cast<const uint2*>(a.marks + first_mark(a, i, first));
    const uint32_t w[2] = {m.x, m.y};
    int kept = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++) kept += (w[j >> 1] >> (16 * (j & 1)) & fuse::kKept) != 0;
    int total;
    int rank = start + block_exclusive_scan(kept, s, total);
    if (!kept) return;
    const gms_dense_fuse_src& me = a.src[i];
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const uint32_t mk = w[j >> 1] >> (16 * (j & 1));
        if (!(mk & fuse::kKept)) continue;
        if (rank < a.fused_cap) {
            const int64_t k = first + j;
            const float* f = me.d_xyz + 3 * k;
            a.xyz[3 * (int64_t)rank] = f[0];
            a.xyz[3 * (int64_t)rank + 1] = f[1];
            a.xyz[3 * (int64_t)rank + 2] = f[2];
            if (a.color)
                for (int c = 0; c < a.channels; c++) a.color[(int64_t)rank * a.channels + c] = me.d_color ? me.d_color[k * a.channels + c] : (uint8_t)0;
            a.source[rank] = i;
            a.index[rank] = (int32_t)k;
            a.support[rank] = (uint8_t)(mk & fuse::kSupportMask);
            a.conflict[rank] = (uint8_t)(mk >> 8 & 0xff);
        }
        rank++;
    }
}

}  // namespace

size_t dense_fuse_ws_bytes(int n_src, int max_cap) { return dense_fuse_layout(n_src, max_cap).total; }

hipError_t launch_dense_fuse(const gms_dense_fuse_src* d_src, int n_src, int max_cap, const int32_t* d_neighbors, int n_nb, int channels, int tol16,
                             int min_support, void* d_ws, int fused_cap, float* d_xyz, uint8_t* d_color, int32_t* d_source, int32_t* d_index,
                             uint8_t* d_support, uint8_t* d_conflict, int32_t* d_counts, hipStream_t stream)
{
    const DenseFuseLayout L = dense_fuse_layout(n_src, max_cap);
    const int nbs = dense_fuse_blocks(max_cap);
    const FuseArgs a{d_src, d_neighbors, ws_ptr<int32_t>(d_ws, L.blocks), ws_ptr<uint8_t>(d_ws, L.marks), d_xyz, d_color, d_source, d_index,
                     d_support, d_conflict, d_counts, n_src, max_cap, nbs, n_nb, channels, tol16, min_support, fused_cap};
    const dim3 grid((uint32_t)nbs, (uint32_t)n_src);
    hipLaunchKernelGGL(fuse_mark_kernel, grid, dim3(kBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(kBlock), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fuse_write_kernel, grid, dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gms
