// sfm_pair_pose_kernels.hip -- two-view and registration records of frame pairs from a view array (arithmetic: sfm_pair_pose_core.h,
// DESIGN.md §4.10d).
//   pair_pose_kernel  one lane per pair. A lane reads its pair's two frame indices, checks them against n_frames before it forms a
//                     view's address, reads the two views (24 doubles and two flags) and writes both records whole. A few hundred
//                     flops per lane: the cost of the stage is the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "sfm_pair_pose_core.h"

namespace gms {
namespace {

__global__ void __launch_bounds__(ppose::kBlock)
pair_pose_kernel(const gms_sfm_view* __restrict__ views, int n_frames, const gms_pair* __restrict__ pairs, int n_pairs,
                 gms_two_view* __restrict__ tv_out, gms_sfm_pair_reg* __restrict__ reg_out)
{
    const int i = blockIdx.x * ppose::kBlock + threadIdx.x;
    if (i >= n_pairs) return;
    gms_two_view tv;
    gms_sfm_pair_reg rg;
    ppose::pair_records(views, n_frames, pairs[i].frame_a, pairs[i].frame_b, tv, rg);
    tv_out[i] = tv;
    reg_out[i] = rg;
}

}  // namespace

hipError_t launch_sfm_pair_poses(const gms_sfm_view* d_views, int n_frames, const gms_pair* d_pairs, int n_pairs, gms_two_view* d_tv,
                                 gms_sfm_pair_reg* d_reg, hipStream_t stream)
{
    hipLaunchKernelGGL(pair_pose_kernel, dim3((uint32_t)((n_pairs + ppose::kBlock - 1) / ppose::kBlock)), dim3(ppose::kBlock), 0, stream,
                       d_views, n_frames, d_pairs, n_pairs, d_tv, d_reg);
    return hipGetLastError();
}

}  // namespace gms
