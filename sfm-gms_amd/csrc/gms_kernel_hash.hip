// gms_kernel_hash.hip -- filter_kernel: the hashed form of the GMS filter for every pair of a launch (overview: gms_kernels.hip;
// the body, hash_pair(), is in gms_kernel_hash.h), its launch and its dynamic-LDS limits.
#include "gms_kernel_hash.h"

namespace gms {

template <int KPT, bool ROT, int NT>
__global__ void __launch_bounds__(NT)
filter_kernel(FilterParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    first_round_stagger(p);
    hash_pair<KPT, ROT, NT>(p, smem, (int)blockIdx.x, (int)threadIdx.x);
}

hipError_t launch_filter_hash(const FilterParams& p, int kpt, int n_pairs, size_t lds_bytes, hipStream_t stream)
{
    return dispatch_kpt_rot(kpt, p.with_rotation != 0, [&](auto k, auto rot) {
        hipLaunchKernelGGL((filter_kernel<decltype(k)::value, decltype(rot)::value, kThreads>), dim3((unsigned)n_pairs), dim3(kThreads), lds_bytes, stream, p);
        return hipGetLastError();
    });
}

hipError_t init_hash_kernels()
{
    return for_each_kpt_rot([](auto k, auto rot) { return allow_full_lds(filter_kernel<decltype(k)::value, decltype(rot)::value, kThreads>); });
}

}  // namespace gms
