// gms_large_common.h -- what the large-pair kernels (above 16 384 matches: gms_kernel_band.hip, gms_kernel_stream.hip,
// gms_kernel_stream_plain.hip, gms_kernel_big.hip) state once: the per-pair flag word between the LDS kernels and the HBM-slab kernel
// that runs behind them, and the steps their kernels share. Internal; included by those .hip files only.
// A helper is used where the kernel's device code stays what it was (tools/asm_compare.py); a few sites keep their own copy of a
// step because any shared form changed their register allocation or schedule -- each says so.
#pragma once
#include "gms_device_common.h"

namespace gms {

// The flag word of a pair (FilterParams::pair_flags for the slab kernel, which filters the pairs with kFlagGeneral set):
constexpr uint32_t kFlagDomain = 1u;    // an input outside the parity domain: the pair fails as a whole
constexpr uint32_t kFlagGeneral = 2u;   // a left cell above 65 535 matches: gms_kernel_big.hip takes the pair

// First keypoint and number of keypoints of the pair's two frames -- for a pair whose frame indices are in range (every kernel tests
// "m < 0 || m > mcap || frame_a / frame_b outside [0, n_frames)" first, spelled out: as a function the test loses its early exits).
// nA <= 0 or nB <= 0: matches, but nothing valid to index.
__device__ __forceinline__ void pair_frame_ranges(const FilterParams& p, const gms_pair& pr, int64_t& offA, int& nA, int64_t& offB, int& nB)
{
    offA = p.frame_off[pr.frame_a];
    offB = p.frame_off[pr.frame_b];
    nA = (int)(p.frame_off[pr.frame_a + 1] - offA);
    nB = (int)(p.frame_off[pr.frame_b + 1] - offB);
}

// Ordered copy-out of a wave: N rounds of 64 consecutive matches from `first`; the survivors (keep(k) of this lane, ballots bal[k] of
// the wave) go to out[pos ...] in input order. The records are requested unconditionally and pinned before the first store: a load
// that only a conditional store uses is sunk into the branch by the compiler and waited for there, one round trip per record.
// Returns the position behind the wave's survivors.
template <int N, class Keep>
__device__ __forceinline__ uint32_t copy_out_wave(const gms_dmatch* __restrict__ matches, gms_dmatch* __restrict__ out, int first, int m, int lane,
                                                  const unsigned long long* bal, Keep&& keep, uint32_t pos)
{
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint4 rec[N];
#pragma unroll
    for (int k = 0; k < N; ++k) rec[k] = *reinterpret_cast<const uint4*>(&matches[min(first + k * 64 + lane, m - 1)]);
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" : "+v"(rec[k].x), "+v"(rec[k].y), "+v"(rec[k].z), "+v"(rec[k].w));
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (keep(k)) *reinterpret_cast<uint4*>(&out[pos + (uint32_t)__popcll(bal[k] & lt)]) = rec[k];
        pos += (uint32_t)__popcll(bal[k]);
    }
    return pos;
}

}  // namespace gms
