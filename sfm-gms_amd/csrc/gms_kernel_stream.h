// gms_kernel_stream.h -- what the two files of the streamed large-pair kernels (16 385 ... 65 536 matches per pair) share:
// gms_kernel_stream.hip (the scale-hypothesis pipeline and the one-workgroup-per-pair stream_dense_kernel) and
// gms_kernel_stream_plain.hip (stream_dense_kernel's default-flags form). The size class, the LDS layout of the one-workgroup-per-pair
// byte matrix that stream_plain_kernel builds on, and the declarations between the files. Internal; included by those .hip files only.
#pragma once
#include "gms_device_common.h"

namespace gms {

constexpr int kSMaxMatches = 1 << 16;                      // (an entry holds 26 bits of original index; beyond 65 536 matches the 16-bit band / tile kernels are the better fit: entries above 255 get likely)

// ---- stream_dense_kernel / stream_plain_kernel: [400][header dword | 400 bytes] | nLeft | scratch words
constexpr uint32_t kDRow = 4u + 400u;                       // header dword + one byte per right cell (offset E(r) = 403 - r)
constexpr uint32_t kDSNleftOff = kLeftN * kDRow;            // 161 600: [400] u16
constexpr uint32_t kDSMiscOff = kDSNleftOff + 2u * kLeftN;  // [32] u32: [0..7] rotation counts, [8] bad input, [9] entry / cell too big, [16..31] wave totals
constexpr uint32_t kDSLdsBytes = kDSMiscOff + 128u;         // 162 528
static_assert(kDSLdsBytes <= kLdsBytes, "stream-dense layout exceeds the LDS");
constexpr int kKeyCountShift = 11, kKeyTagShift = 27;       // row header while binning: grid type << 27 | (count - 1) << 11 | E

// gms_kernel_stream_plain.hip: its kernel's dynamic-LDS limit (init_stream_kernels calls it)
hipError_t init_stream_plain_kernels();
// stream_plain_kernel on n pairs (launch_filter_stream_dense: default flags, unless GMS_STREAM_PLAIN=0)
void launch_stream_plain(const FilterParams& p, int n, uint32_t* codes, uint16_t* nleft, uint32_t* flags, int mcap, hipStream_t stream);

}  // namespace gms
