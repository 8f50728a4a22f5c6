// gms_kernel_dense.h -- what the byte-matrix forms of the GMS filter share (overview: gms_kernels.hip): the LDS layout of the
// 400 x 400 byte matrix, the per-keypoint codes of the frame table and the dense code word, the threshold test on small integers
// and nLeft from the half-cell histogram with the half-cell rule of the mark table and the list of who writes which of its
// fields. Used by gms_kernel_dense.hip (no scale hypotheses), gms_kernel_scales.hip (scale hypotheses) and gms_kernels.hip
// (normalize_kernel writes the codes). Internal.
#pragma once
#include <stdint.h>

#include "ws_layout.h"
// The layout constants and the half-cell geometry below are plain arithmetic that a host compiler builds alone
// (tests/cpp/mark_table_check.cpp); everything that needs the device is behind __HIPCC__.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "gms_device_common.h"
#define GMS_DENSE_HD __host__ __device__ __forceinline__
#define GMS_DENSE_UNROLL _Pragma("unroll")
#else
#define GMS_DENSE_HD inline
#define GMS_DENSE_UNROLL
#endif

namespace gms {

// ------------------------------------------------------------------------------------------------
// The dense path: pairs whose motion matrix fits the LDS as BYTES.
//
// Without scale hypotheses the right grid is 20 x 20, so the reference's motion matrix is 400 x 400; an entry never
// exceeds the number of matches of its left cell, so when no left cell (of any grid type) holds more than 255
// matches the whole matrix fits the CU's LDS as one byte per entry -- 160 000 of the 163 840 bytes.
// assignMatchPairs then is one returning LDS atomic per match (+1 on the entry's byte; the value it returns is the
// count this match produced, folded into the row's running arg-max with one atomicMax) and verifyCellPairs reads
// neighbour counts directly: no hashing, no bucket scans, no probe chains. The kernel is VALU-issue bound (16
// cycles of a SIMD per instruction of the 16-wave workgroup), so the per-match work is cut to the bone:
//   * a row is [header dword | 400 count bytes], the byte of right cell r at offset E(r) = 403 - r; the header
//     holds the running arg-max ((count - 1) << 11) | E(j) while binning (max = highest count, then lowest right
//     cell: the reference's ascending scan with strict '>') and cellPairs after verification;
//   * per match, two registers: the row start of its left cell under grid type 1, and a code word with E(r), the
//     half-cell parities q = (hx & 1) + 20 (hy & 1) and three "not binned under ..." bits. The left cell under grid
//     type g is l1 + (q & M_g), M_g = gx + 20 gy, so the row start is one multiply-add away;
//   * the matrix is zeroed once per pair; after each grid type every match takes its own increment back
//     (one store) instead of 160 KB being cleared again -- dense_pair_plain: not after the last, which nobody reads behind.
// Everything else has to live in the remaining 2.2 KB: the half-cell histogram and the current grid type's nLeft as
// bytes, the rotation counters and a few sink dwords. The DMatch records stay in registers from the first load to
// copy-out, so the match array is read exactly once.
// A pair that does not qualify (a cell above 255 matches, any input outside the parity domain, scale hypotheses) is handed to hash_pair() by the same workgroup; results are identical.
// ------------------------------------------------------------------------------------------------
constexpr int kDenseRightW = 20, kDenseRightN = 400;            // right grid of scale 0: cvRound(20 * 1.0)
constexpr uint32_t kDenseRow = 4u + kDenseRightN;               // header dword + one byte per right cell
constexpr uint32_t kDenseBytes = kLeftN * kDenseRow;            // 161 600
constexpr uint32_t kDenseFineOff = kDenseBytes;                 // [1600] bytes: half-cell histogram of the left points
constexpr uint32_t kDenseNleftOff = kDenseFineOff + kFineN;     // [400] bytes: nLeft of every cell under the current grid type
constexpr uint32_t kDenseMiscOff = kDenseNleftOff + kLeftN;     // [32] dwords: [0..7] rotation counts, [8] domain error,
                                                                //   [9] carry, [11] a cell above 255 matches, [12] an entry
                                                                //   at its limit, [13] a half cell above 255, [16..31] scan scratch
constexpr uint32_t kDenseTrashOff = kDenseMiscOff + 4u * 32u;   // [16] dwords: sinks
constexpr uint32_t kDenseLdsBytes = kDenseTrashOff + 4u * 16u;  // 163 792
static_assert(kDenseBytes % 16 == 0 && kDenseRow % 4 == 0, "rows are dword aligned, the matrix is cleared in uint4s");

#if defined(__HIPCC__)
static_assert(kDenseLdsBytes <= kLdsBytes, "dense layout exceeds the LDS");

// The threshold test of the byte-matrix path: T <= 9 * 255, score <= 9 * 255, n <= 9. For an integer factor up to 1023
// (the reference's default is 6) T * factor^2 and score^2 * n are exact 32-bit integers; when they differ, they differ by
// at least 1 in about 2^32, far more than the reference's three fp64 roundings can move thresh, so their order is the
// reference's answer. Exact ties (and every other factor) take the fp64 route of threshold_rejects().
__device__ __forceinline__ uint32_t dense_factor_sq(double factor)
{
    return (factor >= 1.0 && factor <= 1023.0 && factor == floor(factor)) ? (uint32_t)(factor * factor) : 0u;
}
__device__ __forceinline__ bool dense_threshold_rejects(uint32_t T, uint32_t n, uint32_t score, double factor, bool fast_ok, uint32_t f2i)
{
    if (f2i) {
        const uint32_t a = __umul24(T, f2i), b = __umul24(__umul24(score, score), n);
        if (a != b) return a > b;
    }
    return threshold_rejects(T, n, score, factor, fast_ok);
}

// 8-byte LDS accesses at absolute byte offsets (a multiple of 8), beside gms_device_common.h's ldsa_*: the mark table's entries
using lds_u64_t = __attribute__((address_space(3))) uint64_t;
__device__ __forceinline__ uint64_t ldsa_ld64(uint32_t a) { return *reinterpret_cast<lds_u64_t*>((uintptr_t)a); }
__device__ __forceinline__ void ldsa_st64(uint32_t a, uint64_t v) { *reinterpret_cast<lds_u64_t*>((uintptr_t)a) = v; }
__device__ __forceinline__ void ldsa_st16(uint32_t a, uint32_t v) { *reinterpret_cast<lds_u16_t*>((uintptr_t)a) = (uint16_t)v; }  // one field
#endif

// mNumberPointsInPerCellLeft of cell (x, y) under the grid type shifted by (gx, gy) half cells, from the half-cell histogram --
// which is laid out by cell: one dword per cell of grid type 1, its four half cells in the
// four bytes (byte index (hx & 1) + 2 (hy & 1)) -- the index a left code word yields without arithmetic.
GMS_DENSE_HD uint32_t dense_nleft_cm(const uint8_t* nfine8, int x, int y, int gx, int gy)
{
    const int hx0 = 2 * x - gx, hy0 = 2 * y - gy;
    uint32_t n = 0;
    GMS_DENSE_UNROLL
    for (int dy = 0; dy < 2; ++dy)
        GMS_DENSE_UNROLL
        for (int dx = 0; dx < 2; ++dx) {
            const int hx = hx0 + dx < 0 ? 0 : hx0 + dx, hy = hy0 + dy < 0 ? 0 : hy0 + dy;
            const uint32_t v = nfine8[(((hy >> 1) * kLeftW + (hx >> 1)) << 2) + (hx & 1) + ((hy & 1) << 1)];
            n += (hx0 + dx >= 0 && hy0 + dy >= 0) ? v : 0u;
        }
    return n;
}

// The same geometry the other way round: the cell that owns half cell (hx, hy) under the grid type shifted by (gx, gy) half cells --
// the cell whose dense_nleft_cm counts it --, or -1 where no cell does: the last half cell of a shifted axis (x >= 20 || y >= 20
// -> -1 in the reference, the edge bits of a code word). It is l1 + (q & (gx + 20 gy)) of a match's code word.
constexpr int dense_half_cell_owner(int hx, int hy, int gx, int gy)
{
    return ((hx + gx) >> 1) < kLeftW && ((hy + gy) >> 1) < kLeftH ? ((hy + gy) >> 1) * kLeftW + ((hx + gx) >> 1) : -1;
}
// where a half cell sits in the half-cell histogram (a byte) and in the mark table (an 8-byte entry): by cell of grid type 1
constexpr uint32_t dense_half_cell_slot(int hx, int hy)
{
    return (uint32_t)((((hy >> 1) * kLeftW + (hx >> 1)) << 2) + (hx & 1) + ((hy & 1) << 1));
}
static_assert(dense_half_cell_owner(39, 38, 1, 0) == -1 && dense_half_cell_owner(39, 38, 0, 1) == 19 * kLeftW + 19 &&
              dense_half_cell_owner(0, 0, 1, 1) == 0 && dense_half_cell_owner(1, 1, 1, 1) == kLeftW + 1, "half cells and shifted grids");

// The mark table of dense_pair_plain: behind the last grid type's verification nobody reads the matrix any more (that grid type's
// increments are still in it), and the verdicts of all four grid types -- cellPairs[cell] as E(j*), kDenseMarkNone where the cell
// pair was rejected or the cell is empty, kept in the verifying lanes' registers while the matrix lived -- go into it once per pair:
//   table     8-byte entries of 4 16-bit fields, entry dense_half_cell_slot(hx, hy): field g = the verdict of the cell that owns
//             the half cell under grid type g, kDenseMarkNone where nobody does. A match is an inlier when one field of its left
//             point's entry equals its E(r): one 8-byte read instead of a row header per grid type. A match that is not binned
//             (code word = a sink's) computes "cell" kDenseMarkSinkSlot / 4 from its sink's offset: an entry of its own, none four times.
// The lanes store the fields directly (who writes which: below); kDenseMarkVerdictOff is where an earlier form of the kernel laid
// the verdicts down first, [400] x 4 fields -- nothing is written there now. The table lies above everything the copy-out keeps in
// the area (its scan table: at most 8 KB from offset 0), and its offset fits the 16-bit immediate of an LDS instruction.
constexpr uint32_t kDenseMarkNone = 0xFFFFu;             // never an E(r): those are 4..403, a sink's is 0
constexpr uint32_t kDenseMarkVerdictOff = 16384;
constexpr uint32_t kDenseMarkTableOff = 32768;
constexpr uint32_t kDenseMarkSinkSlot = 4u * ((kDenseTrashOff / 4u * 649u) >> 16);  // 1620: the sinks' "row / 404" is 405
constexpr uint32_t kDenseMarkEntries = kDenseMarkSinkSlot + 1u;
static_assert(((((kDenseTrashOff + 60u) >> 2) * 649u) >> 16) == kDenseMarkSinkSlot / 4u && kDenseMarkSinkSlot >= (uint32_t)kFineN,
              "all sixteen sink dwords divide to one row above the grid");
static_assert(kDenseMarkTableOff + 8u * kDenseMarkEntries <= kDenseBytes && kDenseMarkTableOff + 8u * kDenseMarkEntries < 65536u &&
              kDenseMarkVerdictOff + 8u * kLeftN <= kDenseMarkTableOff, "verdicts and table inside the matrix area, apart");

// Who writes the table (tests/cpp/mark_scatter_check.cpp replays both kinds of writer over all fields). A field is one 16-bit word:
// field f = 4 * entry + grid type, at dense_mark_field_off(f).
//   owned fields    the two verifying lanes of cell (x, y) store the cell's verdict under grid type g into field g of its (up to)
//                   four half cells: dense_cell_half_slot(x, y, gx, gy, dx, dy), dx, dy in {0, 1} -- the inverse of
//                   dense_half_cell_owner(). Where a shifted axis cuts the cell at the image's first half row or column the index is
//                   clamped as dense_nleft_cm clamps it: that store repeats one of the cell's own (same field, same value), so
//                   none of the four is predicated;
//   the others      fields nobody owns -- hx == 39 under the x-shifted grid types, hy == 39 under the y-shifted ones,
//                   kDenseMarkUnownedFields in all -- and the four fields of every entry behind the grid up to the sink's: field
//                   dense_mark_none_field(u), u < kDenseMarkNoneFields, written with kDenseMarkNone by the lanes that do not verify.
// Every field has exactly one writer, for every pair.
constexpr uint32_t dense_mark_field_off(uint32_t field) { return kDenseMarkTableOff + 2u * field; }
constexpr uint32_t dense_cell_half_slot(int x, int y, int gx, int gy, int dx, int dy)
{
    return dense_half_cell_slot(2 * x - gx + dx < 0 ? 0 : 2 * x - gx + dx, 2 * y - gy + dy < 0 ? 0 : 2 * y - gy + dy);
}
constexpr uint32_t kDenseMarkUnownedFields = 2u * kFineW + kFineW + (kFineW - 1u);  // 159: (39, 39) under grid type 4 counts once
constexpr uint32_t kDenseMarkNoneFields = kDenseMarkUnownedFields + 4u * (kDenseMarkEntries - (uint32_t)kFineN);  // 243
constexpr uint32_t dense_mark_none_field(uint32_t u)
{
    constexpr uint32_t w = (uint32_t)kFineW, last = w - 1u;
    return u < 2u * w   ? 4u * dense_half_cell_slot((int)last, (int)(u < w ? u : u - w)) + (u < w ? 1u : 3u)            // hx == 39: grid types 2, 4
           : u < 3u * w ? 4u * dense_half_cell_slot((int)(u - 2u * w), (int)last) + 2u                                  // hy == 39: grid type 3 ...
           : u < kDenseMarkUnownedFields ? 4u * dense_half_cell_slot((int)(u - 3u * w), (int)last) + 3u                 // ... and 4, hx < 39
                                         : 4u * (uint32_t)kFineN + (u - kDenseMarkUnownedFields);                       // behind the grid
}
static_assert(dense_mark_none_field(kDenseMarkNoneFields - 1u) == 4u * kDenseMarkEntries - 1u && dense_cell_half_slot(0, 0, 1, 1, 0, 0) == 0u &&
              dense_cell_half_slot(3, 2, 1, 0, 0, 1) == dense_half_cell_slot(5, 5), "the table's last field; clamping; a cell's half cells");

// dense code word
                                                     // bits 0..4   q = (hx & 1) + 20 * (hy & 1)
constexpr uint32_t kDNever = 1u << 5;                // bit 5       not binned under any grid type
constexpr uint32_t kDEdgeX = 1u << 6;                // bit 6       hx == 39: x >= 20 under the x-shifted grid types
constexpr uint32_t kDEdgeY = 1u << 7;                // bit 7       hy == 39
constexpr int kDEShift = 8;                          // bits 8..16  E(r) = 403 - r, the byte's offset in its row
constexpr uint32_t kDEMask = 0x1FFu;
constexpr int kDAccShift = 17;                       // bits 17..24 inlier-under-rotation bits
constexpr int kDTagShift = 20;                       // arg-max key in a row header: grid type << 20 | (count - 1) << 11 | E(j)

// Besides the normalised point, everything about a keypoint that does not depend on the pair it is matched in is worked out
// by normalize_kernel (keypoint_codes in gms_kernels.hip), once per frame (a frame of a sequence is filtered against hundreds of others): two 16-bit codes per keypoint.
//   lcode  the keypoint as a LEFT point: [q : 5 | x >= 20 under the x-shifted grid types : 1 | y likewise : 1 | cell under grid
//          type 1 : 9] -- q and the edge bits are the low bits of the dense code word as they stand (kDEdgeX / kDEdgeY one place
//          up). Cell values above the grid: kLCellNever (the point is binned under no grid type), kLCellBad (outside the parity
//          domain: negative, non-finite or >= 2^20 after normalisation);
//   rcode  the keypoint as a RIGHT point: E(r) = 403 - r of scale 0 (0 = outside the 20 x 20 grid); top bit: outside the domain;
//   scode  the keypoint as a RIGHT point under scale hypotheses, 32 bits: [cell on the 20 x 20 grid : 9 | cell on the 28 x 28
//          grid : 10 | low bit of the 40 x 40 cell's x, y : 2] -- the 10 x 10, 14 x 14 and 40 x 40 cells follow from these
//          (fl(10 n) = fl(20 n) / 2, fl(14 n) = fl(28 n) / 2, fl(40 n) = 2 fl(20 n) + bit, exactly); kSCodeBad: outside the domain or
//          outside one of the grids coordinate-wise (the reference has no bounds test there: such a pair takes the general path).
constexpr uint32_t kLCellShift = 7, kLCellNever = 510u, kLCellBad = 511u;
constexpr uint32_t kRCodeBad = 1u << 15;
constexpr uint32_t kSCodeBad = 1u << 31;

}  // namespace gms
