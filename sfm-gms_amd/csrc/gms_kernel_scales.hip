// gms_kernel_scales.hip -- filter_kernel_dense_scales: the byte-matrix form of the GMS filter with scale hypotheses (overview:
// gms_kernels.hip; the matrix and its LDS layout: gms_kernel_dense.h), its launch and its dynamic-LDS limits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gms_kernel_dense.h"

namespace gms {

// ------------------------------------------------------------------------------------------------
// Scale hypotheses on the byte matrix (dense_scales_pair): the right grids of scales 0, 1 and 2 are 20 x 20,
// 10 x 10 and 14 x 14, so their motion matrices (400 x 400, 400 x 100, 400 x 196 bytes) fit the LDS like the default
// case; scale 3 (28 x 28: 400 rows of 788 bytes) fits in three bands of left rows; scale 4 (40 x 40: 1604-byte rows) would
// need seven. With scale hypotheses a launch therefore runs two kernels: this one evaluates scales 0..3 (all rotations),
// bounds scale 4 (the probe below, four halo-free bands) and leaves the best hypothesis so far -- count, (scale, rotation),
// the inlier bit of every match -- in a per-pair workspace record together with what is decided; filter_kernel then picks
// the record up, evaluates scale 4 on the hashed path unless the probe bounded it out, and selects and copies out as always
// (getInlierMask's order is scale-outer, rotation-inner with strict '>', so "best of 0..3, then 4" is the same comparison
// sequence). A pair this kernel cannot take (a cell above 255 matches, inputs outside the parity domain) gets an empty record
// and the hashed path evaluates all five scales.
// Everything is dense_pair_rot() (gms_kernel_dense.hip) with a runtime row stride; the records are not kept (nothing is copied out here).
// ------------------------------------------------------------------------------------------------

// The copy-out of a pair whose five scale hypotheses are all decided in the byte-matrix kernel (the probe bounded scale 4 out): the
// survivors in input order, the result record, the optional mask -- what the hashed kernel would otherwise start a workgroup for, read
// the pair's record and 160 KB of DMatch records from HBM for, 100 us after this kernel had them. NOT inlined on purpose: a body of its
// own register allocation, so that nothing here is live through the scale passes (round 3's inlined attempt paid for itself in spills).
// A unit is eight consecutive matches = the byte of a ballot that an eight-lane group holds, in either lane mapping.
template <int KPT, int NT>
__device__ __noinline__ void scales_copy_out(const gms_pair* pairs, const gms_dmatch* all_matches, gms_dmatch* all_out, uint8_t* all_mask,
                                             gms_pair_result* results, uint32_t* smem, int pair_idx, uint32_t bestbits, int dealt,
                                             uint32_t best_count, int best_scale, int best_rot)
{
    constexpr int kUnits = KPT * NT / 8, kWaves = NT / 64;
    static_assert(kUnits <= 2 * NT, "two scan entries per thread");
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gms_pair pr = load_pair(pairs, pair_idx);
    const int m = pr.m;
    const gms_dmatch* __restrict__ matches = all_matches + pr.match_off;
    gms_dmatch* __restrict__ out = all_out + pr.match_off;
    uint32_t* cnt = smem;              // [kUnits] survivors per unit, then in front of it
    uint32_t* wtot = smem + kUnits;    // [kWaves]
    const int ubase = dealt ? (lane >> 3) * (KPT * kWaves) + wave : (tid >> 3);
    const int ustep = dealt ? kWaves : NT / 8;
    __syncthreads();  // (the matrix area is free)
    uint32_t ranks[(KPT + 7) / 8] = {};  // four bits per match: survivors before it in its unit
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        const unsigned long long bal = __ballot((bestbits >> k) & 1u);
        const uint32_t byte = (uint32_t)(bal >> (lane & 56)) & 0xFFu;
        if ((lane & 7) == 0) cnt[ubase + k * ustep] = (uint32_t)__popc(byte);
        ranks[k >> 3] |= (uint32_t)__popc(byte & ((1u << (lane & 7)) - 1u)) << ((k & 7) * 4);
    }
    __syncthreads();
    {   // exclusive scan over the units, two per thread
        const uint32_t a = 2 * tid < kUnits ? cnt[2 * tid] : 0u, b = 2 * tid + 1 < kUnits ? cnt[2 * tid + 1] : 0u;
        uint32_t incl = a + b;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        const uint32_t excl = before + incl - (a + b);
        if (2 * tid < kUnits) cnt[2 * tid] = excl;
        if (2 * tid + 1 < kUnits) cnt[2 * tid + 1] = excl + a;
    }
    __syncthreads();
    // the survivors' records: a round of them requested together, every lane from an address (its own record or the pair's first),
    // pinned before the stores
    constexpr int kRound = KPT % 10 == 0 ? 10 : KPT % 8 == 0 ? 8 : 4;
    static_assert(KPT % kRound == 0, "whole rounds");
#pragma unroll
    for (int k0 = 0; k0 < KPT; k0 += kRound) {
        uint4 rec[kRound];
#pragma unroll
        for (int c = 0; c < kRound; ++c) {
            const int k = k0 + c, i = ((ubase + k * ustep) << 3) | (lane & 7);
            rec[c] = *reinterpret_cast<const uint4*>(&matches[(((bestbits >> k) & 1u) && i < m) ? i : 0]);
        }
#pragma unroll
        for (int c = 0; c < kRound; ++c) asm volatile("" : "+v"(rec[c].x), "+v"(rec[c].y), "+v"(rec[c].z), "+v"(rec[c].w));
#pragma unroll
        for (int c = 0; c < kRound; ++c) {
            const int k = k0 + c, u = ubase + k * ustep, i = (u << 3) | (lane & 7);
            const bool in = ((bestbits >> k) & 1u) && i < m;
            if (all_mask && i < m) all_mask[pr.match_off + i] = in ? 1 : 0;
            if (in) {
                const uint32_t pos = cnt[u] + ((ranks[k >> 3] >> ((k & 7) * 4)) & 15u);
                __builtin_nontemporal_store(u32x4_t{rec[c].x, rec[c].y, rec[c].z, rec[c].w}, reinterpret_cast<u32x4_t*>(&out[pos]));
            }
        }
    }
    if (tid == 0) {
        gms_pair_result r;
        r.n_inliers = (int)best_count;
        r.best_scale = best_scale;
        r.best_rot = best_rot;
        r.status = GMS_OK;
        results[pair_idx] = r;
    }
}

template <int KPT, bool ROT, int NT>
__device__ __forceinline__ bool dense_scales_pair(const FilterParams& p, uint32_t* smem, const int pair_idx, const int tid,
                                                  uint32_t* __restrict__ part)
{
    constexpr int kMcap = KPT * NT;
    constexpr int kNRot = ROT ? 8 : 1;
    constexpr int kChunk = (KPT % 5 == 0) ? 5 : 4;
    static_assert(KPT % kChunk == 0, "KPT must be a multiple of the chunk");
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // Lane mapping (twin of dense_pair_rot's in gms_kernel_dense.hip): in list order a wave instruction holds 64 consecutive matches; DEALT (a run-time choice here: it
    // only moves the loads and the record's bits) gives the wave's eight 8-lane groups eight consecutive matches each from places
    // KPT * 128 matches apart -- a detector that emits keypoints row by row puts consecutive matches into the same cells, and 64 of
    // them in one LDS atomic instruction serialise on a handful of entries.
    const bool dealt = p.dealt != 0;
    const int m_base = dealt ? ((((lane >> 3) * (KPT * (NT / 64)) + wave) << 3) | (lane & 7)) : tid;
    const int m_stride = dealt ? (NT / 64) * 8 : NT;
    auto match_of = [&](int k) -> int { return m_base + k * m_stride; };

    int64_t total_kp;
    const gms_pair pr = load_pair(p.pairs, pair_idx, p, total_kp);  // (and the frame table's header word)
    const int m = pr.m;
    if (!p.with_scale || m <= 0 || m > kMcap || pr.frame_a < 0 || pr.frame_a >= p.n_frames || pr.frame_b < 0 ||
        pr.frame_b >= p.n_frames)
        return false;
    if (p.right_w[0] != 20 || p.right_h[0] != 20 || p.right_w[1] != 10 || p.right_h[1] != 10 || p.right_w[2] != 14 ||
        p.right_h[2] != 14 || p.right_w[3] != 28 || p.right_h[3] != 28)
        return false;
    constexpr uint32_t kSEMask = 0x3FFu;   // E(r) = nr + 3 - r needs 10 bits at 28 x 28 right cells (bits 8..17 of the code word)
    constexpr int kSAccShift = 18;         // rotation bits 18..25
    constexpr int kSProbeBit = 26;         // PROBE: "sits in its row's arg-max entry under some grid type"
    const int64_t offA = p.frame_off[pr.frame_a], offB = p.frame_off[pr.frame_b];
    const int nA = (int)(p.frame_off[pr.frame_a + 1] - offA), nB = (int)(p.frame_off[pr.frame_b + 1] - offB);
    if (nA <= 0 || nB <= 0) return false;
    const gms_dmatch* __restrict__ matches = p.matches + pr.match_off;
    // the frame table's code words (normalize_kernel): frame A's left codes (16 bits), frame B's scale codes (32 bits)
    if (total_kp < 0 || offA + nA > total_kp || offB + nB > total_kp) return false;  // (workgroup-uniform) no header, or frames beyond the table
    const uint16_t* __restrict__ lcodeA = reinterpret_cast<const uint16_t*>(p.pts + total_kp) + offA;
    const uint32_t* __restrict__ scodeB = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(p.pts + total_kp) + 2 * total_kp) + offB;

    const uint8_t* dense8 = reinterpret_cast<const uint8_t*>(smem);
    uint32_t* nfine32 = smem + kDenseFineOff / 4;   // half-cell histogram: one dword per cell of grid type 1, a byte per half cell (as in dense_pair_rot)
    const uint8_t* nfine8 = reinterpret_cast<const uint8_t*>(nfine32);
    uint8_t* nleft8 = reinterpret_cast<uint8_t*>(smem) + kDenseNleftOff;
    uint32_t* misc = smem + kDenseMiscOff / 4;
    uint32_t* trash = smem + kDenseTrashOff / 4;

    GMS_STAMP_DECL
    if (tid < 32) misc[tid] = 0;
    if (tid < 16) trash[tid] = 0;
    if (tid < kFineN / 4) nfine32[tid] = 0;

    // ---- both frames' codes staged in the still unused matrix area, then the pair's (queryIdx, trainIdx) (twin of dense_pair_rot's staging, with four registers and 32-bit codes of frame B)
    const uint32_t phA = (uint32_t)(reinterpret_cast<uintptr_t>(lcodeA) >> 1) & 7u, phB = (uint32_t)(reinterpret_cast<uintptr_t>(scodeB) >> 2) & 3u;
    const uint32_t qA = (phA + (uint32_t)nA + 7u) >> 3, qB = (phB + (uint32_t)nB + 3u) >> 2;  // uint4s of either copy
    const bool staged = (qA + qB) * 16u <= kDenseBytes;  // workgroup-uniform
    const uint4* __restrict__ srcA = reinterpret_cast<const uint4*>(lcodeA - phA);
    const uint4* __restrict__ srcB = reinterpret_cast<const uint4*>(scodeB - phB);
    constexpr int kStageRegs = 4;  // 64 KB of codes (10 900 keypoints a frame) through registers; larger frames finish in a plain loop
    uint4 tb[kStageRegs];
#pragma unroll
    for (int i = 0; i < kStageRegs; ++i) {  // (unconditional: a pair too large to stage just reads a few code words it does not use)
        const uint32_t j = min((uint32_t)(i * NT + tid), qA + qB - 1u);
        const uint4* src = j < qA ? srcA + j : srcB + (j - qA);
        tb[i] = *src;
    }
    uint2 qt[KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) qt[k] = *reinterpret_cast<const uint2*>(&matches[min(match_of(k), m - 1)]);
    const uint32_t staged16 = staged ? qA + qB : 0u;
    {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        uint4* d4 = reinterpret_cast<uint4*>(smem);
        // (staged: the first kStageRegs * NT slots are written below, codes or zeros)
        for (uint32_t i = (staged ? max(staged16, (uint32_t)(kStageRegs * NT)) : 0u) + tid; i < kDenseBytes / 16; i += NT) d4[i] = z4;
    }
    if (staged) {
        // UNCONDITIONAL stores, the data selected: a store under a condition lets the compiler sink its load into the branch, behind
        // the clear, with a wait of its own -- one round trip per register instead of all of them in flight from the top
        static_assert((size_t)kStageRegs * NT * 16 <= kDenseBytes, "the register-staged slots lie inside the matrix area");
        uint4* d4 = reinterpret_cast<uint4*>(smem);
#pragma unroll
        for (int i = 0; i < kStageRegs; ++i) {
            const bool in = (uint32_t)(i * NT + tid) < qA + qB;
            d4[i * NT + tid] = make_uint4(in ? tb[i].x : 0u, in ? tb[i].y : 0u, in ? tb[i].z : 0u, in ? tb[i].w : 0u);
        }
        for (uint32_t j = kStageRegs * NT + tid; j < qA + qB; j += NT) d4[j] = *(j < qA ? srcA + j : srcB + (j - qA));
    }
    const uint16_t* ldsA = reinterpret_cast<const uint16_t*>(smem) + phA;  // left code of frame A's keypoint q at ldsA[q]
    const uint32_t* ldsB = smem + 4u * qA + phB;                           // scale code of frame B's keypoint t at ldsB[t]
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    GMS_STAMP_OUT(4, 10);  // indices landed, codes staged
    // code word as in dense_pair_rot (E = E(r) of the current scale, 10 bits); aux = left cell under grid type 1 : 9 | right cell on the
    // 20 x 20 grid : 9 | on the 28 x 28 grid : 10 | low bit of the 40 x 40 cell's x, y : 2 (the scale code as it stands, 9 bits up)
    uint32_t code[KPT], aux[KPT];
    {
        uint32_t ca[KPT], cb[KPT];
        if (staged) {
#pragma unroll
            for (int k = 0; k < KPT; ++k) ca[k] = ldsA[min(qt[k].x, (uint32_t)(nA - 1))];
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = ldsB[min(qt[k].y, (uint32_t)(nB - 1))];
        } else {
#pragma unroll
            for (int k = 0; k < KPT; ++k) ca[k] = lcodeA[min(qt[k].x, (uint32_t)(nA - 1))];
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = scodeB[min(qt[k].y, (uint32_t)(nB - 1))];
        }
        bool any_bad = false, spill = false;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const bool live = match_of(k) < m;
            const uint32_t cell = ca[k] >> kLCellShift;  // under grid type 1; kLCellNever / kLCellBad above the grid
            const bool ok = ((int)(qt[k].x < (uint32_t)nA) & (int)(qt[k].y < (uint32_t)nB) & (int)(cell != kLCellBad) & (int)((cb[k] & kSCodeBad) == 0u)) != 0;
            const bool binned = live & ok & (cell < kLCellNever);
            const uint32_t sh = ((ca[k] & 1u) << 3) | ((ca[k] & 4u) << 2);  // byte (hx & 1) + 2 (hy & 1) of the cell's dword (twin of dense_pair_rot's)
            const uint32_t old = atomicAdd(binned ? &nfine32[cell] : &trash[lane & 7], 1u << sh);
            spill |= binned & (((old >> sh) & 255u) == 255u);
            any_bad |= live & !ok;
            const uint32_t r0 = cb[k] & 0x1FFu;
            code[k] = binned ? ((ca[k] & 31u) | ((ca[k] & 0x60u) << 1) | ((403u - r0) << kDEShift)) : kDNever;
            aux[k] = binned ? (cell | ((cb[k] & 0x1FFFFFu) << 9)) : 0u;
        }
        if (any_bad) misc[8] = 1;
        if (spill) misc[13] = 1;  // (not misc[11]: that one is written again while slower waves may still be reading this)
    }
    __syncthreads();
    {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        uint4* d4 = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < staged16; i += NT) d4[i] = z4;
        // the sink dwords (see dense_pair_plain): the binning and marking loops below run unpredicated, a match that is not binned in
        // the current pass works on its lane's sink instead. Bit 31 is never cleared (increments land in byte 0, keys end below it).
        if (tid < 16) trash[tid] = 0x80000000u;
        if (tid == 0) misc[15] = 0xFFFFFFFFu;  // "no header": what a match reads in the marking pass when the grid type leaves it out (E = 2047: equal to no E -- a never-binned match carries E = 0 --, and no rotation bits)
        if (tid == 0) misc[14] = 0x7FFu;       // the same for probes, whose nibble form also tests the low 20 bits for the "dirty row" key
    }
    __syncthreads();
    if (misc[8] != 0) {  // an input outside the parity domain (workgroup-uniform)
        __syncthreads();
        return false;
    }
    const bool spilled = misc[13] != 0;  // a half cell above 255 matches: crowded from the start (see dense_pair_rot)
    uint32_t* nl32 = nfine32;            // crowded mode: nLeft as 16-bit counters, two buffers of 400
    const uint32_t sink_at = kDenseTrashOff + 4u * (uint32_t)(lane & 15), none_at = kDenseMiscOff + 4u * 15u, none_probe_at = kDenseMiscOff + 4u * 14u;

    const bool thr_fast = threshold_fast_ok(p.threshold_factor);
    const uint32_t f2i = dense_factor_sq(p.threshold_factor);
    uint32_t best_count = 0, bestbits = 0;
    int best_scale = -1, best_rot = -1;

    // One scale hypothesis. BANDED (scale 3, 28 x 28 right cells: 400 rows of 788 bytes do not fit): the left grid's rows
    // are taken 8 at a time, each band with one halo row on either side in LDS (at most 10 rows = 157 600 bytes); per
    // grid type a band bins the matches of the rows it holds, verifies and marks its own rows' cells and takes every
    // increment back before the next band. (Probes band differently: no halo, as many rows as fit; scale 4 only exists as a probe.)
    // With rotation a lane verifies two of the eight rotations of its cell (four lanes per cell: sub = item & 3 picks rotations
    // 2 sub, 2 sub + 1; the left side of the nine neighbour pairs is shared by the two). Where a rotation pattern sends the
    // eight outer neighbours is a compile-time word (rotation_pack): the lane selects its two at the point of use.

    // PROBE: an upper bound of the scale's inlier count instead of the count itself. A match can only be an inlier of a
    // (scale, rotation) hypothesis if, under some grid type, its right cell IS the arg-max of its left cell's row -- whatever the
    // rotation, whatever verifyCellPairs says about the cell. So: bin as always, flag the matches that sit in their row's arg-max
    // entry, take the increments back, no verify; when the number of flagged matches does not exceed the best count so far, none of
    // the scale's eight rotations can replace the best hypothesis (getInlierMask keeps on strict '>') and the scale is skipped.
    // Costs about 45 % of the scale when it does not help, saves the other 55 % when it does.

    // returns 0 = done, 1 = a cell above 255 matches (everything is run again CROWDED), 2 = a matrix entry at its limit,
    // 3 = PROBE only: the scale cannot win
    auto run_scale = [&](auto banded_c, auto crowded_c, auto probe_c, auto nib_c, const int s) -> int {
        constexpr bool BANDED = decltype(banded_c)::value;
        constexpr bool CROWDED = decltype(crowded_c)::value;
        constexpr bool PROBE = decltype(probe_c)::value;
        // NIB (probes of the two fine grids only): one NIBBLE per entry -- rows half as long, so scale 3's matrix fits whole (400 rows
        // of 396 bytes: a probe in four passes instead of eight) and scale 4's in two bands of ten rows (eight passes instead of
        // sixteen). A probe is an upper bound, so an entry that passes 15 need not stop anything: the add that sees 15 come back (its
        // carry has spoilt the neighbour entry of the same row, never another row: rows are dword-aligned) marks the ROW dirty --
        // the largest key the pass can hold -- and every match of a dirty row counts as a possible inlier: a superset of the exact
        // probe's set, a few matches larger where a row overflowed.
        constexpr bool NIB = decltype(nib_c)::value;
        static_assert(!NIB || (PROBE && !CROWDED), "nibble entries: probes of uncrowded pairs only");
        const uint32_t wr = (uint32_t)p.right_w[s], nr = wr * wr;
        const uint32_t stride = 4u + (NIB ? nr >> 1 : nr);   // header dword + one byte (nibble) per right cell
        const uint32_t e_top = NIB ? nr + 7u : nr + 3u;       // E(r) = e_top - r: the entry's byte (nibble) offset in its row
        const uint32_t wr_magic = 65535u / wr + 1u;      // j / wr == (j * magic) >> 16 for j * wr < 65536
        // scale 4 (probe only): E(r) up to 1603 takes 11 bits and reaches into the rotation bits, which a probe does not use
        const uint32_t emask = (PROBE && s == 4) ? 0x7FFu : kSEMask;
        {   // the code words' E(r) for this scale (scale 0 too: it is not the first one evaluated)
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                uint32_t r;
                if (s == 0) {
                    r = (aux[k] >> 9) & 0x1FFu;
                } else if (s == 3) {
                    r = (aux[k] >> 18) & 0x3FFu;
                } else if (s == 4) {  // double the 20 x 20 cell's coordinates and add the stored low bits: fl(40 n) = 2 fl(20 n) + bit
                    const uint32_t c20 = (aux[k] >> 9) & 0x1FFu, cy = (c20 * 3277u) >> 16, cx = c20 - cy * 20u;
                    r = (2u * cy + ((aux[k] >> 29) & 1u)) * 40u + 2u * cx + ((aux[k] >> 28) & 1u);
                } else {  // halve the finer grid's cell coordinates: 20 -> 10 (s == 1), 28 -> 14 (s == 2)
                    const uint32_t fine = s == 1 ? (aux[k] >> 9) & 0x1FFu : (aux[k] >> 18) & 0x3FFu, wf = s == 1 ? 20u : 28u;
                    const uint32_t fy = (fine * (s == 1 ? 3277u : 2341u)) >> 16, fx = fine - fy * wf;  // fine / wf for fine < 784
                    r = (fy >> 1) * (wf >> 1) + (fx >> 1);
                }
                if (!(code[k] & kDNever)) code[k] = (code[k] & ~(emask << kDEShift)) | ((e_top - r) << kDEShift);
            }
        }
        int status = 0;
        for (int g = 0; g < 4; ++g) {
            const int gx = g & 1, gy = g >> 1;
            const uint32_t q_mask = (uint32_t)(gx + 20 * gy);
            const uint32_t out_mask = kDNever | (gx ? kDEdgeX : 0u) | (gy ? kDEdgeY : 0u);
            uint32_t* nl32cur = nl32 + (g & 1) * (kLeftN / 2);
            const uint16_t* nl16cur = reinterpret_cast<const uint16_t*>(nl32cur);
            if (!CROWDED && tid < kLeftN) {
                const uint32_t n = dense_nleft_cm(nfine8, tid % kLeftW, tid / kLeftW, gx, gy);
                if (n > 255u) misc[11] = 1;
                nleft8[tid] = (uint8_t)n;
            }
            if (CROWDED && !PROBE) {  // nLeft of this grid type by counting (read by verify, behind the first barrier below)
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    const uint32_t cw = code[k];
                    const uint32_t l = (aux[k] & 0x1FFu) + (cw & q_mask);
                    if ((cw & out_mask) == 0) atomicAdd(&nl32cur[l >> 1], 1u << ((l & 1u) << 4));
                }
            }
            // bands: 8 own rows + a halo row on either side (verify reads the neighbour rows); a probe needs no neighbours, so its
            // bands are as many whole rows as fit: 10 at 28 x 28 right cells, 5 at 40 x 40
            const int band_rows = PROBE ? (s == 4 && !NIB ? 5 : 10) : 8, halo = PROBE ? 0 : 1;
            const int n_bands = BANDED ? (kLeftH + band_rows - 1) / band_rows : 1;
            for (int band = 0; band < n_bands; ++band) {
                const int lo = BANDED ? band * band_rows : 0, hi = BANDED ? min(lo + band_rows, kLeftH) : kLeftH;      // own rows
                const int blo = BANDED ? max(lo - halo, 0) : 0, bhi = BANDED ? min(hi + halo, kLeftH) : kLeftH;        // rows held
                const uint32_t cell0 = (uint32_t)(blo * kLeftW), n_held = (uint32_t)((bhi - blo) * kLeftW);
                const uint32_t own0 = (uint32_t)(lo * kLeftW), n_own = (uint32_t)((hi - lo) * kLeftW);
                // arg-max keys carry (grid type, band) in their top bits: every binning pass outranks what the previous one
                // left in the headers (a cellPairs word, below 2^19), so headers are never reset inside a scale
                const uint32_t key_tag = (uint32_t)(BANDED ? g * n_bands + band : g) << kDTagShift;

                // ---- assignMatchPairs
#pragma unroll
                for (int k0 = 0; k0 < KPT; k0 += kChunk) {
                    // Whole matrix in LDS (scales 0..2): unpredicated, a match the grid type leaves out works on its lane's sink (see
                    // dense_pair_plain). Banded (scales 3, 4): most matches are outside the band -- those are skipped, not sunk.
                    uint32_t old[kChunk], at[kChunk], row[kChunk], ee[kChunk];
                    bool in[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t cw = code[k0 + c];
                        const uint32_t l = (aux[k0 + c] & 0x1FFu) + (cw & q_mask) - cell0;
                        in[c] = (cw & out_mask) == 0 && (!BANDED || l < n_held);
                        // at[c]: the entry's bit offset in its dword (bytes: 8 (E & 3); nibbles: 4 (E & 7)); rows are dword-aligned
                        if constexpr (BANDED) {
                            row[c] = __umul24(l, stride);
                            ee[c] = (cw >> kDEShift) & emask;
                            at[c] = NIB ? (ee[c] & 7u) << 2 : (ee[c] & 3u) << 3;
                            old[c] = 0;
                            if (in[c]) old[c] = ldsa_add_rtn(row[c] + (NIB ? (ee[c] >> 3) << 2 : ee[c] & ~3u), 1u << at[c]);
                        } else {
                            row[c] = in[c] ? __umul24(l, stride) : sink_at;  // (not binned under this grid type: the lane's sink, E = 0)
                            ee[c] = in[c] ? ((cw >> kDEShift) & emask) : 0u;
                            at[c] = NIB ? (ee[c] & 7u) << 2 : (ee[c] & 3u) << 3;
                            old[c] = ldsa_add_rtn(row[c] + (NIB ? (ee[c] >> 3) << 2 : ee[c] & ~3u), 1u << at[c]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t before = __builtin_amdgcn_ubfe(old[c], at[c], NIB ? 4 : 8);
                        if (CROWDED && in[c] && before == 255u) misc[12] = 1;  // the entry's byte has just wrapped
                        // (nibbles: the entry has just wrapped -> the row is dirty: the largest key of this pass, no later one replaces it)
                        const uint32_t key = (NIB && before == 15u) ? 0xFFFFFu : (before << 11) | ee[c];
                        if (!BANDED || in[c]) ldsa_max(row[c], key_tag | key);
                    }
                }
                GMS_STAMP_IN(3);  // insert
                __syncthreads();
                GMS_STAMP_IN(11);  // insert: wait for the other waves
                if (!CROWDED && misc[11] != 0) {  // a cell above 255 matches (workgroup-uniform; nothing has been written out)
                    status = 1;
                    break;
                }
                if (CROWDED && misc[12] != 0) {  // a (left cell, right cell) pair above 255 matches
                    status = 2;
                    break;
                }

                // ---- verifyCellPairs for the cells of the own rows. Without rotation: two lanes per left cell, four of the eight outer
                //      neighbour pairs each. With rotation: four lanes per cell, two of the eight rotations each over all eight pairs
                //      (the left side of a pair is shared by the lane's rotations; 1600 items instead of 3200).
                if constexpr (!PROBE) {
                    constexpr int kNR = ROT ? 2 : 1;             // rotations per lane
                    constexpr int kLanesPerCell = ROT ? 4 : 2, kCellShift = ROT ? 2 : 1;
                    const int n_items = (int)n_own * kLanesPerCell;
                    for (int item = tid; item < ((n_items + 63) & ~63); item += NT) {
                        const bool live = item < n_items;
                        const int i = (int)own0 + (live ? (item >> kCellShift) : 0);
                        const int sub = item & (kLanesPerCell - 1);
                        const int half = item & 1;  // !ROT only
                        const int ix = i % kLeftW, iy = i / kLeftW;
                        const uint32_t ni = live ? (CROWDED ? (uint32_t)nl16cur[i] : (uint32_t)nleft8[i]) : 0u;
                        if (__ballot(ni != 0) == 0ull) continue;  // none of this wave's cells has a match under this grid type
                        const uint32_t hdr = ((uint32_t)i - cell0) * (stride >> 2);
                        const uint32_t best = smem[hdr] & ((1u << kDTagShift) - 1u);
                        const uint32_t ej = ni ? (best & 0x7FFu) : nr + 3u;
                        const uint32_t j = nr + 3u - ej;
                        const int jy = (int)((j * wr_magic) >> 16), jx = (int)j - jy * (int)wr;
                        uint32_t score[kNR], tn[kNR];  // tn = (sum of nLeft << 4) | numpair
                        uint32_t rpack[kNR];           // where the lane's rotations send the eight outer neighbours (rotation_pack)
#pragma unroll
                        for (int jr = 0; jr < kNR; ++jr) {
                            score[jr] = tn[jr] = 0;
                            rpack[jr] = sub == 0 ? rotation_pack(jr) : sub == 1 ? rotation_pack(2 + jr) : sub == 2 ? rotation_pack(4 + jr) : rotation_pack(6 + jr);
                        }
#pragma unroll
                        for (int c = 0; c < (ROT ? 8 : 4); ++c) {
                            int ldx, ldy;
                            if (ROT) {
                                const int k = c < 4 ? c : c + 1;
                                ldx = (k % 3) - 1; ldy = (k / 3) - 1;
                            } else {
                                ldx = half ? ((c + 5) % 3) - 1 : (c % 3) - 1;
                                ldy = half ? ((c + 5) / 3) - 1 : (c / 3) - 1;
                            }
                            const int lx = ix + ldx, ly = iy + ldy;
                            const bool okl = ni != 0 && (uint32_t)lx < (uint32_t)kLeftW && (uint32_t)ly < (uint32_t)kLeftH;
                            const uint32_t ll = okl ? (uint32_t)(lx + ly * kLeftW) : (uint32_t)i;  // within one row of an own row: held
                            const uint32_t nll = CROWDED ? (uint32_t)nl16cur[ll] : (uint32_t)nleft8[ll];
                            const uint32_t rowb = (ll - cell0) * stride;
#pragma unroll
                            for (int jr = 0; jr < kNR; ++jr) {
                                int rdx = ldx, rdy = ldy;
                                if (ROT) {
                                    rdx = (int)((rpack[jr] >> (4 * c)) & 3u) - 1;
                                    rdy = (int)((rpack[jr] >> (4 * c + 2)) & 3u) - 1;
                                }
                                const int rx = jx + rdx, ry = jy + rdy;
                                const bool okp = okl && (uint32_t)rx < wr && (uint32_t)ry < wr;
                                const uint32_t cnt = dense8[rowb + (okp ? nr + 3u - (uint32_t)(rx + ry * (int)wr) : 4u)];
                                score[jr] += okp ? cnt : 0u;
                                tn[jr] += okp ? ((nll << 4) | 1u) : 0u;
                            }
                        }
                        uint32_t bits = 0;
                        if (!ROT) {
                            score[0] += dpp_xor1(score[0]);
                            tn[0] += dpp_xor1(tn[0]);
                        }
#pragma unroll
                        for (int jr = 0; jr < kNR; ++jr) {
                            const uint32_t sc = score[jr] + (best >> 11) + 1u, t = tn[jr] + ((ni << 4) | 1u);
                            uint32_t pass = 0;
                            if (ni != 0 && (ROT || half == 0))
                                pass = (CROWDED ? threshold_rejects(t >> 4, t & 15u, sc, p.threshold_factor, thr_fast)
                                                : dense_threshold_rejects(t >> 4, t & 15u, sc, p.threshold_factor, thr_fast, f2i)) ? 0u : 1u;
                            bits |= pass << jr;
                        }
                        if (ROT) {  // the cell's four lanes hold rotations (0,1) (2,3) (4,5) (6,7): gather the quad's bit pairs (DPP quad_perm broadcasts)
                            const uint32_t b0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0x00, 0xF, 0xF, false);
                            const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0x55, 0xF, 0xF, false);
                            const uint32_t b2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0xAA, 0xF, 0xF, false);
                            const uint32_t b3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0xFF, 0xF, 0xF, false);
                            bits = b0 | (b1 << 2) | (b2 << 4) | (b3 << 6);
                        }
                        if (ni != 0 && sub == 0) smem[hdr] = (ej << 8) | bits;
                    }
                    __syncthreads();
                }
                GMS_STAMP_IN(5);  // verify

                // ---- mark the matches of the own rows; every increment of the rows held is taken back
                {
                    if (CROWDED && !PROBE && tid < kLeftN / 2) nl32[((g + 1) & 1) * (kLeftN / 2) + tid] = 0;  // the next grid type's counters (idle now; a barrier follows)
                    uint32_t cr[KPT];
#pragma unroll
                    for (int k = 0; k < KPT; ++k) {
                        const uint32_t cw = code[k];
                        const uint32_t l = (aux[k] & 0x1FFu) + (cw & q_mask);
                        const bool in = (cw & out_mask) == 0 && (!BANDED || l - cell0 < n_held);
                        // the undo is a zero BYTE over the entry: with nibbles that clears the neighbour entry too -- every entry that was
                        // touched is cleared by somebody, nobody reads entries in this phase, all writers store the same value
                        const uint32_t ebyte = NIB ? ((cw >> kDEShift) & emask) >> 1 : (cw >> kDEShift) & emask;
                        if constexpr (BANDED) {
                            const uint32_t row = __umul24(l - cell0, stride);
                            cr[k] = PROBE ? 0x7FFu : 0xFFFFFFFFu;  // "no header" (reads as E = 2047; a probe also tests the low 20 bits for "dirty")
                            if (in) {
                                if (l - own0 < n_own) cr[k] = ldsa_ld32(row);
                                ldsa_st8(row + ebyte, 0u);  // (every reader of the entry is past the barrier: see dense_pair_rot)
                            }
                        } else {
                            const uint32_t row = in ? __umul24(l - cell0, stride) : sink_at;
                            const uint32_t at = row + (in ? ebyte : 0u);
                            cr[k] = ldsa_ld32(in ? row : (PROBE ? none_probe_at : none_at));
                            ldsa_st8(at, 0u);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < KPT; ++k) {
                        if constexpr (PROBE) {  // the header still holds the arg-max key: [tag | count - 1 | E(j*)]; (a row not owned reads as E = 2047)
                            if ((cr[k] & 0x7FFu) == ((code[k] >> kDEShift) & emask) || (NIB && (cr[k] & 0xFFFFFu) == 0xFFFFFu)) code[k] |= 1u << kSProbeBit;
                        } else {
                            const uint32_t x = cr[k] ^ (code[k] & (kSEMask << kDEShift));
                            if (x < 256u) code[k] |= x << kSAccShift;
                        }
                    }
                }
                __syncthreads();
                GMS_STAMP_IN(6);  // mark
            }
            if (status != 0) break;
        }
        if (status != 0) return status;
        // the next scale lays its rows out differently: no header of this one may survive as a count byte
        for (uint32_t c = tid; c < (uint32_t)kLeftN; c += NT)
            if (!BANDED || c < (uint32_t)((PROBE ? (s == 4 && !NIB ? 5 : 10) : 10) * kLeftW)) smem[c * (stride >> 2)] = 0;

        if constexpr (PROBE) {  // ---- how many matches could be inliers at this scale at all
            uint32_t c0 = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) c0 += (uint32_t)__popcll(__ballot((code[k] >> kSProbeBit) & 1u));
            if (lane == 0 && c0) atomicAdd(&misc[0], c0);
            __syncthreads();  // count complete; headers zeroed
            const uint32_t bound = misc[0];
#pragma unroll
            for (int k = 0; k < KPT; ++k) code[k] &= ~(1u << kSProbeBit);
            __syncthreads();
            if (tid < 8) misc[tid] = 0;
            // (a scale that comes BEFORE the best one in the reference's order would also win a tie)
            const bool can_win = bound > best_count || (bound == best_count && s < best_scale);
            if (tid == 0 && p.probe_stats != nullptr) atomicAdd(&p.probe_stats[(NIB ? 4 + 2 * s : 2 * s) + (can_win ? 0 : 1)], 1u);  // (nibble probes of scales 3, 4: words 10..13)
            GMS_STAMP_IN(7);
            return can_win ? 0 : 3;
        }
        // ---- run() return value per rotation of this scale, getInlierMask's strict '>'
        if constexpr (ROT) {
            // a thread's eight counts (at most KPT each) as byte fields of two registers: the four low rotation bits of a match times
            // 0x204081 put bit i at position 8 i (v_mul_u32_u24 + v_and instead of eight ballots per match); widened to 16-bit fields
            // for the wave's sum (row scans on the DPP path + four v_readlane), one LDS atomic per register and wave
            uint32_t a0 = 0, a1 = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                const uint32_t b = code[k] >> kSAccShift;
                a0 += __umul24(b & 15u, 0x204081u) & 0x01010101u;
                a1 += __umul24((b >> 4) & 15u, 0x204081u) & 0x01010101u;
            }
            const uint32_t w0 = wave_sum(a0 & 0x00FF00FFu), w1 = wave_sum((a0 >> 8) & 0x00FF00FFu);    // rotations (0, 2), (1, 3)
            const uint32_t w2 = wave_sum(a1 & 0x00FF00FFu), w3 = wave_sum((a1 >> 8) & 0x00FF00FFu);    // rotations (4, 6), (5, 7)
            if (lane == 0) {
                if (w0) atomicAdd(&misc[0], w0);
                if (w1) atomicAdd(&misc[1], w1);
                if (w2) atomicAdd(&misc[2], w2);
                if (w3) atomicAdd(&misc[3], w3);
            }
        } else {
            uint32_t c0 = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) c0 += (uint32_t)__popcll(__ballot((code[k] >> kSAccShift) & 1u));
            if (lane == 0 && c0) atomicAdd(&misc[0], c0);
        }
        __syncthreads();  // counts complete; headers zeroed
        // getInlierMask walks scale-outer, rotation-inner and keeps on strict '>': the first hypothesis with the largest count wins.
        // Scale 1 is evaluated before scale 0 here (below), so a count that TIES the best replaces it when this scale comes
        // before the best one's.
        int winner = -1;
#pragma unroll
        for (int r = 0; r < kNRot; ++r) {
            const uint32_t c = ROT ? (misc[(r >> 2) * 2 + (r & 1)] >> ((r & 2) << 3)) & 0xFFFFu : misc[0];
            if (c > best_count || (c == best_count && c != 0 && s < best_scale)) {
                best_count = c;
                best_scale = s;
                best_rot = r + 1;
                winner = r;
            }
        }
        if (winner >= 0) {  // the best hypothesis' inliers: one bit per match of the thread (a register -- scale 0's matrix fills the LDS)
            bestbits = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) bestbits |= ((code[k] >> (kSAccShift + winner)) & 1u) << k;
        }
#pragma unroll
        for (int k = 0; k < KPT; ++k) code[k] &= ~(0xFFu << kSAccShift);
        __syncthreads();
        if (tid < 8) misc[tid] = 0;
        GMS_STAMP_IN(7);  // count + select
        return 0;
    };

    // one scale: the probe first where the launch asks for it and there is a best count to beat
    auto eval_scale = [&](auto banded_c, auto crowded_c, const int s) -> int {
        if (((p.probe_scales >> s) & 1) != 0 && best_count > 0) {
            constexpr bool kCrowded = decltype(crowded_c)::value;
            if constexpr (!kCrowded) {
                if (s == 3 && (p.probe_nibble & 8) != 0) {  // the cheap bound first: nibble entries, the whole matrix at once
                    const int pn = run_scale(std::false_type{}, crowded_c, std::true_type{}, std::true_type{}, s);
                    GMS_STAMP_SCALE(5 + s);
                    if (pn == 3) return 0;
                    if (pn != 0) return pn;
                }
            }
            const int pr = run_scale(banded_c, crowded_c, std::true_type{}, std::false_type{}, s);
            GMS_STAMP_SCALE(5 + s);
            if (pr != 0) return pr == 3 ? 0 : pr;
        }
        const int ev = run_scale(banded_c, crowded_c, std::false_type{}, std::false_type{}, s);
        GMS_STAMP_SCALE(s);
        return ev;
    };
    // Order: scale 1 first (the 10 x 10 grid collects at least as many matches per cell pair as the 20 x 20 one and usually has the
    // largest count), then 0, 2, 3: whichever comes first sets the count the probes of the others are measured against, so with the
    // usual winner first scale 0 can be bounded out as well.
    int status = spilled ? 1 : 0;
    bool crowded_mode = false;
    for (int i = 0; i < 3 && status == 0; ++i) status = eval_scale(std::false_type{}, std::false_type{}, i == 0 ? 1 : (i == 1 ? 0 : 2));
    if (status == 0) status = eval_scale(std::true_type{}, std::false_type{}, 3);
    if (status == 1) {
        crowded_mode = true;
        // crowded (dense_pair_rot has the same mode): everything again on a clean matrix, nLeft counted into 16-bit counters and
        // every returned entry count checked; the cell populations do not depend on the scale, so this shows at the first scale
        __syncthreads();
        {
            const uint4 z4 = make_uint4(0, 0, 0, 0);
            uint4* d4 = reinterpret_cast<uint4*>(smem);
            for (uint32_t i = tid; i < kDenseBytes / 16; i += NT) d4[i] = z4;
            if (tid < kLeftN) nl32[tid] = 0;
            if (tid < 8) misc[tid] = 0;
        }
#pragma unroll
        for (int k = 0; k < KPT; ++k) code[k] &= ~(0xFFu << kSAccShift);
        best_count = bestbits = 0;
        best_scale = best_rot = -1;
        __syncthreads();
        status = 0;
        for (int i = 0; i < 3 && status == 0; ++i) status = eval_scale(std::false_type{}, std::true_type{}, i == 0 ? 1 : (i == 1 ? 0 : 2));
        if (status == 0) status = eval_scale(std::true_type{}, std::true_type{}, 3);
    }
    // Scale 4 (40 x 40: 400 rows of 1604 bytes) is the hashed kernel's to evaluate -- but its probe runs here, on four bands of the
    // byte matrix: when it bounds the scale out, the record says all five scales are decided and the hashed kernel only copies out;
    // when it does not, the record says so and the hashed kernel does not probe again.
    uint32_t decided = 4u;
    if (status == 0 && ((p.probe_scales >> 4) & 1) != 0 && best_count > 0 && p.right_w[4] == 40 && p.right_h[4] == 40) {
        int pr = 0;
        if (crowded_mode) {
            pr = run_scale(std::true_type{}, std::true_type{}, std::true_type{}, std::false_type{}, 4);
        } else {
            // the cheap bound first (nibble entries: two bands instead of four); when it cannot bound the scale out, the exact one
            if ((p.probe_nibble & 16) != 0) pr = run_scale(std::true_type{}, std::false_type{}, std::true_type{}, std::true_type{}, 4);
            if ((p.probe_nibble & 16) == 0 || pr == 0) pr = run_scale(std::true_type{}, std::false_type{}, std::true_type{}, std::false_type{}, 4);
        }
        GMS_STAMP_SCALE(9);
        if (pr == 3) decided = 5u;
        else if (pr == 0) decided = 4u | 16u;
        else status = pr;
    }
    if (status != 0) {
        __syncthreads();
        return false;
    }
    __syncthreads();
    if (decided == 5u) {  // (workgroup-uniform) nothing is left for the hashed kernel but the copy-out: done here, its workgroup returns at once
        if (tid == 0) part[0] = 6u;
        scales_copy_out<KPT, NT>(p.pairs, p.matches, p.out, p.mask, p.results, smem, pair_idx, bestbits, dealt ? 1 : 0, best_count, best_scale, best_rot);
        GMS_STAMP_OUT(9, 11);
        GMS_STAMP_FLUSH;
        return true;
    }
    // the record the hashed kernel continues from: scales 0..3 (or all five) are decided
    if (tid == 0) {
        part[0] = decided;
        part[1] = best_count;
        part[2] = (uint32_t)best_scale;
        part[3] = (uint32_t)best_rot;
    }
    // the inlier bit of every match, as a bit mask over the list (bit i & 31 of dword i >> 5). List order: slot k of a wave is one chunk of
    // 64 consecutive matches = one ballot. Dealt: an 8-lane group holds eight consecutive matches = one byte of the mask.
    if (dealt) {
        uint8_t* mask8 = reinterpret_cast<uint8_t*>(part + kPartialHeaderDw);
        // (the lane's first match worked out again from a thread index the compiler cannot connect with the one above: kept alive
        //  from the loads to here, it would cost a register through every scale)
        int t2 = (int)threadIdx.x;
        asm volatile("" : "+v"(t2));
        const int l2 = t2 & 63, base2 = (((l2 >> 3) * (KPT * (NT / 64)) + (t2 >> 6)) << 3) | (l2 & 7);
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const unsigned long long bsel = __ballot((bestbits >> k) & 1u);
            if ((l2 & 7) == 0) mask8[(base2 + k * (NT / 64) * 8) >> 3] = (uint8_t)(bsel >> l2);
        }
    } else {
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const unsigned long long bsel = __ballot((bestbits >> k) & 1u);
            if (lane == 0) {
                const int ch = k * (NT / 64) + wave;
                part[kPartialHeaderDw + 2 * ch] = (uint32_t)bsel;
                part[kPartialHeaderDw + 2 * ch + 1] = (uint32_t)(bsel >> 32);
            }
        }
    }
    GMS_STAMP_OUT(9, 11);  // record written
    GMS_STAMP_FLUSH;
    return true;
}

template <int KPT, bool ROT, int NT>
__global__ void __launch_bounds__(NT)
filter_kernel_dense_scales(FilterParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    first_round_stagger(p);
    uint32_t* part = p.partial + (size_t)blockIdx.x * kPartialStrideDw;
    if (!dense_scales_pair<KPT, ROT, NT>(p, smem, (int)blockIdx.x, (int)threadIdx.x, part)) {
        if (threadIdx.x == 0) part[0] = 0u;  // the hashed kernel evaluates all five scales
    }
}

// Scale hypotheses: scales 0..3 on the byte matrix (records in p.partial), then the hashed kernel for scale 4 and
// for everything the first kernel could not take. p.partial: n_pairs * kPartialStrideDw dwords.
hipError_t launch_filter_scales(const FilterParams& p, int kpt, int n_pairs, hipStream_t stream)
{
    if (n_pairs <= 0) return hipSuccess;
    const hipError_t e = dispatch_kpt_rot(kpt, p.with_rotation != 0, [&](auto k, auto rot) {
        hipLaunchKernelGGL((filter_kernel_dense_scales<decltype(k)::value, decltype(rot)::value, kThreads>), dim3((unsigned)n_pairs), dim3(kThreads), kDenseLdsBytes, stream, p);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    FilterParams q = p;
    q.dense = 0;
    return launch_filter(q, kpt, n_pairs, stream);
}

hipError_t init_scales_kernels()
{
    return for_each_kpt_rot([](auto k, auto rot) { return allow_full_lds(filter_kernel_dense_scales<decltype(k)::value, decltype(rot)::value, kThreads>); });
}

}  // namespace gms
