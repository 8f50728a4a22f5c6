// gms_kernel_dense.hip -- filter_kernel_dense: the byte-matrix form of the GMS filter without scale hypotheses (overview:
// gms_kernels.hip; the matrix and its LDS layout: gms_kernel_dense.h). Two per-pair bodies -- dense_pair_plain() for the
// reference's default flags (the headline workload) and dense_pair_rot() with rotation hypotheses --, the kernel that runs one of
// them and hands the pairs it cannot take to hash_pair() (gms_kernel_hash.h), its launch and its dynamic-LDS limits.
// The end of a pair in dense_pair_plain: the last grid type takes no increments back (nothing reads the matrix behind its
// verification), the verifying lanes store their verdicts straight into the mark table over those bytes, one barrier, and every
// match reads the one entry of its left half cell.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gms_kernel_dense.h"
#include "gms_kernel_hash.h"

namespace gms {

// dense_pair_rot: the byte-matrix path WITH rotation hypotheses (the matrix, its rows and the code word: gms_kernel_dense.h). All
// eight rotations share one binning pass per grid type; verification takes one lane per (cell, rotation).
// false (workgroup-uniform, nothing written to global memory): the pair has to take the general path
template <int KPT, int NT, bool DEALT>
__device__ __forceinline__ bool dense_pair_rot(const FilterParams& p, uint32_t* smem, const int pair_idx, const int tid)
{
    constexpr int kMcap = KPT * NT;
    constexpr int kNRot = 8;
    constexpr int kChunk = (KPT % 5 == 0) ? 5 : 4;
    static_assert(KPT % kChunk == 0, "KPT must be a multiple of the chunk");
    const int lane = tid & 63;
    const int wave = tid >> 6;
    // Which match a lane's k-th record is. Normally a wave instruction takes 64 consecutive matches (k * NT + tid). Inputs in
    // spatial order (a detector scanning rows, a per-pixel grid) make consecutive matches share their (left cell, right cell)
    // entry, and 64 of them in one LDS atomic instruction serialise on one address (1.7x slower on cell-sorted keypoints, DESIGN.md
    // section 6). When the context's recent launches looked like that (order_probe_kernel; the host picks this instantiation), the
    // matches are DEALT instead: the wave's eight 8-lane groups take 8 consecutive matches (one 128-byte line of the match array) from eight places
    // KPT * 128 matches apart. Loads stay whole lines either way; the copy-out below orders 8-match units, which both mappings are
    // made of. Speed only: either mapping gives the same result.
    constexpr int kUnitsPerBlock = KPT * (NT / 64);   // dealt: unit (g, k, wave) = g * this + k * 16 + wave for lane group g
    constexpr bool dealt = DEALT;
    // either way match k of a lane is base + k * stride: (tid, NT) in list order, (its group's first unit, 128) when dealt
    const int m_base = dealt ? ((((lane >> 3) * kUnitsPerBlock + wave) << 3) | (lane & 7)) : tid;
    const int m_stride = dealt ? (NT / 64) * 8 : NT;
    auto match_of = [&](int k) -> int { return m_base + k * m_stride; };

    int64_t total_kp;
    const gms_pair pr = load_pair(p.pairs, pair_idx, p, total_kp);  // (and the frame table's header word)
    const int m = pr.m;
    if (p.with_scale || p.right_w[0] != kDenseRightW || p.right_h[0] != kDenseRightW || m <= 0 || m > kMcap ||
        pr.frame_a < 0 || pr.frame_a >= p.n_frames || pr.frame_b < 0 || pr.frame_b >= p.n_frames)
        return false;
    int64_t offA, offB;
    int nA, nB;
    load_frame_ranges(p.frame_off, pr.frame_a, pr.frame_b, offA, nA, offB, nB);
    if (nA <= 0 || nB <= 0) return false;
    const gms_dmatch* __restrict__ matches = p.matches + pr.match_off;
    // the frame table's code words (written by normalize_kernel behind the points): frame A's left codes, frame B's right codes
    if (total_kp < 0 || offA + nA > total_kp || offB + nB > total_kp) return false;  // (workgroup-uniform) no header, or frames beyond the table
    const uint16_t* __restrict__ lcodeA = reinterpret_cast<const uint16_t*>(p.pts + total_kp) + offA;
    const uint16_t* __restrict__ rcodeB = reinterpret_cast<const uint16_t*>(p.pts + total_kp) + total_kp + offB;

    const uint8_t* dense8 = reinterpret_cast<const uint8_t*>(smem);
    uint32_t* nfine32 = smem + kDenseFineOff / 4;   // half-cell histogram: one dword per cell of grid type 1, a byte per half cell
    const uint8_t* nfine8 = reinterpret_cast<const uint8_t*>(nfine32);
    uint8_t* nleft8 = reinterpret_cast<uint8_t*>(smem) + kDenseNleftOff;
    uint32_t* misc = smem + kDenseMiscOff / 4;
    uint32_t* trash = smem + kDenseTrashOff / 4;

    GMS_STAMP_DECL
#ifdef GMS_PHASE_TIMING
    ph_[14] = wall_clock64();  // absolute start of this workgroup (100 MHz), for the dispatch-phase histogram
#endif
    if (tid < 32) misc[tid] = 0;
    if (tid < 16) trash[tid] = 0;
    if (tid < kFineN / 4) nfine32[tid] = 0;

    // ---- both frames' code words staged in the still unused matrix area (coalesced 16-byte loads from 16-byte aligned addresses:
    //      a frame starts anywhere in the table, so the copy keeps the source's phase and look-ups add it), then the pair's DMatch
    //      records, whole (they stay in registers until copy-out). Loads return in order: the staged codes are complete -- and the
    //      barrier passed -- while the later records are still on their way.
    const uint32_t phA = (uint32_t)(reinterpret_cast<uintptr_t>(lcodeA) >> 1) & 7u, phB = (uint32_t)(reinterpret_cast<uintptr_t>(rcodeB) >> 1) & 7u;
    const uint32_t qA = (phA + (uint32_t)nA + 7u) >> 3, qB = (phB + (uint32_t)nB + 7u) >> 3;  // uint4s of either copy (8 codes each)
    const bool staged = (qA + qB) * 16u <= kDenseBytes;  // workgroup-uniform: both fit (40 400 keypoints a frame, say)
    const uint4* __restrict__ srcA = reinterpret_cast<const uint4*>(lcodeA - phA);
    const uint4* __restrict__ srcB = reinterpret_cast<const uint4*>(rcodeB - phB);
    constexpr int kStageRegs = 3;  // 48 KB of codes (12 288 keypoints a frame) through registers; larger frames finish in a plain loop
    uint4 tb[kStageRegs];
#pragma unroll
    for (int i = 0; i < kStageRegs; ++i) {  // (unconditional: a pair too large to stage just reads a few code words it does not use)
        const uint32_t j = min((uint32_t)(i * NT + tid), qA + qB - 1u);
        const uint4* src = j < qA ? srcA + j : srcB + (j - qA);  // one load either way: select the address, not the data
        tb[i] = *src;
    }
    // Up to 10 matches per thread the whole 16-byte records stay in registers until copy-out (the match array is read
    // once); at 16 per thread that would be 64 registers of a 128-register budget, so there only (queryIdx, trainIdx)
    // are loaded here and the survivors' records are read again at copy-out.
    constexpr bool kKeepRec = KPT <= 10;
    uint4 rec[kKeepRec ? KPT : 1];
    uint2 qt[kKeepRec ? 1 : KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        if (kKeepRec) rec[k] = *reinterpret_cast<const uint4*>(&matches[min(match_of(k), m - 1)]);
        else qt[k] = *reinterpret_cast<const uint2*>(&matches[min(match_of(k), m - 1)]);
    }
    auto query_of = [&](int k) -> uint32_t { return kKeepRec ? rec[k].x : qt[k].x; };
    auto train_of = [&](int k) -> uint32_t { return kKeepRec ? rec[k].y : qt[k].y; };
    // motion.setTo(0) for the part of the matrix area that the staged codes do not occupy: now, while the loads are in flight
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
    const uint16_t* ldsB = reinterpret_cast<const uint16_t*>(smem + 4u * qA) + phB;  // right code of frame B's keypoint t at ldsB[t]
    __syncthreads();
#ifdef GMS_PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GMS_STAMP(4);  // bin: records landed, codes staged
    ph_[15] = wall_clock64();
#endif

    // row1 = byte offset of the left cell's row under grid type 1: a register of its own beside the code word
    uint32_t code[KPT], row1[KPT];
    auto row_of = [&](int k, uint32_t cw, uint32_t q_mask) -> uint32_t { return __umul24(cw & q_mask, kDenseRow) + row1[k]; };
    {
        uint32_t ca[KPT], cb[KPT];
        if (staged) {
#pragma unroll
            for (int k = 0; k < KPT; ++k) ca[k] = ldsA[min(query_of(k), (uint32_t)(nA - 1))];
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = ldsB[min(train_of(k), (uint32_t)(nB - 1))];
        } else {  // frames too large to stage: both gathers go to global memory
#pragma unroll
            for (int k = 0; k < KPT; ++k) ca[k] = lcodeA[min(query_of(k), (uint32_t)(nA - 1))];
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = rcodeB[min(train_of(k), (uint32_t)(nB - 1))];
        }
#ifdef GMS_PHASE_TIMING
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        GMS_STAMP(12);  // bin: gathers landed
#endif
        bool any_bad = false, spill = false;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const bool live = match_of(k) < m;
            const uint32_t e0 = cb[k] & kDEMask;  // E(r) of getGridIndexRight on the 20 x 20 grid, 0 = outside it (no bounds test in the reference)
            // parity domain: indices in range, both points inside it, the right cell inside its grid ('&', not '&&': no branches)
            const uint32_t cell = ca[k] >> kLCellShift;  // under grid type 1; kLCellNever / kLCellBad above the grid
            const bool ok = ((int)(query_of(k) < (uint32_t)nA) & (int)(train_of(k) < (uint32_t)nB) & (int)(cell != kLCellBad) & (int)((cb[k] & kRCodeBad) == 0u) & (int)(e0 != 0u)) != 0;
            const bool binned = live & ok & (cell < kLCellNever);
            // half-cell histogram: dword = the cell under grid type 1, byte = (hx & 1) + 2 (hy & 1); q = (hx & 1) + 20 (hy & 1)
            const uint32_t sh = ((ca[k] & 1u) << 3) | ((ca[k] & 4u) << 2);
            const uint32_t old = atomicAdd(binned ? &nfine32[cell] : &trash[lane & 7], 1u << sh);
            spill |= binned & (((old >> sh) & 255u) == 255u);  // the byte wrapped: > 255 in one half cell
            any_bad |= live & !ok;
            // the dense code word: q as it stands, the edge bits one place up, E(r)
            const uint32_t cw = (ca[k] & 31u) | ((ca[k] & 0x60u) << 1) | (e0 << kDEShift);
            code[k] = binned ? cw : kDNever;
            row1[k] = binned ? __umul24(cell, kDenseRow) : 0u;
        }
        if (any_bad) misc[8] = 1;   // benign races: every writer stores 1
        if (spill) misc[13] = 1;  // (its own flag: misc[11] is written again while slower waves may still be reading this one)
    }
    GMS_STAMP(13);    // bin: codes + half-cell histogram
    __syncthreads();  // histogram complete; every read of the staged frame is done
    GMS_STAMP(0);     // bin: wait for the other waves

    // ---- motion.setTo(0), once: from here on every grid type leaves the matrix as it found it. The row headers are
    //      never reset either: a grid type's arg-max keys carry the type in their top bits, so they outrank
    //      whatever the previous type left there (its cellPairs word, which is below 2^17).
    {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        uint4* d4 = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < staged16; i += NT) d4[i] = z4;  // the rest was cleared while the records were loading
    }
    __syncthreads();
    GMS_STAMP(2);  // clear
    if (misc[8] != 0) {    // an input outside the parity domain (workgroup-uniform; nothing has been written to global memory yet)
        __syncthreads();   // everybody has read the flag before the general path reuses the LDS
        return false;
    }
    const bool spilled = misc[13] != 0;  // a half cell above 255 matches: straight to the crowded mode below

    const bool thr_fast = threshold_fast_ok(p.threshold_factor);
    const uint32_t f2i = dense_factor_sq(p.threshold_factor);
    uint32_t* nl32 = nfine32;  // crowded mode: nLeft as 16-bit counters, two buffers of 400 (one per parity of the grid type)
    auto cell_of = [&](int k, uint32_t cw, uint32_t q_mask) -> uint32_t {
        return (((__umul24(cw & q_mask, kDenseRow) + row1[k]) >> 2) * 649u) >> 16;  // row / 404 for rows below 400
    };

    // The four grid types. CROWDED = some left cell holds more than 255 matches: a matrix entry still only overflows its byte
    // when ONE (left cell, right cell) pair collects more than 255, which crowded scenes rarely do -- so the same byte matrix
    // is used, with nLeft counted per grid type into 16-bit counters (one more LDS atomic per match, over the then useless
    // half-cell histogram) and every returned count checked. Returns 0 = done, 1 = a cell above 255 matches (run again
    // CROWDED), 2 = a matrix entry at its limit (the general path takes the pair).
    auto run_types = [&](auto crowded_c) -> int {
    constexpr bool CROWDED = decltype(crowded_c)::value;
    for (int g = 0; g < 4; ++g) {
        const int gx = g & 1, gy = g >> 1;
        const uint32_t q_mask = (uint32_t)(gx + 20 * gy);                                 // l = l1 + (q & q_mask)
        const uint32_t out_mask = kDNever | (gx ? kDEdgeX : 0u) | (gy ? kDEdgeY : 0u);    // x >= 20 || y >= 20 -> -1 (DLL@0x180047d3d)
        const uint32_t key_tag = (uint32_t)g << kDTagShift;
        uint32_t* nl32cur = nl32 + (g & 1) * (kLeftN / 2);
        const uint16_t* nl16cur = reinterpret_cast<const uint16_t*>(nl32cur);
        if (!CROWDED && tid < kLeftN) {
            // nLeft of this grid type, once per cell (read by verify, behind the next barrier); above 255 a row's entries
            // are no longer guaranteed to fit their bytes
            const uint32_t n = dense_nleft_cm(nfine8, tid % kLeftW, tid / kLeftW, gx, gy);
            if (n > 255u) misc[11] = 1;
            nleft8[tid] = (uint8_t)n;
        }

        // ---- assignMatchPairs: motion[l][r]++ on the byte; the count it produced goes into the row's arg-max
#pragma unroll
        for (int k0 = 0; k0 < KPT; k0 += kChunk) {
            uint32_t old[kChunk], at[kChunk], row[kChunk];
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                const uint32_t cw = code[k0 + c];
                row[c] = row_of(k0 + c, cw, q_mask);
                at[c] = row[c] + ((cw >> kDEShift) & kDEMask);
                old[c] = 0;
                // shift counts are taken modulo 32: at << 3 selects the byte (at & 3)
                if ((cw & out_mask) == 0) {
                    old[c] = atomicAdd(lds_at(smem, at[c] & ~3u), 1u << ((at[c] << 3) & 31u));
                    if (CROWDED) {
                        const uint32_t l = cell_of(k0 + c, cw, q_mask);
                        atomicAdd(&nl32cur[l >> 1], 1u << ((l & 1u) << 4));
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // all of the chunk's atomics are issued before any result is read
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                const uint32_t cw = code[k0 + c];
                const uint32_t before = (old[c] >> ((at[c] << 3) & 31u)) & 255u;  // <= 254, or ...
                if (CROWDED && (cw & out_mask) == 0 && before == 255u) misc[12] = 1;  // ... the entry's byte has just wrapped
                if ((cw & out_mask) == 0) atomicMax(lds_at(smem, row[c]), key_tag | (before << 11) | ((cw >> kDEShift) & kDEMask));
            }
        }
        GMS_STAMP(3);  // insert
        __syncthreads();
        GMS_STAMP(11);  // insert: wait for the other waves
        if (!CROWDED && misc[11] != 0) return 1;  // a cell above 255 matches under this grid type (workgroup-uniform)
        if (CROWDED && misc[12] != 0) return 2;   // a (left cell, right cell) pair above 255 matches

        // ---- verifyCellPairs: one lane per (cell, rotation), all eight outer neighbour pairs each
        {
            constexpr int kItems = kLeftN * 8;
            for (int item = tid; item < ((kItems + 63) & ~63); item += NT) {
                const bool live = item < kItems;
                const int i = live ? (item >> 3) : 0;
                const int rot = item & 7;
                const int ix = i % kLeftW, iy = i / kLeftW;
                const uint32_t ni = live ? (CROWDED ? (uint32_t)nl16cur[i] : (uint32_t)nleft8[i]) : 0u;
                if (__ballot(ni != 0) == 0ull) continue;  // none of this wave's cells has a match under this grid type
                const uint32_t best = smem[i * (kDenseRow / 4)] & ((1u << kDTagShift) - 1u);  // ((max count - 1) << 11) | E(j*), lowest j* among maxima
                const uint32_t ej = ni ? (best & kDEMask) : (uint32_t)(kDenseRightN + 3);
                const int j = kDenseRightN + 3 - (int)ej;
                const int jx = j % kDenseRightW, jy = j / kDenseRightW;
                uint32_t score = 0, tn = 0;  // tn = (sum of nLeft << 4) | numpair
#pragma unroll
                for (int h = 0; h < 8; h += 4) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int k8 = h + c;
                        const int k = k8 < 4 ? k8 : k8 + 1;
                        constexpr int kRingIndex[9] = {0, 1, 2, 7, -1, 3, 6, 5, 4};  // position -> ring index
                        const int q = rotated_position(rot, kRingIndex[k]);
                        const int ldx = (k % 3) - 1, ldy = (k / 3) - 1;
                        const int rdx = position_dx(q), rdy = position_dy(q);
                        const int lx = ix + ldx, ly = iy + ldy;
                        const int rx = jx + rdx, ry = jy + rdy;
                        const bool okl = ni != 0 && (uint32_t)lx < (uint32_t)kLeftW && (uint32_t)ly < (uint32_t)kLeftH;  // ll != -1
                        const bool okp = okl && (uint32_t)rx < (uint32_t)kDenseRightW && (uint32_t)ry < (uint32_t)kDenseRightW;  // rr != -1
                        const uint32_t ll = okl ? (uint32_t)(lx + ly * kLeftW) : 0u;
                        const uint32_t nll = CROWDED ? (uint32_t)nl16cur[ll] : (uint32_t)nleft8[ll];
                        const uint32_t cnt = dense8[ll * kDenseRow + (okp ? (uint32_t)(kDenseRightN + 3 - (rx + ry * kDenseRightW)) : 4u)];
                        score += okp ? cnt : 0u;
                        tn += okp ? ((nll << 4) | 1u) : 0u;
                    }
                }
                score += (best >> 11) + 1u;  // centre pair (k = 4): ll = i, rr = j*, the arg-max count itself
                tn += (ni << 4) | 1u;
                uint32_t pass = 0;
                if (ni != 0)
                    pass = (CROWDED ? threshold_rejects(tn >> 4, tn & 15u, score, p.threshold_factor, thr_fast)
                                    : dense_threshold_rejects(tn >> 4, tn & 15u, score, p.threshold_factor, thr_fast, f2i)) ? 0u : 1u;
                const unsigned long long bal = __ballot(pass);
                const uint32_t bits = (uint32_t)(bal >> (lane & 56)) & 0xFFu;  // the cell's eight lanes: its eight rotations
                // every lane of the cell has read the header above (same wave, program order): it now holds cellPairs[i]
                if (ni != 0 && (lane & 7) == 0) smem[i * (kDenseRow / 4)] = (ej << 8) | bits;
            }
        }
        __syncthreads();
        GMS_STAMP(5);  // verify

        // ---- mark inliers: cellPairs[l] == r, all rotations at once; and take this grid type's increments back
        {
            uint32_t cr[KPT];
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                const uint32_t cw = code[k];
                const uint32_t row = row_of(k, cw, q_mask);
                cr[k] = 0xFFFFFFFFu;
                if ((cw & out_mask) == 0) {
                    cr[k] = smem[row >> 2];
                    if (g < 3) {
                        const uint32_t at = row + ((cw >> kDEShift) & kDEMask);
                        // every reader of the entry is past the barrier: all its matches store the same zero (a plain byte store,
                        // no read-modify-write in the LDS)
                        reinterpret_cast<uint8_t*>(smem)[at] = 0;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                const uint32_t x = cr[k] ^ (code[k] & (kDEMask << kDEShift));  // < 256: same right cell, x = rotation bits
                if (x < 256u) code[k] |= x << kDAccShift;
            }
        }
        if (CROWDED && tid < kLeftN / 2) nl32[((g + 1) & 1) * (kLeftN / 2) + tid] = 0;  // the next grid type's counters (last read two barriers ago)
        __syncthreads();  // the next grid type writes the headers; after the last one the matrix area is reused below
        GMS_STAMP(6);  // mark
    }
    return 0;
    };

    int status = 1;
    if (!spilled) status = run_types(std::false_type{});
    if (status == 1) {
        // crowded: start over on a clean matrix (the abandoned grid type's bytes may have wrapped), no inlier bits yet
        __syncthreads();
        {
            const uint4 z4 = make_uint4(0, 0, 0, 0);
            uint4* d4 = reinterpret_cast<uint4*>(smem);
            for (uint32_t i = tid; i < kDenseBytes / 16; i += NT) d4[i] = z4;
            if (tid < kLeftN) nl32[tid] = 0;
            if (tid == 0) misc[11] = 0;
        }
#pragma unroll
        for (int k = 0; k < KPT; ++k) code[k] &= ~(0xFFu << kDAccShift);
        __syncthreads();
        status = run_types(std::true_type{});
    }
    if (status != 0) {
        __syncthreads();  // everybody has read the flags before the general path reuses the LDS
        return false;
    }


    // ---- run() return value per rotation and getInlierMask's strict '>' over the rotations (one scale)
    int winner = -1;
    {
        uint32_t cnt[kNRot];
#pragma unroll
        for (int r = 0; r < kNRot; ++r) cnt[r] = 0;
#pragma unroll
        for (int k = 0; k < KPT; ++k)
#pragma unroll
            for (int r = 0; r < kNRot; ++r)
                cnt[r] += (uint32_t)__popcll(__ballot((code[k] >> (kDAccShift + r)) & 1u));
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < kNRot; ++r)
                if (cnt[r]) atomicAdd(&misc[r], cnt[r]);
        }
        __syncthreads();
        uint32_t best_count = 0;
#pragma unroll
        for (int r = 0; r < kNRot; ++r) {
            const uint32_t c = misc[r];
            if (c > best_count) {
                best_count = c;
                winner = r;
            }
        }
    }
    GMS_STAMP(7);  // count + select

    // ---- copy-out: surviving DMatch verbatim, in input order (DLL@0x180048340), from the registers.
    constexpr int kWaves = NT / 64;
    uint32_t* cnt_tab = smem;  // in the matrix area
    unsigned long long keep[KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) keep[k] = winner >= 0 ? __ballot((code[k] >> (kDAccShift + max(winner, 0))) & 1u) : 0ull;
    gms_dmatch* __restrict__ out = p.out + pr.match_off;
    uint8_t* mask_out = p.mask ? p.mask + pr.match_off : nullptr;
    uint32_t total = 0;
    if (!dealt) {
        // A chunk is 64 consecutive matches = one wave's k-th record; chunk (k, wave) sits at position k * 16 + wave of the order.
        // Every wave publishes its KPT popcounts, then scans all KPT * 16 of them itself (one barrier, no further exchange).
        constexpr int kScanRegs = (KPT * kWaves + 63) / 64;
#pragma unroll
        for (int k = 0; k < KPT; ++k)
            if (lane == 0) cnt_tab[k * kWaves + wave] = (uint32_t)__popcll(keep[k]);
        __syncthreads();
        uint32_t excl[kScanRegs];
#pragma unroll
        for (int v = 0; v < kScanRegs; ++v) {
            const int idx = v * 64 + lane;
            const uint32_t c = idx < KPT * kWaves ? cnt_tab[idx] : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            excl[v] = total + incl - c;
            total += __shfl(incl, 63);
        }
        GMS_STAMP(8);  // out scan
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int i = k * NT + tid;
            const int ch = k * kWaves + wave;                      // wave-uniform
            static_assert(64 % kWaves == 0, "a wave's chunk never straddles two scan registers");
            const uint32_t base = __shfl(excl[(k * kWaves) >> 6], ch & 63);
            if (i < m) {
                const bool in = (keep[k] >> lane) & 1ull;
                if (mask_out) mask_out[i] = in ? 1 : 0;
                if (in) {
                    const uint32_t pos = base + (uint32_t)__popcll(keep[k] & ((1ull << lane) - 1ull));
                    *reinterpret_cast<uint4*>(&out[pos]) = kKeepRec ? rec[k] : *reinterpret_cast<const uint4*>(&matches[i]);
                }
            }
        }
    } else {
        // Dealt matches: the order is that of the 8-match units (see match_of). Every 8-lane group publishes the popcount of its
        // byte of the wave's ballot, the workgroup scans the KPT * 128 counts (two per thread, two more barriers), and a lane's slot
        // is its unit's base plus its rank in the byte.
        constexpr int kUnits = KPT * NT / 8;
        static_assert(kUnits <= 2 * NT, "two scan entries per thread");
        uint32_t* wave_tot = misc + 16;
#pragma unroll
        for (int k = 0; k < KPT; ++k)
            if ((lane & 7) == 0) cnt_tab[match_of(k) >> 3] = (uint32_t)__popc((uint32_t)(keep[k] >> (lane & 56)) & 0xFFu);
        __syncthreads();
        {
            const uint32_t c0 = 2 * tid < kUnits ? cnt_tab[2 * tid] : 0u, c1 = 2 * tid + 1 < kUnits ? cnt_tab[2 * tid + 1] : 0u;
            uint32_t incl = c0 + c1;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) wave_tot[wave] = incl;
            __syncthreads();
            uint32_t off = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const uint32_t tw = wave_tot[w];
                off += w < wave ? tw : 0u;
                total += tw;
            }
            if (2 * tid < kUnits) cnt_tab[2 * tid] = off + incl - c0 - c1;
            if (2 * tid + 1 < kUnits) cnt_tab[2 * tid + 1] = off + incl - c1;
        }
        __syncthreads();
        GMS_STAMP(8);  // out scan
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const int i = match_of(k);
            if (i < m) {
                const uint32_t byte = (uint32_t)(keep[k] >> (lane & 56)) & 0xFFu;  // the unit's survivors
                const bool in = (byte >> (lane & 7)) & 1u;
                if (mask_out) mask_out[i] = in ? 1 : 0;
                if (in) {
                    const uint32_t pos = cnt_tab[i >> 3] + (uint32_t)__popc(byte & ((1u << (lane & 7)) - 1u));
                    *reinterpret_cast<uint4*>(&out[pos]) = kKeepRec ? rec[k] : *reinterpret_cast<const uint4*>(&matches[i]);
                }
            }
        }
    }
    GMS_STAMP(9);  // copy-out
    GMS_STAMP_FLUSH;
    if (tid == 0) {
        gms_pair_result r;
        r.n_inliers = (int)total;
        r.best_scale = total ? 0 : -1;
        r.best_rot = total ? winner + 1 : -1;
        r.status = GMS_OK;
        p.results[pair_idx] = r;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------
// dense_pair_plain: the byte-matrix path WITHOUT rotation hypotheses (the reference's default flags, DisparityUtil.cpp:149,299 --
// the headline workload), written around the instruction count: the kernel is bound by vector-instruction issue (DESIGN.md
// section 6, which also has the figures of the body this one replaced). Same matrix, same phases and same results as
// dense_pair_rot; what differs:
//   * the code word is [entry under grid type 1 = 404 * cell + E : 18 | E : 9 | q and the two edge bits : 5]: the entry under
//     grid type g is one and + one shift + one multiply-add away, the row header is "entry - E";
//   * nothing is predicated: a match that is not binned under the current grid type (never, or in the last half cell of a shifted
//     axis) swaps its code word for the lane's SINK word -- an entry in the 64 spare bytes behind the matrix -- and runs the same
//     instructions as everybody else (no exec masks, no branches around the LDS atomics);
//   * LDS is addressed by absolute byte offsets (the dynamic segment starts at 0 in these kernels): no "+ base" per access;
//   * inliers are marked once per pair, not once per grid type: the verifying lanes keep cellPairs of all four grid types in a
//     register, and behind the last one a table of the 1600 left half cells x 4 grid types is built in the free matrix area; a
//     match reads the one entry of its half cell and compares four fields with its E (the mark table: gms_kernel_dense.h);
//   * verification: the eight neighbour pairs of a cell are base + s * 403 * d for d in {-21, -20, -19, -1} and s = +-1 (the two
//     lanes of a cell), their validity three compares per axis; an invalid pair reads a byte that is always zero.
// ------------------------------------------------------------------------------------------------
// plain code word
constexpr uint32_t kPEdgeX = 1u << 1, kPEdgeY = 1u << 3;  // in the gaps of q = (hx & 1) + 20 (hy & 1) (bits 0, 2, 4)
constexpr int kPEShift = 5;                                // bits 5..13  E(r); 0 = the sink word (binned nowhere)
constexpr int kPAtShift = 14;                              // bits 14..31 byte offset of the entry under grid type 1: 404 * cell + E
static_assert(kDenseLdsBytes < (1u << 18), "an entry offset is 18 bits");
// byte 3 of a row header is zero at all times (arg-max keys end at bit 21, cellPairs words at bit 8)
constexpr uint32_t kPZeroByte = 3u;

// What dense_pair_plain returns (workgroup-uniform; unless kPairDone nothing has been written to global memory and the LDS is free)
constexpr int kPairGeneral = 0;   // the pair has to take the general path
constexpr int kPairDone = 1;
constexpr int kPairNotIdent = 2;  // IDENT only: not an identity-query pair of a frame whose side record is current

// IDENT: the instantiation for identity-query pairs -- match k of the list is query k and the list has one match per keypoint of
// frame A (what a brute-force matcher without cross-check returns; the host picks the instantiation from what order_probe_kernel
// saw). For such a pair the left half of the binning phase does not depend on the pair: the left code of match k is lcode[k] of
// frame A, a coalesced global load requested at the top beside the records instead of a staged copy and an LDS gather, and the
// half-cell histogram is the frame's own, built once per frame by side_records_kernel (gms_kernels.hip) and copied in here
// (1.6 KB) instead of one returning LDS atomic per match. Only frame B's right codes are staged. Everything is checked per
// pair -- every thread its own matches' queryIdx, the workgroup m == nA, the table's stamp against the side record's,
// the record's (off, n) against this call's frame_off: the workgroup's tests before anything is
// touched, the threads' through a flag word read where the domain flag is read, behind the barriers that follow the staging. A pair
// that fails returns kPairNotIdent and the kernel runs the generic body on it.
template <int KPT, int NT, bool DEALT, bool IDENT>
__device__ __forceinline__ int dense_pair_plain(const FilterParams& p, uint32_t* smem, const int pair_idx, const int tid)
{
    constexpr int kMcap = KPT * NT;
    constexpr int kChunk = (KPT % 5 == 0) ? 5 : 4;
    static_assert(KPT % kChunk == 0, "KPT must be a multiple of the chunk");
    static_assert(NT >= 2 * kLeftN, "verification: two lanes per left cell in one sweep");
    const int lane = tid & 63;
    const int wave = tid >> 6;
    constexpr int kUnitsPerBlock = KPT * (NT / 64);   // (lane mapping: see dense_pair_rot)
    constexpr bool dealt = DEALT;
    const int m_base = dealt ? ((((lane >> 3) * kUnitsPerBlock + wave) << 3) | (lane & 7)) : tid;
    const int m_stride = dealt ? (NT / 64) * 8 : NT;
    auto match_of = [&](int k) -> int { return m_base + k * m_stride; };

    // the absolute LDS offsets below assume the dynamic segment starts at 0 (no static LDS in the kernels that call this)
    if ((uint32_t)(uintptr_t)((lds_u32_t*)smem) != 0u) return kPairGeneral;

    int64_t total_kp;
    const gms_pair pr = load_pair(p.pairs, pair_idx, p, total_kp);  // (and the frame table's header word)
    const int m = pr.m;
    if (p.with_scale || p.with_rotation || p.right_w[0] != kDenseRightW || p.right_h[0] != kDenseRightW || m <= 0 || m > kMcap ||
        pr.frame_a < 0 || pr.frame_a >= p.n_frames || pr.frame_b < 0 || pr.frame_b >= p.n_frames)
        return kPairGeneral;
    // the frame ranges and, right behind them, the pair's DMatch records: the records do not depend on the ranges, so they travel
    // beside them instead of a round trip later.
    // The records of a thread's first kKeep matches stay in registers from here to the copy-out (all of them up to ten matches per
    // thread; at sixteen the first twelve: 16 384 matches per pair 5.58 M pairs/s keeping none, 6.06 M keeping eight, 6.41 M twelve,
    // 6.67 M fourteen -- with 8 bytes of scratch --, 6.21 M all sixteen with 36); the others are loaded as (queryIdx, trainIdx) alone and
    // the survivors among them are read again at the end.
    const FrameRangeWords fr_words = request_frame_ranges(p.frame_off, pr.frame_a, pr.frame_b);
    // IDENT: beside the ranges the head of frame A's side record, the table's stamp (in the spare bytes behind the code arrays;
    // a block without header is left below before the word is looked at) and this thread's dword of the record's histogram. The
    // addresses are selected, never branched on: all of them are readable whatever the pair turns out to be.
    uint4 side_h0 = make_uint4(0, 0, 0, 0);
    uint2 side_h1 = make_uint2(0, 0), tab_stamp = make_uint2(0, 0);
    uint32_t side_hist = 0;
    if constexpr (IDENT) {
        const SideRecord* __restrict__ sr = p.side + min(pr.frame_a, p.side_frames - 1);
        side_h0 = *reinterpret_cast<const uint4*>(sr);
        side_h1 = *reinterpret_cast<const uint2*>(&sr->stamp);
        tab_stamp = *reinterpret_cast<const uint2*>(total_kp >= 0 ? p.pts + 2 * total_kp : p.pts - 2);
        side_hist = sr->hist[min(tid, kLeftN - 1)];
    }
    const gms_dmatch* __restrict__ matches = p.matches + pr.match_off;
    constexpr int kKeep = KPT <= 10 ? KPT : (DEALT ? 10 : 12);  // (the dealt instantiation has two registers less to spare)
    uint4 rec[kKeep];
    uint2 qt[KPT > kKeep ? KPT - kKeep : 1];
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
        if (k < kKeep) { const u32x4_t rv = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(&matches[min(match_of(k), m - 1)])); rec[k] = make_uint4(rv.x, rv.y, rv.z, rv.w); }
        else qt[k - kKeep] = *reinterpret_cast<const uint2*>(&matches[min(match_of(k), m - 1)]);
    }
    int64_t offA, offB;
    int nA, nB;
    take_frame_ranges(fr_words, offA, nA, offB, nB);
    if (nA <= 0 || nB <= 0) return kPairGeneral;
    if (total_kp < 0 || offA + nA > total_kp || offB + nB > total_kp) return kPairGeneral;  // (workgroup-uniform) no header, or frames beyond the table
    const uint16_t* __restrict__ lcodeA = reinterpret_cast<const uint16_t*>(p.pts + total_kp) + offA;
    const uint16_t* __restrict__ rcodeB = reinterpret_cast<const uint16_t*>(p.pts + total_kp) + total_kp + offB;
    uint32_t side_flags = 0;
    if constexpr (IDENT) {
        // what the workgroup can tell without looking at a match: the records belong to this build of this table, the frame is where it
        // was, one match per keypoint. Nothing has been touched yet: the generic body starts from scratch.
        asm volatile("" : "+v"(side_h0.x), "+v"(side_h0.y), "+v"(side_h0.z), "+v"(side_h0.w), "+v"(side_h1.x), "+v"(side_h1.y), "+v"(tab_stamp.x), "+v"(tab_stamp.y));
        const int64_t side_off = (int64_t)(((uint64_t)(uint32_t)uniform((int)side_h0.y) << 32) | (uint32_t)uniform((int)side_h0.x));
        const int side_n = uniform((int)side_h0.z);
        side_flags = (uint32_t)uniform((int)side_h0.w);
        const uint64_t s_side = ((uint64_t)(uint32_t)uniform((int)side_h1.y) << 32) | (uint32_t)uniform((int)side_h1.x);
        const uint64_t s_tab = ((uint64_t)(uint32_t)uniform((int)tab_stamp.y) << 32) | (uint32_t)uniform((int)tab_stamp.x);
        if (p.side_stamp == 0 || s_side == 0 || s_side != s_tab || side_off != offA || side_n != nA || m != nA)
            return kPairNotIdent;
    }

    uint32_t* nfine32 = smem + kDenseFineOff / 4;   // half-cell histogram: one dword per cell of grid type 1, a byte per half cell
    const uint8_t* nfine8 = reinterpret_cast<const uint8_t*>(nfine32);
    uint32_t* misc = smem + kDenseMiscOff / 4;
    uint32_t* trash = smem + kDenseTrashOff / 4;

    GMS_STAMP_DECL
#ifdef GMS_PHASE_TIMING
    ph_[14] = wall_clock64();
#endif
    if (tid < 32) misc[tid] = 0;
    if (tid < 16) trash[tid] = 0;
    if (IDENT ? tid < kLeftN : tid < kFineN / 4) nfine32[tid] = IDENT ? side_hist : 0u;  // (IDENT: the frame's own histogram, complete)

    // ---- staging: both frames' code words into the still unused matrix area, (twin of dense_pair_rot's; the pair's DMatch records were requested above)
    //      IDENT: frame B's alone (qA = 0); a thread's left codes come straight from the table, requested behind the staging loads
    const uint32_t phA = (uint32_t)(reinterpret_cast<uintptr_t>(lcodeA) >> 1) & 7u, phB = (uint32_t)(reinterpret_cast<uintptr_t>(rcodeB) >> 1) & 7u;
    const uint32_t qA = IDENT ? 0u : (phA + (uint32_t)nA + 7u) >> 3, qB = (phB + (uint32_t)nB + 7u) >> 3;
    const bool staged = (qA + qB) * 16u <= kDenseBytes;
    const uint4* __restrict__ srcA = reinterpret_cast<const uint4*>(lcodeA - phA);
    const uint4* __restrict__ srcB = reinterpret_cast<const uint4*>(rcodeB - phB);
    constexpr int kStageRegs = IDENT ? 2 : 3;  // (IDENT: 32 KB, 16 384 keypoints of frame B; larger frames finish in the plain loop)
    uint4 tb[kStageRegs];
#pragma unroll
    for (int i = 0; i < kStageRegs; ++i) {
        const uint32_t j = min((uint32_t)(i * NT + tid), qA + qB - 1u);
        const uint4* src = j < qA ? srcA + j : srcB + (j - qA);
        tb[i] = *src;
    }
    uint32_t ca_id[IDENT ? KPT : 1];
    if constexpr (IDENT) {
#pragma unroll
        for (int k = 0; k < KPT; ++k) ca_id[k] = lcodeA[min(match_of(k), nA - 1)];  // (m == nA: the clamp is the records')
    }
    auto query_of = [&](int k) -> uint32_t { return k < kKeep ? rec[k < kKeep ? k : 0].x : qt[k < kKeep ? 0 : k - kKeep].x; };
    auto train_of = [&](int k) -> uint32_t { return k < kKeep ? rec[k < kKeep ? k : 0].y : qt[k < kKeep ? 0 : k - kKeep].y; };
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
    const uint32_t ldsA = 2u * phA, ldsB = 16u * qA + 2u * phB;  // byte offsets: left code of frame A's keypoint q at ldsA + 2 q
    // IDENT: the left half of every code word -- [404 * cell : 18 | 0 : 9 | q and the edge bits : 5], kLeftNone for a match that is not
    // binned whatever its right side says -- and the identity test, IN FRONT of the barrier: a wave whose loads have landed does this
    // while the others' are still arriving and the vector ALUs are idle (behind the barrier all sixteen waves would share them for it)
    constexpr uint32_t kLeftNone = 0xFFFFFFFFu;
    uint32_t lw[IDENT ? KPT : 1];
    bool moved = false;
    if constexpr (IDENT) {
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const uint32_t c = ca_id[k], cell = c >> kLCellShift;
            const bool live = match_of(k) < m;
            const uint32_t qe = (c & 21u) | ((c >> 4) & kPEdgeX) | ((c >> 3) & kPEdgeY);
            lw[k] = (live & (cell < kLCellNever)) ? ((__umul24(cell, kDenseRow) << kPAtShift) | qe) : kLeftNone;
            moved |= live & (query_of(k) != (uint32_t)match_of(k));
        }
    }
    __syncthreads();
#ifdef GMS_PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    GMS_STAMP(4);
    ph_[15] = wall_clock64();
#endif

    // ---- code words + half-cell histogram
    uint32_t code[KPT];
    const uint32_t cw_sink = (kDenseTrashOff + 4u * (uint32_t)(lane & 15)) << kPAtShift;  // E = 0, q = 0, no edge bit
    {
        uint32_t ca[KPT], cb[KPT];
        if constexpr (IDENT) {
#pragma unroll
            for (int k = 0; k < KPT; ++k) ca[k] = 0;  // (not looked at: lw has what the left code said)
        }
        if (staged) {
            if constexpr (!IDENT) {
#pragma unroll
                for (int k = 0; k < KPT; ++k) ca[k] = ldsa_ld16(ldsA + 2u * min(query_of(k), (uint32_t)(nA - 1)));
            }
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = ldsa_ld16(ldsB + 2u * min(train_of(k), (uint32_t)(nB - 1)));
        } else {
            if constexpr (!IDENT) {
#pragma unroll
                for (int k = 0; k < KPT; ++k) ca[k] = lcodeA[min(query_of(k), (uint32_t)(nA - 1))];
            }
#pragma unroll
            for (int k = 0; k < KPT; ++k) cb[k] = rcodeB[min(train_of(k), (uint32_t)(nB - 1))];
        }
#ifdef GMS_PHASE_TIMING
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        GMS_STAMP(12);
#endif
        // IDENT: the left side of a match's test is the frame's (a bad left code anywhere in frame A is in side_flags: every keypoint
        // is matched), the histogram is in place; what is left per match is the right side, and that the match is where it should be
        bool any_bad = IDENT && (side_flags & kSideBadLeft) != 0u, spill = false;
#pragma unroll
        for (int k = 0; k < KPT; ++k) {
            const bool live = match_of(k) < m;
            const uint32_t e0 = cb[k] & kDEMask;
            const uint32_t cell = ca[k] >> kLCellShift;
            bool ok, binned;
            if constexpr (IDENT) {
                ok = ((int)(train_of(k) < (uint32_t)nB) & (int)((cb[k] & kRCodeBad) == 0u) & (int)(e0 != 0u)) != 0;
                any_bad |= live & !ok;
                // E into both of its fields of the left word (disjoint bit fields: the sum is the generic body's code word)
                code[k] = (ok & (lw[k] != kLeftNone)) ? lw[k] + __umul24(e0, (1u << kPAtShift) | (1u << kPEShift)) : cw_sink;
                continue;
            } else {
                ok = ((int)(query_of(k) < (uint32_t)nA) & (int)(train_of(k) < (uint32_t)nB) & (int)(cell != kLCellBad) & (int)((cb[k] & kRCodeBad) == 0u) & (int)(e0 != 0u)) != 0;
                binned = live & ok & (cell < kLCellNever);
                const uint32_t sh = ((ca[k] & 1u) << 3) | ((ca[k] & 4u) << 2);  // (half-cell histogram: twin of dense_pair_rot's)
                const uint32_t old = ldsa_add_rtn(binned ? kDenseFineOff + 4u * cell : kDenseTrashOff + 4u * (uint32_t)(lane & 7), 1u << sh);
                spill |= binned & (((old >> sh) & 255u) == 255u);
            }
            any_bad |= live & !ok;
            const uint32_t qe = (ca[k] & 21u) | ((ca[k] >> 4) & kPEdgeX) | ((ca[k] >> 3) & kPEdgeY);
            const uint32_t at1 = __umul24(cell, kDenseRow) + e0;
            code[k] = binned ? ((at1 << kPAtShift) | (e0 << kPEShift) | qe) : cw_sink;
        }
        if (any_bad) misc[8] = 1;
        if (spill) misc[13] = 1;
        if (IDENT && moved) misc[10] = 1;  // (its own word: the generic body, not the general path, takes the pair)
    }
    GMS_STAMP(13);
    __syncthreads();
    GMS_STAMP(0);

    // ---- motion.setTo(0), once (see dense_pair_rot)
    {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
        uint4* d4 = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < staged16; i += NT) d4[i] = z4;
        // the sink dwords from here on: bit 31 set, and nothing below ever clears it (increments land in byte 0, arg-max keys end at
        // bit 21, the undo stores a zero into byte 0). (Nobody compares a sink dword any more: a sink word's E is 0, which no field of
        // the mark table equals.)
        if (tid < 16) trash[tid] = 0x80000000u;
    }
    __syncthreads();
    GMS_STAMP(2);
    if (IDENT && misc[10] != 0) {  // a match that is not where the identity says (workgroup-uniform): the left codes were somebody else's
        __syncthreads();
        return kPairNotIdent;
    }
    if (misc[8] != 0) {
        __syncthreads();
        return kPairGeneral;
    }
    const bool spilled = IDENT ? (side_flags & kSideSpill) != 0u : misc[13] != 0;

    const bool thr_fast = threshold_fast_ok(p.threshold_factor);
    const uint32_t f2i = dense_factor_sq(p.threshold_factor);
    // cellPairs of this thread's cell under two of the four grid types, 16 bits each: E(j*) or kDenseMarkNone. The even lane of a
    // verifying pair decides and keeps grid types 1 and 2, the odd lane is handed 3 and 4 (one DPP move). They stay here until
    // the last grid type is through -- the LDS has no room for them while the matrix lives -- and then go into the mark table
    // (gms_kernel_dense.h), where every match looks its four verdicts up at once.
    uint32_t vd = 0;


    // L2 prefetch for the workgroup that follows this one on the CU: workgroups are handed out in order, one per CU, so that is
    // pair_idx + (number of CUs) -- on the same XCD (256 = 8 x 32)
    const uint32_t* __restrict__ pf_base = nullptr;
    uint32_t pf_lines = 0, pf_sink = 0, pf_sink2 = 0;
    {
        const int nxt = pair_idx + p.prefetch_ahead;
        if (p.prefetch_ahead > 0 && nxt < p.n_pairs) {
            const gms_pair pn = load_pair(p.pairs, nxt);
            // (only what that pair's own workgroup will read as well: a pair it would refuse before reading -- frames out of range,
            //  a negative offset -- is not touched either)
            if (pn.m > 0 && pn.m <= kMcap && pn.match_off >= 0 && pn.frame_a >= 0 && pn.frame_a < p.n_frames && pn.frame_b >= 0 &&
                pn.frame_b < p.n_frames) {
                pf_base = reinterpret_cast<const uint32_t*>(p.matches + pn.match_off);
                pf_lines = min(((uint32_t)pn.m * 16u + 127u) >> 7, 2u * NT);   // (the array's first line may start a little earlier: close enough)
            }
        }
    }

    auto run_types = [&](auto crowded_c) -> int {
    constexpr bool CROWDED = decltype(crowded_c)::value;
    for (int g = 0; g < 4; ++g) {
        const int gx = g & 1, gy = g >> 1;
        const uint32_t q_mask = (uint32_t)(gx + 20 * gy);                               // entry = entry1 + 404 * (q & q_mask)
        const uint32_t x_mask = (gx ? kPEdgeX : 0u) | (gy ? kPEdgeY : 0u);              // x >= 20 || y >= 20 -> -1 (DLL@0x180047d3d)
        const uint32_t key_tag = (uint32_t)g << kDTagShift;
        const uint32_t nl_cur = kDenseFineOff + (uint32_t)(g & 1) * (kLeftN * 2u);      // crowded: 16-bit nLeft counters, two buffers
        if (!CROWDED && g == p.prefetch_type && pf_lines) {
            // touch the match records of the pair this CU's NEXT workgroup will filter (one dword per 128-byte line): they are in the
            // XCD's L2 when that workgroup asks for them. Late on purpose -- one grid type before the end -- so that only a few
            // CUs' worth of lines sit in the 4 MB at any time (touched at the start of a pair they are evicted before use).
            // (two independent loads, consumed only before the copy-out: nothing waits for them here)
            // (sixteen matches per thread, IDENT: the two line addresses are worked out here, not once in front of the
            //  grid types -- four registers that the loop does not have; 12 to 16 bytes of scratch otherwise)
            uint32_t pt = (uint32_t)tid;
            if constexpr (IDENT && KPT > 10) asm volatile("" : "+v"(pt));
            if (pt < pf_lines) pf_sink = pf_base[32u * pt];
            if (pt + NT < pf_lines) pf_sink2 = pf_base[32u * (pt + NT)];
        }
        if (!CROWDED && tid < kLeftN) {
            const uint32_t n = dense_nleft_cm(nfine8, tid % kLeftW, tid / kLeftW, gx, gy);
            if (n > 255u) misc[11] = 1;
            ldsa_st8(kDenseNleftOff + (uint32_t)tid, n);
        }

        // ---- assignMatchPairs
        uint32_t ae[KPT];  // the entry of every match under this grid type (a sink's own for the matches it does not bin)
#pragma unroll
        for (int k0 = 0; k0 < KPT; k0 += kChunk) {
            uint32_t old[kChunk], at[kChunk], cg[kChunk], sh[kChunk];
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                const uint32_t cw = code[k0 + c];
                cg[c] = (cw & x_mask) ? cw_sink : cw;
                at[c] = mad24_vsv(cg[c] & q_mask, kDenseRow, cg[c] >> kPAtShift);
                sh[c] = at[c] << 3;  // (shifts and bit-field extracts read its low five bits: 8 * (entry & 3))
                asm("" : "+v"(sh[c]));
                old[c] = ldsa_add_rtn(at[c] & ~3u, 1u << (sh[c] & 31u));
                if (CROWDED) {
                    const uint32_t l = (((at[c] - ((cg[c] >> kPEShift) & kDEMask)) >> 2) * 649u) >> 16;  // row / 404 (the sink: 405)
                    ldsa_add(nl_cur + 4u * (l >> 1), 1u << ((l & 1u) << 4));
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // all of the chunk's atomics are issued before any result is read
#pragma unroll
            for (int c = 0; c < kChunk; ++c) {
                const uint32_t e = (cg[c] >> kPEShift) & kDEMask;
                const uint32_t before = __builtin_amdgcn_ubfe(old[c], sh[c], 8);  // <= 254, or ...
                if (CROWDED && e != 0u && before == 255u) misc[12] = 1;                // ... the entry's byte has just wrapped
                ldsa_max(at[c] - e, key_tag | (before << 11) | e);
                ae[k0 + c] = at[c];
            }
        }
        GMS_STAMP(3);
        __syncthreads();
        GMS_STAMP(11);
        if (!CROWDED && misc[11] != 0) return 1;
        if (CROWDED && misc[12] != 0) return 2;

        // ---- verifyCellPairs
        if (tid < 2 * kLeftN) {
            // lane pair of cell i = tid >> 1; the even lane takes the neighbour pairs at d = -21, -20, -19, -1 (positions 0..3 of
            // the 3 x 3 block), the odd lane the mirrored ones (positions 8..5): s = +-1
            // (sixteen matches per thread: what follows from the lane alone is worked out here, per grid type, instead of a dozen
            //  registers of signs, steps and limits held across the binning passes, which do not have them)
            uint32_t vt = (uint32_t)tid;
            if constexpr (KPT > 10) asm volatile("" : "+v"(vt));
            const uint32_t vi = vt >> 1;
            const uint32_t viy = (vi * 3277u) >> 16, vix = vi - 20u * viy;  // vi / 20, vi % 20 for vi < 400
            const bool vodd = (vt & 1u) != 0;
            // (everything that does not depend on j* is read at once: the cell's nLeft, its header, the four neighbours' nLeft)
            const int s1 = vodd ? -1 : 1;
            const uint32_t nlb = (CROWDED ? nl_cur + 2u * vi : kDenseNleftOff + vi);
            const uint32_t hdr = vi * kDenseRow;
            const uint32_t ni = CROWDED ? ldsa_ld16(nlb) : ldsa_ld8(nlb);
            const uint32_t hdr_word = ldsa_ld32(hdr);
            uint32_t nl4[4];
            {
                constexpr int kD[4] = {-21, -20, -19, -1};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t na = nlb + (uint32_t)((CROWDED ? 2 : 1) * s1 * kD[c]);
                    nl4[c] = CROWDED ? ldsa_ld16(na) : ldsa_ld8(na);
                }
            }
            uint32_t ej = 0;
            bool pass = false;  // the cell pair (i, j*) stands: decided by the even lane
            if (__ballot(ni != 0) != 0ull) {
                const uint32_t best = hdr_word & ((1u << kDTagShift) - 1u);  // ((max count - 1) << 11) | E(j*), lowest j* among maxima
                ej = ni ? (best & kDEMask) : (uint32_t)(kDenseRightN + 3);
                const uint32_t j = (uint32_t)(kDenseRightN + 3) - ej;
                const uint32_t jy = (j * 3277u) >> 16, jx = j - 20u * jy;
                const uint32_t lo = vodd ? 19u : 0u, hi = 19u - lo;
                const bool okA = (vix != lo) & (jx != lo);   // one step against s along x stays inside both grids
                const bool okB = (vix != hi) & (jx != hi);   // one step with s along x
                const bool okC = (viy != lo) & (jy != lo);   // one step against s along y
                const int s403 = vodd ? -403 : 403;
                const uint32_t base = hdr + ej;
                uint32_t score = 0, tn = 0;  // tn = (sum of nLeft << 4) | numpair
                auto side = [&](int c, int d, bool valid) {
                    const uint32_t a = valid ? base + (uint32_t)(s403 * d) : kPZeroByte;
                    score += ldsa_ld8(a);
                    tn += valid ? ((nl4[c] << 4) | 1u) : 0u;
                };
                side(0, -21, okA & okC);
                side(1, -20, okC);
                side(2, -19, okB & okC);
                side(3, -1, okA);
                score += dpp_xor1(score);
                tn += dpp_xor1(tn);
                score += (best >> 11) + 1u;  // centre pair: ll = i, rr = j*, the arg-max count itself
                tn += (ni << 4) | 1u;
                if (ni != 0 && !vodd) {
                    const bool rej = CROWDED ? threshold_rejects(tn >> 4, tn & 15u, score, p.threshold_factor, thr_fast)
                                             : dense_threshold_rejects(tn >> 4, tn & 15u, score, p.threshold_factor, thr_fast, f2i);
                    pass = !rej;
                }
            }
            // cellPairs[i] as E(j*); none: an empty cell, a rejected pair. Grid types 3 and 4 are kept by the odd lane.
            uint32_t verdict = pass ? ej : kDenseMarkNone;
            if (g >> 1) verdict = dpp_xor1(verdict);
            // the lane's first grid type ends up in the low half, its second in the high half (a restart in crowded mode shifts
            // two new ones in). The row header keeps its arg-max key: the next grid type's keys outrank it, nobody else reads it.
            if ((uint32_t)(g >> 1) == (vt & 1u)) vd = (vd >> 16) | (verdict << 16);
        }
        __syncthreads();
        GMS_STAMP(5);
        // Nothing reads the matrix behind the last grid type's verification: the mark table and the copy-out's count table, which
        // reuse the area, write every word before they read it, and the next workgroup on the CU clears the LDS itself. So the last
        // grid type leaves its increments (and the crowded counters) where they are: it ends here. (workgroup-uniform; one loop body)
        if (g != 3) {
            // ---- take this grid type's increments back (plain zero bytes: see dense_pair_rot); every reader of the matrix is past
            //      the barrier.
#pragma unroll
            for (int k = 0; k < KPT; ++k) ldsa_st8(ae[k], 0u);
            if (CROWDED && tid < kLeftN / 2) ldsa_st32(kDenseFineOff + (uint32_t)((g + 1) & 1) * (kLeftN * 2u) + 4u * (uint32_t)tid, 0u);
            __syncthreads();
            GMS_STAMP(6);
        }
    }
    return 0;
    };

    int status = 1;
    if (!spilled) status = run_types(std::false_type{});
    if (status == 1) {
        // crowded: start over on a clean matrix (the abandoned grid type's bytes may have wrapped), no inlier bits yet
        __syncthreads();
        {
            const uint4 z4 = make_uint4(0, 0, 0, 0);
            uint4* d4 = reinterpret_cast<uint4*>(smem);
            for (uint32_t i = tid; i < kDenseBytes / 16; i += NT) d4[i] = z4;
            if (tid < kLeftN) nfine32[tid] = 0;
            if (tid == 0) misc[11] = 0;
        }
        if (tid < 16) trash[tid] = 0x80000000u;
        __syncthreads();
        status = run_types(std::true_type{});
    }
    if (status != 0) {
        __syncthreads();
        return kPairGeneral;
    }

    // ---- mark inliers (cellPairs[l] == r under some grid type), once per pair: the matrix area is free behind the last barrier
    //      of the grid types' verification (the last grid type's increments still lie in it: every field below is written before it
    //      is read). The verdicts go from the registers straight into the mark table -- all of it, for every pair: neither the
    //      matrix's bytes nor what the previous workgroup left in the LDS is ever read --, and a match reads the one entry of its left
    //      half cell. Who writes which field: gms_kernel_dense.h.
    static_assert(NT > 2 * kLeftN, "the lanes that do not verify write the fields nobody owns");
    if (tid < 2 * kLeftN) {
        // a verifying lane: its cell's verdicts under its two grid types into field g of the cell's four half cells (unpredicated:
        // a half cell cut off by the image's border is clamped onto one of the cell's own, same field, same value)
        const uint32_t vi = (uint32_t)tid >> 1, viy = (vi * 3277u) >> 16, vix = vi - 20u * viy;
        const int gy = tid & 1;
#pragma unroll
        for (int gx = 0; gx < 2; ++gx)
#pragma unroll
            for (int d = 0; d < 4; ++d)
                ldsa_st16(dense_mark_field_off(4u * dense_cell_half_slot((int)vix, (int)viy, gx, gy, d & 1, d >> 1) + 2u * (uint32_t)gy + (uint32_t)gx),
                          gx ? vd >> 16 : vd);
    } else {
        for (uint32_t u = (uint32_t)tid - 2u * kLeftN; u < kDenseMarkNoneFields; u += (uint32_t)NT - 2u * kLeftN)
            ldsa_st16(dense_mark_field_off(dense_mark_none_field(u)), kDenseMarkNone);
    }
    __syncthreads();
    uint32_t acc = 0;  // bit KPT - 1 - k: match k of this thread is an inlier under some grid type
#pragma unroll
    for (int k0 = 0; k0 < KPT; k0 += kChunk) {
        uint64_t t[kChunk];
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const uint32_t cw = code[k0 + c];
            const uint32_t row = (cw >> kPAtShift) - ((cw >> kPEShift) & kDEMask);   // 404 * the cell under grid type 1; a sink's own dword
            const uint32_t cell = ((row >> 2) * 649u) >> 16;                         // row / 404 (the sinks: kDenseMarkSinkSlot / 4)
            t[c] = ldsa_ld64(kDenseMarkTableOff + (cell << 5) + ((cw & 1u) << 3) + ((cw & 4u) << 2));  // entry dense_half_cell_slot()
        }
#pragma unroll
        for (int c = 0; c < kChunk; ++c) {
            const uint32_t e = (code[k0 + c] >> kPEShift) & kDEMask;  // (a sink's 0 equals no field: none is not an E)
            const uint32_t lo = (uint32_t)t[c], hi = (uint32_t)(t[c] >> 32);
            const bool in = ((lo & 0xFFFFu) == e) | ((lo >> 16) == e) | ((hi & 0xFFFFu) == e) | ((hi >> 16) == e);
            acc = 2u * acc + (in ? 1u : 0u);
        }
    }
    GMS_STAMP(1);  // mark table: the verdicts' scatter, its barrier, look-up
    GMS_STAMP(7);
    if (p.prefetch_type == 4 && pf_lines) {  // (diagnostic setting: as late as possible)
        if ((uint32_t)tid < pf_lines) pf_sink = pf_base[32u * (uint32_t)tid];
        if ((uint32_t)tid + NT < pf_lines) pf_sink2 = pf_base[32u * ((uint32_t)tid + NT)];
    }
    // (never true: keeps the prefetch loads alive; they landed long ago, and no copy-out store has been issued yet)
    if (p.prefetch_type != 4 && (pf_sink ^ pf_sink2) == 0x9E3779B9u && p.n_pairs < 0) trash[0] = pf_sink;

    // ---- copy-out: surviving DMatch verbatim, in input order (DLL@0x180048340), from the registers (see dense_pair_rot)
    constexpr int kWaves = NT / 64;
    uint32_t* cnt_tab = smem;  // (below the mark table, which slower waves may still be reading)
    unsigned long long keep[KPT];
#pragma unroll
    for (int k = 0; k < KPT; ++k) keep[k] = __ballot((acc >> (KPT - 1 - k)) & 1u);
    gms_dmatch* __restrict__ out = p.out + pr.match_off;
    uint8_t* mask_out = p.mask ? p.mask + pr.match_off : nullptr;
    uint32_t total = 0;
    if (!dealt) {
        uint32_t row_base[KPT];

        // A chunk is 64 consecutive matches = one wave's k-th record; chunk (k, wave) sits at position k * 16 + wave of the order, so the
        // sixteen chunks of one k are one 16-lane DPP row of the published counts: a row-wise scan on the vector ALU (four DPP adds
        // per register, no LDS round trips), the rows' totals added up in scalar registers.
        constexpr int kScanRegs = (KPT * kWaves + 63) / 64;
        static_assert(kWaves == 16, "one DPP row per k");
#pragma unroll
        for (int k = 0; k < KPT; ++k)
            if (lane == 0) cnt_tab[k * kWaves + wave] = (uint32_t)__popcll(keep[k]);
        __syncthreads();
        uint32_t excl[kScanRegs];
#pragma unroll
        for (int v = 0; v < kScanRegs; ++v) {
            const int idx = v * 64 + lane;
            const uint32_t c = idx < KPT * kWaves ? cnt_tab[idx] : 0u;
            uint32_t incl = c;
            incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, true);  // row_shr:1, zeros shifted in
            incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, true);
            incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, true);
            incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, true);
            excl[v] = incl - c;  // within its row
            (void)idx;
            // totals of this register's rows, in order (scalar)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = v * 4 + r;
                if (k < KPT) {
                    row_base[k] = total;
                    total += (uint32_t)__builtin_amdgcn_readlane((int)incl, r * 16 + 15);
                }
            }
        }
        GMS_STAMP(8);
        const int wave_s = __builtin_amdgcn_readfirstlane(wave);
        // The records that were not kept in registers (KPT above kKeep) are read again, two at a time: requested together, the survivor's
        // own or -- address selected -- the pair's first, and pinned before the stores (a load inside the survivor's branch is waited for
        // there, one round trip per record).
        auto put = [&](int k, const uint4& rv) {
            const int i = k * NT + tid;
            const uint32_t base = row_base[k] + (uint32_t)__builtin_amdgcn_readlane((int)excl[k >> 2], (k & 3) * 16 + wave_s);
            if (i < m) {
                const bool in = (keep[k] >> lane) & 1ull;
                if (mask_out) mask_out[i] = in ? 1 : 0;
                if (in) {
                    const uint32_t pos = base + (uint32_t)__popcll(keep[k] & ((1ull << lane) - 1ull));
                    __builtin_nontemporal_store(u32x4_t{rv.x, rv.y, rv.z, rv.w}, reinterpret_cast<u32x4_t*>(&out[pos]));
                }
            }
        };
#pragma unroll
        for (int k = 0; k < kKeep; ++k) put(k, rec[k]);  // (their registers are free for the records read again)
        constexpr int kBatch = 2;
#pragma unroll
        for (int k0 = kKeep; k0 < KPT; k0 += kBatch) {
            uint4 again[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const int k = k0 + j < KPT ? k0 + j : KPT - 1, i = k * NT + tid;
                again[j] = *reinterpret_cast<const uint4*>(&matches[(i < m && ((keep[k] >> lane) & 1ull)) ? i : 0]);
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) asm volatile("" : "+v"(again[j].x), "+v"(again[j].y), "+v"(again[j].z), "+v"(again[j].w));
#pragma unroll
            for (int j = 0; j < kBatch; ++j)
                if (k0 + j < KPT) put(k0 + j, again[j]);
        }
    } else {
        constexpr int kUnits = KPT * NT / 8;
        static_assert(kUnits <= 2 * NT, "two scan entries per thread");
        uint32_t* wave_tot = misc + 16;
#pragma unroll
        for (int k = 0; k < KPT; ++k)
            if ((lane & 7) == 0) cnt_tab[match_of(k) >> 3] = (uint32_t)__popc((uint32_t)(keep[k] >> (lane & 56)) & 0xFFu);
        __syncthreads();
        {
            const uint32_t c0 = 2 * tid < kUnits ? cnt_tab[2 * tid] : 0u, c1 = 2 * tid + 1 < kUnits ? cnt_tab[2 * tid + 1] : 0u;
            uint32_t incl = c0 + c1;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) wave_tot[wave] = incl;
            __syncthreads();
            uint32_t off = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const uint32_t tw = wave_tot[w];
                off += w < wave ? tw : 0u;
                total += tw;
            }
            if (2 * tid < kUnits) cnt_tab[2 * tid] = off + incl - c0 - c1;
            if (2 * tid + 1 < kUnits) cnt_tab[2 * tid + 1] = off + incl - c1;
        }
        __syncthreads();
        GMS_STAMP(8);
        auto put = [&](int k, const uint4& rv) {
            const int i = match_of(k);
            if (i < m) {
                const uint32_t byte = (uint32_t)(keep[k] >> (lane & 56)) & 0xFFu;
                const bool in = (byte >> (lane & 7)) & 1u;
                if (mask_out) mask_out[i] = in ? 1 : 0;
                if (in) {
                    const uint32_t pos = cnt_tab[i >> 3] + (uint32_t)__popc(byte & ((1u << (lane & 7)) - 1u));
                    __builtin_nontemporal_store(u32x4_t{rv.x, rv.y, rv.z, rv.w}, reinterpret_cast<u32x4_t*>(&out[pos]));
                }
            }
        };
#pragma unroll
        for (int k = 0; k < kKeep; ++k) put(k, rec[k]);
        constexpr int kBatch = 2;  // (see the list-order branch)
#pragma unroll
        for (int k0 = kKeep; k0 < KPT; k0 += kBatch) {
            uint4 again[kBatch];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                const int k = k0 + j < KPT ? k0 + j : KPT - 1, i = match_of(k);
                const bool in = i < m && (((uint32_t)(keep[k] >> (lane & 56)) >> (lane & 7)) & 1u) != 0u;
                again[j] = *reinterpret_cast<const uint4*>(&matches[in ? i : 0]);
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) asm volatile("" : "+v"(again[j].x), "+v"(again[j].y), "+v"(again[j].z), "+v"(again[j].w));
#pragma unroll
            for (int j = 0; j < kBatch; ++j)
                if (k0 + j < KPT) put(k0 + j, again[j]);
        }
    }
    GMS_STAMP(9);
    GMS_STAMP_FLUSH;
    if (p.prefetch_type == 4 && (pf_sink ^ pf_sink2) == 0x9E3779B9u && p.n_pairs < 0) trash[0] = pf_sink;
    if (tid == 0) {
        gms_pair_result r;
        r.n_inliers = (int)total;
        r.best_scale = total ? 0 : -1;
        r.best_rot = total ? 1 : -1;
        r.status = GMS_OK;
        p.results[pair_idx] = r;
    }
    return kPairDone;
}

// IDENT (default flags only): the identity-query body first; a pair it turns down is counted (p.ident_misses: the host takes launches
// that meet such pairs off this instantiation) and filtered by the generic body, same workgroup, same launch.
template <int KPT, bool ROT, int NT, bool DEALT, bool IDENT>
__global__ void __launch_bounds__(NT)
filter_kernel_dense(FilterParams p)
{
    static_assert(!(ROT && IDENT), "the identity-query body is dense_pair_plain's");
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    first_round_stagger(p);
    bool done;
    if constexpr (ROT) {
        done = dense_pair_rot<KPT, NT, DEALT>(p, smem, (int)blockIdx.x, (int)threadIdx.x);
    } else {
        int r = dense_pair_plain<KPT, NT, DEALT, IDENT>(p, smem, (int)blockIdx.x, (int)threadIdx.x);
        if constexpr (IDENT) {
            if (r == kPairNotIdent) {
                if (threadIdx.x == 0 && p.ident_misses) atomicAdd(p.ident_misses, 1u);
                r = dense_pair_plain<KPT, NT, DEALT, false>(p, smem, (int)blockIdx.x, (int)threadIdx.x);
            }
        }
        done = r == kPairDone;
    }
    if (!done) hash_pair<KPT, ROT, NT>(p, smem, (int)blockIdx.x, (int)threadIdx.x);
}

// Test hook: the threshold comparison in device fp64 -- and, where the operands are in its range, the byte-matrix
// path's integer form of it, which must agree (a disagreement is reported as 2).
__global__ void threshold_kernel(const int32_t* T, const int32_t* n, const int32_t* score, double factor,
                                 int count, uint8_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const uint32_t t = (uint32_t)T[i], nn = (uint32_t)n[i], sc = (uint32_t)score[i];
        const bool general = threshold_rejects(t, nn, sc, factor, threshold_fast_ok(factor));
        uint8_t r = general ? 1 : 0;
        if (t <= 9u * 255u && sc <= 9u * 255u && nn >= 1u && nn <= 9u &&
            dense_threshold_rejects(t, nn, sc, factor, threshold_fast_ok(factor), dense_factor_sq(factor)) != general)
            r = 2;
        out[i] = r;
    }
}

hipError_t launch_threshold(const int32_t* d_T, const int32_t* d_n, const int32_t* d_score, double factor,
                            int count, uint8_t* d_out, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(threshold_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, d_T, d_n, d_score,
                       factor, count, d_out);
    return hipGetLastError();
}

hipError_t launch_filter_dense(const FilterParams& p, int kpt, int n_pairs, size_t lds_bytes, hipStream_t stream)
{
    const size_t lds = lds_bytes > kDenseLdsBytes ? lds_bytes : (size_t)kDenseLdsBytes;  // (the fallback's table may need more)
    return dispatch_kpt_rot(kpt, p.with_rotation != 0, [&](auto k, auto rot) {
        constexpr int KPT = decltype(k)::value;
        constexpr bool ROT = decltype(rot)::value;
        if constexpr (!ROT) {
            if (p.ident && p.side != nullptr && p.side_frames >= 1 && p.side_stamp != 0) {
                if (p.dealt) hipLaunchKernelGGL((filter_kernel_dense<KPT, false, kThreads, true, true>), dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, p);
                else hipLaunchKernelGGL((filter_kernel_dense<KPT, false, kThreads, false, true>), dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, p);
                return hipGetLastError();
            }
        }
        if (p.dealt) hipLaunchKernelGGL((filter_kernel_dense<KPT, ROT, kThreads, true, false>), dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, p);
        else hipLaunchKernelGGL((filter_kernel_dense<KPT, ROT, kThreads, false, false>), dim3((unsigned)n_pairs), dim3(kThreads), lds, stream, p);
        return hipGetLastError();
    });
}

hipError_t init_dense_kernels()
{
    return for_each_kpt_rot([](auto k, auto rot) {
        constexpr int KPT = decltype(k)::value;
        constexpr bool ROT = decltype(rot)::value;
        hipError_t e = allow_full_lds(filter_kernel_dense<KPT, ROT, kThreads, false, false>);
        if (e == hipSuccess) e = allow_full_lds(filter_kernel_dense<KPT, ROT, kThreads, true, false>);
        if constexpr (!ROT) {
            if (e == hipSuccess) e = allow_full_lds(filter_kernel_dense<KPT, false, kThreads, false, true>);
            if (e == hipSuccess) e = allow_full_lds(filter_kernel_dense<KPT, false, kThreads, true, true>);
        }
        return e;
    });
}

}  // namespace gms
