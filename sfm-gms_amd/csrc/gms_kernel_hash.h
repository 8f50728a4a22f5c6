// gms_kernel_hash.h -- the hashed form of the GMS filter (overview: gms_kernels.hip): the bucket and region helpers of its table
// and hash_pair(), the per-pair body. A header because two kernels inline the body: filter_kernel (gms_kernel_hash.hip) and, as the
// fallback for the pairs its byte matrix cannot take, filter_kernel_dense (gms_kernel_dense.hip). Internal; .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_device_common.h"

namespace gms {

// byte offset (0, 4, 8, 12) of the slot of bucket v whose key is r (kr = r << 21), or -1
__device__ __forceinline__ int bucket_find(const uint4& v, uint32_t kr)
{
    int o = -1;
    o = ((v.w ^ kr) <= kSlotCountMask) ? 12 : o;
    o = ((v.z ^ kr) <= kSlotCountMask) ? 8 : o;
    o = ((v.y ^ kr) <= kSlotCountMask) ? 4 : o;
    o = ((v.x ^ kr) <= kSlotCountMask) ? 0 : o;
    return o;
}
__device__ __forceinline__ int bucket_first_empty(const uint4& v)
{
    int o = -1;
    o = (v.w == kEmpty) ? 12 : o;
    o = (v.z == kEmpty) ? 8 : o;
    o = (v.y == kEmpty) ? 4 : o;
    o = (v.x == kEmpty) ? 0 : o;
    return o;
}
__device__ __forceinline__ uint32_t bucket_count(const uint4& v, uint32_t kr)
{
    uint32_t c = 0;
    c = ((v.w ^ kr) <= kSlotCountMask) ? v.w : c;
    c = ((v.z ^ kr) <= kSlotCountMask) ? v.z : c;
    c = ((v.y ^ kr) <= kSlotCountMask) ? v.y : c;
    c = ((v.x ^ kr) <= kSlotCountMask) ? v.x : c;
    return c & kSlotCountMask;
}

// A region is one header bucket followed by nb data buckets; d = (header bucket << 16) | nb.
// Header dword 0 is the running arg-max of the cell's row, kept inverted so that the table's 0xFFFFFFFF
// fill means "nothing yet": ~((count << 11) | (2047 - right cell)), updated with atomicMin. The largest
// key ever reached by a slot is its final one, so the minimum over all updates is the row's arg-max with
// the lowest right cell winning ties -- the reference's ascending scan with strict '>'.
__device__ __forceinline__ void header_update(uint32_t* tab, uint32_t d, uint32_t r, uint32_t count)
{
    atomicMin(lds_at(tab, (d >> 16) << 4), ~((count << 11) | (2047u - r)));
}

// motion[l][r]++, general form: walk the region from its hashed bucket.
// Every lane terminates: the region always has an empty slot.
__device__ __forceinline__ void region_insert_general(uint32_t* tab, uint32_t d, uint32_t r)
{
    const uint32_t nb = d & 0xFFFFu, first = (d >> 16) + 1u;
    if (nb == 0) return;
    const uint32_t kr = r << kSlotRShift;
    uint32_t b = bucket_of(r, nb);
    for (uint32_t guard = 0; guard < 8u * nb + 8u; ++guard) {
        const uint32_t boff = (first + b) << 4;
        const uint4 v = *reinterpret_cast<const uint4*>(lds_at(tab, boff));
        const int f = bucket_find(v, kr);
        if (f >= 0) {
            const uint32_t old = atomicAdd(lds_at(tab, boff + (uint32_t)f), 1u);
            header_update(tab, d, r, (old & kSlotCountMask) + 1u);
            return;
        }
        const int e = bucket_first_empty(v);
        if (e >= 0) {
            const uint32_t prev = atomicCAS(lds_at(tab, boff + (uint32_t)e), kEmpty, kr | 1u);
            if (prev == kEmpty) {
                header_update(tab, d, r, 1u);
                return;
            }
            continue;  // the slot went to somebody else (maybe to this very key): look at the bucket again
        }
        if (++b == nb) b = 0;
    }
}

// motion[l][r], general form, starting one bucket after the hashed one (which was full without the key).
__device__ __forceinline__ uint32_t region_lookup_general(const uint32_t* tab, uint32_t d, uint32_t r)
{
    const uint32_t nb = d & 0xFFFFu, first = (d >> 16) + 1u;
    const uint32_t kr = r << kSlotRShift;
    uint32_t b = bucket_of(r, nb);
    for (uint32_t guard = 1; guard < nb; ++guard) {
        if (++b == nb) b = 0;
        const uint4 v = *reinterpret_cast<const uint4*>(tab + ((first + b) << 2));
        if (bucket_find(v, kr) >= 0) return bucket_count(v, kr);
        if (bucket_first_empty(v) >= 0) return 0;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The filter: one 1024-thread workgroup per pair, KPT matches per thread held in registers.
// The kernel is VALU-issue bound, so the per-match work is kept to a few instructions: the left cell of
// a match under grid type g is never computed per match -- a per-pair table indexed by the match's
// half-cell index gives the table region (insert) and the verified cell result (mark) with one LDS read.
// ------------------------------------------------------------------------------------------------
template <int KPT, bool ROT, int NT>
__device__ __forceinline__ void hash_pair(const FilterParams& p, uint32_t* smem, const int pair_idx, const int tid)
{
    constexpr int kMcap = KPT * NT;
    constexpr int kNRot = ROT ? 8 : 1;
    // matches a thread keeps in flight through the LDS stages: 5 (4) with 128 registers per thread, 10 with 256
    constexpr int kChunk = (NT <= 512 && KPT % 10 == 0) ? 10 : (KPT % 5 == 0) ? 5 : 4;
    static_assert(KPT % kChunk == 0, "KPT must be a multiple of the chunk");
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // with scale hypotheses the byte-matrix kernel may have evaluated scales 0..2 already (see dense_scales_pair): its
    // record holds the best hypothesis so far, and this kernel continues with scale 3. The record's four header words in one load,
    // requested in front of the pair's record (one round trip for both: see load_pair).
    const uint32_t* __restrict__ part = p.partial ? p.partial + (size_t)pair_idx * kPartialStrideDw : nullptr;
    uint4 part_hdr = make_uint4(0u, 0u, 0u, 0u);
    if (part != nullptr) part_hdr = *reinterpret_cast<const uint4*>(part);
    const gms_pair pr = load_pair(p.pairs, pair_idx);
    if (part != nullptr) asm volatile("" : "+v"(part_hdr.x), "+v"(part_hdr.y), "+v"(part_hdr.z), "+v"(part_hdr.w));
    const uint32_t part0 = (uint32_t)uniform((int)part_hdr.x);  // workgroup-uniform: 0, or what the first kernel decided:
    if (part0 == 6u) return;                                     //   6: everything, the survivors copied out as well (scales_copy_out)
    const int m = pr.m;
    const gms_dmatch* __restrict__ matches = p.matches + pr.match_off;

    const uint32_t T = p.table_slots;              // multiple of 4
    uint32_t* tab = smem;                          // per-left-cell regions of [r | count] slots
    uint32_t* nfine = tab + T;                     // [1664] 40 x 40 half-cell histogram of the left points; later reused as
    uint32_t* fres = nfine;                        //        per half-cell (j* << 8) | rotation bits that pass
    uint32_t* nleft4 = nfine + kFineStride;        // [4][400] mNumberPointsInPerCellLeft per grid type
    uint32_t* desc4 = nleft4 + 4 * kLeftN;         // [4][400] (header bucket << 16) | data buckets
    uint32_t* fdesc4 = desc4 + 4 * kLeftN;         // [4][1664] the same, per half-cell: region of the cell it falls in
    uint32_t* bestmask = fdesc4 + 4 * kFineStride; // kMcap / 32
    uint32_t* chunk_base = bestmask + (kMcap >> 5);// kMcap / 64 + 1
    uint32_t* misc = chunk_base + (kMcap >> 6) + 1;// [0..7] rotation counts, [8] error, [9] carry, [12..15] bucket
                                                   // allocators, [16..] scan scratch
    uint32_t* trash = reinterpret_cast<uint32_t*>((reinterpret_cast<uintptr_t>(misc + 48) + 15) & ~uintptr_t(15));
                                                   // [0..63] add/CAS sink per lane, [64..127] min sink per lane,
                                                   // [128..131] an always-empty bucket (16-byte aligned)

    if (tid < 48) misc[tid] = 0;
    if (tid < 128) trash[tid] = 0;
    if (tid >= 128 && tid < 132) trash[tid] = kEmpty;
    const int scales_done = (int)(part0 & 15u);                  //   scales 0..3 (4) or all five (5: its probe bounded scale 4 out)
    const bool probed4 = (part0 >> 4) != 0;                      //   "scale 4 was probed and cannot be bounded out"
    const bool resumed = scales_done != 0;
    for (int i = tid; i < (kMcap >> 5); i += NT) bestmask[i] = resumed ? part[kPartialHeaderDw + i] : 0u;
    if (scales_done < (p.with_scale ? 5 : 1)) {  // (a pair whose scales are all decided goes straight to the copy-out and touches neither)
        for (int i = tid; i < kFineStride; i += NT) nfine[i] = 0;
        for (int i = tid; i < 4 * kFineStride; i += NT) fdesc4[i] = 0;
    }

    const bool bad_pair = m < 0 || m > kMcap || pr.frame_a < 0 || pr.frame_a >= p.n_frames ||
                          pr.frame_b < 0 || pr.frame_b >= p.n_frames;
    int64_t offA = 0, offB = 0;
    int nA = 0, nB = 0;
    if (!bad_pair) {  // (pair-uniform values into scalar registers: see uniform())
        load_frame_ranges(p.frame_off, pr.frame_a, pr.frame_b, offA, nA, offB, nB);
    }
    const float2* __restrict__ ptsA = p.pts + offA;
    const float2* __restrict__ ptsB = p.pts + offB;
    const int mm = bad_pair ? 0 : m;
    const int n_scales = p.with_scale ? 5 : 1;
    const bool thr_fast = threshold_fast_ok(p.threshold_factor);
    uint32_t best_count = resumed ? (uint32_t)uniform((int)part_hdr.y) : 0u;
    int best_scale = resumed ? uniform((int)part_hdr.z) : -1, best_rot = resumed ? uniform((int)part_hdr.w) : -1;
    GMS_STAMP_DECL
    if (mm == 0 || nA <= 0 || nB <= 0) {  // workgroup-uniform: nothing to filter (or nothing valid to index)
        if (tid == 0) {
            gms_pair_result r;
            r.n_inliers = 0;
            r.best_scale = -1;
            r.best_rot = -1;
            r.status = (bad_pair || m > 0) ? GMS_ERR_DOMAIN : GMS_OK;
            p.results[pair_idx] = r;
        }
        return;
    }
    __syncthreads();

    if (scales_done < n_scales) {  // (workgroup-uniform; otherwise everything is decided and only the copy-out is left)
    // ---- both sides of every match, scale 0: one 8-byte load of (queryIdx, trainIdx), two gathers.
    //      Loads are unconditional on clamped indices (so that all of a thread's loads are in flight
    //      together); validity is applied to the values afterwards.
    uint32_t code[KPT];
    {
        // KPT <= 10: all of a thread's loads in flight together. KPT = 16: in two halves -- sixteen (queryIdx, trainIdx) pairs and
        // sixteen points of either frame at once are 96 registers and spilled (200 bytes of scratch per lane).
        constexpr int kLoad = KPT > 10 ? KPT / 2 : KPT;
        // The train-side gather is 8 bytes from a random line per match: the vector memory pipe takes it one
        // line at a time. When frame B's normalised points fit the (still unused) table area, copy them into LDS
        // with coalesced loads while the match loads are in flight, and gather from LDS instead.
        const bool stage_b = (uint32_t)nB * 2u <= T && nB <= 4 * mm;  // workgroup-uniform
        float2* lds_b = reinterpret_cast<float2*>(tab);
        const int wr = p.right_w[0];
        const uint32_t nr = (uint32_t)(wr * p.right_h[0]);
        const float fwr = (float)wr, fhr = (float)p.right_h[0];
        bool any_bad = false;
#pragma unroll
        for (int k0 = 0; k0 < KPT; k0 += kLoad) {
            int2 qt[kLoad];
#pragma unroll
            for (int k = 0; k < kLoad; ++k) {
                const int i = min((k0 + k) * NT + tid, mm - 1);
                qt[k] = *reinterpret_cast<const int2*>(&matches[i]);
            }
            if (k0 == 0 && stage_b) {
                for (int j = tid; j < nB; j += NT) lds_b[j] = ptsB[j];
                __syncthreads();
            }
#ifdef GMS_PHASE_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            GMS_STAMP(4);  // bin: (queryIdx, trainIdx) loads landed, frame B staged
#endif
            float2 a[kLoad], b[kLoad];
#pragma unroll
            for (int k = 0; k < kLoad; ++k) a[k] = ptsA[min((uint32_t)qt[k].x, (uint32_t)(nA - 1))];
            if (stage_b) {
#pragma unroll
                for (int k = 0; k < kLoad; ++k) b[k] = lds_b[min((uint32_t)qt[k].y, (uint32_t)(nB - 1))];
            } else {
#pragma unroll
                for (int k = 0; k < kLoad; ++k) b[k] = ptsB[min((uint32_t)qt[k].y, (uint32_t)(nB - 1))];
            }
#ifdef GMS_PHASE_TIMING
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            GMS_STAMP(12);  // bin: gathers landed
#endif
#pragma unroll
            for (int k = 0; k < kLoad; ++k) {
                const bool live = (k0 + k) * NT + tid < mm;
                // parity domain: indices in range; coordinates finite, non-negative, < 2^20 -- one unsigned
                // compare on the bit patterns (negative, NaN and Inf patterns are all above 0x49800000 = 2^20;
                // -0.0 was canonicalised away by normalize_kernel)
                const uint32_t worst = max(max(__float_as_uint(a[k].x), __float_as_uint(a[k].y)),
                                           max(__float_as_uint(b[k].x), __float_as_uint(b[k].y)));
                const float fx = 20.0f * a[k].x, fy = 20.0f * a[k].y;   // mulss, rounded to fp32
                // floor == truncation for non-negative values; 2f is exact
                const uint32_t hx = (uint32_t)(int)(fx + fx), hy = (uint32_t)(int)(fy + fy);
                // no bounds test in the reference: r = x + y * wr whatever x and y are. (Clamped to 16 bits so that the product fits the
                // 24-bit multiplier -- unclamped the compiler builds a 64-bit multiply-add; a clamped value is far beyond the grid anyway.)
                const uint32_t r = __umul24(min((uint32_t)(int)(fhr * b[k].y), 0xFFFFu), (uint32_t)wr) + min((uint32_t)(int)(fwr * b[k].x), 0xFFFFu);
                const bool ok = (uint32_t)qt[k].x < (uint32_t)nA && (uint32_t)qt[k].y < (uint32_t)nB &&
                                worst < 0x49800000u && r < nr;
                // hx >= 40 or hy >= 40: x >= 20 or y >= 20 under every grid type, never binned
                const uint32_t f = (live && ok && hx < 40u && hy < 40u) ? hy * kFineW + hx : kFineInvalid;
                if (f != kFineInvalid) atomicAdd(&nfine[f], 1u);
                any_bad |= live && !ok;
                code[k0 + k] = ((live && ok) ? r : 0u) | (f << kFShift);
            }
        }
        if (any_bad) misc[8] = 1;  // benign race: every writer stores 1
    }
    GMS_STAMP(13);    // bin: codes + half-cell histogram
    __syncthreads();  // nfine complete
    GMS_STAMP(0);     // bin: wait for the other waves

    // ---- per grid type, once per pair: nLeft of every cell, its table region, and the half-cell view of it.
    //      Regions may sit in the table in any order, so a cell simply takes the next free buckets from a
    //      per-grid-type counter (misc[12 + g]); 1600 (grid type, cell) items over the workgroup.
    for (int item = tid; item < 4 * kLeftN; item += NT) {
        const int g = item / kLeftN, cell = item - g * kLeftN;
        const int x = cell % kLeftW, y = cell / kLeftW;
        const int hx0 = 2 * x - (g & 1), hy0 = 2 * y - (g >> 1);
        uint32_t n = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int hx = hx0 + dx, hy = hy0 + dy;
                if (hx >= 0 && hy >= 0) n += nfine[hy * kFineW + hx];  // hx, hy <= 39 always
            }
        const uint32_t nb = region_buckets(n, p.region_shift);
        uint32_t d = 0;
        if (nb) d = (atomicAdd(&misc[12 + g], nb + 1u) << 16) | nb;  // header bucket + nb data buckets
        nleft4[item] = n;
        desc4[item] = d;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int hx = hx0 + dx, hy = hy0 + dy;
                if (hx >= 0 && hy >= 0) fdesc4[g * kFineStride + hy * kFineW + hx] = d;
            }
    }
    __syncthreads();
    GMS_STAMP(1);  // region tables

    // With rotation a thread always verifies the same rotation (item & 7 == tid & 7): where the rotation pattern sends each
    // of the eight outer neighbours is worked out once, as (dx + 1) | (dy + 1) << 2 in four bits per neighbour.
    uint32_t rot_pack = 0;
    if (ROT) {
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) {
            const int k = k8 < 4 ? k8 : k8 + 1;
            constexpr int kRingIndex[9] = {0, 1, 2, 7, -1, 3, 6, 5, 4};  // position -> ring index
            const int q = rotated_position(tid & 7, kRingIndex[k]);
            rot_pack |= (uint32_t)((position_dx(q) + 1) | ((position_dy(q) + 1) << 2)) << (4 * k8);
        }
    }
    for (int s = scales_done; s < n_scales; ++s) {
        const int wr = p.right_w[s], hr = p.right_h[s];

        if (s > 0) {
            // ---- getGridIndexRight again for this scale's right grid ------------------------------------------
            const uint32_t nr = (uint32_t)(wr * hr);
            const float fwr = (float)wr, fhr = (float)hr;
            constexpr int kLoad = KPT > 10 ? KPT / 2 : KPT;  // (KPT = 16: in two halves, see above)
            bool any_bad = false;
#pragma unroll
            for (int k0 = 0; k0 < KPT; k0 += kLoad) {
                int t[kLoad];
#pragma unroll
                for (int k = 0; k < kLoad; ++k) t[k] = matches[min((k0 + k) * NT + tid, mm - 1)].trainIdx;
                float2 b[kLoad];
#pragma unroll
                for (int k = 0; k < kLoad; ++k) b[k] = ptsB[min((uint32_t)t[k], (uint32_t)(nB - 1))];
#pragma unroll
                for (int k = 0; k < kLoad; ++k) {
                    const uint32_t fpart = code[k0 + k] & (kFMask << kFShift);
                    const bool had = fpart != (kFineInvalid << kFShift);  // valid at scale 0 (so indices and points are fine)
                    const uint32_t r = __umul24(min((uint32_t)(int)(fhr * b[k].y), 0xFFFFu), (uint32_t)wr) + min((uint32_t)(int)(fwr * b[k].x), 0xFFFFu);
                    const bool ok = r < nr;
                    any_bad |= had && !ok;
                    code[k0 + k] = (had && ok) ? (fpart | r) : (kFineInvalid << kFShift);
                }
            }
            if (any_bad) misc[8] = 1;
        }

        // probe (see dense_scales_pair): pass 0 only bins and flags the matches that sit in their row's arg-max entry; when
        // their number does not exceed the best count so far the scale is skipped, else pass 1 evaluates it as always
        const bool probing = ((p.probe_scales >> s) & 1) != 0 && best_count > 0 && !(s == 4 && probed4);  // workgroup-uniform
        bool skip_scale = false;
        for (int pass = probing ? 0 : 1; pass < 2 && !skip_scale; ++pass) {
        const bool probe = pass == 0;
        for (int g = 0; g < 4; ++g) {
            const uint32_t* nleft = nleft4 + g * kLeftN;
            const uint32_t* desc = desc4 + g * kLeftN;
            const uint32_t* fdesc = fdesc4 + g * kFineStride;

            // ---- motion.setTo(0) (this also resets every region header to "no arg-max yet") ------------------
            {
                const uint4 e4 = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
                uint4* tab4 = reinterpret_cast<uint4*>(tab);
                for (uint32_t i = tid; i < (T >> 2); i += NT) tab4[i] = e4;
            }
            __syncthreads();
            GMS_STAMP(2);  // clear
            // every wave is past the previous grid type's mark (it reads fres): reset it before verify writes
            for (int i = tid; i < kFineStride; i += NT) fres[i] = kNoMatch;

            // ---- assignMatchPairs: motion[l][r]++, kChunk matches in flight per thread. Written without
            //      branches: every lane issues every atomic, and a lane the operation does not apply to is
            //      pointed at its own trash dword instead (the scalar unit that all four SIMDs share, not the
            //      LDS, is what divergent exec-mask handling would saturate here).
            {
                uint32_t pending = 0;
                const uint32_t trash_add = (uint32_t)((trash - tab) + lane) << 2;        // never equals kEmpty
                const uint32_t trash_min = (uint32_t)((trash - tab) + 64 + lane) << 2;
                const uint32_t trash_bkt = (uint32_t)((trash - tab) + 128) << 2;          // one all-empty bucket
#pragma unroll
                for (int k0 = 0; k0 < KPT; k0 += kChunk) {
                    uint32_t slot[kChunk];  // byte offset of the hashed bucket, then of the match's slot
                    uint4 v[kChunk];
                    uint32_t d[kChunk];     // region of the match's left cell under this grid type, 0 = not binned
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) d[c] = fdesc[(code[k0 + c] >> kFShift) & kFMask];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t nb = d[c] & 0xFFFFu;
                        const uint32_t bo = ((d[c] >> 16) + 1u + bucket_of(code[k0 + c] & kRMask, nb)) << 4;
                        slot[c] = nb ? bo : trash_bkt;
                        v[c] = *reinterpret_cast<const uint4*>(lds_at(tab, slot[c]));
                    }
                    // round 1: "+1" where the bucket already holds the right cell, CAS into its first empty slot
                    // where it does not. Slots of a bucket fill lowest-first, so the occupied slots are a prefix.
                    // (A match that is not binned under this grid type was pointed at the trash bucket above and
                    // simply plays there: nothing it does lands in the table, and d = 0 ends its general walk at once.)
                    uint32_t o_add[kChunk], o_cas[kChunk];
                    bool fnd[kChunk], put[kChunk], pend[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t kr = (code[k0 + c] & kRMask) << kSlotRShift;
                        const int f = bucket_find(v[c], kr);
                        const int e = bucket_first_empty(v[c]);
                        fnd[c] = f >= 0;
                        put[c] = f < 0 && e >= 0;
                        pend[c] = f < 0 && e < 0;  // full bucket: leftovers
                        slot[c] += (uint32_t)(f >= 0 ? f : (e & 12));
                        o_add[c] = atomicAdd(lds_at(tab, fnd[c] ? slot[c] : trash_add), 1u);
                        o_cas[c] = atomicCAS(lds_at(tab, put[c] ? slot[c] : trash_add), kEmpty, kr | 1u);
                    }
                    __builtin_amdgcn_sched_barrier(0);  // all of the chunk's atomics are issued before any result is read
                    // round 2: a lost CAS whose winner was the same right cell (common: the true matches of a
                    // cell arrive together) becomes "+1" on that slot; any other winner sends us to the leftovers
                    uint32_t o_again[kChunk];
                    bool won[kChunk];
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t kr = (code[k0 + c] & kRMask) << kSlotRShift;
                        won[c] = put[c] && o_cas[c] == kEmpty;
                        const bool sm = put[c] && !won[c] && (o_cas[c] ^ kr) <= kSlotCountMask;
                        pend[c] = pend[c] || (put[c] && !won[c] && !sm);
                        o_again[c] = atomicAdd(lds_at(tab, sm ? slot[c] : trash_add), 1u);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    // the count this match produced, folded into the cell's running arg-max
#pragma unroll
                    for (int c = 0; c < kChunk; ++c) {
                        const uint32_t count = fnd[c] ? (o_add[c] & kSlotCountMask) + 1u
                                                      : (won[c] ? 1u : (o_again[c] & kSlotCountMask) + 1u);
                        const uint32_t key = ~((count << 11) | (2047u - (code[k0 + c] & kRMask)));
                        const uint32_t hdr = (d[c] >> 16) << 4;
                        atomicMin(lds_at(tab, (pend[c] || (d[c] & 0xFFFFu) == 0) ? trash_min : hdr), key);
                        pending |= pend[c] ? (1u << (k0 + c)) : 0u;
                    }
                }
                GMS_STAMP(3);  // insert: first-probe rounds
                // leftovers, one at a time through the general walk
                while (pending) {
                    const int k1 = __ffs(pending) - 1;
                    pending &= pending - 1u;
                    uint32_t cw = 0;
#pragma unroll
                    for (int k = 0; k < KPT; ++k) cw = (k == k1) ? code[k] : cw;
                    region_insert_general(tab, fdesc[(cw >> kFShift) & kFMask], cw & kRMask);
                }
                GMS_STAMP(10);  // insert: leftovers
            }
            __syncthreads();
            GMS_STAMP(11);  // insert: wait for the other waves
            if (probe) {  // the region header holds ~((max count << 11) | (2047 - j*)): is this match's right cell j*?
#pragma unroll
                for (int k = 0; k < KPT; ++k) {
                    const uint32_t d = fdesc[(code[k] >> kFShift) & kFMask];
                    const uint32_t bi = ~tab[(d >> 16) << 2];
                    if ((d & 0xFFFFu) != 0 && 2047u - (bi & kRMask) == (code[k] & kRMask)) code[k] |= 1u << kAccShift;
                }
                __syncthreads();  // the next grid type's clear overwrites the headers read here
                continue;
            }

            // ---- verifyCellPairs. Without rotation: two lanes per left cell, four neighbour look-ups each, joined
            //      by one DPP exchange. With rotation: one lane per (cell, rotation), eight look-ups in two rounds.
            {
                constexpr int kItems = ROT ? kLeftN * 8 : kLeftN * 2;
                for (int item = tid; item < ((kItems + 63) & ~63); item += NT) {
                    const bool live = item < kItems;
                    const int i = live ? (ROT ? (item >> 3) : (item >> 1)) : 0;
                    const int half = item & 1;  // !ROT only
                    const uint32_t ni = live ? nleft[i] : 0u;
                    if (__ballot(ni != 0) == 0ull) continue;  // none of this wave's cells has a match under this grid type
                    const uint32_t di = desc[i];
                    const uint32_t bi = ni ? ~tab[(di >> 16) << 2] : 0u;  // (max count << 11) | (2047 - j*)
                    const int j = 2047 - (int)(bi & kRMask);
                    const int jx = j % wr, jy = j / wr;
                    const int ix = i % kLeftW, iy = i / kLeftW;
                    // centre pair (k = 4): ll = i, rr = j*, whose count is the arg-max count
                    uint32_t score = 0, tn = 0;  // tn = (sum of nLeft << 4) | numpair
#pragma unroll
                    for (int h = 0; h < (ROT ? 8 : 4); h += 4) {
                        uint32_t dn[4], rq[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            int k;
                            if (ROT) {
                                const int k8 = h + c;
                                k = k8 < 4 ? k8 : k8 + 1;
                            } else {
                                k = half ? c + 5 : c;  // lane 0: neighbours 0..3, lane 1: neighbours 5..8
                            }
                            int ldx, ldy, rdx, rdy;
                            if (ROT) {
                                ldx = (k % 3) - 1; ldy = (k / 3) - 1;  // k is a compile-time constant here
                                rdx = (int)((rot_pack >> (4 * (h + c))) & 3u) - 1;
                                rdy = (int)((rot_pack >> (4 * (h + c) + 2)) & 3u) - 1;
                            } else {
                                // k = c or c + 5, both compile-time: select by lane parity
                                ldx = half ? ((c + 5) % 3) - 1 : (c % 3) - 1;
                                ldy = half ? ((c + 5) / 3) - 1 : (c / 3) - 1;
                                rdx = ldx; rdy = ldy;
                            }
                            const int lx = ix + ldx, ly = iy + ldy;
                            const int rx = jx + rdx, ry = jy + rdy;
                            // the left neighbour does not depend on j*: its two table reads go out together with the
                            // header read instead of behind it
                            const bool okl = ni != 0 && (uint32_t)lx < (uint32_t)kLeftW && (uint32_t)ly < (uint32_t)kLeftH;  // ll != -1
                            const int ll = okl ? lx + ly * kLeftW : 0;
                            const uint32_t nll = nleft[ll], dll = desc[ll];
                            const bool okp = okl && (uint32_t)rx < (uint32_t)wr && (uint32_t)ry < (uint32_t)hr;             // rr != -1
                            rq[c] = okp ? (uint32_t)(rx + ry * wr) : 0u;  // 0: matches no slot of the all-empty stand-in
                            tn += okp ? ((nll << 4) | 1u) : 0u;
                            dn[c] = okp ? dll : 0u;
                        }
                        uint4 v[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const uint32_t nb = dn[c] & 0xFFFFu;
                            v[c] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
                            if (nb) v[c] = *reinterpret_cast<const uint4*>(tab + (((dn[c] >> 16) + 1u + bucket_of(rq[c], nb)) << 2));
                        }
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const uint32_t kr = rq[c] << kSlotRShift;
                            const uint32_t cnt = bucket_count(v[c], kr);  // 0 when the bucket does not hold the right cell
                            score += cnt;
                            // slots fill lowest-first: the bucket is full iff its last slot is taken. Full and
                            // without the key: the key may sit further along the region
                            if (cnt == 0 && v[c].w != kEmpty) score += region_lookup_general(tab, dn[c], rq[c]);
                        }
                    }
                    if (!ROT) {
                        score += dpp_xor1(score);
                        tn += dpp_xor1(tn);
                    }
                    score += bi >> 11;
                    tn += (ni << 4) | 1u;
                    uint32_t pass = 0;
                    if (ni != 0 && (ROT || half == 0)) {
                        pass = threshold_rejects(tn >> 4, tn & 15u, score, p.threshold_factor, thr_fast) ? 0u : 1u;
                    }
                    uint32_t bits = pass;
                    bool writer = ni != 0 && half == 0;
                    if (ROT) {
                        const unsigned long long bal = __ballot(pass);
                        bits = (uint32_t)(bal >> (lane & 56)) & 0xFFu;
                        writer = ni != 0 && (lane & 7) == 0;
                    }
                    if (writer) {
                        // cellPairs[i] as every half-cell of cell i sees it
                        const uint32_t cr = ((uint32_t)j << 8) | bits;
                        const int hx0 = 2 * ix - (g & 1), hy0 = 2 * iy - (g >> 1);
#pragma unroll
                        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 2; ++dx) {
                                const int hx = hx0 + dx, hy = hy0 + dy;
                                if (hx >= 0 && hy >= 0) fres[hy * kFineW + hx] = cr;
                            }
                    }
                }
            }
            __syncthreads();
            GMS_STAMP(5);  // verify

            // ---- mark inliers: cellPairs[l] == r, all rotations at once ---------------------------------------
            {
                uint32_t cr[KPT];
#pragma unroll
                for (int k = 0; k < KPT; ++k) cr[k] = fres[(code[k] >> kFShift) & kFMask];
#pragma unroll
                for (int k = 0; k < KPT; ++k)
                    if ((cr[k] >> 8) == (code[k] & kRMask)) code[k] |= cr[k] << kAccShift;
            }
            GMS_STAMP(6);  // mark
        }
        if (probe) {
            uint32_t c0 = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k) c0 += (uint32_t)__popcll(__ballot((code[k] >> kAccShift) & 1u));
            if (lane == 0 && c0) atomicAdd(&misc[0], c0);
            __syncthreads();
            skip_scale = misc[0] <= best_count;
#pragma unroll
            for (int k = 0; k < KPT; ++k) code[k] &= (1u << kAccShift) - 1u;
            __syncthreads();
            if (tid == 0) {
                misc[0] = 0;
                if (p.probe_stats != nullptr) atomicAdd(&p.probe_stats[2 * s + (skip_scale ? 1 : 0)], 1u);
            }
        }
        }
        if (skip_scale) continue;

        // ---- run() return value for each rotation of this scale ---------------------------------------
        {
            uint32_t cnt[kNRot];
#pragma unroll
            for (int r = 0; r < kNRot; ++r) cnt[r] = 0;
#pragma unroll
            for (int k = 0; k < KPT; ++k)
#pragma unroll
                for (int r = 0; r < kNRot; ++r)
                    cnt[r] += (uint32_t)__popcll(__ballot((code[k] >> (kAccShift + r)) & 1u));
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < kNRot; ++r)
                    if (cnt[r]) atomicAdd(&misc[r], cnt[r]);
            }
        }
        __syncthreads();

        // ---- getInlierMask: keep on strict '>' (scale outer, rotation inner) ---------------------------
        int winner = -1;
#pragma unroll
        for (int r = 0; r < kNRot; ++r) {
            const uint32_t c = misc[r];
            if (c > best_count) {
                best_count = c;
                best_scale = s;
                best_rot = r + 1;
                winner = r;
            }
        }
        if (winner >= 0) {
#pragma unroll
            for (int k = 0; k < KPT; ++k) {
                const unsigned long long b = __ballot((code[k] >> (kAccShift + winner)) & 1u);
                if (lane == 0) {
                    const int ch = k * (NT / 64) + wave;  // chunk of 64 consecutive matches
                    bestmask[2 * ch] = (uint32_t)b;
                    bestmask[2 * ch + 1] = (uint32_t)(b >> 32);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KPT; ++k) code[k] &= (1u << kAccShift) - 1u;
        __syncthreads();
        if (tid < 8) misc[tid] = 0;
        GMS_STAMP(7);  // count + select
    }
    }
    __syncthreads();

    // ---- copy-out: surviving DMatch verbatim, in input order (DLL@0x180048340) -----------------------
    const bool failed = misc[8] != 0;
    const int n_chunks = (mm + 63) >> 6;
    {
        // exclusive scan of per-chunk popcounts; NT chunks per round, carry in misc[9]
        uint32_t* wave_tot = misc + 16;
        for (int base = 0; base < n_chunks; base += NT) {
            const int c = base + tid;
            const uint32_t v = (c < n_chunks && !failed) ? __popc(bestmask[2 * c]) + __popc(bestmask[2 * c + 1]) : 0u;
            uint32_t incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (lane == 63) wave_tot[wave] = incl;
            __syncthreads();
            uint32_t wave_off = misc[9];
            for (int w = 0; w < wave; ++w) wave_off += wave_tot[w];
            if (c < n_chunks) chunk_base[c] = wave_off + incl - v;
            __syncthreads();
            if (tid == NT - 1) misc[9] = wave_off + incl;
            __syncthreads();
        }
    }
    const uint32_t total = misc[9];
    GMS_STAMP(8);  // out scan

    gms_dmatch* __restrict__ out = p.out + pr.match_off;
    uint8_t* mask_out = p.mask ? p.mask + pr.match_off : nullptr;
    constexpr int kOut = KPT % 10 == 0 ? 10 : KPT % 8 == 0 ? 8 : kChunk;  // records requested together (nothing else is live here)
    static_assert(KPT % kOut == 0, "whole rounds");
#pragma unroll
    for (int k0 = 0; k0 < KPT; k0 += kOut) {
        uint32_t pos[kOut];
        uint4 v[kOut];
        uint32_t inm = 0;
#pragma unroll
        for (int c = 0; c < kOut; ++c) {
            const int i = (k0 + c) * NT + tid;
            const int ch = i >> 6;
            pos[c] = 0;
            bool in = false;
            if (i < mm) {
                const unsigned long long bits =
                    failed ? 0ull : ((unsigned long long)bestmask[2 * ch] | ((unsigned long long)bestmask[2 * ch + 1] << 32));
                in = (bits >> lane) & 1ull;
                if (mask_out) mask_out[i] = in ? 1 : 0;
                if (in) {
                    inm |= 1u << c;
                    pos[c] = chunk_base[ch] + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));
                }
            }
            // the survivor's record -- requested UNCONDITIONALLY, the address selected (everybody else reads the pair's first record:
            // one line): a load inside the branch is waited for inside the branch, one round trip per record, and this kernel
            // reads the records from HBM (the byte-matrix kernel had them long ago)
            v[c] = *reinterpret_cast<const uint4*>(&matches[in ? i : 0]);
        }
#pragma unroll
        for (int c = 0; c < kOut; ++c) asm volatile("" : "+v"(v[c].x), "+v"(v[c].y), "+v"(v[c].z), "+v"(v[c].w));  // (all of the round's records before its first store)
#pragma unroll
        for (int c = 0; c < kOut; ++c)
            if ((inm >> c) & 1u) *reinterpret_cast<uint4*>(&out[pos[c]]) = v[c];
    }
    GMS_STAMP(9);  // copy-out
    GMS_STAMP_FLUSH_AT(pair_idx + (resumed ? p.n_pairs : 0));  // (behind the byte-matrix kernel's stamps of the same launch)
    if (tid == 0) {
        gms_pair_result r;
        r.n_inliers = failed ? 0 : (int)total;
        r.best_scale = failed ? -1 : best_scale;
        r.best_rot = failed ? -1 : best_rot;
        r.status = failed ? GMS_ERR_DOMAIN : GMS_OK;
        p.results[pair_idx] = r;
    }
}

}  // namespace gms
