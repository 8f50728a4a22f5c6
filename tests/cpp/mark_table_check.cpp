// tests/test_mark_table_layout.py: the half-cell rule of the byte-matrix kernel's mark table (dense_half_cell_owner in
// gms_kernel_dense.h) as plain arithmetic, no device. For all 1600 half cells x 4 grid types the owning cell is what a match's code
// word yields -- row = cell under grid type 1 + (q & (gx + 20 gy)), nobody where an edge bit meets a shifted axis --, and every
// (cell, grid type) owns exactly the half cells that dense_nleft_cm sums for it. Prints "mark_table: ok" or the first violation.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "gms_kernel_dense.h"

static int fail(const char* what, int hx, int hy, int g, int got, int want)
{
    std::printf("mark_table: %s at half cell (%d, %d), grid type %d: %d, expected %d\n", what, hx, hy, g + 1, got, want);
    return 1;
}

int main()
{
    using namespace gms;
    static_assert(kFineW == 2 * kLeftW && kFineN == 4 * kLeftN, "four half cells per cell");
    static_assert(kDenseMarkTableOff % 8 == 0 && kDenseMarkVerdictOff % 8 == 0, "8-byte entries");
    static_assert(kDenseMarkVerdictOff + 8u * kLeftN <= kDenseMarkTableOff && kDenseMarkTableOff + 8u * kDenseMarkEntries <= kDenseBytes,
                  "verdicts and table lie inside the matrix area, apart");
    static_assert(kDenseMarkSinkSlot >= (uint32_t)kFineN && kDenseMarkSinkSlot < kDenseMarkEntries, "the sink's entry is nobody's half cell");
    static uint8_t hist[kFineN];
    int owned[4][kLeftN];
    std::memset(owned, 0, sizeof owned);
    for (int hy = 0; hy < kFineW; ++hy)
        for (int hx = 0; hx < kFineW; ++hx) {
            // what normalize_kernel puts into a left code: the cell under grid type 1, q, the edge bits
            const int cell1 = (hy >> 1) * kLeftW + (hx >> 1);
            const int q = (hx & 1) + 20 * (hy & 1);
            const bool edge_x = hx == kFineW - 1, edge_y = hy == kFineW - 1;
            // its byte of the half-cell histogram and its entry of the mark table, as a match finds it from its code word
            const int slot = (int)dense_half_cell_slot(hx, hy);
            if (slot != 4 * cell1 + (q & 1) + ((q & 4) >> 1)) return fail("slot", hx, hy, 0, slot, 4 * cell1 + (q & 1) + ((q & 4) >> 1));
            std::memset(hist, 0, sizeof hist);
            hist[slot] = 1;
            for (int g = 0; g < 4; ++g) {
                const int gx = g & 1, gy = g >> 1;
                const bool binned = !((gx && edge_x) || (gy && edge_y));
                const int row = cell1 + (q & (gx + 20 * gy));
                const int owner = dense_half_cell_owner(hx, hy, gx, gy);
                if (owner != (binned ? row : -1)) return fail("owner against the code-word rule", hx, hy, g, owner, binned ? row : -1);
                if (owner >= kLeftN) return fail("owner outside the grid", hx, hy, g, owner, kLeftN - 1);
                if (owner >= 0) ++owned[g][owner];
                // the only cell whose nLeft counts this half cell is its owner
                for (int cell = 0; cell < kLeftN; ++cell) {
                    const int n = (int)dense_nleft_cm(hist, cell % kLeftW, cell / kLeftW, gx, gy);
                    if (n != (cell == owner ? 1 : 0)) return fail("dense_nleft_cm of another cell", hx, hy, g, n, cell == owner ? 1 : 0);
                }
            }
        }
    // a cell owns four half cells, two where a shifted axis cuts it at the image's first half row or column, one in that corner
    for (int g = 0; g < 4; ++g)
        for (int cell = 0; cell < kLeftN; ++cell) {
            const int gx = g & 1, gy = g >> 1;
            const int want = ((gx && cell % kLeftW == 0) ? 1 : 2) * ((gy && cell / kLeftW == 0) ? 1 : 2);
            if (owned[g][cell] != want) return fail("half cells of a cell", cell % kLeftW, cell / kLeftW, g, owned[g][cell], want);
        }
    std::printf("mark_table: ok\n");
    return 0;
}
