// tests/test_mark_scatter_layout.py: who writes which field of the byte-matrix kernel's mark table (gms_kernel_dense.h), as plain
// arithmetic, no device. The kernel's verifying lanes store their verdicts straight into the table -- lane t, cell t >> 1, grid types
// 2 (t & 1) and 2 (t & 1) + 1, the four half cells dense_cell_half_slot() names, unpredicated --, the idle lanes store "none" into
// the fields dense_mark_none_field() enumerates. This program replays both with the header's functions over all
// kDenseMarkEntries x 4 fields: every field has exactly one writer (a clamped store repeats one of its writer's own), the writer of
// an owned field is dense_half_cell_owner()'s cell, and the none-writers' fields are exactly those that function gives to nobody
// plus the entries from kFineN up to the sink's. Prints "mark_scatter: ok" or the first violation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gms_kernel_dense.h"

static int fail(const char* what, long a, long b, long got, long want)
{
    std::printf("mark_scatter: %s at (%ld, %ld): %ld, expected %ld\n", what, a, b, got, want);
    return 1;
}

int main()
{
    using namespace gms;
    constexpr int kThreads = 1024;  // the workgroup of every instantiation of the kernel
    constexpr uint32_t kFields = 4u * kDenseMarkEntries;
    static_assert(kThreads > 2 * kLeftN, "there are idle lanes");
    static_assert(dense_mark_field_off(kFields - 1u) + 2u == kDenseMarkTableOff + 8u * kDenseMarkEntries && dense_mark_field_off(0) == kDenseMarkTableOff,
                  "fields are the table's 16-bit words, in order");
    constexpr int kNobody = -2, kNone = -1;  // writer of a field: a cell, kNone for a none-writer
    std::vector<int> writer(kFields, kNobody), hits(kFields, 0);

    // ---- the verifying lanes
    for (int t = 0; t < 2 * kLeftN; ++t) {
        const int cell = t >> 1, x = cell % kLeftW, y = cell / kLeftW;
        for (int j = 0; j < 2; ++j) {
            const int g = 2 * (t & 1) + j, gx = g & 1, gy = g >> 1;
            int real = 0;
            // the stores whose half cell exists, then the clamped ones: those must repeat one of the first kind
            for (int pass = 0; pass < 2; ++pass)
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        const int hx = 2 * x - gx + dx, hy = 2 * y - gy + dy;
                        const bool clamped = hx < 0 || hy < 0;
                        if (clamped != (pass == 1)) continue;
                        const uint32_t slot = dense_cell_half_slot(x, y, gx, gy, dx, dy);
                        if (slot >= (uint32_t)kFineN) return fail("slot outside the half cells", cell, g, slot, kFineN - 1);
                        const uint32_t f = 4u * slot + (uint32_t)g;
                        if (!clamped) {
                            if (slot != dense_half_cell_slot(hx, hy)) return fail("slot of a half cell", cell, g, slot, dense_half_cell_slot(hx, hy));
                            if (dense_half_cell_owner(hx, hy, gx, gy) != cell) return fail("owner of a written field", hx, hy, dense_half_cell_owner(hx, hy, gx, gy), cell);
                            if (writer[f] != kNobody) return fail("second writer of a field", slot, g, cell, writer[f]);
                            writer[f] = cell;
                            ++hits[f];
                            ++real;
                        } else if (writer[f] != cell || hits[f] != 1) {
                            return fail("clamped store outside its writer's fields", slot, g, writer[f], cell);
                        }
                    }
            const int want = ((gx && x == 0) ? 1 : 2) * ((gy && y == 0) ? 1 : 2);
            if (real != want) return fail("half cells of a cell", cell, g, real, want);
        }
    }

    // ---- the idle lanes: the loop the kernel runs
    long none_fields = 0;
    for (int t = 2 * kLeftN; t < kThreads; ++t)
        for (uint32_t u = (uint32_t)(t - 2 * kLeftN); u < kDenseMarkNoneFields; u += (uint32_t)(kThreads - 2 * kLeftN)) {
            const uint32_t f = dense_mark_none_field(u);
            if (f >= kFields) return fail("none field outside the table", t, u, f, kFields - 1);
            if (writer[f] != kNobody) return fail("second writer of a field (none)", f >> 2, f & 3, kNone, writer[f]);
            writer[f] = kNone;
            ++hits[f];
            ++none_fields;
        }
    if (none_fields != (long)kDenseMarkNoneFields) return fail("none fields written", 0, 0, none_fields, kDenseMarkNoneFields);

    // ---- every field once; the none-writers' set is where nobody owns the half cell, and the entries behind the grid
    long unowned = 0;
    for (uint32_t f = 0; f < kFields; ++f) {
        const uint32_t slot = f >> 2;
        const int g = (int)(f & 3u);
        if (hits[f] != 1) return fail("writers of a field", slot, g, hits[f], 1);
        int owner = -1;
        if (slot < (uint32_t)kFineN) {
            const int c1 = (int)(slot >> 2), hx = 2 * (c1 % kLeftW) + (int)(slot & 1u), hy = 2 * (c1 / kLeftW) + (int)((slot >> 1) & 1u);
            if (dense_half_cell_slot(hx, hy) != slot) return fail("slot round trip", hx, hy, dense_half_cell_slot(hx, hy), slot);
            owner = dense_half_cell_owner(hx, hy, g & 1, g >> 1);
            if (owner < 0) ++unowned;
        }
        if (writer[f] != (owner >= 0 ? owner : kNone)) return fail("writer of a field", slot, g, writer[f], owner >= 0 ? owner : kNone);
    }
    if (unowned != (long)kDenseMarkUnownedFields) return fail("fields nobody owns", 0, 0, unowned, kDenseMarkUnownedFields);
    if (kDenseMarkNoneFields != kDenseMarkUnownedFields + 4u * (kDenseMarkEntries - (uint32_t)kFineN))
        return fail("none fields", 0, 0, kDenseMarkNoneFields, kDenseMarkUnownedFields + 4u * (kDenseMarkEntries - (uint32_t)kFineN));
    std::printf("mark_scatter: ok\n");
    return 0;
}
