// tests/cpp/bf_select_host.cpp -- a host build of sfm-gms_amd/csrc/bf_select_core.h for the CPU tests (tests/test_bf_select_ref.py).
// The product library only runs bf_select_core.h on the GPU; this exposes its sort to ctypes.
#include "bf_select_core.h"

extern "C" {

// the first k places of MSVC std::sort over n (d, ix) records, in place
void bf_host_sort_prefix(float* d, int* ix, long n, long k)
{
    int32_t stk[3 * gms::bfsel::kSortStack];
    gms::bfsel::msvc_sort_prefix(d, ix, n, k, stk);
}
}
