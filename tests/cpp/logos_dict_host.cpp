// tests/cpp/logos_dict_host.cpp -- a host build of sfm-gms_amd/csrc/logos_dict_core.h for the CPU tests
// (tests/test_logos_dict_ref.py): the draws, distances, weights and the quantised mean the trainer's kernels run, exposed to ctypes.
#include "logos_dict_core.h"

using namespace gms::logos_dict;

extern "C" {

unsigned long long dict_host_draw(unsigned long long seed, unsigned long long set, unsigned long long attempt, unsigned long long centre,
                                  unsigned long long trial)
{
    return draw(seed, set, attempt, centre, trial);
}

unsigned long long dict_host_mulhi64(unsigned long long a, unsigned long long b) { return mulhi64(a, b); }

// rows [n, 128] against one centre: the fp32 distance and its weight
void dict_host_l2(const float* rows, long long n, const float* centre, float* d, unsigned long long* w)
{
    for (long long i = 0; i < n; i++) {
        d[i] = l2_sq(rows + i * kL2Dims, centre);
        w[i] = l2_weight(d[i]);
    }
}

void dict_host_hamming(const uint32_t* rows, long long n, const uint32_t* centre, unsigned long long* w)
{
    for (long long i = 0; i < n; i++) w[i] = hamming_weight(rows + i * kHammingWords, centre);
}

void dict_host_in_domain(const float* x, long long n, int* ok)
{
    for (long long i = 0; i < n; i++) ok[i] = l2_in_domain(x[i]) ? 1 : 0;
}

void dict_host_quantise(const float* x, long long n, long long* q)
{
    for (long long i = 0; i < n; i++) q[i] = quantise(x[i]);
}

// the mean of n rows of `dims` elements
void dict_host_mean(const float* rows, long long n, int dims, float* out)
{
    for (int k = 0; k < dims; k++) {
        int64_t s = 0;
        for (long long i = 0; i < n; i++) s += quantise(rows[i * dims + k]);
        out[k] = l2_mean(s, n);
    }
}

int dict_host_majority(long long ones, long long count) { return majority(ones, count) ? 1 : 0; }

long long dict_host_workspace_bytes(int kind, long long total_rows, int n_sets, int n_words, int attempts, int max_iters)
{
    const Params p = {kind, n_sets, n_words, attempts, max_iters, kind == 0 ? 32 : 512, total_rows, 0};
    return params_ok(p) ? layout(p).total : 0;
}

}  // extern "C"
