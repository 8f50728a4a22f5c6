// tests/cpp/logos_host.cpp -- a host build of sfm-gms_amd/csrc/logos_core.h for the CPU tests (tests/test_logos_oracle.py).
// The product library only runs logos_core.h on the GPU; this exposes the same functions to ctypes.
#include "logos_core.h"

using namespace gms::logos;

extern "C" {

void logos_host_logf(const float* x, int n, float* y)
{
    for (int i = 0; i < n; i++) y[i] = logf_(x[i]);
}

void logos_host_acosf(const float* x, int n, float* y)
{
    for (int i = 0; i < n; i++) y[i] = acosf_(x[i]);
}

// the keypoint domain of the entry points, and the wrapped difference of two orientations (radians)
int logos_host_kp_ok(float x, float y, float angle) { return kp_ok(x, y, angle) ? 1 : 0; }

float logos_host_orientation(float angle_deg) { return orientation(angle_deg); }

float logos_host_rel_ori(float o1, float o2) { return rel_ori(o1, o2); }

// the first k places of the DLL's std::sort over n (d, ix) records, in place
void logos_host_sort_head(float* d, int* ix, long n, long k) { msvc_sort_head(d, ix, n, k); }

// support of each candidate (ci[c], cj[c]); pts*: (x, y, size, angle) per keypoint; nb*: 5 neighbour indices per keypoint (-1 pad)
void logos_host_support(const float* kp1, const int* l1, const int* nb1, const float* kp2, const int* l2, const int* nb2,
                        const long long* ci, const long long* cj, long long m, int* support, float* rel_o_out)
{
    auto pt = [](const float* k) { return Pt{k[0], k[1], orientation(k[3]), logf_(k[2])}; };
    for (long long c = 0; c < m; c++) {
        const long long i = ci[c], j = cj[c];
        const Pt p = pt(kp1 + 4 * i), q = pt(kp2 + 4 * j);
        const float ro = rel_ori(p.ori, q.ori), rs = p.logscale - q.logscale;
        int s = 0;
        for (int u = 0; u < kNum; u++) {
            const int a = nb1[kNum * i + u];
            if (a < 0) continue;
            for (int v = 0; v < kNum; v++) {
                const int b = nb2[kNum * j + v];
                if (b < 0 || l1[a] != l2[b]) continue;
                s += consistent(p, q, ro, rs, pt(kp1 + 4 * a), pt(kp2 + 4 * b)) ? 1 : 0;
            }
        }
        support[c] = s;
        rel_o_out[c] = ro;
    }
}
}
