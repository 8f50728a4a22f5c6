// logos_kernels.hip -- cv::xfeatures2d::matchLOGOS on gfx950 (LOGOS): gms_logos_match of include/gms.h.
//
// Per frame: the point table (x, y, orientation, logf(size)) and every point's five nearest other points (brute force over LDS
// tiles, squared float distance); where distances tie across the fifth place, the point is redone by the reference's own
// std::sort order (logos_core.h msvc_sort_head). Per pair, one lane per query keypoint i walks the train keypoints j in
// ascending order -- that is the DLL's candidate order -- and counts, for every candidate with nn1[i] == nn2[j], the consistent
// neighbour pairs (logos_core.h). Candidates with support go into the orientation histogram; an exclusive scan of the per-query
// counts gives every query its output range, so the survivors of the global test come out in the DLL's order without a sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gms.h"
#include "logos_core.h"

namespace gms {
void record_hip_error(int e);  // gms_capi.cpp: what gms_last_hip_error() reports
}

namespace {

using gms::logos::Pt;
constexpr int kBlock = 256;
constexpr int kNum = gms::logos::kNum;

__global__ void __launch_bounds__(kBlock) logos_points_kernel(const gms_keypoint* __restrict__ kp, int n, Pt* __restrict__ pts)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const gms_keypoint k = kp[i];
    pts[i] = Pt{k.x, k.y, gms::logos::orientation(k.angle), gms::logos::logf_(k.size)};
}

// the kNum nearest other points of each point; -1 pads when the frame has fewer than kNum + 1 points
// Ties: where more than kNum other points lie at or within the kNum-th distance, which of them the DLL keeps is the order its
// std::sort leaves them in; such points go on tie_list, and logos_knn_ties_kernel redoes them by that sort.
__global__ void __launch_bounds__(kBlock) logos_knn_kernel(const Pt* __restrict__ pts, int n, int32_t* __restrict__ nb,
                                                            int32_t* __restrict__ tie_list, int32_t* __restrict__ tie_count)
{
    __shared__ float sx[kBlock], sy[kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float x = 0.0f, y = 0.0f;
    if (i < n) {
        x = pts[i].x;
        y = pts[i].y;
    }
    float bd[kNum];
    int bi[kNum];
#pragma unroll
    for (int k = 0; k < kNum; k++) {
        bd[k] = INFINITY;
        bi[k] = -1;
    }
    for (int base = 0; base < n; base += kBlock) {
        __syncthreads();
        const int t = base + threadIdx.x;
        if (t < n) {
            sx[threadIdx.x] = pts[t].x;
            sy[threadIdx.x] = pts[t].y;
        }
        __syncthreads();
        const int cnt = min(kBlock, n - base);
        if (i < n) {
            for (int u = 0; u < cnt; u++) {
                const int j = base + u;
                if (j == i) continue;
                const float d = gms::logos::dist2(x, y, sx[u], sy[u]);
                // strict '<' against the last kept: j ascends, so an equal distance keeps the lower index in front
                if (bi[kNum - 1] >= 0 && !(d < bd[kNum - 1])) continue;
                float cd = d;
                int ci = j;
#pragma unroll
                for (int k = 0; k < kNum; k++) {
                    const bool take = bi[k] < 0 || cd < bd[k];
                    const float td = bd[k];
                    const int ti = bi[k];
                    if (take) {
                        bd[k] = cd;
                        bi[k] = ci;
                        cd = td;
                        ci = ti;
                        if (ti < 0) break;
                    }
                }
            }
        }
    }
    // second pass: how many other points lie at or within the last kept distance
    const int kk = min(kNum, n - 1);
    const float dk = kk > 0 ? bd[kk - 1] : 0.0f;
    int within = 0;
    for (int base = 0; base < n; base += kBlock) {
        __syncthreads();
        const int t = base + threadIdx.x;
        if (t < n) {
            sx[threadIdx.x] = pts[t].x;
            sy[threadIdx.x] = pts[t].y;
        }
        __syncthreads();
        const int cnt = min(kBlock, n - base);
        if (i < n && kk > 0) {
            for (int u = 0; u < cnt; u++)
                within += (base + u != i && !(dk < gms::logos::dist2(x, y, sx[u], sy[u]))) ? 1 : 0;
        }
    }
    if (i < n) {
#pragma unroll
        for (int k = 0; k < kNum; k++) nb[(int64_t)i * kNum + k] = bi[k];
        if (within > kk) tie_list[atomicAdd(tie_count, 1)] = i;
    }
}

// the points of tie_list again, by the DLL's own ordering: all n - 1 distances in index order into this lane's workspace slice
// (n - 1 floats, then n - 1 ints), MSVC std::sort over them as far as the first kNum places need, those kNum indices
__global__ void __launch_bounds__(kBlock) logos_knn_ties_kernel(const Pt* __restrict__ pts, int n, const int32_t* __restrict__ tie_list,
                                                                 int n_ties, float* __restrict__ work, int32_t* __restrict__ nb)
{
    const int lanes = gridDim.x * kBlock;
    const int lane = blockIdx.x * kBlock + threadIdx.x;
    const long m = n - 1;
    float* d = work + (size_t)lane * 2 * (size_t)m;
    int32_t* ix = reinterpret_cast<int32_t*>(d + m);
    for (int t = lane; t < n_ties; t += lanes) {
        const int i = tie_list[t];
        const float x = pts[i].x, y = pts[i].y;
        long k = 0;
        for (int j = 0; j < n; j++) {
            if (j == i) continue;
            d[k] = gms::logos::dist2(x, y, pts[j].x, pts[j].y);
            ix[k] = j;
            k++;
        }
        gms::logos::msvc_sort_head(d, ix, m, kNum);
        for (int q = 0; q < kNum; q++) nb[(int64_t)i * kNum + q] = ix[q];
    }
}

__device__ __forceinline__ int support_of(const Pt* __restrict__ p1, const int32_t* __restrict__ l1, const int32_t* __restrict__ nb1,
                                          const Pt* __restrict__ p2, const int32_t* __restrict__ l2, const int32_t* __restrict__ nb2,
                                          int i, int j, const Pt& p, const Pt& q, float rel_o, float rel_s)
{
    int s = 0;
    for (int u = 0; u < kNum; u++) {
        const int a = nb1[(int64_t)i * kNum + u];
        if (a < 0) continue;
        const int la = l1[a];
        const Pt pa = p1[a];
        for (int v = 0; v < kNum; v++) {
            const int b = nb2[(int64_t)j * kNum + v];
            if (b < 0 || l2[b] != la) continue;
            s += gms::logos::consistent(p, q, rel_o, rel_s, pa, p2[b]) ? 1 : 0;
        }
    }
    return s;
}

// pass 1: per query i, the number of candidates, the number with support, and the histogram of the supported candidates' relOri
__global__ void __launch_bounds__(kBlock) logos_support_kernel(const Pt* __restrict__ p1, const int32_t* __restrict__ l1,
                                                                const int32_t* __restrict__ nb1, int n1, const Pt* __restrict__ p2,
                                                                const int32_t* __restrict__ l2, const int32_t* __restrict__ nb2, int n2,
                                                                int64_t* __restrict__ n_cand, int64_t* __restrict__ n_supp,
                                                                int32_t* __restrict__ bins)
{
    __shared__ int32_t hist[gms::logos::kBins];
    for (int b = threadIdx.x; b < gms::logos::kBins; b += kBlock) hist[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n1) {
        const Pt p = p1[i];
        const int32_t li = l1[i];
        int64_t nc = 0, ns = 0;
        for (int j = 0; j < n2; j++) {
            if (l2[j] != li) continue;
            nc++;
            const Pt q = p2[j];
            const float rel_o = gms::logos::rel_ori(p.ori, q.ori);
            const float rel_s = p.logscale - q.logscale;
            if (support_of(p1, l1, nb1, p2, l2, nb2, i, j, p, q, rel_o, rel_s) > 0) {
                ns++;
                atomicAdd(&hist[gms::logos::bin_of(rel_o)], 1);
            }
        }
        n_cand[i] = nc;
        n_supp[i] = ns;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < gms::logos::kBins; b += kBlock)
        if (hist[b]) atomicAdd(&bins[b], hist[b]);
}

// the peak of the histogram (one lane: 189 bins)
__global__ void logos_peak_kernel(const int32_t* __restrict__ bins, float* __restrict__ peak, int32_t* __restrict__ peak_bin)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int b = 0;
    *peak = gms::logos::peak_orientation(bins, &b);
    *peak_bin = b;
}

// pass 2 (count) and pass 3 (write): the supported, globally consistent candidates of query i, in ascending j
template <bool kWrite>
__global__ void __launch_bounds__(kBlock) logos_select_kernel(const Pt* __restrict__ p1, const int32_t* __restrict__ l1,
                                                               const int32_t* __restrict__ nb1, int n1, const Pt* __restrict__ p2,
                                                               const int32_t* __restrict__ l2, const int32_t* __restrict__ nb2, int n2,
                                                               const float* __restrict__ peak, int64_t* __restrict__ n_keep,
                                                               const int64_t* __restrict__ off, gms_dmatch* __restrict__ out)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n1) return;
    const float g = *peak;
    const Pt p = p1[i];
    const int32_t li = l1[i];
    int64_t k = 0;
    int64_t o = kWrite ? off[i] : 0;
    for (int j = 0; j < n2; j++) {
        if (l2[j] != li) continue;
        const Pt q = p2[j];
        const float rel_o = gms::logos::rel_ori(p.ori, q.ori);
        if (!gms::logos::globally_consistent(rel_o, g)) continue;
        const float rel_s = p.logscale - q.logscale;
        if (support_of(p1, l1, nb1, p2, l2, nb2, i, j, p, q, rel_o, rel_s) == 0) continue;
        if (kWrite) out[o++] = gms_dmatch{i, j, -1, 0.0f};
        k++;
    }
    if (!kWrite) n_keep[i] = k;
}

// exclusive scan of n int64 counts in one workgroup; off[n] = total
__global__ void __launch_bounds__(1024) logos_scan_kernel(const int64_t* __restrict__ cnt, int n, int64_t* __restrict__ off)
{
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int64_t s = 0;
    for (int k = lo; k < hi; k++) s += cnt[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int k = lo; k < hi; k++) {
        off[k] = run;
        run += cnt[k];
    }
    if (t == 1023) off[n] = part[1023];
}

int hip_ok(hipError_t e)
{
    if (e == hipSuccess) return GMS_OK;
    gms::record_hip_error((int)e);
    return GMS_ERR_HIP;
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

int blocks(int n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

extern "C" int gms_logos_match(const gms_keypoint* kp1, int n1, const gms_keypoint* kp2, int n2, const int32_t* nn1, const int32_t* nn2,
                               gms_dmatch* out, int64_t out_cap, int64_t* n_out, gms_logos_result* result)
{
    if (n_out) *n_out = 0;
    if (result) *result = gms_logos_result{0, 0, 0, -1, GMS_OK};
    if (n1 < 0 || n2 < 0 || out_cap < 0 || !n_out) return GMS_ERR_BAD_ARG;
    if ((n1 > 0 && (!kp1 || !nn1)) || (n2 > 0 && (!kp2 || !nn2)) || (out_cap > 0 && !out)) return GMS_ERR_BAD_ARG;
    // the keypoint domain (logos_core.h kp_ok), before any allocation or copy: outside it the wrap loops of rel_ori would not end
    for (int f = 0; f < 2; f++) {
        const gms_keypoint* k = f ? kp2 : kp1;
        for (int i = 0, m = f ? n2 : n1; i < m; i++) {
            if (gms::logos::kp_ok(k[i].x, k[i].y, k[i].angle)) continue;
            if (result) result->status = GMS_ERR_DOMAIN;
            return GMS_ERR_DOMAIN;
        }
    }
    if (n1 == 0 || n2 == 0) return GMS_OK;

    DevBuf kp, lab, pts, nb, cnt, bins, peak, keep, koff, dout, ties, work;
    const int n = n1 + n2;
    int rc;
#define LOGOS_TRY(x) do { if ((rc = hip_ok(x)) != GMS_OK) return rc; } while (0)
    LOGOS_TRY(kp.alloc(sizeof(gms_keypoint) * (size_t)n));
    LOGOS_TRY(lab.alloc(sizeof(int32_t) * (size_t)n));
    LOGOS_TRY(pts.alloc(sizeof(Pt) * (size_t)n));
    LOGOS_TRY(nb.alloc(sizeof(int32_t) * kNum * (size_t)n));
    LOGOS_TRY(cnt.alloc(sizeof(int64_t) * 2 * (size_t)n1));
    LOGOS_TRY(bins.alloc(sizeof(int32_t) * gms::logos::kBins));
    LOGOS_TRY(peak.alloc(sizeof(float) + sizeof(int32_t)));
    LOGOS_TRY(keep.alloc(sizeof(int64_t) * (size_t)n1));
    LOGOS_TRY(koff.alloc(sizeof(int64_t) * ((size_t)n1 + 1)));
    LOGOS_TRY(ties.alloc(sizeof(int32_t) * ((size_t)n + 2)));
    gms_keypoint* d_kp = kp.as<gms_keypoint>();
    int32_t* d_lab = lab.as<int32_t>();
    Pt* d_pts = pts.as<Pt>();
    int32_t* d_nb = nb.as<int32_t>();
    LOGOS_TRY(hipMemcpy(d_kp, kp1, sizeof(gms_keypoint) * (size_t)n1, hipMemcpyHostToDevice));
    LOGOS_TRY(hipMemcpy(d_kp + n1, kp2, sizeof(gms_keypoint) * (size_t)n2, hipMemcpyHostToDevice));
    LOGOS_TRY(hipMemcpy(d_lab, nn1, sizeof(int32_t) * (size_t)n1, hipMemcpyHostToDevice));
    LOGOS_TRY(hipMemcpy(d_lab + n1, nn2, sizeof(int32_t) * (size_t)n2, hipMemcpyHostToDevice));
    LOGOS_TRY(hipMemset(bins.p, 0, sizeof(int32_t) * gms::logos::kBins));
    LOGOS_TRY(hipMemset(ties.p, 0, sizeof(int32_t) * 2));

    const Pt *p1 = d_pts, *p2 = d_pts + n1;
    const int32_t *l1 = d_lab, *l2 = d_lab + n1, *nb1 = d_nb, *nb2 = d_nb + (size_t)kNum * n1;
    int64_t* n_cand = cnt.as<int64_t>();
    int64_t* n_supp = n_cand + n1;
    float* d_peak = peak.as<float>();
    int32_t* d_peak_bin = reinterpret_cast<int32_t*>(d_peak + 1);

    logos_points_kernel<<<blocks(n), kBlock>>>(d_kp, n, d_pts);
    int32_t* tie_count = ties.as<int32_t>();    // [2]: frame 1, frame 2; then the two lists
    int32_t* tie_list1 = tie_count + 2;
    int32_t* tie_list2 = tie_list1 + n1;
    logos_knn_kernel<<<blocks(n1), kBlock>>>(p1, n1, d_nb, tie_list1, tie_count);
    logos_knn_kernel<<<blocks(n2), kBlock>>>(p2, n2, d_nb + (size_t)kNum * n1, tie_list2, tie_count + 1);
    LOGOS_TRY(hipGetLastError());
    int32_t n_ties[2] = {0, 0};
    LOGOS_TRY(hipMemcpy(n_ties, tie_count, sizeof n_ties, hipMemcpyDeviceToHost));
    if (n_ties[0] > 0 || n_ties[1] > 0) {
        // one workspace slice of 2 (n - 1) words per lane, at most 256 MiB in all
        const size_t slice = 2 * sizeof(float) * (size_t)(std::max(n1, n2) - 1);
        const int max_ties = std::max(n_ties[0], n_ties[1]);
        const int lanes = (int)std::min<size_t>((size_t)blocks(max_ties) * kBlock,
                                                std::max<size_t>(kBlock, ((size_t)256 << 20) / slice / kBlock * kBlock));
        LOGOS_TRY(work.alloc(slice * (size_t)lanes));
        if (n_ties[0] > 0)
            logos_knn_ties_kernel<<<lanes / kBlock, kBlock>>>(p1, n1, tie_list1, n_ties[0], work.as<float>(), d_nb);
        if (n_ties[1] > 0)
            logos_knn_ties_kernel<<<lanes / kBlock, kBlock>>>(p2, n2, tie_list2, n_ties[1], work.as<float>(),
                                                             d_nb + (size_t)kNum * n1);
    }
    logos_support_kernel<<<blocks(n1), kBlock>>>(p1, l1, nb1, n1, p2, l2, nb2, n2, n_cand, n_supp, bins.as<int32_t>());
    logos_peak_kernel<<<1, 64>>>(bins.as<int32_t>(), d_peak, d_peak_bin);
    logos_select_kernel<false><<<blocks(n1), kBlock>>>(p1, l1, nb1, n1, p2, l2, nb2, n2, d_peak, keep.as<int64_t>(), nullptr, nullptr);
    logos_scan_kernel<<<1, 1024>>>(keep.as<int64_t>(), n1, koff.as<int64_t>());
    LOGOS_TRY(hipGetLastError());

    int64_t total = 0;
    std::vector<int64_t> counts(2 * (size_t)n1);
    int32_t peak_bin = -1;
    LOGOS_TRY(hipMemcpy(&total, koff.as<int64_t>() + n1, sizeof(int64_t), hipMemcpyDeviceToHost));
    LOGOS_TRY(hipMemcpy(counts.data(), n_cand, sizeof(int64_t) * 2 * (size_t)n1, hipMemcpyDeviceToHost));
    LOGOS_TRY(hipMemcpy(&peak_bin, d_peak_bin, sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t nc = 0, ns = 0;
    for (int k = 0; k < n1; k++) {
        nc += counts[k];
        ns += counts[(size_t)n1 + k];
    }
    if (result) *result = gms_logos_result{nc, ns, total, ns ? peak_bin : -1, GMS_OK};
    *n_out = total;
    if (total > out_cap) {
        if (result) result->status = GMS_ERR_CAPACITY;
        return GMS_ERR_CAPACITY;
    }
    if (total == 0) return GMS_OK;
    LOGOS_TRY(dout.alloc(sizeof(gms_dmatch) * (size_t)total));
    logos_select_kernel<true><<<blocks(n1), kBlock>>>(p1, l1, nb1, n1, p2, l2, nb2, n2, d_peak, nullptr, koff.as<int64_t>(),
                                                      dout.as<gms_dmatch>());
    LOGOS_TRY(hipGetLastError());
    LOGOS_TRY(hipMemcpy(out, dout.p, sizeof(gms_dmatch) * (size_t)total, hipMemcpyDeviceToHost));
#undef LOGOS_TRY
    return GMS_OK;
}
