// sfm_ba_kernels.hip -- bundle adjustment behind the registration (the arithmetic is sfm_ba_core.h, the workspace
// SfmBaLayout in ws_layout.h). Stream-ordered launches in a fixed sequence, no grid-wide barrier, nothing else:
//
//   sba_init_kernel        every workspace word a later kernel reads; the outputs start as copies of the inputs
//   sba_mark_kernel        one workgroup per pair: rank by wave ballots, then per kept match of an ok pair the cloud entry of its track
//                          (binary search in d_cloud_id) written at both keypoints -- the observation table
//   sba_count_kernel       per keypoint: its track's count (integer atomic) and its undistorted measurement
//   sba_tile / sba_scan / sba_offsets_kernel   the exclusive prefix of the counts over the cloud entries
//   sba_fill_kernel        the tracks' lists (integer atomic cursor; the order is mended next)
//   sba_tracks_kernel      one lane per track: its list sorted by keypoint, two keypoints of a frame, the status, re-triangulation
//   per outer iteration:
//   sba_linearise_kernel   per observation: sqrt(w) Jc, sqrt(w) Jp, sqrt(w) r at the current views and points
//   sba_track_build_kernel one lane per track: (V + lambda diag V)^-1 and -sum Jp^T r, in list order
//   sba_frame_build_kernel one workgroup per frame: U, the reduced right-hand side, the preconditioner's Cholesky factor
//   sba_cg_init_kernel     one workgroup: x = 0, r = b, z = M^-1 r, p = z
//   n_cg times  sba_cg_track_kernel   one lane per track:     q_t = V^-1 sum W_o^T p_f(o)              } the hot pair
//               sba_cg_frame_kernel   one workgroup per frame: q_f = U_f p_f - sum W_o q_t(o)           }
//               sba_cg_update_kernel  one workgroup: alpha, x, r, z, the stopping rule, beta, p
//   sba_step_kernel        the points back-substituted and the candidate views
//   sba_cost_kernel        one workgroup per frame: Huber cost, sum of squares and active count of its observations
//   sba_decide_kernel      one workgroup: accept or drop, lambda, the flags; an accepted step's views
//   sba_commit_kernel      an accepted step's points
//   sba_final_kernel / sba_points_kernel   the gauge factor, the summary, the rescale
// After "done" the device-side flag turns every kernel of the loop into a no-op. Sums: a track's run in its list's order on one
// lane; a frame's and the ones over frames as lane-strided partial sums folded in one fixed tree (wave shuffles, then the four
// waves in order). The only atomics are integer sums and one integer minimum. LDS: at most 1028 bytes per workgroup (the prefix
// sum's 257 ints; the widest fold, the 21 entries of a symmetric 6 x 6 from 4 waves, takes 672), against the 160 KB of a CU: LDS
// never limits occupancy here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gms_kernels.h"
#include "sfm_ba_core.h"
#include "twoview_core.h"

namespace gms {
namespace {

constexpr int kB = 256;
enum { kLambda = 0, kCost, kSq, kRz, kRz0, kCost0, kSq0, kFactor };                              // scal
enum { kLmDone = 0, kCgDone, kAcceptedNow, kItersRun, kItersAcc, kCgIters, kActive = 8, kActive0 = 10 };  // flags (kActive*: int64)

struct SbaIn {
    const gms_keypoint* kp;
    const int64_t* frame_off;
    const gms_pair* pairs;
    const gms_dmatch* matches;
    const uint8_t* mask;
    const gms_sfm_view* views;
    const gms_sfm_pair_reg* reg;
    const int32_t* track;
    const double* cloud;
    const int32_t* cloud_id;
    const gms_sfm_summary* reg_summary;
    int64_t total_kp, total_m, cloud_cap;
    int n_frames, n_pairs;
};
struct SbaWs {
    int32_t *kp_track, *kp_frame, *list;
    double *uv, *jc, *jp, *res;
    int32_t *t_cnt, *t_off, *t_fill, *t_used, *tiles;
    double *xc, *vinv, *gp, *qt;
    gms_sfm_view* cand;
    double *U, *L;
    int32_t *lok, *free_;
    double *b, *x, *r, *z, *p, *q, *part, *costp;
    long long* actp;
    double* scal;
    int32_t* flags;
};
struct SbaOut {
    gms_sfm_view* views;
    double* cloud;
    int32_t* status;
    gms_sfm_ba_summary* summary;
};

__device__ __forceinline__ int64_t n_cloud(const SbaIn& in)
{
    const int64_t n = in.reg_summary->n_tracks;
    return n < 0 ? 0 : (n < in.cloud_cap ? n : in.cloud_cap);
}

// v[i] summed over the workgroup, for every lane: lane-order tree inside a wave, then the waves in order. s: kB / 64 * N doubles.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* s, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < N; i++) {
        double a = v[i];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
        if (lane == 0) s[wave * N + i] = a;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = ((s[i] + s[N + i]) + s[2 * N + i]) + s[3 * N + i];
    __syncthreads();
}

// the keypoints of frame f, inside the arrays
__device__ __forceinline__ void frame_range(const SbaIn& in, int f, int64_t& g0, int64_t& g1)
{
    g0 = in.frame_off[f];
    g1 = in.frame_off[f + 1];
    if (g0 < 0) g0 = 0;
    if (g1 > in.total_kp) g1 = in.total_kp;
}

__global__ void __launch_bounds__(kB)
sba_init_kernel(SbaIn in, SbaWs ws, SbaOut out, double lambda0)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g < in.total_kp) {
        ws.kp_track[g] = -1;
        ws.kp_frame[g] = 0;
        ws.list[g] = 0;
    }
    if (g < in.cloud_cap) {
        ws.t_cnt[g] = 0;
        ws.t_off[g] = 0;
        ws.t_fill[g] = 0;
        ws.t_used[g] = 0;
        for (int e = 0; e < 3; e++) out.cloud[3 * g + e] = in.cloud[3 * g + e];
        out.status[g] = sba::kFew;
    }
    if (g < in.n_frames) {
        const gms_sfm_view v = in.views[g];
        out.views[g] = v;
        ws.cand[g] = v;
        ws.free_[g] = (v.registered != 0 && v.pair >= 0) ? 1 : 0;
        ws.lok[g] = 0;
        for (int e = 0; e < 6; e++) ws.b[6 * g + e] = ws.x[6 * g + e] = ws.r[6 * g + e] = ws.z[6 * g + e] = ws.p[6 * g + e] = ws.q[6 * g + e] = 0.0;
        ws.part[g] = 0.0;
        ws.costp[2 * g] = ws.costp[2 * g + 1] = 0.0;
        ws.actp[g] = 0;
    }
    if (g == 0) {
        for (int e = 0; e < 16; e++) {
            ws.scal[e] = 0.0;
            ws.flags[e] = 0;
        }
        ws.scal[kLambda] = lambda0;
        ws.scal[kFactor] = 1.0;
        *out.summary = gms_sfm_ba_summary{};
    }
}

__global__ void __launch_bounds__(kB)
sba_mark_kernel(SbaIn in, SbaWs ws)
{
    __shared__ unsigned s_wave[kB / 64];
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gms_pair pr = in.pairs[i];
    // (uniform over the workgroup) a pair whose frames, offsets or match range do not fit the arrays has no observations
    if (in.reg[i].status != GMS_OK) return;
    // (match_off against total_m - m: their sum need not fit 64 bits)
    if (pr.frame_a < 0 || pr.frame_a >= in.n_frames || pr.frame_b < 0 || pr.frame_b >= in.n_frames || pr.m < 0 || pr.match_off < 0 ||
        pr.match_off > in.total_m - (int64_t)pr.m)
        return;
    if (!in.views[pr.frame_a].registered || !in.views[pr.frame_b].registered) return;
    const int64_t oa = in.frame_off[pr.frame_a], ob = in.frame_off[pr.frame_b];
    const int64_t na = in.frame_off[pr.frame_a + 1] - oa, nb = in.frame_off[pr.frame_b + 1] - ob;
    if (oa < 0 || ob < 0 || na < 0 || nb < 0 || oa + na > in.total_kp || ob + nb > in.total_kp) return;
    const int64_t nc = n_cloud(in);
    unsigned before_all = 0;
    for (int base = 0; base < pr.m; base += kB) {
        const int k = base + tid;
        const bool set = k < pr.m && in.mask[pr.match_off + k] != 0;
        const unsigned long long bal = __ballot(set);
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned before = before_all, total = 0;
        for (int w = 0; w < kB / 64; ++w) {
            before += w < wave ? s_wave[w] : 0u;
            total += s_wave[w];
        }
        __syncthreads();
        before_all += total;
        if (!set) continue;
        const unsigned rank = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));  // (rank <= k < m: inside the pair's range)
        const gms_dmatch m = in.matches[pr.match_off + k];
        if ((uint32_t)m.queryIdx >= (uint32_t)na || (uint32_t)m.trainIdx >= (uint32_t)nb) continue;
        const int32_t T = in.track[pr.match_off + rank];
        if (T < 0) continue;
        int64_t lo = 0, hi = nc;  // the first entry with cloud_id >= T
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (in.cloud_id[mid] < T) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= nc || in.cloud_id[lo] != T) continue;
        const int64_t ga = oa + m.queryIdx, gb = ob + m.trainIdx;  // (every writer of a keypoint stores the same values: one component)
        ws.kp_track[ga] = (int32_t)lo;
        ws.kp_frame[ga] = pr.frame_a;
        ws.kp_track[gb] = (int32_t)lo;
        ws.kp_frame[gb] = pr.frame_b;
    }
}

__global__ void __launch_bounds__(kB)
sba_count_kernel(SbaIn in, SbaWs ws, tv::Camera cam)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g >= in.total_kp) return;
    const int c = ws.kp_track[g];
    if (c < 0) return;
    atomicAdd(&ws.t_cnt[c], 1);
    double u, v;
    tv::undistort_point(cam, (double)in.kp[g].x, (double)in.kp[g].y, u, v);
    ws.uv[2 * g] = u;
    ws.uv[2 * g + 1] = v;
}

// exclusive prefix of t_cnt over the cloud entries: tile t holds entries [t * kSbaScanTile, ...), thread tid kPerThread consecutive ones
constexpr int kPerThread = kSbaScanTile / kB;

__device__ __forceinline__ int tile_scan(int v, int* s, int tid)  // exclusive prefix of v over the workgroup; s[kB] = the total
{
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kB; o <<= 1) {
        const int x = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    if (tid == kB - 1) s[kB] = s[tid];
    const int incl = s[tid];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kB)
sba_tile_kernel(SbaWs ws, int64_t cloud_cap)
{
    __shared__ int s[kB + 1];
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kSbaScanTile + (int64_t)tid * kPerThread;
    int n = 0;
    for (int e = 0; e < kPerThread; e++) n += c0 + e < cloud_cap ? ws.t_cnt[c0 + e] : 0;
    tile_scan(n, s, tid);
    if (tid == 0) ws.tiles[blockIdx.x] = s[kB];
}

__global__ void __launch_bounds__(kB)
sba_scan_kernel(SbaWs ws, int n_tiles)
{
    __shared__ int s[kB + 1];
    const int tid = (int)threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n_tiles; base += kB) {
        const int t = base + tid;
        const int v = t < n_tiles ? ws.tiles[t] : 0;
        const int ex = tile_scan(v, s, tid);
        if (t < n_tiles) ws.tiles[t] = carry + ex;
        carry += s[kB];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kB)
sba_offsets_kernel(SbaWs ws, int64_t cloud_cap)
{
    __shared__ int s[kB + 1];
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kSbaScanTile + (int64_t)tid * kPerThread;
    int n = 0;
    for (int e = 0; e < kPerThread; e++) n += c0 + e < cloud_cap ? ws.t_cnt[c0 + e] : 0;
    int at = ws.tiles[blockIdx.x] + tile_scan(n, s, tid);
    for (int e = 0; e < kPerThread; e++) {
        if (c0 + e >= cloud_cap) break;
        ws.t_off[c0 + e] = at;
        at += ws.t_cnt[c0 + e];
    }
}

__global__ void __launch_bounds__(kB)
sba_fill_kernel(SbaIn in, SbaWs ws)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g >= in.total_kp) return;
    const int c = ws.kp_track[g];
    if (c < 0) return;
    const int64_t at = (int64_t)ws.t_off[c] + atomicAdd(&ws.t_fill[c], 1);
    if (at < in.total_kp) ws.list[at] = (int32_t)g;  // (the counts sum to at most total_kp)
}

__global__ void __launch_bounds__(kB)
sba_tracks_kernel(SbaIn in, SbaWs ws, SbaOut out, double f, int retriangulate)
{
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= n_cloud(in)) return;
    const int n = ws.t_cnt[c];
    int32_t* L = ws.list + ws.t_off[c];
    if ((int64_t)ws.t_off[c] + n > in.total_kp) return;
    bool multi = n > in.n_frames;  // more keypoints than frames: two share one, and the list need not be put in order
    if (!multi) {
        for (int a = 1; a < n; a++) {  // insertion sort: a used track has one keypoint per frame at the most
            const int32_t v = L[a];
            int b = a - 1;
            while (b >= 0 && L[b] > v) {
                L[b + 1] = L[b];
                --b;
            }
            L[b + 1] = v;
        }
        for (int a = 1; a < n; a++) multi = multi || ws.kp_frame[L[a]] == ws.kp_frame[L[a - 1]];  // a frame's keypoints are a range
    }
    if (multi) {
        out.status[c] = sba::kMulti;
        atomicAdd((unsigned long long*)&out.summary->n_tracks_multi, 1ull);
        return;
    }
    if (n < 2) return;  // (kFew, from the first kernel)
    int32_t status = sba::kRefined;
    if (retriangulate) {
        double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, Ai[9], X[3];
        for (int a = 0; a < n; a++) {
            const int64_t g = L[a];
            const gms_sfm_view& v = in.views[ws.kp_frame[g]];
            sba::ray_add(v.R, v.t, ws.uv[2 * g], ws.uv[2 * g + 1], A, b);
        }
        bool ok = sba::inv3_sym(A, Ai);
        sba::mat3_vec(Ai, b, X);
        ok = ok && sba::finite3(X);
        for (int a = 0; a < n && ok; a++) {
            const int64_t g = L[a];
            const gms_sfm_view& v = in.views[ws.kp_frame[g]];
            double Pc[3], r[2];
            ok = sba::residual(v.R, v.t, X, ws.uv[2 * g], ws.uv[2 * g + 1], f, Pc, r);
        }
        if (ok)
            for (int e = 0; e < 3; e++) out.cloud[3 * c + e] = X[e];
        else
            status = sba::kKept;
    }
    out.status[c] = status;
    ws.t_used[c] = 1;
    atomicAdd((unsigned long long*)&out.summary->n_tracks_used, 1ull);
    atomicAdd((unsigned long long*)&out.summary->n_obs, (unsigned long long)n);
}

// the observation at keypoint g, if it is one of a used track
__device__ __forceinline__ bool observation(const SbaWs& ws, int64_t g, int64_t& c)
{
    c = ws.kp_track[g];
    return c >= 0 && ws.t_used[c] != 0;
}

__global__ void __launch_bounds__(kB)
sba_linearise_kernel(SbaIn in, SbaWs ws, SbaOut out, double f, double huber_px)
{
    if (ws.flags[kLmDone]) return;
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    int64_t c;
    if (g >= in.total_kp || !observation(ws, g, c)) return;
    const int fr = ws.kp_frame[g];
    const gms_sfm_view v = out.views[fr];
    const double X[3] = {out.cloud[3 * c], out.cloud[3 * c + 1], out.cloud[3 * c + 2]};
    double Pc[3], r[2], Jc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, Jp[6] = {0, 0, 0, 0, 0, 0};
    if (sba::residual(v.R, v.t, X, ws.uv[2 * g], ws.uv[2 * g + 1], f, Pc, r)) {
        sba::jacobians(v.R, v.t, Pc, f, Jc, Jp);
        double w, rho;
        sba::huber(r, huber_px, w, rho);
        const double sw = sqrt(w);
        for (int e = 0; e < 12; e++) Jc[e] = ws.free_[fr] ? Jc[e] * sw : 0.0;  // (a frame that is no parameter has no Jc)
        for (int e = 0; e < 6; e++) Jp[e] *= sw;
        r[0] *= sw;
        r[1] *= sw;
    }
    for (int e = 0; e < 12; e++) ws.jc[12 * g + e] = Jc[e];
    for (int e = 0; e < 6; e++) ws.jp[6 * g + e] = Jp[e];
    ws.res[2 * g] = r[0];
    ws.res[2 * g + 1] = r[1];
}

__global__ void __launch_bounds__(kB)
sba_track_build_kernel(SbaIn in, SbaWs ws)
{
    if (ws.flags[kLmDone]) return;
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= in.cloud_cap || !ws.t_used[c]) return;
    const int n = ws.t_cnt[c];
    const int32_t* L = ws.list + ws.t_off[c];
    double V[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
    for (int a = 0; a < n; a++) {
        const int64_t g = L[a];
        const double* J = ws.jp + 6 * g;
        const double r0 = ws.res[2 * g], r1 = ws.res[2 * g + 1];
        for (int i = 0; i < 3; i++) {
            for (int j = i; j < 3; j++) V[3 * i + j] += J[i] * J[j] + J[3 + i] * J[3 + j];
            gp[i] += J[i] * r0 + J[3 + i] * r1;
        }
    }
    const double lam = ws.scal[kLambda];
    for (int i = 0; i < 3; i++) {
        V[4 * i] *= 1.0 + lam;
        for (int j = 0; j < i; j++) V[3 * i + j] = V[3 * j + i];
        ws.gp[3 * c + i] = -gp[i];
    }
    double Vi[9];
    sba::inv3_sym(V, Vi);
    for (int e = 0; e < 9; e++) ws.vinv[9 * c + e] = Vi[e];
}

__global__ void __launch_bounds__(kB)
sba_frame_build_kernel(SbaIn in, SbaWs ws)
{
    __shared__ double s[(kB / 64) * 21];
    if (ws.flags[kLmDone]) return;
    const int fr = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!ws.free_[fr]) return;
    int64_t g0, g1;
    frame_range(in, fr, g0, g1);
    double U[21], E[21], gb[12];  // upper triangles, row by row; gb: sum Jc^T r, then sum W y
    for (int e = 0; e < 21; e++) U[e] = E[e] = 0.0;
    for (int e = 0; e < 12; e++) gb[e] = 0.0;
    for (int64_t g = g0 + tid; g < g1; g += kB) {
        int64_t c;
        if (!observation(ws, g, c)) continue;  // (a keypoint of this frame's range is an observation of this frame)
        const double* Jc = ws.jc + 12 * g;
        const double* Jp = ws.jp + 6 * g;
        const double* Vi = ws.vinv + 9 * c;
        const double r0 = ws.res[2 * g], r1 = ws.res[2 * g + 1];
        double y[3], W[18], WV[18];
        sba::mat3_vec(Vi, ws.gp + 3 * c, y);
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 3; j++) W[3 * i + j] = Jc[i] * Jp[j] + Jc[6 + i] * Jp[3 + j];
        for (int i = 0; i < 6; i++)
            for (int k = 0; k < 3; k++) WV[3 * i + k] = W[3 * i] * Vi[k] + W[3 * i + 1] * Vi[3 + k] + W[3 * i + 2] * Vi[6 + k];
        int e = 0;
        for (int i = 0; i < 6; i++) {
            for (int j = i; j < 6; j++, e++) {
                U[e] += Jc[i] * Jc[j] + Jc[6 + i] * Jc[6 + j];
                E[e] += WV[3 * i] * W[3 * j] + WV[3 * i + 1] * W[3 * j + 1] + WV[3 * i + 2] * W[3 * j + 2];
            }
            gb[i] += Jc[i] * r0 + Jc[6 + i] * r1;
            gb[6 + i] += W[3 * i] * y[0] + W[3 * i + 1] * y[1] + W[3 * i + 2] * y[2];
        }
    }
    block_sum<21>(U, s, tid);
    block_sum<21>(E, s, tid);
    block_sum<12>(gb, s, tid);
    if (tid != 0) return;
    const double lam = ws.scal[kLambda];
    double Uf[36], M[36], Lf[36];
    int e = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, e++) {
            const double u = i == j ? U[e] * (1.0 + lam) : U[e];
            Uf[6 * i + j] = Uf[6 * j + i] = u;
            M[6 * i + j] = M[6 * j + i] = u - E[e];
        }
    ws.lok[fr] = sba::chol6(M, Lf) ? 1 : 0;
    for (int k = 0; k < 36; k++) {
        ws.U[36 * fr + k] = Uf[k];
        ws.L[36 * fr + k] = Lf[k];
    }
    for (int i = 0; i < 6; i++) ws.b[6 * fr + i] = -gb[i] - gb[6 + i];
}

// z_f = M_f^-1 r_f (0 without a factor) and r_f . z_f, its entries summed in order
__device__ __forceinline__ double precondition(const SbaWs& ws, int fr)
{
    double z[6] = {0, 0, 0, 0, 0, 0};
    if (ws.lok[fr]) sba::chol6_solve(ws.L + 36 * fr, ws.r + 6 * fr, z);
    double d = 0.0;
    for (int e = 0; e < 6; e++) {
        ws.z[6 * fr + e] = z[e];
        d += ws.r[6 * fr + e] * z[e];
    }
    return d;
}

__global__ void __launch_bounds__(kB)
sba_cg_init_kernel(SbaIn in, SbaWs ws)
{
    __shared__ double s[kB / 64];
    if (ws.flags[kLmDone]) return;
    const int tid = (int)threadIdx.x;
    double rz[1] = {0.0};
    for (int fr = tid; fr < in.n_frames; fr += kB) {
        if (!ws.free_[fr]) continue;
        for (int e = 0; e < 6; e++) {
            ws.x[6 * fr + e] = 0.0;
            ws.r[6 * fr + e] = ws.b[6 * fr + e];
        }
        rz[0] += precondition(ws, fr);
        for (int e = 0; e < 6; e++) ws.p[6 * fr + e] = ws.z[6 * fr + e];
    }
    block_sum<1>(rz, s, tid);
    if (tid == 0) {
        ws.scal[kRz] = ws.scal[kRz0] = rz[0];
        ws.flags[kCgDone] = (isfinite(rz[0]) && rz[0] > 0.0) ? 0 : 1;
    }
}

__global__ void __launch_bounds__(kB)
sba_cg_track_kernel(SbaIn in, SbaWs ws)
{
    if (ws.flags[kLmDone] || ws.flags[kCgDone]) return;
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= in.cloud_cap || !ws.t_used[c]) return;
    const int n = ws.t_cnt[c];
    const int32_t* L = ws.list + ws.t_off[c];
    double acc[3] = {0, 0, 0};
    for (int a = 0; a < n; a++) {
        const int64_t g = L[a];
        const double* Jc = ws.jc + 12 * g;
        const double* Jp = ws.jp + 6 * g;
        const double* p = ws.p + 6 * ws.kp_frame[g];
        double s0 = 0.0, s1 = 0.0;
        for (int e = 0; e < 6; e++) {
            s0 += Jc[e] * p[e];
            s1 += Jc[6 + e] * p[e];
        }
        for (int i = 0; i < 3; i++) acc[i] += Jp[i] * s0 + Jp[3 + i] * s1;
    }
    double q[3];
    sba::mat3_vec(ws.vinv + 9 * c, acc, q);
    for (int i = 0; i < 3; i++) ws.qt[3 * c + i] = q[i];
}

__global__ void __launch_bounds__(kB)
sba_cg_frame_kernel(SbaIn in, SbaWs ws)
{
    __shared__ double s[(kB / 64) * 6];
    if (ws.flags[kLmDone] || ws.flags[kCgDone]) return;
    const int fr = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!ws.free_[fr]) return;
    int64_t g0, g1;
    frame_range(in, fr, g0, g1);
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t g = g0 + tid; g < g1; g += kB) {
        int64_t c;
        if (!observation(ws, g, c)) continue;  // (a keypoint of this frame's range is an observation of this frame)
        const double* Jc = ws.jc + 12 * g;
        const double* Jp = ws.jp + 6 * g;
        const double* q = ws.qt + 3 * c;
        const double s0 = Jp[0] * q[0] + Jp[1] * q[1] + Jp[2] * q[2], s1 = Jp[3] * q[0] + Jp[4] * q[1] + Jp[5] * q[2];
        for (int e = 0; e < 6; e++) acc[e] += Jc[e] * s0 + Jc[6 + e] * s1;
    }
    block_sum<6>(acc, s, tid);
    if (tid != 0) return;
    const double* U = ws.U + 36 * fr;
    const double* p = ws.p + 6 * fr;
    double pq = 0.0;
    for (int i = 0; i < 6; i++) {
        double u = 0.0;
        for (int j = 0; j < 6; j++) u += U[6 * i + j] * p[j];
        const double q = u - acc[i];
        ws.q[6 * fr + i] = q;
        pq += p[i] * q;
    }
    ws.part[fr] = pq;
}

__global__ void __launch_bounds__(kB)
sba_cg_update_kernel(SbaIn in, SbaWs ws, double cg_tol)
{
    __shared__ double s[kB / 64];
    if (ws.flags[kLmDone] || ws.flags[kCgDone]) return;  // (uniform: the flags change only behind a barrier below, or in another launch)
    const int tid = (int)threadIdx.x;
    double v[1] = {0.0};
    for (int fr = tid; fr < in.n_frames; fr += kB)
        if (ws.free_[fr]) v[0] += ws.part[fr];
    block_sum<1>(v, s, tid);
    const double pq = v[0], rz = ws.scal[kRz], rz0 = ws.scal[kRz0];
    __syncthreads();  // every lane has read the scalars before lane 0 writes them
    if (tid == 0) ws.flags[kCgIters] += 1;
    if (!(isfinite(pq) && pq > 0.0)) {
        if (tid == 0) ws.flags[kCgDone] = 1;
        return;
    }
    const double alpha = rz / pq;
    v[0] = 0.0;
    for (int fr = tid; fr < in.n_frames; fr += kB) {
        if (!ws.free_[fr]) continue;
        for (int e = 0; e < 6; e++) {
            ws.x[6 * fr + e] += alpha * ws.p[6 * fr + e];
            ws.r[6 * fr + e] -= alpha * ws.q[6 * fr + e];
        }
        v[0] += precondition(ws, fr);
    }
    block_sum<1>(v, s, tid);
    const double rz_new = v[0];
    if (!isfinite(rz_new) || rz_new <= cg_tol * cg_tol * rz0) {
        if (tid == 0) ws.flags[kCgDone] = 1;
        return;
    }
    const double beta = rz_new / rz;
    for (int fr = tid; fr < in.n_frames; fr += kB) {
        if (!ws.free_[fr]) continue;
        for (int e = 0; e < 6; e++) ws.p[6 * fr + e] = ws.z[6 * fr + e] + beta * ws.p[6 * fr + e];
    }
    if (tid == 0) ws.scal[kRz] = rz_new;
}

// grid over max(cloud entries, frames): the points back-substituted, the candidate views
__global__ void __launch_bounds__(kB)
sba_step_kernel(SbaIn in, SbaWs ws, SbaOut out)
{
    if (ws.flags[kLmDone]) return;
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c < in.n_frames) {
        gms_sfm_view v = out.views[c];
        if (ws.free_[c]) {
            const double* x = ws.x + 6 * c;
            double E[9], R[9];
            sba::rodrigues(x, E);
            sba::mat3_mul(E, v.R, R);
            for (int e = 0; e < 9; e++) v.R[e] = R[e];
            for (int e = 0; e < 3; e++) v.t[e] = v.t[e] + x[3 + e];
        }
        ws.cand[c] = v;
    }
    if (c >= in.cloud_cap || !ws.t_used[c]) return;
    const int n = ws.t_cnt[c];
    const int32_t* L = ws.list + ws.t_off[c];
    double acc[3] = {0, 0, 0};
    for (int a = 0; a < n; a++) {
        const int64_t g = L[a];
        const double* Jc = ws.jc + 12 * g;
        const double* Jp = ws.jp + 6 * g;
        const double* x = ws.x + 6 * ws.kp_frame[g];
        double s0 = 0.0, s1 = 0.0;
        for (int e = 0; e < 6; e++) {
            s0 += Jc[e] * x[e];
            s1 += Jc[6 + e] * x[e];
        }
        for (int i = 0; i < 3; i++) acc[i] += Jp[i] * s0 + Jp[3 + i] * s1;
    }
    double rhs[3], d[3];
    for (int i = 0; i < 3; i++) rhs[i] = ws.gp[3 * c + i] - acc[i];
    sba::mat3_vec(ws.vinv + 9 * c, rhs, d);
    for (int i = 0; i < 3; i++) ws.xc[3 * c + i] = out.cloud[3 * c + i] + d[i];
}

// one workgroup per frame: the cost of its observations at (views, X). gated: 0 for the first cost, which always runs.
__global__ void __launch_bounds__(kB)
sba_cost_kernel(SbaIn in, SbaWs ws, const gms_sfm_view* __restrict__ views, const double* __restrict__ X, double f, double huber_px, int gated)
{
    __shared__ double s[(kB / 64) * 3];
    if (gated && ws.flags[kLmDone]) return;
    const int fr = (int)blockIdx.x, tid = (int)threadIdx.x;
    int64_t g0, g1;
    frame_range(in, fr, g0, g1);
    const gms_sfm_view v = views[fr];
    double acc[3] = {0, 0, 0};
    for (int64_t g = g0 + tid; g < g1; g += kB) {
        int64_t c;
        if (!observation(ws, g, c)) continue;  // (a keypoint of this frame's range is an observation of this frame)
        const double P[3] = {X[3 * c], X[3 * c + 1], X[3 * c + 2]};
        double Pc[3], r[2], w, rho;
        if (!sba::residual(v.R, v.t, P, ws.uv[2 * g], ws.uv[2 * g + 1], f, Pc, r)) continue;
        sba::huber(r, huber_px, w, rho);
        acc[0] += rho;
        acc[1] += r[0] * r[0] + r[1] * r[1];
        acc[2] += 1.0;
    }
    block_sum<3>(acc, s, tid);
    if (tid == 0) {
        ws.costp[2 * fr] = acc[0];
        ws.costp[2 * fr + 1] = acc[1];
        ws.actp[fr] = (long long)acc[2];  // (a count below 2^53: exact)
    }
}

// the frames' shares summed: cost, sum of squares, active observations
__device__ __forceinline__ void total_cost(const SbaIn& in, const SbaWs& ws, double* s, int tid, double& cost, double& sq, long long& act)
{
    double v[3] = {0, 0, 0};
    for (int fr = tid; fr < in.n_frames; fr += kB) {
        v[0] += ws.costp[2 * fr];
        v[1] += ws.costp[2 * fr + 1];
        v[2] += (double)ws.actp[fr];
    }
    block_sum<3>(v, s, tid);
    cost = v[0];
    sq = v[1];
    act = (long long)v[2];
}

__global__ void __launch_bounds__(kB)
sba_cost0_kernel(SbaIn in, SbaWs ws, SbaOut out)
{
    __shared__ double s[(kB / 64) * 3];
    __shared__ int s_free;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_free = 0;
    __syncthreads();
    int nf = 0;
    for (int fr = tid; fr < in.n_frames; fr += kB) nf += ws.free_[fr];
    if (nf) atomicAdd(&s_free, nf);
    double cost, sq;
    long long act;
    total_cost(in, ws, s, tid, cost, sq, act);  // (its barriers stand behind the atomics)
    if (tid != 0) return;
    ws.scal[kCost] = ws.scal[kCost0] = cost;
    ws.scal[kSq] = ws.scal[kSq0] = sq;
    *(long long*)(ws.flags + kActive) = act;
    *(long long*)(ws.flags + kActive0) = act;
    out.summary->n_frames_free = s_free;
    ws.flags[kLmDone] = (out.summary->n_obs > 0 && s_free > 0) ? 0 : 1;
}

__global__ void __launch_bounds__(kB)
sba_decide_kernel(SbaIn in, SbaWs ws, SbaOut out, double ftol)
{
    __shared__ double s[(kB / 64) * 3];
    __shared__ int s_accept;
    const int tid = (int)threadIdx.x;
    if (ws.flags[kLmDone]) {  // (uniform: written below only by lane 0 behind the last barrier)
        if (tid == 0) ws.flags[kAcceptedNow] = 0;
        return;
    }
    double c_new, sq_new;
    long long act_new;
    total_cost(in, ws, s, tid, c_new, sq_new, act_new);
    if (tid == 0) {
        const double cost = ws.scal[kCost];
        const long long act = *(long long*)(ws.flags + kActive);
        const bool accept = isfinite(c_new) && c_new < cost && act_new >= act;
        s_accept = accept ? 1 : 0;
        ws.flags[kItersRun] += 1;
        ws.flags[kAcceptedNow] = accept ? 1 : 0;
        const double lam = ws.scal[kLambda];
        if (accept) {
            ws.flags[kItersAcc] += 1;
            if (cost - c_new <= ftol * cost) ws.flags[kLmDone] = 1;
            ws.scal[kCost] = c_new;
            ws.scal[kSq] = sq_new;
            *(long long*)(ws.flags + kActive) = act_new;
            const double l = lam / 10.0;
            ws.scal[kLambda] = l > 1e-12 ? l : 1e-12;
        } else {
            ws.scal[kLambda] = 10.0 * lam;
        }
    }
    __syncthreads();
    if (!s_accept) return;
    for (int fr = tid; fr < in.n_frames; fr += kB) out.views[fr] = ws.cand[fr];
}

__global__ void __launch_bounds__(kB)
sba_commit_kernel(SbaIn in, SbaWs ws, SbaOut out)
{
    if (!ws.flags[kAcceptedNow]) return;
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= in.cloud_cap || !ws.t_used[c]) return;
    for (int e = 0; e < 3; e++) out.cloud[3 * c + e] = ws.xc[3 * c + e];
}

__global__ void __launch_bounds__(kB)
sba_final_kernel(SbaIn in, SbaWs ws, SbaOut out, int rescale)  // rescale: n_iters > 0 -- without an outer iteration nothing is touched
{
    __shared__ int s_first;
    __shared__ double s_factor;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_first = INT32_MAX;
    __syncthreads();
    for (int i = tid; i < in.n_pairs; i += kB)
        if (in.reg[i].status == GMS_OK && in.reg[i].link < 0) atomicMin(&s_first, i);
    __syncthreads();
    if (tid == 0) {
        double factor = 1.0;
        if (rescale && s_first != INT32_MAX) {
            const int b = in.pairs[s_first].frame_b;
            if (b >= 0 && b < in.n_frames) {
                const gms_sfm_view& v = out.views[b];
                double c[3];
                for (int i = 0; i < 3; i++) c[i] = -(v.R[i] * v.t[0] + v.R[3 + i] * v.t[1] + v.R[6 + i] * v.t[2]);
                const double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
                if (isfinite(n) && n > 0.0) factor = 1.0 / n;
            }
        }
        s_factor = factor;
        ws.scal[kFactor] = factor;
        gms_sfm_ba_summary& o = *out.summary;
        const long long act0 = *(long long*)(ws.flags + kActive0), act = *(long long*)(ws.flags + kActive);
        o.cost0 = ws.scal[kCost0];
        o.cost = ws.scal[kCost];
        o.rms0_px = act0 ? sqrt(ws.scal[kSq0] / (double)act0) : 0.0;
        o.rms_px = act ? sqrt(ws.scal[kSq] / (double)act) : 0.0;
        o.lambda = ws.scal[kLambda];
        o.n_active = act;
        o.iters_run = ws.flags[kItersRun];
        o.iters_accepted = ws.flags[kItersAcc];
        o.cg_iters = ws.flags[kCgIters];
        o.status = act ? GMS_OK : GMS_ERR_NO_MODEL;
    }
    __syncthreads();
    const double factor = s_factor;
    for (int fr = tid; fr < in.n_frames; fr += kB)
        for (int e = 0; e < 3; e++) out.views[fr].t[e] = out.views[fr].t[e] * factor;
}

__global__ void __launch_bounds__(kB)
sba_points_kernel(SbaIn in, SbaWs ws, SbaOut out)
{
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= in.cloud_cap || !ws.t_used[c]) return;
    const double factor = ws.scal[kFactor];
    for (int e = 0; e < 3; e++) out.cloud[3 * c + e] = out.cloud[3 * c + e] * factor;
}

}  // namespace

size_t sfm_ba_ws_bytes(int n_frames, int64_t total_kp, int64_t cloud_cap) { return sfm_ba_layout(n_frames, total_kp, cloud_cap).total; }

hipError_t launch_sfm_ba(const gms_camera& camera, const gms_sfm_ba_params& prm, const gms_keypoint* d_kp, const int64_t* d_frame_off,
                         int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs, int64_t total_m, const gms_dmatch* d_filtered,
                         const uint8_t* d_mask, const gms_sfm_view* d_views, const gms_sfm_pair_reg* d_reg, const int32_t* d_track,
                         int64_t cloud_cap, const double* d_cloud, const int32_t* d_cloud_id, const gms_sfm_summary* d_reg_summary, void* d_ws,
                         gms_sfm_view* d_views_out, double* d_cloud_out, int32_t* d_track_status, gms_sfm_ba_summary* d_summary,
                         hipStream_t stream)
{
    const SfmBaLayout L = sfm_ba_layout(n_frames, total_kp, cloud_cap);
    const size_t F6 = 6 * (size_t)n_frames;
    double* vec = ws_ptr<double>(d_ws, L.vec);
    const SbaWs ws = {ws_ptr<int32_t>(d_ws, L.kp_track), ws_ptr<int32_t>(d_ws, L.kp_frame), ws_ptr<int32_t>(d_ws, L.list),
                      ws_ptr<double>(d_ws, L.uv), ws_ptr<double>(d_ws, L.jc), ws_ptr<double>(d_ws, L.jp), ws_ptr<double>(d_ws, L.res),
                      ws_ptr<int32_t>(d_ws, L.t_cnt), ws_ptr<int32_t>(d_ws, L.t_off), ws_ptr<int32_t>(d_ws, L.t_fill),
                      ws_ptr<int32_t>(d_ws, L.t_used), ws_ptr<int32_t>(d_ws, L.tiles), ws_ptr<double>(d_ws, L.xc), ws_ptr<double>(d_ws, L.vinv),
                      ws_ptr<double>(d_ws, L.gp), ws_ptr<double>(d_ws, L.qt), ws_ptr<gms_sfm_view>(d_ws, L.cand), ws_ptr<double>(d_ws, L.U),
                      ws_ptr<double>(d_ws, L.L), ws_ptr<int32_t>(d_ws, L.lok), ws_ptr<int32_t>(d_ws, L.free_), vec, vec + F6, vec + 2 * F6,
                      vec + 3 * F6, vec + 4 * F6, vec + 5 * F6, ws_ptr<double>(d_ws, L.part), ws_ptr<double>(d_ws, L.costp),
                      ws_ptr<long long>(d_ws, L.actp), ws_ptr<double>(d_ws, L.scal), ws_ptr<int32_t>(d_ws, L.flags)};
    const SbaIn in = {d_kp, d_frame_off, d_pairs, d_filtered, d_mask, d_views, d_reg, d_track, d_cloud, d_cloud_id, d_reg_summary,
                      total_kp, total_m, cloud_cap, n_frames, n_pairs};
    const SbaOut out = {d_views_out, d_cloud_out, d_track_status, d_summary};
    const tv::Camera cam = {camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2, camera.k3};
    const double f = 0.5 * (camera.fx + camera.fy);
    hipError_t e = hipSuccess;
#define SBA_STAGE(...)                   \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        e = hipGetLastError();           \
        if (e != hipSuccess) return e;   \
    } while (0)
    auto blocks = [](int64_t n) { return dim3((uint32_t)(n > 0 ? (n + kB - 1) / kB : 1)); };
    const int64_t init_n = std::max<int64_t>(std::max<int64_t>(total_kp, cloud_cap), n_frames);
    const int n_tiles = (int)((cloud_cap + kSbaScanTile - 1) / kSbaScanTile);
    const dim3 per_frame((uint32_t)n_frames), one(1), tb(kB);
    SBA_STAGE(sba_init_kernel, blocks(init_n), tb, 0, stream, in, ws, out, prm.lambda0);
    if (n_pairs > 0 && total_m > 0 && cloud_cap > 0) SBA_STAGE(sba_mark_kernel, dim3((uint32_t)n_pairs), tb, 0, stream, in, ws);
    if (total_kp > 0 && cloud_cap > 0) {
        SBA_STAGE(sba_count_kernel, blocks(total_kp), tb, 0, stream, in, ws, cam);
        SBA_STAGE(sba_tile_kernel, dim3((uint32_t)n_tiles), tb, 0, stream, ws, cloud_cap);
        SBA_STAGE(sba_scan_kernel, one, tb, 0, stream, ws, n_tiles);
        SBA_STAGE(sba_offsets_kernel, dim3((uint32_t)n_tiles), tb, 0, stream, ws, cloud_cap);
        SBA_STAGE(sba_fill_kernel, blocks(total_kp), tb, 0, stream, in, ws);
        SBA_STAGE(sba_tracks_kernel, blocks(cloud_cap), tb, 0, stream, in, ws, out, f, prm.retriangulate);
    }
    SBA_STAGE(sba_cost_kernel, per_frame, tb, 0, stream, in, ws, (const gms_sfm_view*)d_views_out, (const double*)d_cloud_out, f, prm.huber_px, 0);
    SBA_STAGE(sba_cost0_kernel, one, tb, 0, stream, in, ws, out);
    if (total_kp > 0 && cloud_cap > 0) {
        for (int it = 0; it < prm.n_iters; it++) {
            SBA_STAGE(sba_linearise_kernel, blocks(total_kp), tb, 0, stream, in, ws, out, f, prm.huber_px);
            SBA_STAGE(sba_track_build_kernel, blocks(cloud_cap), tb, 0, stream, in, ws);
            SBA_STAGE(sba_frame_build_kernel, per_frame, tb, 0, stream, in, ws);
            SBA_STAGE(sba_cg_init_kernel, one, tb, 0, stream, in, ws);
            for (int k = 0; k < prm.n_cg; k++) {
                SBA_STAGE(sba_cg_track_kernel, blocks(cloud_cap), tb, 0, stream, in, ws);
                SBA_STAGE(sba_cg_frame_kernel, per_frame, tb, 0, stream, in, ws);
                SBA_STAGE(sba_cg_update_kernel, one, tb, 0, stream, in, ws, prm.cg_tol);
            }
            SBA_STAGE(sba_step_kernel, blocks(std::max<int64_t>(cloud_cap, n_frames)), tb, 0, stream, in, ws, out);
            SBA_STAGE(sba_cost_kernel, per_frame, tb, 0, stream, in, ws, (const gms_sfm_view*)ws.cand, (const double*)ws.xc, f, prm.huber_px, 1);
            SBA_STAGE(sba_decide_kernel, one, tb, 0, stream, in, ws, out, prm.ftol);
            SBA_STAGE(sba_commit_kernel, blocks(cloud_cap), tb, 0, stream, in, ws, out);
        }
    }
    SBA_STAGE(sba_final_kernel, one, tb, 0, stream, in, ws, out, prm.n_iters > 0 ? 1 : 0);
    if (cloud_cap > 0) SBA_STAGE(sba_points_kernel, blocks(cloud_cap), tb, 0, stream, in, ws, out);
#undef SBA_STAGE
    return hipSuccess;
}

}  // namespace gms
