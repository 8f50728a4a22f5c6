// sfm_register_kernels.hip -- many two-view results into one frame (the arithmetic is sfm_register_core.h, the
// workspace SfmRegisterLayout in ws_layout.h). Stream-ordered launches, nothing else:
//
//   sfr_init_kernel      every workspace word a later kernel reads, the world points (0) and the tracks (-1)
//   sfr_rank_kernel      one workgroup per pair: rank = non-zero mask bytes before each match (wave ballots), and the slot table:
//                        atomicMin of the match index into ONE int32 table over the global keypoints -- a frame is registered by one
//                        pair, so the tables of all links are disjoint parts of it
//   sfr_link_kernel      one workgroup per pair: the valid link ratios packed into the workspace, then their lower median by radix
//                        select on the bit patterns (positive doubles order as uint64): 8 passes over a 256-bin LDS histogram, exact,
//                        no sort. Scaling a pair's ratios by the link's cumulative scale is monotone, so no median waits for a scale.
//   sfr_compose_kernel   one lane walks the pairs in plan order: ok, the cumulative scale, the view; the workgroup stages the pairs'
//                        records in LDS for it
//   sfr_world_kernel     W = G_a.R^T (S p - G_a.t)
//   sfr_merge_kernel / sfr_flatten_kernel   union-find over the global keypoints with atomicMin on the roots (as portrait mode's), then
//                        per root its keypoints, and through a table of (root, frame) keys whether two of them share a frame
//   (merge, estimate and spread take an optional keep plane, DESIGN.md §4.10e: a match whose byte is 0 is no edge and no estimate)
//   sfr_estimate_kernel  per point its track; per root the least (pair, rank) key (64-bit atomicMin) and the estimates
//   sfr_spread_kernel    per root the largest distance to the representative (atomicMax on the bit pattern)
//   sfr_tile_kernel / sfr_scan_kernel / sfr_cloud_kernel   the roots compacted in ascending order by a prefix sum over the keypoints
// Every atomic is an integer minimum, maximum or sum: the result does not depend on the order the lanes arrive in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gms_kernels.h"
#include "sfm_register_core.h"

namespace gms {
namespace {

constexpr int kB = 256;
constexpr unsigned long long kEmpty = ~0ull;

struct SfrIn {
    const int64_t* frame_off;
    const gms_pair* pairs;
    const gms_sfm_plan_entry* plan;
    const gms_dmatch* matches;
    const uint8_t* mask;
    const double* pts;
    const gms_two_view* tv;
    int64_t total_kp, total_m;
    int n_frames, n_pairs, root;
};
struct SfrWs {
    int32_t* rank;
    unsigned long long* rho;
    int32_t *slot, *parent, *member;
    uint32_t *obs, *est, *multi;
    unsigned long long *repkey, *spread, *hash;
    int32_t *tiles, *npts, *ok;
    uint32_t hash_mask;
};

// What a kernel needs of pair i, with everything that indexes memory checked: a pair whose frames, offsets or match range do not
// fit the arrays has no matches and does not register.
struct PairInfo {
    int64_t off, oa, ob;
    int n, na, nb, a;
    gms_sfm_plan_entry pl;
};
__device__ __forceinline__ PairInfo pair_info(const SfrIn& in, int i)
{
    PairInfo p = {};
    const gms_pair pr = in.pairs[i];
    p.pl = in.plan[i];
    p.a = pr.frame_a;
    sfr::PairRanges fr = {};
    // (a link points back: the walk in pair order is the plan's)
    if (!sfr::pair_fits(pr, in.frame_off, in.n_frames, in.total_kp, in.total_m, &fr) || !sfr::plan_entry_fits(p.pl, i)) {
        p = PairInfo{};
        p.pl = gms_sfm_plan_entry{0, -1, 0, 0};
        return p;
    }
    p.oa = fr.oa;
    p.ob = fr.ob;
    p.na = (int)fr.na;
    p.nb = (int)fr.nb;
    p.off = pr.match_off;
    p.n = sfr::pair_count(pr, in.tv[i]);
    return p;
}
// match k of the pair: kept when its mask byte is set and both indices lie inside their frames
__device__ __forceinline__ bool kept(const SfrIn& in, const PairInfo& p, int k, gms_dmatch& m)
{
    if (k >= p.n || in.mask[p.off + k] == 0) return false;
    m = in.matches[p.off + k];
    return (uint32_t)m.queryIdx < (uint32_t)p.na && (uint32_t)m.trainIdx < (uint32_t)p.nb;
}

// with a keep plane, whether match k of the pair feeds the tracks; the links and the points do not ask
__device__ __forceinline__ bool on_plane(const uint8_t* keep, const PairInfo& p, int k) { return !keep || keep[p.off + k] != 0; }

__device__ __forceinline__ int uf_find(const int32_t* L, int a)
{
    int p = L[a];
    while (p != a) {
        a = p;
        p = L[a];
    }
    return a;
}
// the roots only ever decrease: a root is its component's lowest keypoint so far
__device__ __forceinline__ void uf_union(int32_t* L, int a, int b)
{
    for (;;) {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kB)
sfr_init_kernel(SfrWs ws, int64_t total_kp, int64_t total_m, int64_t hash_slots, double* __restrict__ world, int32_t* __restrict__ track)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g < total_kp) {
        ws.slot[g] = sfr::kNoSlot;
        ws.parent[g] = (int32_t)g;
        ws.member[g] = 0;
        ws.obs[g] = 0;
        ws.est[g] = 0;
        ws.multi[g] = 0;
        ws.repkey[g] = kEmpty;
        ws.spread[g] = 0;
    }
    if (g < hash_slots) ws.hash[g] = kEmpty;
    if (g < total_m) {
        track[g] = -1;
        world[3 * g] = 0.0;
        world[3 * g + 1] = 0.0;
        world[3 * g + 2] = 0.0;
    }
}

__global__ void __launch_bounds__(kB)
sfr_rank_kernel(SfrIn in, SfrWs ws)
{
    __shared__ unsigned s_wave[kB / 64];
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PairInfo p = pair_info(in, i);
    const bool root_table = p.pl.registers && p.pl.link < 0 && p.a == in.root;  // the first pair out of the root: role 0 links name its queryIdx
    unsigned before_all = 0;
    for (int base = 0; base < p.n; base += kB) {
        const int k = base + tid;
        const bool set = k < p.n && in.mask[p.off + k] != 0;
        const unsigned long long b = __ballot(set);
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(b);
        __syncthreads();
        unsigned before = before_all, total = 0;
        for (int w = 0; w < kB / 64; ++w) {
            before += w < wave ? s_wave[w] : 0u;
            total += s_wave[w];
        }
        __syncthreads();
        if (k < p.n) ws.rank[p.off + k] = (int32_t)(before + (unsigned)__popcll(b & ((1ull << lane) - 1ull)));
        gms_dmatch m;
        if (p.pl.registers && kept(in, p, k, m)) {
            atomicMin(&ws.slot[p.ob + m.trainIdx], k);
            if (root_table) atomicMin(&ws.slot[p.oa + m.queryIdx], k);
        }
        before_all += total;
    }
    if (tid == 0) ws.npts[i] = (int32_t)before_all;
}

__global__ void __launch_bounds__(kB)
sfr_link_kernel(SfrIn in, SfrWs ws, gms_sfm_pair_reg* __restrict__ reg)
{
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_count, s_target;
    __shared__ unsigned long long s_prefix;
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    const PairInfo p = pair_info(in, i);
    const int j = p.pl.registers ? p.pl.link : -1;
    bool measure = j >= 0 && sfr::base_ok(p.pl, in.tv[i]);
    PairInfo pj = {};
    if (measure) {
        pj = pair_info(in, j);
        measure = sfr::base_ok(pj.pl, in.tv[j]);
    }
    if (!measure) {  // (uniform over the workgroup)
        if (tid == 0) {
            reg[i].n_links = 0;
            reg[i].r = 0.0;
        }
        return;
    }
    if (tid == 0) s_count = 0;
    __syncthreads();
    const int role = p.pl.role != 0 ? 1 : 0;
    double Rj[9], tj[3];
    for (int e = 0; e < 9; e++) Rj[e] = in.tv[j].R[e];
    for (int e = 0; e < 3; e++) tj[e] = in.tv[j].t[e];
    unsigned long long* __restrict__ rho = ws.rho + p.off;
    for (int base = 0; base < p.n; base += kB) {
        const int k = base + tid;
        gms_dmatch m;
        bool valid = false;
        double ratio = 0.0;
        if (kept(in, p, k, m)) {
            const int32_t s = ws.slot[p.oa + m.queryIdx];
            if (s != sfr::kNoSlot && s < pj.n) {
                const double* pjp = in.pts + 3 * (pj.off + ws.rank[pj.off + s]);
                const double* pip = in.pts + 3 * (p.off + ws.rank[p.off + k]);
                const double Pj[3] = {pjp[0], pjp[1], pjp[2]}, Y[3] = {pip[0], pip[1], pip[2]};
                double X[3];
                sfr::link_point(role, Rj, tj, Pj, X);
                valid = sfr::link_valid(X, Y);
                if (valid) ratio = sfr::link_ratio(X, Y);
            }
        }
        const unsigned long long b = __ballot(valid);
        unsigned wave_base = 0;
        if (lane == 0 && b) wave_base = atomicAdd(&s_count, (unsigned)__popcll(b));  // one LDS atomic per wave and pass
        wave_base = (unsigned)__shfl((int)wave_base, 0);
        if (valid) rho[wave_base + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = (unsigned long long)__double_as_longlong(ratio);
    }
    __syncthreads();  // the packed ratios are visible to the workgroup
    const unsigned L = s_count;
    if (L == 0) {
        if (tid == 0) {
            reg[i].n_links = 0;
            reg[i].r = 0.0;
        }
        return;
    }
    if (tid == 0) {
        s_target = (L - 1) / 2;
        s_prefix = 0;
    }
    for (int pass = 7; pass >= 0; --pass) {
        s_hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (unsigned e = tid; e < L; e += kB) {
            const unsigned long long v = rho[e];
            if (pass == 7 || (v >> (8 * (pass + 1))) == prefix) atomicAdd(&s_hist[(unsigned)(v >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned t = s_target, d = 0;
            while (d < 255 && t >= s_hist[d]) t -= s_hist[d++];
            s_target = t;
            s_prefix = (prefix << 8) | d;
        }
        __syncthreads();
    }
    if (tid == 0) {
        reg[i].n_links = (int32_t)L;
        reg[i].r = __longlong_as_double((long long)s_prefix);
    }
}

// what the walk needs of a pair, staged in LDS by the whole workgroup, kB pairs at a time
struct SfrStaged {
    double R[9], t[3], r;
    int32_t a, b, link, role, depth, registers, base, n_links;
};

__global__ void __launch_bounds__(kB)
sfr_compose_kernel(SfrIn in, SfrWs ws, int min_links, gms_sfm_view* __restrict__ views, gms_sfm_pair_reg* __restrict__ reg,
                   gms_sfm_summary* __restrict__ summary)
{
    __shared__ SfrStaged s_p[kB];
    const int tid = (int)threadIdx.x;
    for (int f = tid; f < in.n_frames; f += kB) {
        gms_sfm_view v = {};
        v.pair = -1;
        if (f == in.root) {
            v.R[0] = v.R[4] = v.R[8] = 1.0;
            v.registered = 1;
        }
        views[f] = v;
    }
    // The walk itself is one lane's: a pair needs its link's outcome. What does not depend on the order -- the pair's record, its
    // plan entry, the link kernel's count and median -- the workgroup loads side by side; the walk then reads LDS, and in a chain
    // the link's outcome and the view of frame_a are the previous step's, still in registers.
    int n_reg = 1, n_ok = 0;
    int prev_i = -1, prev_ok = 0, prev_b = -1;
    double prev_S = 0.0;
    gms_sfm_view prev_G = {};
    for (int base = 0; base < in.n_pairs; base += kB) {
        const int mine = base + tid;
        if (mine < in.n_pairs) {
            const PairInfo p = pair_info(in, mine);
            SfrStaged& s = s_p[tid];
            s.registers = p.pl.registers ? 1 : 0;
            s.link = p.pl.registers ? p.pl.link : -1;
            s.role = p.pl.role != 0 ? 1 : 0;
            s.depth = p.pl.depth;
            s.a = s.b = s.base = s.n_links = 0;
            s.r = 0.0;
            if (p.pl.registers) {
                const gms_pair pr = in.pairs[mine];
                const gms_two_view& t = in.tv[mine];
                s.a = pr.frame_a;
                s.b = pr.frame_b;
                s.base = sfr::base_ok(p.pl, t) ? 1 : 0;
                for (int e = 0; e < 9; e++) s.R[e] = t.R[e];
                for (int e = 0; e < 3; e++) s.t[e] = t.t[e];
                if (s.link >= 0) {  // (the link kernel's)
                    s.n_links = reg[mine].n_links;
                    s.r = reg[mine].r;
                }
            }
        }
        __syncthreads();  // (also behind the views' first values)
        if (tid == 0) {
            const int n = in.n_pairs - base < kB ? in.n_pairs - base : kB;
            for (int k = 0; k < n; k++) {
                const SfrStaged& s = s_p[k];
                const int i = base + k;
                gms_sfm_pair_reg o = {};
                o.link = -1;
                o.status = GMS_SFM_SKIPPED;
                int ok = 0;
                if (s.registers) {
                    const int j = s.link;
                    o.n_links = s.n_links;
                    o.r = s.r;
                    o.depth = s.depth;
                    o.link = j;
                    o.role = s.role;
                    const gms_sfm_view Ga = s.a == prev_b ? prev_G : views[s.a];  // (prev_b: registered by the last ok pair)
                    ok = s.base && Ga.registered;
                    double S = 1.0;
                    if (ok && j >= 0) {
                        const int ok_j = j == prev_i ? prev_ok : ws.ok[j];
                        const double S_j = j == prev_i ? prev_S : reg[j].S;
                        ok = ok_j && o.n_links >= min_links;
                        S = S_j * o.r;
                    }
                    o.status = ok ? GMS_OK : GMS_ERR_NO_MODEL;
                    if (ok) {
                        o.S = S;
                        gms_sfm_view Gb = {};
                        sfr::compose_view(s.R, s.t, S, Ga.R, Ga.t, Gb.R, Gb.t);
                        Gb.registered = 1;
                        Gb.pair = i;
                        views[s.b] = Gb;
                        prev_b = s.b;
                        prev_G = Gb;
                        n_reg++;
                        n_ok++;
                    }
                    prev_i = i;
                    prev_ok = ok;
                    prev_S = o.S;
                }
                ws.ok[i] = ok;
                reg[i] = o;
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    gms_sfm_summary s = {};
    s.n_registered = n_reg;
    s.n_ok_pairs = n_ok;
    *summary = s;  // (the cloud kernels add the track counts)
}

// grid: pairs x chunks of kB matches
__global__ void __launch_bounds__(kB)
sfr_world_kernel(SfrIn in, SfrWs ws, const gms_sfm_view* __restrict__ views, const gms_sfm_pair_reg* __restrict__ reg,
                 double* __restrict__ world)
{
    const int i = (int)blockIdx.x;
    if (!ws.ok[i]) return;
    const int rank = (int)(blockIdx.y * kB + threadIdx.x);
    if (rank >= ws.npts[i]) return;
    const gms_pair pr = in.pairs[i];
    const gms_sfm_view& Ga = views[pr.frame_a];
    const double* p = in.pts + 3 * (pr.match_off + rank);
    const double P[3] = {p[0], p[1], p[2]};
    double W[3];
    sfr::world_point(Ga.R, Ga.t, reg[i].S, P, W);
    double* o = world + 3 * (pr.match_off + rank);
    o[0] = W[0];
    o[1] = W[1];
    o[2] = W[2];
}

__global__ void __launch_bounds__(kB)
sfr_merge_kernel(SfrIn in, SfrWs ws, const uint8_t* __restrict__ keep)
{
    const int i = (int)blockIdx.x;
    if (!ws.ok[i]) return;
    const PairInfo p = pair_info(in, i);
    const int k = (int)(blockIdx.y * kB + threadIdx.x);
    gms_dmatch m;
    if (!kept(in, p, k, m) || !on_plane(keep, p, k)) return;
    const int u = (int)(p.oa + m.queryIdx), v = (int)(p.ob + m.trainIdx);
    ws.member[u] = 1;  // (benign races: every writer stores 1)
    ws.member[v] = 1;
    uf_union(ws.parent, u, v);
}

__global__ void __launch_bounds__(kB)
sfr_flatten_kernel(SfrIn in, SfrWs ws)
{
    const int64_t g = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (g >= in.total_kp) return;
    const int root = uf_find(ws.parent, (int)g);
    ws.parent[g] = root;  // a shorter path to the same root: finds that run beside this one stay right
    if (!ws.member[g]) return;
    atomicAdd(&ws.obs[root], 1u);
    int lo = 0, hi = in.n_frames;  // the frame of g: the last f with frame_off[f] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (in.frame_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    const unsigned long long key = ((unsigned long long)(unsigned)root << 32) | (unsigned)lo;
    unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & ws.hash_mask;
    for (unsigned step = 0; step <= ws.hash_mask; ++step) {  // at most total_kp keys in at least twice as many slots
        const unsigned long long old = atomicCAS(&ws.hash[h], kEmpty, key);
        if (old == kEmpty) break;
        if (old == key) {
            ws.multi[root] = 1;
            break;
        }
        h = (h + 1) & ws.hash_mask;
    }
}

__global__ void __launch_bounds__(kB)
sfr_estimate_kernel(SfrIn in, SfrWs ws, const uint8_t* __restrict__ keep, int32_t* __restrict__ track)
{
    const int i = (int)blockIdx.x;
    if (!ws.ok[i]) return;
    const PairInfo p = pair_info(in, i);
    const int k = (int)(blockIdx.y * kB + threadIdx.x);
    gms_dmatch m;
    if (!kept(in, p, k, m) || !on_plane(keep, p, k)) return;
    const int root = ws.parent[p.oa + m.queryIdx];
    const int rank = ws.rank[p.off + k];
    track[p.off + rank] = root;
    atomicMin(&ws.repkey[root], ((unsigned long long)(unsigned)i << 32) | (unsigned)rank);
    atomicAdd(&ws.est[root], 1u);
}

__device__ __forceinline__ const double* rep_point(const SfrIn& in, const double* world, unsigned long long key)
{
    return world + 3 * (in.pairs[(int)(key >> 32)].match_off + (int64_t)(key & 0xFFFFFFFFull));
}

__global__ void __launch_bounds__(kB)
sfr_spread_kernel(SfrIn in, SfrWs ws, const uint8_t* __restrict__ keep, const double* __restrict__ world)
{
    const int i = (int)blockIdx.x;
    if (!ws.ok[i]) return;
    const PairInfo p = pair_info(in, i);
    const int k = (int)(blockIdx.y * kB + threadIdx.x);
    gms_dmatch m;
    if (!kept(in, p, k, m) || !on_plane(keep, p, k)) return;
    const int root = ws.parent[p.oa + m.queryIdx];
    const double* w = world + 3 * (p.off + ws.rank[p.off + k]);
    const double* c = rep_point(in, world, ws.repkey[root]);
    const double dx = w[0] - c[0], dy = w[1] - c[1], dz = w[2] - c[2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    if (d == d) atomicMax(&ws.spread[root], (unsigned long long)__double_as_longlong(d));  // (a distance that is no number does not count)
}

// ordered compaction of the roots: tile t holds keypoints [t * kSfrScanTile, ...), thread tid of it kSfrScanTile / kB consecutive ones
constexpr int kPerThread = kSfrScanTile / kB;

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
sfr_tile_kernel(SfrWs ws, int64_t total_kp)
{
    __shared__ int s[kB + 1];
    const int tid = (int)threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * kSfrScanTile + (int64_t)tid * kPerThread;
    int n = 0;
    for (int e = 0; e < kPerThread; e++) n += (g0 + e < total_kp && ws.obs[g0 + e] > 0) ? 1 : 0;
    tile_scan(n, s, tid);
    if (tid == 0) ws.tiles[blockIdx.x] = s[kB];
}

__global__ void __launch_bounds__(kB)
sfr_scan_kernel(SfrWs ws, int n_tiles, gms_sfm_summary* __restrict__ summary)
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
    if (tid == 0) summary->n_tracks = carry;
}

__global__ void __launch_bounds__(kB)
sfr_cloud_kernel(SfrIn in, SfrWs ws, const double* __restrict__ world, int64_t cloud_cap, double* __restrict__ cloud,
                 int32_t* __restrict__ cloud_id, int32_t* __restrict__ cloud_obs, int32_t* __restrict__ cloud_est,
                 double* __restrict__ cloud_spread, gms_sfm_summary* __restrict__ summary)
{
    __shared__ int s[kB + 1];
    __shared__ unsigned long long s_est, s_multi;
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        s_est = 0;
        s_multi = 0;
    }
    const int64_t g0 = (int64_t)blockIdx.x * kSfrScanTile + (int64_t)tid * kPerThread;
    int n = 0;
    for (int e = 0; e < kPerThread; e++) n += (g0 + e < in.total_kp && ws.obs[g0 + e] > 0) ? 1 : 0;
    int64_t c = (int64_t)ws.tiles[blockIdx.x] + tile_scan(n, s, tid);
    unsigned long long est = 0, multi = 0;
    for (int e = 0; e < kPerThread; e++) {
        const int64_t g = g0 + e;
        if (g >= in.total_kp || ws.obs[g] == 0) continue;
        est += ws.est[g];
        multi += ws.multi[g];
        if (c < cloud_cap && ws.repkey[g] != kEmpty) {  // (a root with keypoints has an edge, so an estimate)
            const double* w = rep_point(in, world, ws.repkey[g]);
            cloud[3 * c] = w[0];
            cloud[3 * c + 1] = w[1];
            cloud[3 * c + 2] = w[2];
            cloud_id[c] = (int32_t)g;
            cloud_obs[c] = (int32_t)ws.obs[g];
            cloud_est[c] = (int32_t)ws.est[g];
            cloud_spread[c] = __longlong_as_double((long long)ws.spread[g]);
        }
        ++c;
    }
    if (est) atomicAdd(&s_est, est);
    if (multi) atomicAdd(&s_multi, multi);
    __syncthreads();
    if (tid == 0) {
        if (s_est) atomicAdd((unsigned long long*)&summary->n_points, s_est);
        if (s_multi) atomicAdd((unsigned long long*)&summary->n_multi, s_multi);
    }
}

}  // namespace

size_t sfm_register_ws_bytes(int n_pairs, int64_t total_kp, int64_t total_m) { return sfm_register_layout(n_pairs, total_kp, total_m).total; }

hipError_t launch_sfm_register(const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                               const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_m, const gms_dmatch* d_filtered,
                               const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links,
                               void* d_ws, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_world, int32_t* d_track,
                               int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                               double* d_cloud_spread, gms_sfm_summary* d_summary, hipStream_t stream, const uint8_t* d_keep)
{
    const SfmRegisterLayout L = sfm_register_layout(n_pairs, total_kp, total_m);
    const int64_t hash_slots = (int64_t)sfr_hash_slots((size_t)total_kp);
    const SfrWs ws = {ws_ptr<int32_t>(d_ws, L.rank), ws_ptr<unsigned long long>(d_ws, L.rho), ws_ptr<int32_t>(d_ws, L.slot),
                      ws_ptr<int32_t>(d_ws, L.parent), ws_ptr<int32_t>(d_ws, L.member), ws_ptr<uint32_t>(d_ws, L.obs),
                      ws_ptr<uint32_t>(d_ws, L.est), ws_ptr<uint32_t>(d_ws, L.multi), ws_ptr<unsigned long long>(d_ws, L.repkey),
                      ws_ptr<unsigned long long>(d_ws, L.spread), ws_ptr<unsigned long long>(d_ws, L.hash), ws_ptr<int32_t>(d_ws, L.tiles),
                      ws_ptr<int32_t>(d_ws, L.npts), ws_ptr<int32_t>(d_ws, L.ok), (uint32_t)(hash_slots - 1)};
    const SfrIn in = {d_frame_off, d_pairs, d_plan, d_filtered, d_mask, d_points3d, d_tv, total_kp, total_m, n_frames, n_pairs, root};
    hipError_t e = hipSuccess;
#define SFR_STAGE(...)                   \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        e = hipGetLastError();           \
        if (e != hipSuccess) return e;   \
    } while (0)
    const int64_t init_n = hash_slots > total_m ? hash_slots : total_m;  // (hash_slots > total_kp)
    SFR_STAGE(sfr_init_kernel, dim3((uint32_t)((init_n + kB - 1) / kB)), dim3(kB), 0, stream, ws, total_kp, total_m, hash_slots, d_world, d_track);
    const bool work = n_pairs > 0 && max_m > 0;
    const dim3 per_pair((uint32_t)(n_pairs > 0 ? n_pairs : 1));
    const dim3 per_match((uint32_t)(n_pairs > 0 ? n_pairs : 1), (uint32_t)((max_m + kB - 1) / kB));
    if (n_pairs > 0) {
        SFR_STAGE(sfr_rank_kernel, per_pair, dim3(kB), 0, stream, in, ws);
        SFR_STAGE(sfr_link_kernel, per_pair, dim3(kB), 0, stream, in, ws, d_reg);
    }
    SFR_STAGE(sfr_compose_kernel, dim3(1), dim3(kB), 0, stream, in, ws, min_links, d_views, d_reg, d_summary);
    if (work) {
        SFR_STAGE(sfr_world_kernel, per_match, dim3(kB), 0, stream, in, ws, d_views, d_reg, d_world);
        SFR_STAGE(sfr_merge_kernel, per_match, dim3(kB), 0, stream, in, ws, d_keep);
    }
    if (total_kp > 0) {
        const int n_tiles = (int)((total_kp + kSfrScanTile - 1) / kSfrScanTile);
        SFR_STAGE(sfr_flatten_kernel, dim3((uint32_t)((total_kp + kB - 1) / kB)), dim3(kB), 0, stream, in, ws);
        if (work) {
            SFR_STAGE(sfr_estimate_kernel, per_match, dim3(kB), 0, stream, in, ws, d_keep, d_track);
            SFR_STAGE(sfr_spread_kernel, per_match, dim3(kB), 0, stream, in, ws, d_keep, d_world);
        }
        SFR_STAGE(sfr_tile_kernel, dim3((uint32_t)n_tiles), dim3(kB), 0, stream, ws, total_kp);
        SFR_STAGE(sfr_scan_kernel, dim3(1), dim3(kB), 0, stream, ws, n_tiles, d_summary);
        SFR_STAGE(sfr_cloud_kernel, dim3((uint32_t)n_tiles), dim3(kB), 0, stream, in, ws, d_world, cloud_cap, d_cloud, d_cloud_id, d_cloud_obs,
                  d_cloud_est, d_cloud_spread, d_summary);
    }
#undef SFR_STAGE
    return hipSuccess;
}

}  // namespace gms
