// tests/test_sfm_register_ref.py: a host build of sfm_register_core.h (the plan, a pair's match count, when a link counts, its ratio,
// the pose and point transforms) as the kernels use them, around plain loops: slots by a minimum per keypoint, the lower median by a
// sort. The test holds the result to the numpy statement tests/sfm_register_ref.py.
//   sfr_host_plan(pairs, n_pairs, n_frames, root, plan out) -> 0, or -1 on a frame index out of range
//   sfr_host_register(frame_off, n_frames, pairs, n_pairs, matches, mask, points3d, tv, root, min_links, views out, reg out,
//                     world out [total match slots][3], zeroed by the caller) -> 0 / -1
// -DSFR_HOST_MAIN: a stand-alone program (for a sanitizer run) that registers a small chain and prints its scales.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sfm_register_core.h"

namespace {

struct Kept {
    int k, q, t, rank;
};
// the pair's matches with a non-zero mask byte and both indices inside their frames; *n_pts: non-zero mask bytes
std::vector<Kept> kept_of(const gms_pair& pr, const gms_two_view& tv, const int64_t* frame_off, const gms_dmatch* m, const uint8_t* mask, int* n_pts)
{
    std::vector<Kept> out;
    const int n = sfr::pair_count(pr, tv);
    const int64_t na = frame_off[pr.frame_a + 1] - frame_off[pr.frame_a], nb = frame_off[pr.frame_b + 1] - frame_off[pr.frame_b];
    int rank = 0;
    for (int k = 0; k < n; k++) {
        if (!mask[pr.match_off + k]) continue;
        const gms_dmatch& d = m[pr.match_off + k];
        if (d.queryIdx >= 0 && d.queryIdx < na && d.trainIdx >= 0 && d.trainIdx < nb) out.push_back({k, d.queryIdx, d.trainIdx, rank});
        rank++;
    }
    *n_pts = rank;
    return out;
}

}  // namespace

extern "C" {

int sfr_host_plan(const gms_pair* pairs, int n_pairs, int n_frames, int root, gms_sfm_plan_entry* plan)
{
    std::vector<int32_t> reg_by((size_t)(n_frames > 0 ? n_frames : 0));
    return n_frames > 0 && sfr::plan(pairs, n_pairs, n_frames, root, reg_by.data(), plan) ? 0 : -1;
}

int sfr_host_register(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* matches,
                      const uint8_t* mask, const double* pts, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                      gms_sfm_pair_reg* reg, double* world)
{
    std::vector<gms_sfm_plan_entry> plan((size_t)n_pairs);
    if (sfr_host_plan(pairs, n_pairs, n_frames, root, plan.data()) != 0) return -1;
    for (int f = 0; f < n_frames; f++) {
        views[f] = gms_sfm_view{};
        views[f].pair = -1;
    }
    views[root].R[0] = views[root].R[4] = views[root].R[8] = 1.0;
    views[root].registered = 1;
    std::vector<std::vector<Kept>> kept((size_t)n_pairs);
    std::vector<int> n_pts((size_t)n_pairs), ok((size_t)n_pairs, 0);
    for (int i = 0; i < n_pairs; i++) kept[i] = kept_of(pairs[i], tv[i], frame_off, matches, mask, &n_pts[i]);
    for (int i = 0; i < n_pairs; i++) {
        gms_sfm_pair_reg o = {};
        o.link = -1;
        o.status = GMS_SFM_SKIPPED;
        reg[i] = o;
        if (!plan[i].registers) continue;
        const gms_pair& pr = pairs[i];
        const int j = plan[i].link, role = plan[i].role;
        o.depth = plan[i].depth;
        o.link = j;
        o.role = role;
        bool good = sfr::base_ok(plan[i], tv[i]);
        double S = 1.0;
        if (j >= 0) {
            std::vector<double> rho;
            if (sfr::base_ok(plan[i], tv[i]) && sfr::base_ok(plan[j], tv[j])) {
                const int64_t na = frame_off[pr.frame_a + 1] - frame_off[pr.frame_a];
                std::vector<int32_t> slot((size_t)na, sfr::kNoSlot), rank_of((size_t)na, 0);
                for (const Kept& e : kept[j]) {
                    const int kp = role == 1 ? e.t : e.q;
                    if (e.k < slot[kp]) {
                        slot[kp] = e.k;
                        rank_of[kp] = e.rank;
                    }
                }
                for (const Kept& e : kept[i]) {
                    if (slot[e.q] == sfr::kNoSlot) continue;
                    double X[3];
                    sfr::link_point(role, tv[j].R, tv[j].t, pts + 3 * (pairs[j].match_off + rank_of[e.q]), X);
                    const double* Y = pts + 3 * (pr.match_off + e.rank);
                    if (sfr::link_valid(X, Y)) rho.push_back(sfr::link_ratio(X, Y));
                }
            }
            std::sort(rho.begin(), rho.end());
            o.n_links = (int32_t)rho.size();
            o.r = rho.empty() ? 0.0 : rho[(rho.size() - 1) / 2];
            good = good && ok[j] && o.n_links >= min_links;
            if (good) S = reg[j].S * o.r;
        }
        o.status = good ? GMS_OK : GMS_ERR_NO_MODEL;
        if (good) {
            ok[i] = 1;
            o.S = S;
            const gms_sfm_view Ga = views[pr.frame_a];
            gms_sfm_view Gb = {};
            sfr::compose_view(tv[i].R, tv[i].t, S, Ga.R, Ga.t, Gb.R, Gb.t);
            Gb.registered = 1;
            Gb.pair = i;
            views[pr.frame_b] = Gb;
            for (int r = 0; r < n_pts[i]; r++) sfr::world_point(Ga.R, Ga.t, S, pts + 3 * (pr.match_off + r), world + 3 * (pr.match_off + r));
        }
        reg[i] = o;
    }
    return 0;
}

}  // extern "C"

#ifdef SFR_HOST_MAIN
int main()
{
    // three frames of 40 keypoints that all show one point set; pair (1, 2) measures the scene at half the unit of pair (0, 1)
    const int n_kp = 40, n_frames = 3, n_pairs = 2;
    int64_t frame_off[4] = {0, 40, 80, 120};
    gms_pair pairs[2] = {{0, 1, n_kp, 0, 0}, {1, 2, n_kp, 0, 64}};
    std::vector<gms_dmatch> m(64 + n_kp);
    std::vector<uint8_t> mask(64 + n_kp, 0);
    std::vector<double> pts(3 * (64 + n_kp), 0.0), world(3 * (64 + n_kp), 0.0);
    gms_two_view tv[2] = {};
    for (int p = 0; p < n_pairs; p++) {
        tv[p].R[0] = tv[p].R[4] = tv[p].R[8] = 1.0;
        tv[p].t[0] = 1.0;
        tv[p].n_points = n_kp;
        tv[p].n_triangulated = n_kp;
        for (int k = 0; k < n_kp; k++) {
            const int64_t at = pairs[p].match_off + k;
            m[at] = gms_dmatch{k, k, 0, 0.0f};
            mask[at] = 1;
            const double X[3] = {0.1 * k - 2.0 + p, 0.05 * k, 5.0 + 0.01 * k};  // the point in camera p, in pair 0's unit
            for (int c = 0; c < 3; c++) pts[3 * at + c] = X[c] * (p == 0 ? 1.0 : 0.5);
        }
    }
    gms_sfm_view views[3];
    gms_sfm_pair_reg reg[2];
    if (sfr_host_register(frame_off, n_frames, pairs, n_pairs, m.data(), mask.data(), pts.data(), tv, 0, 8, views, reg, world.data()) != 0) return 1;
    std::printf("sfr_host: tiny %d %d %.6f %.6f\n", reg[0].status, reg[1].n_links, reg[1].S, views[2].t[0]);
    return reg[1].n_links == n_kp && reg[1].S == 2.0 ? 0 : 1;
}
#endif
