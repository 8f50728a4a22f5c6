// tests/test_sfm_register_ref.py: a host build of sfm_register_core.h (the plan, a pair's match count, when a link counts, its ratio,
// the pose and point transforms) as the kernels use them, around plain loops: slots by a minimum per keypoint, the lower median by a
// sort. The test holds the result to the numpy statement tests/sfm_register_ref.py.
//   sfr_host_plan(pairs, n_pairs, n_frames, root, plan out) -> 0, or -1 on a frame index out of range
//   sfr_host_register(frame_off, n_frames, pairs, n_pairs, total_m, plan in or null, matches, mask, points3d, tv, root, min_links,
//                     views out, reg out, world out [total_m][3], zeroed by the caller) -> 0 / -1
//     total_m: the length of the match arrays. plan in: the plan to walk; null: the pair list's own. A pair that is not
//     sfr::pair_fits, or whose plan entry is not sfr::plan_entry_fits, has no matches and the entry {0, -1, 0, 0}, as in the kernels.
// -DSFR_HOST_MAIN: a stand-alone program (for a sanitizer run) that registers a small chain and prints its scales, then hands
// sfr::pair_fits and sfr_host_register records that do not fit -- among them a match_off whose sum with m does not fit 64 bits.
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
std::vector<Kept> kept_of(const gms_pair& pr, const gms_two_view& tv, const sfr::PairRanges& fr, const gms_dmatch* m, const uint8_t* mask, int* n_pts)
{
    std::vector<Kept> out;
    const int n = sfr::pair_count(pr, tv);
    const int64_t na = fr.na, nb = fr.nb;
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

int sfr_host_register(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, int64_t total_m,
                      const gms_sfm_plan_entry* plan_in, const gms_dmatch* matches, const uint8_t* mask, const double* pts,
                      const gms_two_view* tv, int root, int min_links, gms_sfm_view* views, gms_sfm_pair_reg* reg, double* world)
{
    std::vector<gms_sfm_plan_entry> plan((size_t)n_pairs);
    if (n_frames < 1 || root < 0 || root >= n_frames) return -1;
    if (plan_in) plan.assign(plan_in, plan_in + n_pairs);
    else if (sfr_host_plan(pairs, n_pairs, n_frames, root, plan.data()) != 0) return -1;
    std::vector<sfr::PairRanges> fr((size_t)n_pairs);
    std::vector<int> fits((size_t)n_pairs, 0);
    for (int i = 0; i < n_pairs; i++) {
        fits[i] = sfr::pair_fits(pairs[i], frame_off, n_frames, frame_off[n_frames], total_m, &fr[i]) && sfr::plan_entry_fits(plan[i], i);
        if (!fits[i]) plan[i] = gms_sfm_plan_entry{0, -1, 0, 0};
    }
    for (int f = 0; f < n_frames; f++) {
        views[f] = gms_sfm_view{};
        views[f].pair = -1;
    }
    views[root].R[0] = views[root].R[4] = views[root].R[8] = 1.0;
    views[root].registered = 1;
    std::vector<std::vector<Kept>> kept((size_t)n_pairs);
    std::vector<int> n_pts((size_t)n_pairs), ok((size_t)n_pairs, 0);
    for (int i = 0; i < n_pairs; i++)
        if (fits[i]) kept[i] = kept_of(pairs[i], tv[i], fr[i], matches, mask, &n_pts[i]);
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
                const int64_t na = fr[i].na;
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
    const int64_t total_m = 64 + n_kp, total_kp = frame_off[n_frames];
    gms_sfm_view views[3];
    gms_sfm_pair_reg reg[2];
    if (sfr_host_register(frame_off, n_frames, pairs, n_pairs, total_m, nullptr, m.data(), mask.data(), pts.data(), tv, 0, 8, views, reg,
                          world.data()) != 0)
        return 1;
    std::printf("sfr_host: tiny %d %d %.6f %.6f\n", reg[0].status, reg[1].n_links, reg[1].S, views[2].t[0]);
    if (reg[1].n_links != n_kp || reg[1].S != 2.0) return 1;

    // Records that do not fit (tests/sfm_register_cases.py, misfit_records): frame_a = n_frames, frame_b = -1, m = -3, match_off = -1, a
    // range that ends 5 slots past the arrays, and match_off = 2^63 - 2 with m = 5, whose sum does not fit 64 bits. The predicate
    // says no to each without forming that sum, and yes to the ranges that end exactly with the arrays.
    const gms_pair misfit[6] = {{n_frames, 2, 10, 0, 0}, {1, -1, 10, 0, 0},           {1, 2, -3, 0, 0},
                                {1, 2, 10, 0, -1},       {1, 2, 10, 0, total_m - 5}, {1, 2, 5, 0, INT64_MAX - 1}};
    const gms_pair snug[3] = {{1, 2, 10, 0, total_m - 10}, {1, 2, 0, 0, total_m}, {0, 1, (int32_t)total_m, 0, 0}};
    sfr::PairRanges fr;
    int wrong = 0;
    for (const gms_pair& pr : misfit) wrong += sfr::pair_fits(pr, frame_off, n_frames, total_kp, total_m, &fr) ? 1 : 0;
    for (const gms_pair& pr : snug) wrong += sfr::pair_fits(pr, frame_off, n_frames, total_kp, total_m, &fr) ? 0 : 1;
    wrong += sfr::pair_fits(snug[0], frame_off, n_frames, total_kp - 1, total_m, &fr) ? 1 : 0;   // frame 2 ends past the keypoints
    wrong += sfr::pair_fits(snug[0], frame_off, n_frames, total_kp, -1, &fr) ? 1 : 0;
    const gms_sfm_plan_entry self = {1, 4, 1, 1}, forward = {1, 6, 1, 1}, below = {1, -2, 1, 1}, none = {1, -1, 0, 0}, idle = {0, 99, 0, 0};
    wrong += sfr::plan_entry_fits(self, 4) || sfr::plan_entry_fits(forward, 4) || sfr::plan_entry_fits(below, 4) ? 1 : 0;
    wrong += sfr::plan_entry_fits(none, 0) && sfr::plan_entry_fits(idle, 4) && sfr::plan_entry_fits(self, 5) ? 0 : 1;
    // The same records behind the chain, each planned to register frame 3 off pair 1 with pair 0's matches and points, and a pair
    // (3, 4) that hangs on the last of them: all skipped with zeros, the dependant without a model, the chain's records unchanged.
    const int64_t frame_off5[6] = {0, 40, 80, 120, 160, 200};
    gms_pair all[9] = {pairs[0], pairs[1]};
    gms_sfm_plan_entry plan[9] = {{1, -1, 0, 0}, {1, 0, 1, 1}};
    gms_two_view tv9[9] = {tv[0], tv[1]};
    for (int k = 0; k < 7; k++) {
        all[2 + k] = k < 6 ? misfit[k] : gms_pair{3, 4, n_kp, 0, 0};
        if (k == 0) all[2 + k].frame_a = 5;  // (n_frames of this call)
        plan[2 + k] = k < 6 ? gms_sfm_plan_entry{1, 1, 1, 2} : gms_sfm_plan_entry{1, 7, 1, 3};
        tv9[2 + k] = tv[0];
    }
    gms_sfm_view views5[5];
    gms_sfm_pair_reg reg9[9];
    std::vector<double> world9(world.size(), 0.0);
    if (sfr_host_register(frame_off5, 5, all, 9, total_m, plan, m.data(), mask.data(), pts.data(), tv9, 0, 8, views5, reg9, world9.data()) != 0)
        return 1;
    const gms_sfm_pair_reg skipped = {0.0, 0.0, 0, 0, -1, 0, GMS_SFM_SKIPPED, 0};
    for (int k = 0; k < 6; k++) wrong += std::memcmp(&reg9[2 + k], &skipped, sizeof skipped) != 0 ? 1 : 0;
    wrong += reg9[8].status == GMS_ERR_NO_MODEL && reg9[8].n_links == 0 && reg9[8].link == 7 ? 0 : 1;
    wrong += std::memcmp(reg9, reg, sizeof reg) != 0 || std::memcmp(views5, views, sizeof views) != 0 || world9 != world ? 1 : 0;
    wrong += views5[3].registered || views5[4].registered ? 1 : 0;
    std::printf("sfr_host: misfit records, %d wrong\n", wrong);
    return wrong == 0 ? 0 : 1;
}
#endif
