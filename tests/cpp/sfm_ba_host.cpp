// The host build of sfm_ba_core.h behind a C interface for tests/test_sfm_ba_ref.py, which holds it against the
// numpy statement, and -- with -DSBA_HOST_MAIN -- a stand-alone program that runs the same code on a tiny problem and sweeps the
// workspace's layout, for a build with the sanitizers.
#include <stdio.h>
#include <string.h>

#include "sfm_ba_core.h"
#include "ws_layout.h"

extern "C" {

// one observation at (R, t, X): active, Pc, r, Jc, Jp (zeros when inactive), Huber's w and rho of r
int sba_host_observation(const double* R, const double* t, const double* X, double u, double v, double f, double huber_px, double* Pc, double* r,
                         double* Jc, double* Jp, double* w, double* rho)
{
    memset(Jc, 0, 12 * sizeof(double));
    memset(Jp, 0, 6 * sizeof(double));
    const bool active = sba::residual(R, t, X, u, v, f, Pc, r);
    if (active) sba::jacobians(R, t, Pc, f, Jc, Jp);
    sba::huber(r, huber_px, *w, *rho);
    return active ? 1 : 0;
}
void sba_host_rodrigues(const double* w, double* E) { sba::rodrigues(w, E); }
int sba_host_inv3(const double* V, double* I) { return sba::inv3_sym(V, I) ? 1 : 0; }
int sba_host_solve6(const double* M, const double* b, double* x)
{
    double L[36];
    if (!sba::chol6(M, L)) return 0;
    sba::chol6_solve(L, b, x);
    return 1;
}
// the rays of n observations summed in order, then X = A^-1 b
int sba_host_triangulate(const double* R, const double* t, const double* uv, int n, double* X)
{
    double A[9] = {0}, b[3] = {0}, Ai[9];
    for (int i = 0; i < n; i++) sba::ray_add(R + 9 * i, t + 3 * i, uv[2 * i], uv[2 * i + 1], A, b);
    const bool ok = sba::inv3_sym(A, Ai);
    sba::mat3_vec(Ai, b, X);
    return ok ? 1 : 0;
}
int sba_host_params_ok(const gms_sfm_ba_params* p) { return sba::params_ok(*p) ? 1 : 0; }

// the layout: regions in order, 256-byte aligned, none overlapping, each long enough, inside the total. Returns the bad cases.
int sba_host_layout_check()
{
    int bad = 0;
    const int64_t Ks[] = {0, 1, 63, 4096, 100001}, Cs[] = {0, 1, 4095, 4097, 50000};
    const int Fs[] = {1, 2, 12, 1000};
    for (int64_t K : Ks)
        for (int64_t Cc : Cs)
            for (int F : Fs) {
                const gms::SfmBaLayout L = gms::sfm_ba_layout(F, K, Cc);
                const size_t k = (size_t)K, c = (size_t)Cc, f = (size_t)F;
                const size_t at[] = {L.kp_track, L.kp_frame, L.list, L.uv, L.jc, L.jp, L.res, L.t_cnt, L.t_off, L.t_fill, L.t_used, L.tiles, L.xc,
                                     L.vinv, L.gp, L.qt, L.cand, L.U, L.L, L.lok, L.free_, L.vec, L.part, L.costp, L.actp, L.scal, L.flags, L.total};
                const size_t need[] = {4 * k, 4 * k, 4 * k, 16 * k, 96 * k, 48 * k, 16 * k, 4 * c, 4 * c, 4 * c, 4 * c,
                                       4 * ((c + gms::kSbaScanTile - 1) / gms::kSbaScanTile + 1), 24 * c, 72 * c, 24 * c, 24 * c, sizeof(gms_sfm_view) * f,
                                       288 * f, 288 * f, 4 * f, 4 * f, 288 * f, 8 * f, 16 * f, 8 * f, 128, 64};
                const int n = (int)(sizeof(need) / sizeof(need[0]));
                if (at[0] != 0) bad++;
                for (int i = 0; i < n; i++)
                    if (at[i] % 256 != 0 || at[i + 1] < at[i] + need[i]) bad++;
            }
    return bad;
}
}

#ifdef SBA_HOST_MAIN
int main()
{
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0, 0, 0}, t1[3] = {-1, 0, 0}, X[3] = {0.5, 0.25, 4.0};
    double Pc[3], r[2], Jc[12], Jp[6], w, rho;
    const int a = sba_host_observation(R, t1, X, -0.125, 0.0625, 800.0, 2.0, Pc, r, Jc, Jp, &w, &rho);
    const double RR[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1}, tt[6] = {0, 0, 0, -1, 0, 0}, uv[4] = {0.125, 0.0625, -0.125, 0.0625};
    double Y[3], E[9];
    const int ok = sba_host_triangulate(RR, tt, uv, 2, Y);
    const double wv[3] = {0.0, 0.0, 1e-3};
    sba_host_rodrigues(wv, E);
    double M[36] = {0}, b[6] = {1, 2, 3, 4, 5, 6}, x[6];
    for (int i = 0; i < 6; i++) M[7 * i] = 2.0;
    const int s = sba_host_solve6(M, b, x);
    (void)t0;
    printf("sba_host: tiny %d %.6f %.6f %d %.6f %.6f %.6f %d %.6f layout %d bad\n", a, r[0], r[1], ok, Y[0], Y[1], Y[2], s, x[5], sba_host_layout_check());
    return 0;
}
#endif
