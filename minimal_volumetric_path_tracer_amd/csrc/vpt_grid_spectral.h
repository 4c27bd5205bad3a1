/*
 * vpt_grid_spectral.h -- spectral tracking in a chromatic medium on the density grid of vpt_grid.h (estimator 16,
 * vpt_hetero_spectral.h): Kutz, Habel, Li and Novak 2017, "Spectral and decomposition tracking for rendering
 * heterogeneous volumes".  One walk under the largest channel's extinction carries a weight per colour channel, so no
 * channel needs a pdf under another channel's extinction and nothing walks the grid's optical depth.  Written once and
 * compiled for the host (vpt_host.cpp: vpt_grid_spectral_probe_host) and the device, like vpt_grid_chroma.h.  An
 * extension: the reference has no counterpart.
 *
 * Per unit density channel k has the scattering coefficient ss[k] and the extinction st[k] = sa[k] + ss[k] > 0
 * (ChromaCoef, vpt_hetero_chroma.h).  The launch constants (vpt_grid_spectral_consts):
 *   sb = st[0] > st[1] ? st[0] : st[1];  sb = sb > st[2] ? sb : st[2];      the bounding extinction
 *   f[k] = st[k] / sb                                                       the largest channel's f is x / x == 1.0
 *   alb[k] = ss[k] / st[k]                                                  the collision's albedo, estimator 14's w's place
 * Everything is FP64 without contraction, in exactly this order.  mu is the majorant of the walk: rho_max in the global
 * walkers, the super-voxel's majorant in the local ones.
 *
 * Chromatic ratio tracking (vpt_grid_spectral_ratio_m, _lm_m): vpt_grid_ratio_m / vpt_grid_ratio_lm_m statement for
 * statement under sigma_t = sb -- the entry tests, the draws, the DDA, the boundary tests, the caps -- with the vector T[3]
 * in That's place, from (1.0, 1.0, 1.0).  At a tentative point with density rho:
 *   rho >= mu:  T[k] = T[k] * (1.0 - f[k]), k = 0, 1, 2; then the walk returns if T[0] == 0.0 and T[1] == 0.0 and
 *               T[2] == 0.0, and goes on otherwise (the largest channel is 0.0 from here on, the others still estimate)
 *   else        q = rho / mu;  T[k] = T[k] * (1.0 - f[k] * q)
 * Every "none" exit returns T as it stands; the step cap returns NaN in every channel.  There is no second draw: `steps`
 * is the number of draws.  A zero-length segment is 1.0 in every channel without a draw: the callers test the length
 * before they walk (GridSpectralTr::along, as GridRatioTr::along does), so the walker over [0, 0] is the scalar one's.
 * The largest channel: 1.0 * q == q, so its T is vpt_grid_ratio_*_m's That under sb bit for bit, with the same draws, on
 * every ray where that returns a non-zero value; where that returns +0.0 at rho >= mu this walk goes on for the other two.
 * Grey extinction (st[0] == st[1] == st[2]): every f[k] is 1.0, the three products are the scalar walker's one, and at
 * rho >= mu T * (1.0 - 1.0) is +0.0 in every channel and the walk returns: the scalar walker's value, draws, steps and end
 * state bit for bit, with no branch on the colour.
 *
 * Spectral delta track (vpt_grid_spectral_track_m, _lm_m): vpt_grid_track_m / vpt_grid_track_lm_m's walk under sb.  It
 * takes the path's throughput beta[3] and carries the weight W[3], from (1.0, 1.0, 1.0).  At a tentative point that passed
 * the boundary test, with density rho (vpt_grid_spectral_collide):
 *   q = rho >= mu ? 1.0 : rho / mu
 *   r[k] = f[k] * q;  n[k] = 1.0 - r[k];  h[k] = fabs(beta[k]) * W[k]
 *   hs = (h[0] + h[1]) + h[2];  where hs is not finite or not > 0.0:  h[0] = h[1] = h[2] = 1.0
 *   a_r = (h[0] * r[0] + h[1] * r[1]) + h[2] * r[2];  a_n = (h[0] * n[0] + h[1] * n[1]) + h[2] * n[2];  c = a_r + a_n
 *   a_n == 0.0: a real collision, NO draw;  else draw xi: real iff xi * c < a_r
 *   real:  g = c / a_r;  W[k] = W[k] * (r[k] * g);  the track returns the distance
 *   null:  g = c / a_n;  W[k] = W[k] * (n[k] * g);  the walk goes on from the tentative point
 * "None" returns -1 with W as the surface's weight; the step cap returns NaN (W is then what the walk had).  This is the
 * history-aware average variant: the probabilities a_r / c and a_n / c average the channels' real and null fractions
 * weighted by what the path carries, W included.  Channel k's expected weight over one tentative point is
 * (a_r / c) r[k] (c / a_r) + (a_n / c) n[k] (c / a_n) = r[k] + n[k] for the real and the null branch separately, whatever h
 * is: unbiased in every channel.  With beta = (1, 1, 1), h == W and sum_k W[k] r[k] (c / a_r) = c = sum_k W[k] (r[k] + n[k])
 * = sum_k W[k] on both branches: W[0] + W[1] + W[2] stays 3 up to rounding and no weight exceeds 3; in general
 * sum_k |beta[k]| W[k] stays sum_k |beta[k]|.
 * Grey extinction is a branch here, taken on a launch constant: the decisions xi * c < a_r and xi' * mu < rho round
 * differently, so vpt_grid_spectral_track calls the scalar track of estimator 10 under st[0] with W = (1.0, 1.0, 1.0): the
 * same draws, no extra one.
 *
 * vpt_grid_spectral_one is both walkers as the probes report them (vpt.h: vpt_grid_spectral_probe), each from the same
 * start state.
 */
#ifndef VPT_GRID_SPECTRAL_H
#define VPT_GRID_SPECTRAL_H

#include "vpt_grid_chroma.h"

/* the launch constants (header comment) */
typedef struct vpt_spectral_consts {
    double sb, f[3], alb[3];
    int grey;
} vpt_spectral_consts;

VPT_GR vpt_spectral_consts vpt_grid_spectral_consts(const double ss[3], const double st[3])
{
    vpt_spectral_consts k;
    double sb = st[0] > st[1] ? st[0] : st[1];
    sb = sb > st[2] ? sb : st[2];
    k.sb = sb;
    k.f[0] = st[0] / sb;
    k.f[1] = st[1] / sb;
    k.f[2] = st[2] / sb;
    k.alb[0] = ss[0] / st[0];
    k.alb[1] = ss[1] / st[1];
    k.alb[2] = ss[2] / st[2];
    k.grey = vpt_grid_chroma_grey(st);
    return k;
}

/* the ratio walkers' update at a tentative point (header comment): 1 where the walk returns */
VPT_GR int vpt_grid_spectral_weigh(const double f[3], double rho, double mu, double T[3])
{
    if (rho >= mu) {
        T[0] = T[0] * (1.0 - f[0]);
        T[1] = T[1] * (1.0 - f[1]);
        T[2] = T[2] * (1.0 - f[2]);
        return T[0] == 0.0 && T[1] == 0.0 && T[2] == 0.0;
    }
    const double q = rho / mu;
    T[0] = T[0] * (1.0 - f[0] * q);
    T[1] = T[1] * (1.0 - f[1] * q);
    T[2] = T[2] * (1.0 - f[2] * q);
    return 0;
}

/* chromatic ratio tracking under the global majorant (header comment): vpt_grid_ratio_m with T[3] in That's place */
VPT_GR void vpt_grid_spectral_ratio_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                      double sb, const double f[3], uint64_t* X, uint32_t* steps, double T[3])
{
    double t0, t1;
    if (steps) *steps = 0;
    T[0] = T[1] = T[2] = 1.0;
    if (!(G->rho_max > 0.0)) return;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return;
    double t = t0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        t = t + (-VPT_GRID_LOG(1 - vpt_erand48(X)) / (G->rho_max * sb));
        if (steps) *steps = (uint32_t)(k + 1);
        if (t > tmax || t >= t1 || t != t) return;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
        if (vpt_grid_spectral_weigh(f, rho, G->rho_max, T)) return;
    }
    T[0] = T[1] = T[2] = (double)NAN;
}

/* the same with local majorants (G->block >= 1): vpt_grid_ratio_lm_m's walk, restated as that restates the track's */
VPT_GR void vpt_grid_spectral_ratio_lm_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                         double sb, const double f[3], uint64_t* X, uint32_t* steps, double T[3])
{
    double t0, t1;
    if (steps) *steps = 0;
    T[0] = T[1] = T[2] = 1.0;
    if (!(G->rho_max > 0.0)) return;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        i[a] = vpt_grid_axis_index(G, a, o[a] + d[a] * t0) / G->block;
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        tn[a] = step[a] ? (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    const int max_cross = G->nb[0] + G->nb[1] + G->nb[2] + 4;
    double t = t0;
    int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
    double te = tn[a];
    double mu = te > t ? (double)G->maj[((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0]] : 0.0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        double rem = -VPT_GRID_LOG(1 - vpt_erand48(X));
        if (steps) *steps = (uint32_t)(k + 1);
        double tc = 0.0;
        int c = 0;
        for (; c < max_cross; ++c) {
            if (te > t) {
                if (mu > 0.0) {
                    const double s = mu * sb;
                    tc = t + (rem / s);
                    if (tc < te) break;  /* a tentative collision */
                    rem = rem - s * (te - t);
                }
                t = te;
            }
            if (!(te < t1) || te > tmax) return;
            i[a] += step[a];
            if (i[a] < 0 || i[a] >= G->nb[a]) return;
            tn[a] = (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a];
            a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
            te = tn[a];
            mu = te > t ? (double)G->maj[((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0]] : 0.0;
        }
        if (c == max_cross) return;
        if (tc > tmax || tc >= t1) return;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * tc, o[1] + d[1] * tc, o[2] + d[2] * tc);
        if (vpt_grid_spectral_weigh(f, rho, mu, T)) return;
        t = tc;
    }
    T[0] = T[1] = T[2] = (double)NAN;
}

/* the track's decision at a tentative point (header comment): 1 for a real collision, 0 for a null one; W is updated */
VPT_GR int vpt_grid_spectral_collide(const double f[3], const double beta[3], double rho, double mu, double W[3], uint64_t* X)
{
    const double q = rho >= mu ? 1.0 : rho / mu;
    const double r0 = f[0] * q, r1 = f[1] * q, r2 = f[2] * q;
    const double n0 = 1.0 - r0, n1 = 1.0 - r1, n2 = 1.0 - r2;
    double h0 = __builtin_fabs(beta[0]) * W[0], h1 = __builtin_fabs(beta[1]) * W[1], h2 = __builtin_fabs(beta[2]) * W[2];
    const double hs = (h0 + h1) + h2;
    if (!(hs > 0.0) || !(hs <= VPT_GRID_BIG)) h0 = h1 = h2 = 1.0;
    const double a_r = (h0 * r0 + h1 * r1) + h2 * r2;
    const double a_n = (h0 * n0 + h1 * n1) + h2 * n2;
    const double c = a_r + a_n;
    int real = 1;
    if (!(a_n == 0.0)) real = vpt_erand48(X) * c < a_r;
    if (real) {
        const double g = c / a_r;
        W[0] = W[0] * (r0 * g);
        W[1] = W[1] * (r1 * g);
        W[2] = W[2] * (r2 * g);
        return 1;
    }
    const double g = c / a_n;
    W[0] = W[0] * (n0 * g);
    W[1] = W[1] * (n1 * g);
    W[2] = W[2] * (n2 * g);
    return 0;
}

/* the spectral delta track under the global majorant (header comment): vpt_grid_track_m's walk and results */
VPT_GR double vpt_grid_spectral_track_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                        double sb, const double f[3], const double beta[3], uint64_t* X, uint32_t* steps,
                                        double W[3])
{
    double t0, t1;
    if (steps) *steps = 0;
    W[0] = W[1] = W[2] = 1.0;
    if (!(G->rho_max > 0.0)) return -1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return -1.0;
    double t = t0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        t = t + (-VPT_GRID_LOG(1 - vpt_erand48(X)) / (G->rho_max * sb));
        if (steps) *steps = (uint32_t)(k + 1);
        if (t > tmax || t >= t1 || t != t) return -1.0;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
        if (vpt_grid_spectral_collide(f, beta, rho, G->rho_max, W, X)) return t;
    }
    return (double)NAN;
}

/* the same with local majorants (G->block >= 1): vpt_grid_track_lm_m's walk */
VPT_GR double vpt_grid_spectral_track_lm_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                           double sb, const double f[3], const double beta[3], uint64_t* X, uint32_t* steps,
                                           double W[3])
{
    double t0, t1;
    if (steps) *steps = 0;
    W[0] = W[1] = W[2] = 1.0;
    if (!(G->rho_max > 0.0)) return -1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return -1.0;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        i[a] = vpt_grid_axis_index(G, a, o[a] + d[a] * t0) / G->block;
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        tn[a] = step[a] ? (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    const int max_cross = G->nb[0] + G->nb[1] + G->nb[2] + 4;
    double t = t0;
    int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
    double te = tn[a];
    double mu = te > t ? (double)G->maj[((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0]] : 0.0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        double rem = -VPT_GRID_LOG(1 - vpt_erand48(X));
        if (steps) *steps = (uint32_t)(k + 1);
        double tc = 0.0;
        int c = 0;
        for (; c < max_cross; ++c) {
            if (te > t) {  /* (a super-voxel the rounding left without length is passed over) */
                if (mu > 0.0) {
                    const double s = mu * sb;
                    tc = t + (rem / s);
                    if (tc < te) break;  /* a tentative collision */
                    rem = rem - s * (te - t);
                }
                t = te;
            }
            if (!(te < t1) || te > tmax) return -1.0;
            i[a] += step[a];
            if (i[a] < 0 || i[a] >= G->nb[a]) return -1.0;
            tn[a] = (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a];
            a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
            te = tn[a];
            mu = te > t ? (double)G->maj[((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0]] : 0.0;
        }
        if (c == max_cross) return -1.0;
        if (tc > tmax || tc >= t1) return -1.0;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * tc, o[1] + d[1] * tc, o[2] + d[2] * tc);
        if (vpt_grid_spectral_collide(f, beta, rho, mu, W, X)) return tc;
        t = tc;
    }
    return (double)NAN;
}

/* every transmittance factor of estimator 16 over [0, tmax], tmax > 0; lm, tl are constants at every call */
VPT_GR void vpt_grid_spectral_ratio(const vpt_grid_fields* G, const int tl, const int lm, const vpt_spectral_consts* k,
                                    const double o[3], const double d[3], double tmax, uint64_t* X, uint32_t* steps, double T[3])
{
    if (lm) vpt_grid_spectral_ratio_lm_m(G, tl, o, d, tmax, k->sb, k->f, X, steps, T);
    else vpt_grid_spectral_ratio_m(G, tl, o, d, tmax, k->sb, k->f, X, steps, T);
}

/* the track of estimator 16's decision; under grey extinction estimator 10's, with the weight 1.0 (header comment) */
VPT_GR double vpt_grid_spectral_track(const vpt_grid_fields* G, const int tl, const int lm, const vpt_spectral_consts* k,
                                      const double beta[3], const double o[3], const double d[3], double tmax, uint64_t* X,
                                      uint32_t* steps, double W[3])
{
    if (k->grey) {
        W[0] = W[1] = W[2] = 1.0;
        return vpt_grid_chroma_track(G, tl, lm, o, d, tmax, k->sb, X, steps);
    }
    return lm ? vpt_grid_spectral_track_lm_m(G, tl, o, d, tmax, k->sb, k->f, beta, X, steps, W)
              : vpt_grid_spectral_track_m(G, tl, o, d, tmax, k->sb, k->f, beta, X, steps, W);
}

/* both walkers from the state X0, as the probes report them: the track (t_coll; w = W at "none", W times the albedo at a
 * collision, +0 at the cap; its steps and end state), then the ratio walk over [0, tmax] */
VPT_GR void vpt_grid_spectral_one(const vpt_grid_fields* G, const int tl, const int lm, const vpt_spectral_consts* k,
                                  const double beta[3], const double o[3], const double d[3], double tmax, uint64_t X0,
                                  double* t_coll, double w[3], uint32_t* steps, uint64_t* X_track, double T[3],
                                  uint32_t* ratio_steps, uint64_t* X_ratio)
{
    uint64_t X = X0;
    double W[3];
    const double tc = vpt_grid_spectral_track(G, tl, lm, k, beta, o, d, tmax, &X, steps, W);
    *t_coll = tc;
    *X_track = X;
    if (tc != tc) w[0] = w[1] = w[2] = 0.0;
    else if (tc >= 0) {
        w[0] = W[0] * k->alb[0];
        w[1] = W[1] * k->alb[1];
        w[2] = W[2] * k->alb[2];
    } else {
        w[0] = W[0];
        w[1] = W[1];
        w[2] = W[2];
    }
    X = X0;
    vpt_grid_spectral_ratio(G, tl, lm, k, o, d, tmax, &X, ratio_steps, T);
    *X_ratio = X;
}

#endif
