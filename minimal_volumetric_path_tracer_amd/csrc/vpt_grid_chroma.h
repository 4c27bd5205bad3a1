/*
 * vpt_grid_chroma.h -- one distance decision in a chromatic medium on the density grid of vpt_grid.h (estimator 14,
 * vpt_hetero_chroma.h): hero-channel delta tracking with the balance heuristic over the three channels (spectral MIS;
 * Miller, Georgiev and Jarosz 2019, the family of vpt_grid_mis.h).  Written once and compiled for the host
 * (vpt_host.cpp: vpt_grid_chroma_probe_host) and the device, like vpt_grid_mis.h.  An extension: the reference has no
 * counterpart.
 *
 * Per unit density channel k has the scattering coefficient ss[k] and the extinction st[k] = sa[k] + ss[k] > 0.  A ray
 * o + d t with surface distance t (MAXFLOAT on a miss) and the stream state X.  Everything is FP64 without contraction,
 * in exactly this order:
 *   hero     st[0] == st[1] == st[2] (grey extinction): h = 0, no draw.  Else xi = erand48(X); h = (int)(xi * 3), 2 where
 *            that is more.
 *   track    tc = vpt_grid_track_lm_m or vpt_grid_track_m (G, tl, o, d, t, st[h], X, steps): estimator 10's track under
 *            the hero's extinction.  tc != tc is the step cap, tc < 0 "none", else a collision at tc.
 *   tau      the grid's optical depth vpt_grid_tau / vpt_grid_tau_tl over [0, tc] at a collision and over [0, t] at
 *            "none": one deterministic walk, no draw.
 *   e        x_k = st[k] * tau;  mn = x_0 < x_1 ? x_0 : x_1;  mn = mn < x_2 ? mn : x_2;  e_k = exp((x_k - mn) * -1.0)
 *            The channel with the smallest x_k has e_k == exp(-0) == 1, the others lie in [0, 1]: the sums below are
 *            >= 1 times a positive coefficient and nothing is 0 / 0, whatever tau is.
 *   w        at a collision:  den = ((st[0] * e_0 + st[1] * e_1) + st[2] * e_2) / 3.0, but den = st[0] under grey extinction
 *            (below);  w_k = (ss[k] * e_k) / den
 *   ws       at "none":       ws_k = e_k / (((e_0 + e_1) + e_2) / 3.0)
 *   T        a transmittance factor over a segment of optical depth tau:  T_k = exp(st[k] * tau * -1.0)
 * The hero is uniform, so a collision at t has the marginal density (1 / 3) sum_j st[j] rho(t) exp(-st[j] tau) and "none"
 * the probability (1 / 3) sum_j exp(-st[j] tau(t)).  Channel k's integrand over the marginal is w_k and ws_k (rho(t) and
 * exp(-mn) cancel): the one-sample balance heuristic over the three hero choices, unbiased in every channel, with
 * w_k <= 3 ss[k] / st[k] and ws_k <= 3.
 * Grey extinction (a launch constant): every x_k is the same number, so every e_k is exp(-0) == 1.0 and ws_k is
 * 1 / (3 / 3.0) == 1.0.  The mean of three equal terms is the term, but ((s + s) + s) / 3.0 is not s for every double:
 * 3 s is rounded, and the quotient rounds back to a neighbour of s for about 15 % of random doubles (s = 1.4 is one;
 * scripts/grid_chroma_sanitize.cpp and tests/test_grid_chroma.py count them).  So under grey extinction den is the
 * mean's exact value st[0] and not the rounded expression: w_k == ss[k] / st in the bits of estimator 10's albedo, and no
 * hero draw is taken -- the decision is estimator 10's, draw for draw.
 *
 * vpt_grid_chroma_one is one whole decision as the probes report it (vpt.h: vpt_grid_chroma_probe).
 */
#ifndef VPT_GRID_CHROMA_H
#define VPT_GRID_CHROMA_H

#include "vpt_grid.h"

/* the three extinctions are one number: no hero draw, and the weights are estimator 10's scalars */
VPT_GR int vpt_grid_chroma_grey(const double st[3]) { return st[0] == st[1] && st[1] == st[2]; }

/* the hero channel (header comment) */
VPT_GR int vpt_grid_chroma_hero(const double st[3], uint64_t* X)
{
    if (vpt_grid_chroma_grey(st)) return 0;
    const int h = (int)(vpt_erand48(X) * 3);
    return h < 2 ? h : 2;
}

/* st[h] without an indexed load: the coefficients are launch constants in registers on the device */
VPT_GR double vpt_grid_chroma_pick(const double st[3], int h) { return h == 0 ? st[0] : (h == 1 ? st[1] : st[2]); }

/* the delta track under the extinction sigma_t = st[h]; lm, tl are constants at every call */
VPT_GR double vpt_grid_chroma_track(const vpt_grid_fields* G, const int tl, const int lm, const double o[3], const double d[3],
                                    double t, double sigma_t, uint64_t* X, uint32_t* steps)
{
    return lm ? vpt_grid_track_lm_m(G, tl, o, d, t, sigma_t, X, steps) : vpt_grid_track_m(G, tl, o, d, t, sigma_t, X, steps);
}

/* the optical depth over [0, t]; tl is a constant at every call */
VPT_GR double vpt_grid_chroma_tau(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double t)
{
    return tl ? vpt_grid_tau_tl(G, o, d, t) : vpt_grid_tau(G, o, d, t);
}

/* e_k (header comment) */
VPT_GR void vpt_grid_chroma_e(const double st[3], double tau, double e[3])
{
    const double x0 = st[0] * tau, x1 = st[1] * tau, x2 = st[2] * tau;
    double mn = x0 < x1 ? x0 : x1;
    mn = mn < x2 ? mn : x2;
    e[0] = VPT_GRID_EXP((x0 - mn) * -1.0);
    e[1] = VPT_GRID_EXP((x1 - mn) * -1.0);
    e[2] = VPT_GRID_EXP((x2 - mn) * -1.0);
}

/* the weight of a collision behind the optical depth tau: the albedo's place in estimator 10 */
VPT_GR void vpt_grid_chroma_w(const double ss[3], const double st[3], double tau, double w[3])
{
    double e[3];
    vpt_grid_chroma_e(st, tau, e);
    const double den = vpt_grid_chroma_grey(st) ? st[0] : ((st[0] * e[0] + st[1] * e[1]) + st[2] * e[2]) / 3.0;
    w[0] = (ss[0] * e[0]) / den;
    w[1] = (ss[1] * e[1]) / den;
    w[2] = (ss[2] * e[2]) / den;
}

/* the weight of "none" behind the optical depth tau */
VPT_GR void vpt_grid_chroma_ws(const double st[3], double tau, double ws[3])
{
    double e[3];
    vpt_grid_chroma_e(st, tau, e);
    const double den = ((e[0] + e[1]) + e[2]) / 3.0;
    ws[0] = e[0] / den;
    ws[1] = e[1] / den;
    ws[2] = e[2] / den;
}

/* the transmittance of every channel over a segment of optical depth tau: vpt_grid_transmittance's operations */
VPT_GR void vpt_grid_chroma_T(const double st[3], double tau, double T[3])
{
    T[0] = VPT_GRID_EXP(st[0] * tau * -1.0);
    T[1] = VPT_GRID_EXP(st[1] * tau * -1.0);
    T[2] = VPT_GRID_EXP(st[2] * tau * -1.0);
}

/* one decision (header comment).  *t_coll = the collision distance, -1 for "none", NaN at the step cap; *tau and w: the
 * optical depth over [0, *t_coll] and w at a collision, over [0, t] and ws at "none", +0 at the cap */
VPT_GR void vpt_grid_chroma_one(const vpt_grid_fields* G, const int tl, const int lm, const double ss[3], const double st[3],
                                const double o[3], const double d[3], double t, uint64_t* X, int* hero, double* t_coll,
                                double* tau, double w[3], uint32_t* steps)
{
    const int h = vpt_grid_chroma_hero(st, X);
    *hero = h;
    const double tc = vpt_grid_chroma_track(G, tl, lm, o, d, t, vpt_grid_chroma_pick(st, h), X, steps);
    *t_coll = tc;
    *tau = 0.0;
    w[0] = w[1] = w[2] = 0.0;
    if (tc != tc) return;
    if (tc >= 0) {
        *tau = vpt_grid_chroma_tau(G, tl, o, d, tc);
        vpt_grid_chroma_w(ss, st, *tau, w);
    } else {
        *tau = vpt_grid_chroma_tau(G, tl, o, d, t);
        vpt_grid_chroma_ws(st, *tau, w);
    }
}

#endif
