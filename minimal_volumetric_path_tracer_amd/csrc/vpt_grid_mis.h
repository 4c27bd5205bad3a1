/*
 * vpt_grid_mis.h -- the one-sample combination of the two distance strategies of the density grid (estimator 13,
 * vpt_hetero_mis.h): a delta track (vpt_grid.h; density sigma_t rho T, blind to the light) and the equi-angular distance
 * toward the picked light (vpt_grid_eqa.h; blind to the transmittance), under the balance heuristic.  Written once and
 * compiled for the host (vpt_host.cpp: vpt_grid_mis_probe_host) and the device, like vpt_grid_eqa.h, whose libm macros
 * it reuses.  An extension: the reference has no counterpart.
 *
 * A ray o + d t with surface distance t (MAXFLOAT on a miss), the picked light's position lp, sigma_t per unit density,
 * the track fraction q in [0, 1] and the stream state X.  Everything is FP64 without contraction, in exactly this order:
 *   (a, b) = vpt_grid_eqa_interval(G, o, d, t)
 *   x      = erand48(X)                      the equi-angular draw, always (estimator 12's)
 *   psurf  = vpt_grid_eqa_psurf(G, tl, o, d, t, sigma_t)      exact, no draw
 *   c      = erand48(X)                      one coin: the strategy, and estimator 12's surface coin
 *   c < q:   the track strategy.  tc = vpt_grid_track_lm_m or vpt_grid_track_m (G, tl, o, d, t, sigma_t, X, steps) --
 *            further draws; tc != tc is the step cap (a NaN result), tc < 0 the surface, else dist = tc and
 *              s = dist - proj;  pe = D / fabs(tb - ta) / (s * s + D * D) * (1 - psurf)
 *            with D, proj, ta, tb formed exactly as vpt_grid_eqa_distance forms them (vpt_grid_mis_pe)
 *   else:    the equi-angular strategy.  cc = (c - q) / (1 - q); cc < psurf is the surface, else
 *              dist = vpt_grid_eqa_distance(o, d, lp, a, b, x, psurf, &pe)        pe carries 1 - psurf
 *   rho_t = vpt_grid_lookup(G, tl, o + d dist);  rho_t == 0: the path ends, no draw, no contribution
 *   T     = vpt_grid_eqa_psurf(G, tl, o, d, dist, sigma_t)
 *   pff   = sigma_t * rho_t * T
 *   pdf   = q * pff + (1 - q) * pe
 * The surface has probability psurf under either strategy (a delta track reaches t with the transmittance over [0, t]),
 * and the medium distance has the marginal density q sigma_t rho T + (1 - q) (1 - psurf) p_eq = pdf.  A vertex weighted
 * sigma_s rho T / pdf is therefore unbiased, and its weight is bounded by (sigma_s / sigma_t) / q and by
 * sigma_s rho T / ((1 - q) (1 - psurf) p_eq) at once.
 * q == 0 is estimator 12 bit for bit and draw for draw: c < 0 is never true, (c - 0) / (1 - 0) is c and
 * 0 * pff + 1 * pe is pe.  q == 1 always tracks and never divides by 1 - q.  A light on the ray's line (D == 0) keeps
 * the reference's 0 / 0, as in estimator 12.
 *
 * vpt_grid_mis_one is one whole decision as the probes report it (vpt.h: vpt_grid_mis_probe).
 */
#ifndef VPT_GRID_MIS_H
#define VPT_GRID_MIS_H

#include "vpt_grid_eqa.h"

/* the equi-angular pdf times 1 - psurf of a distance `dist` that the other strategy chose: vpt_grid_eqa_distance's
 * geometry and its pdf, operation for operation, with s = dist - proj in place of the sampled s */
VPT_GR double vpt_grid_mis_pe(const double o[3], const double d[3], const double lp[3], double a, double b, double dist,
                              double psurf)
{
    const double dvx = lp[0] - o[0], dvy = lp[1] - o[1], dvz = lp[2] - o[2];
    const double dvn = VPT_GRID_SQRT(dvx * dvx + dvy * dvy + dvz * dvz);
    const double proj = (dvx * d[0] + dvy * d[1] + dvz * d[2]) / (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double D = VPT_GRID_SQRT(dvn * dvn - proj * proj);
    const double ta = VPT_GRID_ATAN2(a - proj, D);
    const double tb = VPT_GRID_ATAN2(b - proj, D);
    const double s = dist - proj;
    return D / VPT_GRID_FABS(tb - ta) / (s * s + D * D) * (1 - psurf);
}

/* the delta track of the track strategy; lm, tl are constants at every call */
VPT_GR double vpt_grid_mis_track(const vpt_grid_fields* G, const int tl, const int lm, const double o[3], const double d[3],
                                 double t, double sigma_t, uint64_t* X, uint32_t* steps)
{
    return lm ? vpt_grid_track_lm_m(G, tl, o, d, t, sigma_t, X, steps) : vpt_grid_track_m(G, tl, o, d, t, sigma_t, X, steps);
}

/* the combined pdf of a medium distance from the track's density pff = sigma_t rho_t T and the equi-angular pe */
VPT_GR double vpt_grid_mis_pdf(double q, double sigma_t, double rho_t, double T, double pe)
{
    const double pff = sigma_t * rho_t * T;
    return q * pff + (1 - q) * pe;
}

/* what vpt_grid_mis_distance found */
#define VPT_MIS_SURFACE 0
#define VPT_MIS_MEDIUM 1
#define VPT_MIS_CAP 2 /* the track's step cap: *dist is its NaN */

/* the distance decision up to the sampled distance, from the two draws x and c (header comment); the track's draws come
 * from *X.  *strategy = 1 where the track was taken.  VPT_MIS_MEDIUM: *dist is the distance and *pe the equi-angular
 * pdf times 1 - psurf there; an equi-angular distance is taken as it comes, as estimator 12 takes it */
VPT_GR int vpt_grid_mis_distance(const vpt_grid_fields* G, const int tl, const int lm, double sigma_t, double q,
                                 const double o[3], const double d[3], double t, const double lp[3], double a, double b,
                                 double x, double psurf, double c, uint64_t* X, int* strategy, double* dist, double* pe,
                                 uint32_t* steps)
{
    if (c < q) {
        *strategy = 1;
        const double tc = vpt_grid_mis_track(G, tl, lm, o, d, t, sigma_t, X, steps);
        if (tc != tc) {
            *dist = tc;
            return VPT_MIS_CAP;
        }
        if (tc < 0) return VPT_MIS_SURFACE;
        *dist = tc;
        *pe = vpt_grid_mis_pe(o, d, lp, a, b, tc, psurf);
        return VPT_MIS_MEDIUM;
    }
    *strategy = 0;
    const double cc = (c - q) / (1 - q);
    if (cc < psurf) return VPT_MIS_SURFACE;
    *dist = vpt_grid_eqa_distance(o, d, lp, a, b, x, psurf, pe);
    return VPT_MIS_MEDIUM;
}

/* one decision (header comment): the draws x and c from *X, then the track's where c < q.  *dist = -1 on the surface
 * and NaN at the step cap; the outputs a branch does not reach are +0, by vpt_grid_eqa_one's convention: *pdf, *pe, *T
 * and *rho_t on the surface and at the cap, and *T where *rho_t == 0 (the path ends there, and nothing reads it; *pdf is
 * then the formula's value on that +0, which is vpt_grid_eqa_one's pdf at q == 0).  *steps: the track's
 * tentative steps, 0 under the equi-angular strategy */
VPT_GR void vpt_grid_mis_one(const vpt_grid_fields* G, const int tl, const int lm, double sigma_t, double q, const double o[3],
                             const double d[3], double t, const double lp[3], uint64_t* X, double* psurf, int* strategy,
                             double* dist, double* pdf, double* pe, double* T, double* rho_t, uint32_t* steps)
{
    double a, b;
    vpt_grid_eqa_interval(G, o, d, t, &a, &b);
    const double x = vpt_erand48(X);
    const double ps = vpt_grid_eqa_psurf(G, tl, o, d, t, sigma_t);
    *psurf = ps;
    *dist = -1.0;
    *pdf = 0.0;
    *pe = 0.0;
    *T = 0.0;
    *rho_t = 0.0;
    *steps = 0;
    const double c = vpt_erand48(X);
    double ds = 0.0, pq = 0.0;
    const int ev = vpt_grid_mis_distance(G, tl, lm, sigma_t, q, o, d, t, lp, a, b, x, ps, c, X, strategy, &ds, &pq, steps);
    if (ev == VPT_MIS_SURFACE) return;
    *dist = ds;
    if (ev == VPT_MIS_CAP) return;
    *pe = pq;
    const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * ds, o[1] + d[1] * ds, o[2] + d[2] * ds);
    *rho_t = rho;
    double tr = 0.0;
    if (rho != 0.0) tr = vpt_grid_eqa_psurf(G, tl, o, d, ds, sigma_t);
    *T = tr;
    *pdf = vpt_grid_mis_pdf(q, sigma_t, rho, tr, pq);
}

#endif
