/*
 * vpt_grid_eqa.h -- equi-angular distance sampling in the density grid of vpt_grid.h (estimator 12,
 * vpt_hetero_eqa.h).  Written once and compiled for the host (vpt_host.cpp: vpt_grid_eqa_probe_host) and the
 * device, like vpt_grid.h.  An extension: the reference samples equi-angularly in a homogeneous medium only
 * (equiAngularParams2, include/volumetricBasicFunctions.h:209-223; equiAngularProb,
 * include/vptSamplingFunctions.h:60-62; MISVPTTracerRecursive, include/vptShadeMethods.h:1345-1481).
 *
 * A ray o + d t with surface distance t (MAXFLOAT on a miss), a light at lp, the equi-angular draw x and the
 * medium's sigma_t per unit density.  Everything is FP64 without contraction, in exactly this operation order:
 *   interval   the slab test gives (t0, t1) or none; a = t0 > 0 ? t0 : +0.0, b = t < t1 ? t : t1; without a slab
 *              interval a = +0.0 and b = t.  The medium lies in [a, b].  With the origin inside the box and the hit
 *              inside it a is +0.0 and b is t bit for bit.
 *   psurf      the grid's transmittance exp(sigma_t * tau * -1.0) over [0, t] (vpt_grid_tau / vpt_grid_tau_tl): the
 *              probability of the surface branch, exp(-0) = 1 where the ray meets no density.  No draw.
 *   distance   dv = lp - o; dvn = sqrt(dv . dv); proj = (dv . d) / (d . d); D = sqrt(dvn * dvn - proj * proj)
 *              ta = atan2(a - proj, D); tb = atan2(b - proj, D)
 *              s = D * tan((1 - x) * ta + x * tb); dist = s + proj
 *              pdf = D / fabs(tb - ta) / (s * s + D * D) * (1 - psurf)
 *              With a = +0.0 these are the reference's operations on tMax = b, operation for operation; a light on the
 *              ray's line (D == 0) keeps the reference's 0 / 0.
 * The distance is equi-angular in [a, b], so its density is D / ((tb - ta) (s^2 + D^2)); the factor 1 - psurf is the
 * probability of the medium branch.  Nothing here tracks: there is no majorant and no null collision.
 *
 * vpt_grid_eqa_one is one whole decision as the probes report it (vpt.h: vpt_grid_eqa_probe): the draw x, the coin
 * (coin < psurf is the surface), and on the medium branch the density at the sampled point and, where that is not
 * zero, the transmittance over [0, dist].
 */
#ifndef VPT_GRID_EQA_H
#define VPT_GRID_EQA_H

#include "vpt_grid.h"

/* libm's on the host; the device units define them to the device library's (vpt_math.h), which reproduces libm bit
 * for bit */
#ifndef VPT_GRID_ATAN2
#define VPT_GRID_ATAN2 atan2
#define VPT_GRID_TAN tan
#define VPT_GRID_SQRT sqrt
#define VPT_GRID_FABS fabs
#endif

/* the medium's interval [*a, *b] of the ray up to the surface distance t (header comment) */
VPT_GR void vpt_grid_eqa_interval(const vpt_grid_fields* G, const double o[3], const double d[3], double t, double* a,
                                  double* b)
{
    double t0, t1;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) {
        *a = 0.0;
        *b = t;
        return;
    }
    *a = t0 > 0.0 ? t0 : 0.0;
    *b = t < t1 ? t : t1;
}

/* the probability of the surface branch: the transmittance over [0, t]; tl is a constant at every call */
VPT_GR double vpt_grid_eqa_psurf(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double t,
                                 double sigma_t)
{
    return tl ? vpt_grid_transmittance_tl(G, o, d, t, sigma_t) : vpt_grid_transmittance(G, o, d, t, sigma_t);
}

/* the equi-angular distance in [a, b] toward lp from the draw x, and its pdf times 1 - psurf (header comment) */
VPT_GR double vpt_grid_eqa_distance(const double o[3], const double d[3], const double lp[3], double a, double b, double x,
                                    double psurf, double* pdf)
{
    const double dvx = lp[0] - o[0], dvy = lp[1] - o[1], dvz = lp[2] - o[2];
    const double dvn = VPT_GRID_SQRT(dvx * dvx + dvy * dvy + dvz * dvz);
    const double proj = (dvx * d[0] + dvy * d[1] + dvz * d[2]) / (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double D = VPT_GRID_SQRT(dvn * dvn - proj * proj);
    const double ta = VPT_GRID_ATAN2(a - proj, D);
    const double tb = VPT_GRID_ATAN2(b - proj, D);
    const double s = D * VPT_GRID_TAN((1 - x) * ta + x * tb);
    *pdf = D / VPT_GRID_FABS(tb - ta) / (s * s + D * D) * (1 - psurf);
    return s + proj;
}

/* one decision (header comment): two draws from *X, always.  *dist = -1 where the coin chose the surface, and *pdf,
 * *T and *rho_t are +0 there; *T is +0 too where *rho_t == 0 (the path ends there, and nothing reads it) */
VPT_GR void vpt_grid_eqa_one(const vpt_grid_fields* G, const int tl, double sigma_t, const double o[3], const double d[3],
                             double t, const double lp[3], uint64_t* X, double* psurf, double* dist, double* pdf, double* T,
                             double* rho_t)
{
    double a, b;
    vpt_grid_eqa_interval(G, o, d, t, &a, &b);
    const double x = vpt_erand48(X);
    const double ps = vpt_grid_eqa_psurf(G, tl, o, d, t, sigma_t);
    *psurf = ps;
    *dist = -1.0;
    *pdf = 0.0;
    *T = 0.0;
    *rho_t = 0.0;
    if (vpt_erand48(X) < ps) return;
    const double ds = vpt_grid_eqa_distance(o, d, lp, a, b, x, ps, pdf);
    *dist = ds;
    const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * ds, o[1] + d[1] * ds, o[2] + d[2] * ds);
    *rho_t = rho;
    if (rho == 0.0) return;
    *T = vpt_grid_eqa_psurf(G, tl, o, d, ds, sigma_t);
}

#endif
