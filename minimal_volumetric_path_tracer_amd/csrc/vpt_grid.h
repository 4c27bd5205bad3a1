/*
 * vpt_grid.h -- heterogeneous medium: a density grid, its optical depth and delta tracking.  Written once
 * and compiled for the host (vpt_host.cpp: vpt_grid_probe_host) and the device (estimator 10, vpt_hetero.h),
 * like vpt_accum.h, so that the GPU and the host state it once.  An extension in the sense HG and the depth
 * cap are: defined here, the reference has no counterpart.
 *
 * Density: nx x ny x nz float32 voxels rho >= 0, x fastest, piecewise constant inside the world box
 * [lo, hi]; rho = 0 outside.  The medium's coefficients are rho(x) sigma_a and rho(x) sigma_s (vpt_medium's
 * values are per unit density, so the albedo is constant).  The majorant is the global maximum rho_max.
 * Voxel index per axis: min(n - 1, (int)floor((p - lo) * inv_cell)) with inv_cell = n / (hi - lo) formed on
 * the host in double (a point the rounding left a hair below lo is held at voxel 0).  rho is widened to
 * double on load.  Everything is FP64 without contraction, in exactly this operation order; the division is
 * the correctly rounded one.  Directions are unit vectors (callers normalise), distances are along them.
 *
 * Optical depth tau(o, d, tmax): the line integral of rho over o + d t, t in [0, tmax], walked voxel by
 * voxel with a 3-D DDA; the pieces are added in traversal order (tau = tau + rho * (te - t)).  The
 * transmittance is exp(sigma_t * tau * -1.0).  No random draw.
 *
 * Delta tracking (o, d, tmax, sigma_t, erand48 state X): "none" (-1) when rho_max == 0 or the slab test
 * leaves no interval [t0, t1], t0 >= 0; else from t = t0:
 *   1. t = t + (-log(1 - xi) / (rho_max * sigma_t))                 one draw
 *   2. none if t > tmax or t >= t1
 *   3. rho = density(o + d t)
 *   4. rho >= rho_max: a real collision at t, NO draw
 *   5. else draw xi'; xi' * rho_max < rho: a real collision at t
 * capped at 2^22 tentative steps (a capped track returns NaN, like trace_ray_marching's step cap).  The
 * no-draw rule at the majorant is deliberate: with rho == 1 everywhere and the origin inside the box the
 * first step is 0 + (-log(1 - xi) / (1 sigma_t)), the reference's freeFlightSample bit for bit from the same
 * single draw, so estimator 10 on a uniform grid walks estimator 0's paths draw for draw.
 */
#ifndef VPT_GRID_H
#define VPT_GRID_H

#include <math.h>
#include <stdint.h>

#include "vpt_rng.h"

/* exp and log: libm's on the host; the device units define them to the device library's (vpt_math.h), which
 * reproduces libm bit for bit */
#ifndef VPT_GRID_EXP
#define VPT_GRID_EXP exp
#define VPT_GRID_LOG log
#endif

#ifdef __HIPCC__
#define VPT_GR __host__ __device__ static inline __attribute__((always_inline))
#else
#define VPT_GR static inline
#endif

#define VPT_GRID_MAX_VOXELS (1 << 27)
#define VPT_GRID_MAX_TRACK_STEPS (1 << 22)
#define VPT_GRID_BIG 1.7976931348623157e+308

/* the grid as the walkers read it (host or device pointer in rho); filled by vpt_grid_view_init */
typedef struct vpt_grid_view {
    int32_t n[3];          /* nx, ny, nz */
    int32_t pad_;
    double lo[3], hi[3];
    double inv_cell[3];    /* n / (hi - lo) */
    double cell[3];        /* (hi - lo) / n */
    double rho_max;
    const float* rho;
} vpt_grid_view;

/* 0 when valid, else 1 dimension < 1 or too many voxels, 2 box not finite or hi <= lo, 3 a density that is
 * NaN, negative or infinite (density may be NULL: dimensions and box only) */
static inline int vpt_grid_bad(const int32_t n[3], const double lo[3], const double hi[3], const float* density)
{
    if (n[0] < 1 || n[1] < 1 || n[2] < 1) return 1;
    if ((int64_t)n[0] * n[1] > VPT_GRID_MAX_VOXELS || (int64_t)n[0] * n[1] * n[2] > VPT_GRID_MAX_VOXELS) return 1;
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] - lo[a] == 0.0 && hi[a] - hi[a] == 0.0 && hi[a] > lo[a] && (hi[a] - lo[a]) - (hi[a] - lo[a]) == 0.0))
            return 2;
    if (density) {
        const int64_t nv = (int64_t)n[0] * n[1] * n[2];
        for (int64_t i = 0; i < nv; ++i)
            if (!(density[i] >= 0.0f && density[i] - density[i] == 0.0f)) return 3;
    }
    return 0;
}

/* host: the view of a valid grid (rho_max scanned here; `rho` is the pointer the walkers will read) */
static inline void vpt_grid_view_init(vpt_grid_view* G, const int32_t n[3], const double lo[3], const double hi[3],
                                      const float* density, const float* rho)
{
    const int64_t nv = (int64_t)n[0] * n[1] * n[2];
    float mx = 0.0f;
    for (int64_t i = 0; i < nv; ++i)
        if (density[i] > mx) mx = density[i];
    for (int a = 0; a < 3; ++a) {
        G->n[a] = n[a];
        G->lo[a] = lo[a];
        G->hi[a] = hi[a];
        G->inv_cell[a] = (double)n[a] / (hi[a] - lo[a]);
        G->cell[a] = (hi[a] - lo[a]) / (double)n[a];
    }
    G->pad_ = 0;
    G->rho_max = (double)mx;
    G->rho = rho;
}

VPT_GR int vpt_grid_axis_index(const vpt_grid_view* G, int a, double p)
{
    const double f = floor((p - G->lo[a]) * G->inv_cell[a]);
    if (!(f >= 0.0)) return 0;  /* a hair below lo (or NaN) */
    return f < (double)G->n[a] ? (int)f : G->n[a] - 1;
}

/* density at a point of the box (the caller has clipped to it) */
VPT_GR double vpt_grid_density(const vpt_grid_view* G, double px, double py, double pz)
{
    const int ix = vpt_grid_axis_index(G, 0, px), iy = vpt_grid_axis_index(G, 1, py), iz = vpt_grid_axis_index(G, 2, pz);
    return (double)G->rho[((int64_t)iz * G->n[1] + iy) * G->n[0] + ix];
}

/* slab test of o + d t against the box: the interval [*t0, *t1] with *t0 >= 0; returns 0 when there is none.
 * An axis with d == 0 takes part through o alone (lo <= o < hi). */
VPT_GR int vpt_grid_slab(const vpt_grid_view* G, const double o[3], const double d[3], double* t0, double* t1)
{
    double a0 = 0.0, a1 = VPT_GRID_BIG;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0) {
            if (!(o[a] >= G->lo[a] && o[a] < G->hi[a])) return 0;
            continue;
        }
        const double inv = 1.0 / d[a];
        double ta = (G->lo[a] - o[a]) * inv, tb = (G->hi[a] - o[a]) * inv;
        if (ta > tb) {
            const double s = ta;
            ta = tb;
            tb = s;
        }
        if (ta > a0) a0 = ta;
        if (tb < a1) a1 = tb;
        if (ta != ta || tb != tb) return 0;
    }
    *t0 = a0;
    *t1 = a1;
    return a0 < a1;
}

/* optical depth over t in [0, tmax] (header comment) */
VPT_GR double vpt_grid_tau(const vpt_grid_view* G, const double o[3], const double d[3], double tmax)
{
    double t0, t1;
    if (!(tmax > 0.0) || !(G->rho_max > 0.0)) return 0.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return 0.0;
    const double tend = t1 < tmax ? t1 : tmax;
    if (!(t0 < tend)) return 0.0;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        i[a] = vpt_grid_axis_index(G, a, o[a] + d[a] * t0);
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        /* the next plane of this axis: the voxel's upper face going up, its lower face going down */
        tn[a] = step[a] ? ((G->lo[a] + (double)(i[a] + (step[a] > 0)) * G->cell[a]) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    double tau = 0.0, t = t0;
    const int max_steps = G->n[0] + G->n[1] + G->n[2] + 4;
    for (int k = 0; k < max_steps; ++k) {
        const int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
        const double te = tn[a] < tend ? tn[a] : tend;
        if (te > t) {
            const double rho = (double)G->rho[((int64_t)i[2] * G->n[1] + i[1]) * G->n[0] + i[0]];
            tau = tau + rho * (te - t);
            t = te;
        }
        if (!(tn[a] < tend)) break;
        i[a] += step[a];
        if (i[a] < 0 || i[a] >= G->n[a]) break;
        tn[a] = ((G->lo[a] + (double)(i[a] + (step[a] > 0)) * G->cell[a]) - o[a]) * inv[a];
    }
    return tau;
}

VPT_GR double vpt_grid_transmittance(const vpt_grid_view* G, const double o[3], const double d[3], double tmax,
                                     double sigma_t)
{
    return VPT_GRID_EXP(sigma_t * vpt_grid_tau(G, o, d, tmax) * -1.0);
}

/* delta tracking (header comment): the collision distance, -1 for "none", NaN for a capped track; *X is the
 * erand48 state, advanced by the draws taken; *steps (optional) counts the tentative steps */
VPT_GR double vpt_grid_track(const vpt_grid_view* G, const double o[3], const double d[3], double tmax, double sigma_t,
                             uint64_t* X, uint32_t* steps)
{
    double t0, t1;
    if (steps) *steps = 0;
    if (!(G->rho_max > 0.0)) return -1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return -1.0;
    double t = t0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        t = t + (-VPT_GRID_LOG(1 - vpt_erand48(X)) / (G->rho_max * sigma_t));
        if (steps) *steps = (uint32_t)(k + 1);
        if (t > tmax || t >= t1 || t != t) return -1.0;
        const double rho = vpt_grid_density(G, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
        if (rho >= G->rho_max) return t;
        if (vpt_erand48(X) * G->rho_max < rho) return t;
    }
    return (double)NAN;
}

#endif
