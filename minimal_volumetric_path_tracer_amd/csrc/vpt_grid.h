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
 *
 * Local majorants (opt-in: vpt_grid_view.block = B >= 1, 0 = none; vpt_grid_track_lm).  The voxels are grouped
 * into cubic super-voxels of B voxels per axis, nb[a] = ceil(n[a] / B) of them (the last of an axis may be
 * partial); maj[bz][by][bx] is the float32 maximum of rho over the block, built on the host next to the
 * rho_max scan and widened to double on load.  Super-voxel planes are voxel planes, formed with vpt_grid_tau's
 * expression lo + (double)k * cell, k = ib * B, so the two walkers never disagree on a plane; the two
 * outermost planes of an axis are lo and hi themselves, so that the exit distance of a single super-voxel is
 * the slab test's t1 bit for bit.  The track: "none" with no draw when rho_max == 0 or the slab test leaves no
 * interval; else from t = t0, in the super-voxel of the entry point, each tentative step:
 *   1. draw xi; rem = -log(1 - xi), the optical depth still to cover             one draw, one step counted
 *   2. walk the super-voxels by DDA; in one with majorant mu and exit plane at te (only where te > t):
 *        mu == 0: skipped -- no draw, no density fetch, rem untouched
 *        else s = mu * sigma_t, tc = t + (rem / s); tc < te: a tentative collision at tc (3.)
 *        else rem = rem - s * (te - t)
 *      then t = te; none if te >= t1 or te > tmax, or when the walk leaves the grid; crossing takes no draw
 *   3. none if tc > tmax or tc >= t1; rho = density(o + d tc); rho >= mu: a real collision, NO draw; else draw
 *      xi'; xi' * mu < rho: a real collision; else t = tc and the next tentative step (1.) goes on in the same
 *      super-voxel
 * capped at 2^22 tentative steps (NaN) and at nb[0] + nb[1] + nb[2] + 4 crossings per tentative step (none).
 * Choices the description above leaves open, made so that one super-voxel (B >= max(n)) is the global track
 * bit for bit -- results, step counts, end states: a step is counted where xi is drawn (the global track
 * counts the step that ends in "none" too), so `steps` is the number of xi draws; s is formed as mu * sigma_t
 * and the candidate as t + (rem / s), the global track's t + (-log(1 - xi) / (rho_max * sigma_t)); a NaN
 * candidate fails tc < te and ends at the boundary test as "none".  With B = 1 the majorant is the voxel's own
 * density, no collision is null, and a track takes exactly one draw: analytic inversion of the optical depth.
 *
 * Ratio tracking (Novak et al. 2014; vpt_grid_ratio, vpt_grid_ratio_lm; estimator 11, vpt_hetero.h): a stochastic,
 * unbiased estimate That of exp(-sigma_t tau(o, d, tmax)) whose cost follows the majorant optical depth, not the
 * grid's resolution.  That = 1.0 with no draw exactly where the track returns "none" without one; else the
 * track's tentative points from the same state (step 1 and 2 above, with the global or the local majorant mu):
 * wherever the track returns "none" the estimate returns That; at a tentative point with density rho:
 * rho >= mu returns +0.0, else That = That * (1.0 - rho / mu) and the walk goes on.  There is NO second draw, so
 * `steps` is the number of draws.  Capped like the track (NaN).  With B >= max(n) the local estimate is the global
 * one bit for bit; with B = 1 a ray takes one draw and That is 1.0 where the track (B = 1) from the same state
 * returns "none" and +0.0 where it collides, with the same end state.
 *
 * Trilinear interpolation (opt-in: vpt_grid_view.interp = 1, carried in the word that was pad_; 0 = nearest, all of
 * the above).  The voxel values sit at the voxel centres lo + (i + 0.5) cell.  Lookup, per axis, for a point of the box:
 *   u = (p - lo) * inv_cell - 0.5;  !(u > 0): u = 0 (a NaN too);  u > n - 1: u = n - 1
 *   i0 = (int)floor(u) held to [0, max(n - 2, 0)];  i1 = min(i0 + 1, n - 1);  f = u - (double)i0, in [0, 1]
 * so the field is clamped at the border, not faded: constant along an axis in the outer half voxel, and zero outside
 * the box as before (the support and the slab test do not change).  The eight voxels are widened to double on load
 * and combined with lerp(a, b, f) = a + f * (b - a): four lerps along x, two along y, one along z.  A lerp returns a
 * exactly when a == b, so a uniform field's lookup is the nearest one bit for bit.
 * Overshoot: with 0 <= f <= 1 and b >= a the rounded product f * (b - a) is at most the rounded b - a, so a lerp is
 * at most fl(a + fl(b - a)), which is b or the double above it (and at most a where b < a: the product is <= 0).  One
 * ulp per lerp, three lerps deep: the lookup is at most three ulps above the largest of its eight corners -- above
 * the majorant by that much at most.  The walkers test rho >= mu before they use rho: such a value is a certain
 * collision (track) or the estimate +0.0 (ratio), never a weight 1 - rho / mu < 0.
 * Majorants: rho_max stays the global one.  A super-voxel's majorant is the maximum over its voxels dilated by one
 * voxel on every side (clamped to the grid): a point of super-voxel k has u in [kB - 0.5, (k + 1)B - 0.5), so it reads
 * voxels kB - 1 .. (k + 1)B, and a tentative point the rounding put a hair past the exit plane still does.  The
 * majorant grid is rebuilt when the grid, the block or the mode changes.  B >= max(n) is one super-voxel whose
 * majorant is rho_max: the global walk bit for bit.  B = 1 is no longer analytic inversion: the majorant is the maximum
 * of 27 voxels, collisions can be null, and a track can take more than one draw.
 * Track and ratio tracking: the four walkers above statement for statement; only the density at a tentative point is
 * the trilinear lookup (the walkers take the mode as a constant argument, vpt_grid_*_m).
 * Optical depth (vpt_grid_tau_tl): vpt_grid_tau's entry logic (tmax, rho_max, the slab test, tend); the DDA walks the
 * interpolation cells, n + 1 per axis, bounded by lo, lo + ((double)k + 0.5) * cell for k = 0 .. n - 1, and hi
 * (vpt_grid_tl_plane, the one expression).  Inside a cell the field along the ray is a polynomial of degree <= 3 in t,
 * which Simpson's rule integrates exactly: for each piece [t, te] with te > t
 *   tm = 0.5 * (t + te);  r0, rm, r1 = the lookup at o + d t, o + d tm, o + d te
 *   tau = tau + (((r0 + 4.0 * rm) + r1) * (te - t)) * (1.0 / 6.0)
 * and r1 is carried into the next piece as its r0 (the same expression, the same bits).  The entry cell of an axis is
 * floor((p - lo) * inv_cell - 0.5) + 1 held to [0, n]; a cell the rounding left without length is passed over, and
 * since the integrand is looked up by position, never by cell index, a cut misplaced by an ulp costs an ulp.  Capped
 * at n[0] + n[1] + n[2] + 7 pieces.  No draw; T = exp(sigma_t * tau * -1.0) as before.
 *
 * Emission (opt-in: vpt_grid_view.emit != NULL; vpt_grid_track_em_m, vpt_grid_track_lm_em_m).  An emission grid eps, float32
 * >= 0, on the density grid's box and resolution; the medium's source term is sigma_a rho(x) eps(x) rgb, radiance per unit
 * length -- Kirchhoff's form: where nothing absorbs, nothing emits.  eps(x) is looked up as rho(x) is: the voxel's value
 * (nearest), or the same eight voxels and weights as the density lookup, lerp for lerp (trilinear); zero outside the box.
 * The emitting walkers are the two tracks above statement for statement -- the same draws, t_coll, end state and step
 * count, bit for bit -- and score the collision estimator on every tentative collision: wherever the track has fetched rho at
 * a tentative point that passed the boundary test (step 2 of the global track, step 3 of the local one),
 *   esum = esum + ((rho * eps) / mu)        mu = rho_max, or the super-voxel's majorant
 * before rho is tested against mu, so null and real collisions and the no-draw case rho >= mu all score; a tentative point
 * the boundary test rejects scores nothing, and an empty super-voxel is skipped as before (rho = 0 there).  esum starts at
 * +0 and the terms are added in the order they occur.  Under the nearest lookup both factors are widened float32 values, so
 * the product is exact, and with mu == rho the score is eps bit for bit.  E[esum] = sigma_t * integral of
 * T(t) rho(t) eps(t) dt over the tracked segment, T = exp(-sigma_t tau): a tentative point falls into dt with probability
 * density T_mu(t) mu sigma_t summed over the null-collision histories, which is sigma_t mu T(t) once the nulls are weighed.
 *
 * Residual ratio tracking (Novak et al. 2014, section 5.1; vpt_grid_residual_lm_m; estimator 15, vpt_hetero_residual.h): ratio
 * tracking with local majorants over a control density under the field.  Beside the block maxima the host builds the block
 * minima ctl[bz][by][bx], the float32 minimum of rho over the super-voxel (vpt_grid_control_build; under the trilinear field
 * over the block dilated by one voxel on every side, vpt_grid_control_build_tl, as the maxima are); they lie directly behind
 * the nbv = nb[0] nb[1] nb[2] maxima of the majorant allocation, ctl = maj + nbv, and the walker takes the pointer as an
 * argument of its own (vpt_grid_fields is what it was).  In a block with minimum mn and majorant mu the part
 * exp(-sigma_t mn len) of the transmittance is taken analytically and only the residual rho - mn is tracked, against the
 * residual majorant mr = mu - mn.  The walk is vpt_grid_ratio_lm_m's statement for statement -- the entry tests (1.0 with no
 * draw, *tauc = +0.0), the DDA, the eager draw rem = -log(1 - xi) at the head of each tentative step, the caps -- with:
 *   per super-voxel entered (te > t): mn = (double)ctl[idx] beside mu; mr = mu - mn; !(mr > 0.0): skipped -- no candidate,
 *        rem untouched; else s = mr * sigma_t, tc = t + (rem / s), tested and rem reduced as before
 *   the control optical depth tauc, from +0.0, takes tauc = tauc + mn * (e - t) for every stretch [t, e] the walk passes in a
 *        block, in traversal order: up to a block's exit plane (e = min(te, tend), tend = min(tmax, t1), only where e > t, before
 *        t = te); up to a tentative point that passed the boundary test (e = tc, after the test, before the lookup); and where
 *        the boundary test rejects the tentative point, up to tend (only where tend > t).  So at every "none" exit tauc is mn
 *        integrated over [t0, tend], skipped and uniform blocks included; at the +0.0 exit it is the integral up to the
 *        tentative point; a walk that runs into the crossing cap returns what it has
 *   at a tentative point with density rho: rho >= mu returns +0.0; else if (rho > mn) That = That * (1.0 - (rho - mn) / mr)
 *        (a trilinear lookup may fall an ulp below the smallest of its corners as it may rise above the largest: hence the
 *        test, not an unconditional multiply, and the weight stays in [0, 1]); t = tc and the walk goes on.  No second draw:
 *        `steps` is the number of draws
 *   every "none" exit returns That * exp(sigma_t * tauc * -1.0) (vpt_grid_transmittance's operand order); a capped walk NaN.
 * Two identities follow.  (i) With ctl == 0 in every block the value, the end state and the step count are
 * vpt_grid_ratio_lm_m's bit for bit: mu - 0.0 == mu, (rho - 0.0) / mu == rho / mu, the multiply by 1.0 that is skipped at
 * rho == 0 changes no bit, and That * exp(-0) == That.  (ii) Where every super-voxel is uniform (mn == mu) no block has a
 * candidate: the walk takes exactly one draw and returns exp(-sigma_t tauc), the exact transmittance up to the order of the
 * sum, with zero variance -- at B = 1 under the nearest lookup on every field.  The estimate lies in [0, exp(-sigma_t tauc)].
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

/* the grid as the walkers read it (host or device pointer in rho): vpt_grid_fields, filled by vpt_grid_view_init.  The
 * view extends it by one pointer, `emit`, after every other field, and only the emitting walkers take the view: every
 * other walker takes the fields (a view converts to them), so a kernel without emission keeps a vpt_grid_fields -- the
 * object it kept before emission existed, under another name -- and its code is what it was */
typedef struct vpt_grid_fields {
    int32_t n[3];          /* nx, ny, nz */
    int32_t interp;        /* 0 nearest, 1 trilinear (header comment); the word that was padding */
    double lo[3], hi[3];
    double inv_cell[3];    /* n / (hi - lo) */
    double cell[3];        /* (hi - lo) / n */
    double rho_max;
    const float* rho;
    /* local majorants (header comment); block == 0: none, maj is not read */
    const float* maj;      /* nb[2] x nb[1] x nb[0] block maxima, x fastest */
    int32_t nb[3];
    int32_t block;
} vpt_grid_fields;
typedef struct vpt_grid_view : vpt_grid_fields {
    /* emission (header comment); NULL: none.  After every other field */
    const float* emit;     /* nz x ny x nx, the density's layout */
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

/* host: the view of a valid grid whose largest voxel is mx (`rho` is the pointer the walkers will read) */
static inline void vpt_grid_view_fill(vpt_grid_view* G, const int32_t n[3], const double lo[3], const double hi[3], float mx,
                                      const float* rho)
{
    for (int a = 0; a < 3; ++a) {
        G->n[a] = n[a];
        G->lo[a] = lo[a];
        G->hi[a] = hi[a];
        G->inv_cell[a] = (double)n[a] / (hi[a] - lo[a]);
        G->cell[a] = (hi[a] - lo[a]) / (double)n[a];
    }
    G->interp = 0;
    G->rho_max = (double)mx;
    G->rho = rho;
    G->maj = 0;
    G->nb[0] = G->nb[1] = G->nb[2] = 0;
    G->block = 0;
    G->emit = 0;
}

/* host: the same, with rho_max scanned here from the host's copy of the voxels */
static inline void vpt_grid_view_init(vpt_grid_view* G, const int32_t n[3], const double lo[3], const double hi[3],
                                      const float* density, const float* rho)
{
    const int64_t nv = (int64_t)n[0] * n[1] * n[2];
    float mx = 0.0f;
    for (int64_t i = 0; i < nv; ++i)
        if (density[i] > mx) mx = density[i];
    vpt_grid_view_fill(G, n, lo, hi, mx, rho);
}

/* host: the super-voxel counts of block size B >= 1 and the block maxima of `density` into out (nb[2] x nb[1] x
 * nb[0] floats, x fastest) */
static inline void vpt_grid_majorant_counts(const int32_t n[3], int32_t B, int32_t nb[3])
{
    for (int a = 0; a < 3; ++a) nb[a] = (n[a] - 1) / B + 1;
}

static inline void vpt_grid_majorant_build(const int32_t n[3], int32_t B, const float* density, float* out)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(n, B, nb);
    const int64_t nbv = (int64_t)nb[0] * nb[1] * nb[2];
    for (int64_t i = 0; i < nbv; ++i) out[i] = 0.0f;
    for (int32_t z = 0; z < n[2]; ++z)
        for (int32_t y = 0; y < n[1]; ++y) {
            const float* row = density + ((int64_t)z * n[1] + y) * n[0];
            float* orow = out + ((int64_t)(z / B) * nb[1] + y / B) * nb[0];
            for (int32_t x = 0; x < n[0]; ++x)
                if (row[x] > orow[x / B]) orow[x / B] = row[x];
        }
}

/* the same for the trilinear field (header comment): every block's maximum is taken over its voxels dilated by one
 * voxel on every side, so a voxel counts for every block that the voxels next to it lie in */
static inline void vpt_grid_majorant_build_tl(const int32_t n[3], int32_t B, const float* density, float* out)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(n, B, nb);
    const int64_t nbv = (int64_t)nb[0] * nb[1] * nb[2];
    for (int64_t i = 0; i < nbv; ++i) out[i] = 0.0f;
    for (int32_t z = 0; z < n[2]; ++z) {
        const int32_t bz0 = (z > 0 ? z - 1 : 0) / B, bz1 = (z + 1 < n[2] ? z + 1 : n[2] - 1) / B;
        for (int32_t y = 0; y < n[1]; ++y) {
            const int32_t by0 = (y > 0 ? y - 1 : 0) / B, by1 = (y + 1 < n[1] ? y + 1 : n[1] - 1) / B;
            const float* row = density + ((int64_t)z * n[1] + y) * n[0];
            for (int32_t x = 0; x < n[0]; ++x) {
                const int32_t bx0 = (x > 0 ? x - 1 : 0) / B, bx1 = (x + 1 < n[0] ? x + 1 : n[0] - 1) / B;
                for (int32_t bz = bz0; bz <= bz1; ++bz)
                    for (int32_t by = by0; by <= by1; ++by) {
                        float* orow = out + ((int64_t)bz * nb[1] + by) * nb[0];
                        for (int32_t bx = bx0; bx <= bx1; ++bx)
                            if (row[x] > orow[bx]) orow[bx] = row[x];
                    }
            }
        }
    }
}

/* host: the block minima of `density` into out, the layout and the blocks of vpt_grid_majorant_build: the control grid of
 * residual ratio tracking (header comment).  Every block holds a voxel, so every minimum is a voxel's value */
static inline void vpt_grid_control_build(const int32_t n[3], int32_t B, const float* density, float* out)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(n, B, nb);
    const int64_t nbv = (int64_t)nb[0] * nb[1] * nb[2];
    for (int64_t i = 0; i < nbv; ++i) out[i] = INFINITY;
    for (int32_t z = 0; z < n[2]; ++z)
        for (int32_t y = 0; y < n[1]; ++y) {
            const float* row = density + ((int64_t)z * n[1] + y) * n[0];
            float* orow = out + ((int64_t)(z / B) * nb[1] + y / B) * nb[0];
            for (int32_t x = 0; x < n[0]; ++x)
                if (row[x] < orow[x / B]) orow[x / B] = row[x];
        }
}

/* the same for the trilinear field: every block's minimum over its voxels dilated by one voxel on every side, as
 * vpt_grid_majorant_build_tl dilates the maximum */
static inline void vpt_grid_control_build_tl(const int32_t n[3], int32_t B, const float* density, float* out)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(n, B, nb);
    const int64_t nbv = (int64_t)nb[0] * nb[1] * nb[2];
    for (int64_t i = 0; i < nbv; ++i) out[i] = INFINITY;
    for (int32_t z = 0; z < n[2]; ++z) {
        const int32_t bz0 = (z > 0 ? z - 1 : 0) / B, bz1 = (z + 1 < n[2] ? z + 1 : n[2] - 1) / B;
        for (int32_t y = 0; y < n[1]; ++y) {
            const int32_t by0 = (y > 0 ? y - 1 : 0) / B, by1 = (y + 1 < n[1] ? y + 1 : n[1] - 1) / B;
            const float* row = density + ((int64_t)z * n[1] + y) * n[0];
            for (int32_t x = 0; x < n[0]; ++x) {
                const int32_t bx0 = (x > 0 ? x - 1 : 0) / B, bx1 = (x + 1 < n[0] ? x + 1 : n[0] - 1) / B;
                for (int32_t bz = bz0; bz <= bz1; ++bz)
                    for (int32_t by = by0; by <= by1; ++by) {
                        float* orow = out + ((int64_t)bz * nb[1] + by) * nb[0];
                        for (int32_t bx = bx0; bx <= bx1; ++bx)
                            if (row[x] < orow[bx]) orow[bx] = row[x];
                    }
            }
        }
    }
}

/* host: the majorant allocation of block size B >= 1 as the context and the host probes keep it -- the nbv block maxima and
 * directly behind them the nbv block minima (out: 2 nbv floats), for the nearest (tl == 0) or the trilinear field.  The
 * view's maj points at the first half; the residual walker's ctl is vpt_grid_control_of */
static inline void vpt_grid_majorant_control_build(const int32_t n[3], int32_t B, int tl, const float* density, float* out)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(n, B, nb);
    const int64_t nbv = (int64_t)nb[0] * nb[1] * nb[2];
    if (tl) {
        vpt_grid_majorant_build_tl(n, B, density, out);
        vpt_grid_control_build_tl(n, B, density, out + nbv);
    } else {
        vpt_grid_majorant_build(n, B, density, out);
        vpt_grid_control_build(n, B, density, out + nbv);
    }
}

/* host: turns the majorant grid of an initialised view on (B >= 1, `maj` the pointer the walkers will read) or
 * off (B == 0) */
static inline void vpt_grid_view_set_majorant(vpt_grid_view* G, int32_t B, const float* maj)
{
    G->block = B;
    G->maj = B ? maj : 0;
    if (B) vpt_grid_majorant_counts(G->n, B, G->nb);
    else G->nb[0] = G->nb[1] = G->nb[2] = 0;
}

VPT_GR int vpt_grid_axis_index(const vpt_grid_fields* G, int a, double p)
{
    const double f = floor((p - G->lo[a]) * G->inv_cell[a]);
    if (!(f >= 0.0)) return 0;  /* a hair below lo (or NaN) */
    return f < (double)G->n[a] ? (int)f : G->n[a] - 1;
}

/* density at a point of the box (the caller has clipped to it) */
VPT_GR double vpt_grid_density(const vpt_grid_fields* G, double px, double py, double pz)
{
    const int ix = vpt_grid_axis_index(G, 0, px), iy = vpt_grid_axis_index(G, 1, py), iz = vpt_grid_axis_index(G, 2, pz);
    return (double)G->rho[((int64_t)iz * G->n[1] + iy) * G->n[0] + ix];
}

/* one axis of the trilinear lookup (header comment): the two voxel indices and the weight of the upper one */
VPT_GR void vpt_grid_tl_axis(const vpt_grid_fields* G, int a, double p, int* i0, int* i1, double* f)
{
    const int n = G->n[a];
    double u = (p - G->lo[a]) * G->inv_cell[a] - 0.5;
    if (!(u > 0.0)) u = 0.0;  /* the outer half voxel below (or NaN) */
    if (u > (double)(n - 1)) u = (double)(n - 1);
    int i = (int)floor(u);
    const int top = n - 2 > 0 ? n - 2 : 0;
    if (i > top) i = top;
    if (i < 0) i = 0;
    *i0 = i;
    *i1 = i + 1 < n ? i + 1 : n - 1;
    *f = u - (double)i;
}

VPT_GR double vpt_grid_lerp(double a, double b, double f)
{
    return a + f * (b - a);
}

/* trilinear density at a point of the box (header comment) */
VPT_GR double vpt_grid_density_tl(const vpt_grid_fields* G, double px, double py, double pz)
{
    int x0, x1, y0, y1, z0, z1;
    double fx, fy, fz;
    vpt_grid_tl_axis(G, 0, px, &x0, &x1, &fx);
    vpt_grid_tl_axis(G, 1, py, &y0, &y1, &fy);
    vpt_grid_tl_axis(G, 2, pz, &z0, &z1, &fz);
    const int64_t r00 = ((int64_t)z0 * G->n[1] + y0) * G->n[0] + x0, r01 = ((int64_t)z0 * G->n[1] + y1) * G->n[0] + x0;
    const int64_t r10 = ((int64_t)z1 * G->n[1] + y0) * G->n[0] + x0, r11 = ((int64_t)z1 * G->n[1] + y1) * G->n[0] + x0;
    /* the eight fetches are four x-adjacent pairs (dx is 0 only where nx == 1).  Plain 32-bit loads: fetching a pair
     * with one 64-bit load where its address is 8-byte aligned was measured and lost */
    const int dx = x1 - x0;
    const double c00 = vpt_grid_lerp((double)G->rho[r00], (double)G->rho[r00 + dx], fx);
    const double c01 = vpt_grid_lerp((double)G->rho[r01], (double)G->rho[r01 + dx], fx);
    const double c10 = vpt_grid_lerp((double)G->rho[r10], (double)G->rho[r10 + dx], fx);
    const double c11 = vpt_grid_lerp((double)G->rho[r11], (double)G->rho[r11 + dx], fx);
    return vpt_grid_lerp(vpt_grid_lerp(c00, c01, fy), vpt_grid_lerp(c10, c11, fy), fz);
}

/* the density as the walkers read it at a tentative point; tl is a constant at every call, so one lookup remains */
VPT_GR double vpt_grid_lookup(const vpt_grid_fields* G, const int tl, double px, double py, double pz)
{
    return tl ? vpt_grid_density_tl(G, px, py, pz) : vpt_grid_density(G, px, py, pz);
}

/* slab test of o + d t against the box: the interval [*t0, *t1] with *t0 >= 0; returns 0 when there is none.
 * An axis with d == 0 takes part through o alone (lo <= o < hi). */
VPT_GR int vpt_grid_slab(const vpt_grid_fields* G, const double o[3], const double d[3], double* t0, double* t1)
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
VPT_GR double vpt_grid_tau(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax)
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

/* plane j of the interpolation cells of axis a, j = 0 .. n + 1: cell c lies between planes c and c + 1 */
VPT_GR double vpt_grid_tl_plane(const vpt_grid_fields* G, int a, int j)
{
    if (j <= 0) return G->lo[a];
    if (j > G->n[a]) return G->hi[a];
    return G->lo[a] + ((double)(j - 1) + 0.5) * G->cell[a];
}

/* optical depth of the trilinear field over t in [0, tmax] (header comment) */
VPT_GR double vpt_grid_tau_tl(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax)
{
    double t0, t1;
    if (!(tmax > 0.0) || !(G->rho_max > 0.0)) return 0.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return 0.0;
    const double tend = t1 < tmax ? t1 : tmax;
    if (!(t0 < tend)) return 0.0;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        const double f = floor(((o[a] + d[a] * t0) - G->lo[a]) * G->inv_cell[a] - 0.5) + 1.0;
        i[a] = !(f >= 0.0) ? 0 : (f < (double)G->n[a] ? (int)f : G->n[a]);
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        tn[a] = step[a] ? (vpt_grid_tl_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    double tau = 0.0, t = t0;
    double r0 = vpt_grid_density_tl(G, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
    const int max_steps = G->n[0] + G->n[1] + G->n[2] + 7;
    for (int k = 0; k < max_steps; ++k) {
        const int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
        const double te = tn[a] < tend ? tn[a] : tend;
        if (te > t) {
            const double tm = 0.5 * (t + te);
            const double rm = vpt_grid_density_tl(G, o[0] + d[0] * tm, o[1] + d[1] * tm, o[2] + d[2] * tm);
            const double r1 = vpt_grid_density_tl(G, o[0] + d[0] * te, o[1] + d[1] * te, o[2] + d[2] * te);
            tau = tau + (((r0 + 4.0 * rm) + r1) * (te - t)) * (1.0 / 6.0);
            t = te;
            r0 = r1;
        }
        if (!(tn[a] < tend)) break;
        i[a] += step[a];
        if (i[a] < 0 || i[a] > G->n[a]) break;
        tn[a] = (vpt_grid_tl_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a];
    }
    return tau;
}

VPT_GR double vpt_grid_transmittance(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax,
                                     double sigma_t)
{
    return VPT_GRID_EXP(sigma_t * vpt_grid_tau(G, o, d, tmax) * -1.0);
}

VPT_GR double vpt_grid_transmittance_tl(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax,
                                        double sigma_t)
{
    return VPT_GRID_EXP(sigma_t * vpt_grid_tau_tl(G, o, d, tmax) * -1.0);
}

/* delta tracking (header comment): the collision distance, -1 for "none", NaN for a capped track; *X is the
 * erand48 state, advanced by the draws taken; *steps (optional) counts the tentative steps */
VPT_GR double vpt_grid_track_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax, double sigma_t,
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
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
        if (rho >= G->rho_max) return t;
        if (vpt_erand48(X) * G->rho_max < rho) return t;
    }
    return (double)NAN;
}

/* the plane below super-voxel kb of axis a (kb == nb[a]: the plane above the last one); header comment */
VPT_GR double vpt_grid_block_plane(const vpt_grid_fields* G, int a, int kb)
{
    if (kb <= 0) return G->lo[a];
    if (kb >= G->nb[a]) return G->hi[a];
    return G->lo[a] + (double)(kb * G->block) * G->cell[a];
}

/* delta tracking with local majorants (header comment; G->block >= 1): vpt_grid_track's arguments and
 * results */
VPT_GR double vpt_grid_track_lm_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                double sigma_t, uint64_t* X, uint32_t* steps)
{
    double t0, t1;
    if (steps) *steps = 0;
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
    /* the current super-voxel: its exit axis and plane and its majorant, kept across null collisions (one
     * majorant fetch per super-voxel entered, none per tentative step) */
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
                    const double s = mu * sigma_t;
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
        if (rho >= mu) return tc;
        if (vpt_erand48(X) * mu < rho) return tc;
        t = tc;
    }
    return (double)NAN;
}

/* ratio tracking (header comment): the estimate That of exp(-sigma_t tau(o, d, tmax)), NaN for a capped walk;
 * *X is the erand48 state, advanced by the draws taken; *steps (optional) counts them */
VPT_GR double vpt_grid_ratio_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax, double sigma_t,
                             uint64_t* X, uint32_t* steps)
{
    double t0, t1;
    if (steps) *steps = 0;
    if (!(G->rho_max > 0.0)) return 1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return 1.0;
    double t = t0, That = 1.0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        t = t + (-VPT_GRID_LOG(1 - vpt_erand48(X)) / (G->rho_max * sigma_t));
        if (steps) *steps = (uint32_t)(k + 1);
        if (t > tmax || t >= t1 || t != t) return That;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t);
        if (rho >= G->rho_max) return 0.0;
        That = That * (1.0 - rho / G->rho_max);
    }
    return (double)NAN;
}

/* ratio tracking with local majorants (header comment; G->block >= 1): vpt_grid_ratio's arguments and results.
 * The walk is vpt_grid_track_lm's, restated: sharing it would put the weight into the track's loop */
VPT_GR double vpt_grid_ratio_lm_m(const vpt_grid_fields* G, const int tl, const double o[3], const double d[3], double tmax,
                                double sigma_t, uint64_t* X, uint32_t* steps)
{
    double t0, t1;
    if (steps) *steps = 0;
    if (!(G->rho_max > 0.0)) return 1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return 1.0;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        i[a] = vpt_grid_axis_index(G, a, o[a] + d[a] * t0) / G->block;
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        tn[a] = step[a] ? (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    const int max_cross = G->nb[0] + G->nb[1] + G->nb[2] + 4;
    double t = t0, That = 1.0;
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
                    const double s = mu * sigma_t;
                    tc = t + (rem / s);
                    if (tc < te) break;  /* a tentative collision */
                    rem = rem - s * (te - t);
                }
                t = te;
            }
            if (!(te < t1) || te > tmax) return That;
            i[a] += step[a];
            if (i[a] < 0 || i[a] >= G->nb[a]) return That;
            tn[a] = (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a];
            a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
            te = tn[a];
            mu = te > t ? (double)G->maj[((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0]] : 0.0;
        }
        if (c == max_cross) return That;
        if (tc > tmax || tc >= t1) return That;
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * tc, o[1] + d[1] * tc, o[2] + d[2] * tc);
        if (rho >= mu) return 0.0;
        That = That * (1.0 - rho / mu);
        t = tc;
    }
    return (double)NAN;
}

/* the control grid behind the majorants of a view with a majorant grid (header comment): ctl = maj + nbv */
VPT_GR const float* vpt_grid_control_of(const vpt_grid_fields* G)
{
    return G->maj + (int64_t)G->nb[0] * G->nb[1] * G->nb[2];
}

/* residual ratio tracking over the block minima ctl (header comment; G->block >= 1): vpt_grid_ratio_lm_m's arguments and
 * results, and the control optical depth in *tauc_out.  The walk is that walker's, restated */
VPT_GR double vpt_grid_residual_lm_m(const vpt_grid_fields* G, const float* ctl, const int tl, const double o[3], const double d[3],
                                   double tmax, double sigma_t, uint64_t* X, uint32_t* steps, double* tauc_out)
{
    double t0, t1;
    if (steps) *steps = 0;
    *tauc_out = 0.0;
    if (!(G->rho_max > 0.0)) return 1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return 1.0;
    const double tend = t1 < tmax ? t1 : tmax;
    int i[3], step[3];
    double tn[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        i[a] = vpt_grid_axis_index(G, a, o[a] + d[a] * t0) / G->block;
        step[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = step[a] ? 1.0 / d[a] : 0.0;
        tn[a] = step[a] ? (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] : VPT_GRID_BIG;
    }
    const int max_cross = G->nb[0] + G->nb[1] + G->nb[2] + 4;
    double t = t0, That = 1.0, tauc = 0.0;
    int a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
    double te = tn[a];
    double mu = 0.0, mn = 0.0;
    if (te > t) {
        const int64_t idx = ((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0];
        mu = (double)G->maj[idx];
        mn = (double)ctl[idx];
    }
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        double rem = -VPT_GRID_LOG(1 - vpt_erand48(X));
        if (steps) *steps = (uint32_t)(k + 1);
        double tc = 0.0;
        int c = 0;
        for (; c < max_cross; ++c) {
            if (te > t) {
                const double mr = mu - mn;
                if (mr > 0.0) {
                    const double s = mr * sigma_t;
                    tc = t + (rem / s);
                    if (tc < te) break;  /* a tentative collision */
                    rem = rem - s * (te - t);
                }
                const double e = te < tend ? te : tend;
                if (e > t) tauc = tauc + mn * (e - t);
                t = te;
            }
            if (!(te < t1) || te > tmax) {
                *tauc_out = tauc;
                return That * VPT_GRID_EXP(sigma_t * tauc * -1.0);
            }
            i[a] += step[a];
            if (i[a] < 0 || i[a] >= G->nb[a]) {
                *tauc_out = tauc;
                return That * VPT_GRID_EXP(sigma_t * tauc * -1.0);
            }
            tn[a] = (vpt_grid_block_plane(G, a, i[a] + (step[a] > 0)) - o[a]) * inv[a];
            a = tn[0] <= tn[1] ? (tn[0] <= tn[2] ? 0 : 2) : (tn[1] <= tn[2] ? 1 : 2);
            te = tn[a];
            mu = 0.0;
            mn = 0.0;
            if (te > t) {
                const int64_t idx = ((int64_t)i[2] * G->nb[1] + i[1]) * G->nb[0] + i[0];
                mu = (double)G->maj[idx];
                mn = (double)ctl[idx];
            }
        }
        if (c == max_cross) {
            *tauc_out = tauc;
            return That * VPT_GRID_EXP(sigma_t * tauc * -1.0);
        }
        if (tc > tmax || tc >= t1) {
            if (tend > t) tauc = tauc + mn * (tend - t);
            *tauc_out = tauc;
            return That * VPT_GRID_EXP(sigma_t * tauc * -1.0);
        }
        tauc = tauc + mn * (tc - t);
        const double rho = vpt_grid_lookup(G, tl, o[0] + d[0] * tc, o[1] + d[1] * tc, o[2] + d[2] * tc);
        if (rho >= mu) {
            *tauc_out = tauc;
            return 0.0;
        }
        if (rho > mn) That = That * (1.0 - (rho - mn) / (mu - mn));
        t = tc;
    }
    *tauc_out = tauc;
    return (double)NAN;
}

/* density and emission at a point of the box (header comment): vpt_grid_lookup's value in *rho, bit for bit, and eps from
 * the same voxels and weights */
VPT_GR void vpt_grid_lookup_em(const vpt_grid_view* G, const int tl, double px, double py, double pz, double* rho, double* eps)
{
    if (!tl) {
        const int ix = vpt_grid_axis_index(G, 0, px), iy = vpt_grid_axis_index(G, 1, py), iz = vpt_grid_axis_index(G, 2, pz);
        const int64_t r = ((int64_t)iz * G->n[1] + iy) * G->n[0] + ix;
        *rho = (double)G->rho[r];
        *eps = (double)G->emit[r];
        return;
    }
    int x0, x1, y0, y1, z0, z1;
    double fx, fy, fz;
    vpt_grid_tl_axis(G, 0, px, &x0, &x1, &fx);
    vpt_grid_tl_axis(G, 1, py, &y0, &y1, &fy);
    vpt_grid_tl_axis(G, 2, pz, &z0, &z1, &fz);
    const int64_t r00 = ((int64_t)z0 * G->n[1] + y0) * G->n[0] + x0, r01 = ((int64_t)z0 * G->n[1] + y1) * G->n[0] + x0;
    const int64_t r10 = ((int64_t)z1 * G->n[1] + y0) * G->n[0] + x0, r11 = ((int64_t)z1 * G->n[1] + y1) * G->n[0] + x0;
    const int dx = x1 - x0;
    const double c00 = vpt_grid_lerp((double)G->rho[r00], (double)G->rho[r00 + dx], fx);
    const double c01 = vpt_grid_lerp((double)G->rho[r01], (double)G->rho[r01 + dx], fx);
    const double c10 = vpt_grid_lerp((double)G->rho[r10], (double)G->rho[r10 + dx], fx);
    const double c11 = vpt_grid_lerp((double)G->rho[r11], (double)G->rho[r11 + dx], fx);
    *rho = vpt_grid_lerp(vpt_grid_lerp(c00, c01, fy), vpt_grid_lerp(c10, c11, fy), fz);
    const double e00 = vpt_grid_lerp((double)G->emit[r00], (double)G->emit[r00 + dx], fx);
    const double e01 = vpt_grid_lerp((double)G->emit[r01], (double)G->emit[r01 + dx], fx);
    const double e10 = vpt_grid_lerp((double)G->emit[r10], (double)G->emit[r10 + dx], fx);
    const double e11 = vpt_grid_lerp((double)G->emit[r11], (double)G->emit[r11 + dx], fx);
    *eps = vpt_grid_lerp(vpt_grid_lerp(e00, e01, fy), vpt_grid_lerp(e10, e11, fy), fz);
}

/* the emission alone (the models and the probes' callers; the walkers use the pair above) */
VPT_GR double vpt_grid_emission(const vpt_grid_view* G, const int tl, double px, double py, double pz)
{
    double rho, eps;
    vpt_grid_lookup_em(G, tl, px, py, pz, &rho, &eps);
    return eps;
}

/* the emitting track (header comment; G->emit != NULL): vpt_grid_track_m with the collision estimator's sum in *esum */
VPT_GR double vpt_grid_track_em_m(const vpt_grid_view* G, const int tl, const double o[3], const double d[3], double tmax,
                                  double sigma_t, uint64_t* X, uint32_t* steps, double* esum)
{
    double t0, t1;
    if (steps) *steps = 0;
    *esum = 0.0;
    if (!(G->rho_max > 0.0)) return -1.0;
    if (!vpt_grid_slab(G, o, d, &t0, &t1)) return -1.0;
    double t = t0;
    for (int k = 0; k < VPT_GRID_MAX_TRACK_STEPS; ++k) {
        t = t + (-VPT_GRID_LOG(1 - vpt_erand48(X)) / (G->rho_max * sigma_t));
        if (steps) *steps = (uint32_t)(k + 1);
        if (t > tmax || t >= t1 || t != t) return -1.0;
        double rho, eps;
        vpt_grid_lookup_em(G, tl, o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t, &rho, &eps);
        *esum = *esum + ((rho * eps) / G->rho_max);
        if (rho >= G->rho_max) return t;
        if (vpt_erand48(X) * G->rho_max < rho) return t;
    }
    return (double)NAN;
}

/* the emitting track with local majorants (header comment; G->block >= 1, G->emit != NULL): vpt_grid_track_lm_m with
 * the collision estimator's sum in *esum */
VPT_GR double vpt_grid_track_lm_em_m(const vpt_grid_view* G, const int tl, const double o[3], const double d[3], double tmax,
                                     double sigma_t, uint64_t* X, uint32_t* steps, double* esum)
{
    double t0, t1;
    if (steps) *steps = 0;
    *esum = 0.0;
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
            if (te > t) {
                if (mu > 0.0) {
                    const double s = mu * sigma_t;
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
        double rho, eps;
        vpt_grid_lookup_em(G, tl, o[0] + d[0] * tc, o[1] + d[1] * tc, o[2] + d[2] * tc, &rho, &eps);
        *esum = *esum + ((rho * eps) / mu);
        if (rho >= mu) return tc;
        if (vpt_erand48(X) * mu < rho) return tc;
        t = tc;
    }
    return (double)NAN;
}

/* the nearest-lookup walkers under the names they have always had */
VPT_GR double vpt_grid_track(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax, double sigma_t,
        uint64_t* X, uint32_t* steps)
{
    return vpt_grid_track_m(G, 0, o, d, tmax, sigma_t, X, steps);
}
VPT_GR double vpt_grid_track_lm(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax, double sigma_t,
        uint64_t* X, uint32_t* steps)
{
    return vpt_grid_track_lm_m(G, 0, o, d, tmax, sigma_t, X, steps);
}
VPT_GR double vpt_grid_ratio(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax, double sigma_t,
        uint64_t* X, uint32_t* steps)
{
    return vpt_grid_ratio_m(G, 0, o, d, tmax, sigma_t, X, steps);
}
VPT_GR double vpt_grid_ratio_lm(const vpt_grid_fields* G, const double o[3], const double d[3], double tmax, double sigma_t,
        uint64_t* X, uint32_t* steps)
{
    return vpt_grid_ratio_lm_m(G, 0, o, d, tmax, sigma_t, X, steps);
}

#endif
