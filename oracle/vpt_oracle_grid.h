/*
 * vpt_oracle_grid.h -- TEST INFRASTRUCTURE ONLY: the oracle's statement of the heterogeneous medium, written
 * from the specification (the header comments of csrc/vpt_grid.h and csrc/vpt_hetero.h),
 * not from the walkers: it includes none of the product's grid code and is organised differently.  The product
 * states every walker once per kind (track, ratio, emitting track; global and local majorant); here ONE generator
 * yields a ray's tentative points -- the draws, the step count, the boundary test -- for the global or the local
 * majorant, and ONE consumer applies the rule of the track, of ratio tracking or of the emitting track at each
 * point.  Everything that draws keeps the specification's operation order, FP64 without contraction.
 * The distance decisions of estimators 12, 13 and 14 follow at the end, on the same pieces, and behind them the walkers
 * of estimators 15 and 16: the residual ratio walk over the block minima, chromatic ratio tracking and the spectral track.
 *
 * Included by vpt_oracle.c after xi(c), M_EXP, M_LOG and v3 exist; plain C11.
 */
#ifndef VPT_ORACLE_GRID_H
#define VPT_ORACLE_GRID_H

#define OG_BIG 1.7976931348623157e+308
#define OG_MAX_STEPS (1 << 22)

/* ------------------------------------------------------------------ the grid (global state, next to g_s) */
typedef struct {
    int set;               /* a density grid is present */
    int n[3];              /* nx, ny, nz */
    int interp;            /* 0 nearest, 1 trilinear */
    int B;                 /* super-voxel size in voxels, 0: global majorant only */
    int nb[3];             /* super-voxels per axis: ceil(n / B) */
    double lo[3], hi[3];
    double inv_cell[3];    /* n / (hi - lo) */
    double cell[3];        /* (hi - lo) / n */
    double rho_max;
    float* rho;            /* [nz][ny][nx] */
    float* maj;            /* [nbz][nby][nbx], B >= 1 */
    float* ctl;            /* the control grid of estimator 15: the block minima, maj's layout and blocks */
    float* eps;            /* emission grid, rho's layout; NULL: none */
    double rgb[3];
} og_grid;

static og_grid g_grid;
static int g_hetero_fault = 0;  /* orc_hetero_set_fault: the mistake a heterogeneous tracer commits on purpose (tests) */

static void og_free(float** p)
{
    free(*p);
    *p = NULL;
}

static void og_clear(void)
{
    og_free(&g_grid.rho);
    og_free(&g_grid.maj);
    og_free(&g_grid.ctl);
    og_free(&g_grid.eps);
    memset(&g_grid, 0, sizeof g_grid);
}

static inline size_t og_at(int ix, int iy, int iz) { return ((size_t)iz * (size_t)g_grid.n[1] + (size_t)iy) * (size_t)g_grid.n[0] + (size_t)ix; }

/* super-voxel majorants: the float32 maximum over the block's voxels; under trilinear the block is dilated by one
 * voxel on every side (held to the grid), since a point of the block reads the voxels next to it too.  Beside them the
 * control grid: the float32 minimum over the same voxels (every block holds one) */
static void og_build_majorants(void)
{
    og_grid* G = &g_grid;
    const int B = G->B, dil = G->interp ? 1 : 0;
    for (int a = 0; a < 3; ++a) G->nb[a] = (G->n[a] + B - 1) / B;
    G->maj = (float*)malloc(sizeof(float) * (size_t)G->nb[0] * (size_t)G->nb[1] * (size_t)G->nb[2]);
    G->ctl = (float*)malloc(sizeof(float) * (size_t)G->nb[0] * (size_t)G->nb[1] * (size_t)G->nb[2]);
    for (int bz = 0; bz < G->nb[2]; ++bz)
        for (int by = 0; by < G->nb[1]; ++by)
            for (int bx = 0; bx < G->nb[0]; ++bx) {
                const int b[3] = {bx, by, bz};
                int first[3], last[3];
                for (int a = 0; a < 3; ++a) {
                    first[a] = b[a] * B - dil;
                    last[a] = (b[a] + 1) * B - 1 + dil;
                    if (first[a] < 0) first[a] = 0;
                    if (last[a] > G->n[a] - 1) last[a] = G->n[a] - 1;
                }
                float mx = 0.0f, mn = INFINITY;
                for (int z = first[2]; z <= last[2]; ++z)
                    for (int y = first[1]; y <= last[1]; ++y)
                        for (int x = first[0]; x <= last[0]; ++x) {
                            if (G->rho[og_at(x, y, z)] > mx) mx = G->rho[og_at(x, y, z)];
                            if (G->rho[og_at(x, y, z)] < mn) mn = G->rho[og_at(x, y, z)];
                        }
                G->maj[((size_t)bz * (size_t)G->nb[1] + (size_t)by) * (size_t)G->nb[0] + (size_t)bx] = mx;
                G->ctl[((size_t)bz * (size_t)G->nb[1] + (size_t)by) * (size_t)G->nb[0] + (size_t)bx] = mn;
            }
}

/* 0, or -1 for a grid the specification does not define (dimensions, box, a density that is not finite and >= 0) */
static int og_set(const float* rho, int nx, int ny, int nz, const double lo[3], const double hi[3], int block, int interp)
{
    if (nx < 1 || ny < 1 || nz < 1 || block < 0 || (interp != 0 && interp != 1)) return -1;
    const size_t nv = (size_t)nx * (size_t)ny * (size_t)nz;
    for (int a = 0; a < 3; ++a)
        if (!(hi[a] > lo[a]) || !isfinite(lo[a]) || !isfinite(hi[a]) || !isfinite(hi[a] - lo[a])) return -1;
    for (size_t i = 0; i < nv; ++i)
        if (!(rho[i] >= 0.0f) || !isfinite(rho[i])) return -1;
    og_clear();
    og_grid* G = &g_grid;
    G->n[0] = nx;
    G->n[1] = ny;
    G->n[2] = nz;
    G->interp = interp;
    G->B = block;
    G->rho = (float*)malloc(sizeof(float) * nv);
    memcpy(G->rho, rho, sizeof(float) * nv);
    float mx = 0.0f;
    for (size_t i = 0; i < nv; ++i)
        if (rho[i] > mx) mx = rho[i];
    G->rho_max = (double)mx;
    for (int a = 0; a < 3; ++a) {
        G->lo[a] = lo[a];
        G->hi[a] = hi[a];
        G->inv_cell[a] = (double)G->n[a] / (hi[a] - lo[a]);
        G->cell[a] = (hi[a] - lo[a]) / (double)G->n[a];
    }
    if (block >= 1) og_build_majorants();
    G->set = 1;
    return 0;
}

/* ------------------------------------------------------------------ lookups */
/* voxel index of one axis: min(n - 1, floor((p - lo) * inv_cell)); a point a hair below lo is held at voxel 0 */
static int og_voxel(int a, double p)
{
    const double f = floor((p - g_grid.lo[a]) * g_grid.inv_cell[a]);
    if (!(f >= 0.0)) return 0;
    if (f >= (double)g_grid.n[a]) return g_grid.n[a] - 1;
    return (int)f;
}

/* one axis of the trilinear lookup: u = (p - lo) * inv_cell - 0.5 held to [0, n - 1]; i0 = floor(u) held to
 * [0, max(n - 2, 0)]; i1 = min(i0 + 1, n - 1); f = u - i0 */
static void og_tl_weights(int a, double p, int* i0, int* i1, double* f)
{
    const int n = g_grid.n[a];
    double u = (p - g_grid.lo[a]) * g_grid.inv_cell[a] - 0.5;
    if (!(u > 0.0)) u = 0.0;
    if (u > (double)(n - 1)) u = (double)(n - 1);
    int i = (int)floor(u);
    const int top = n - 2 > 0 ? n - 2 : 0;
    if (i > top) i = top;
    if (i < 0) i = 0;
    *i0 = i;
    *i1 = i + 1 < n - 1 ? i + 1 : n - 1;
    *f = u - (double)i;
}

static inline double og_lerp(double a, double b, double f) { return a + f * (b - a); }

/* a field (rho or eps) at a point of the box: the voxel's value, or four lerps along x, two along y, one along z */
static double og_field(const float* F, const double p[3])
{
    if (!g_grid.interp) return (double)F[og_at(og_voxel(0, p[0]), og_voxel(1, p[1]), og_voxel(2, p[2]))];
    int x0, x1, y0, y1, z0, z1;
    double fx, fy, fz;
    og_tl_weights(0, p[0], &x0, &x1, &fx);
    og_tl_weights(1, p[1], &y0, &y1, &fy);
    og_tl_weights(2, p[2], &z0, &z1, &fz);
    const double c00 = og_lerp((double)F[og_at(x0, y0, z0)], (double)F[og_at(x1, y0, z0)], fx);
    const double c01 = og_lerp((double)F[og_at(x0, y1, z0)], (double)F[og_at(x1, y1, z0)], fx);
    const double c10 = og_lerp((double)F[og_at(x0, y0, z1)], (double)F[og_at(x1, y0, z1)], fx);
    const double c11 = og_lerp((double)F[og_at(x0, y1, z1)], (double)F[og_at(x1, y1, z1)], fx);
    return og_lerp(og_lerp(c00, c01, fy), og_lerp(c10, c11, fy), fz);
}

static double og_field_on_ray(const float* F, const double o[3], const double d[3], double t)
{
    const double p[3] = {o[0] + d[0] * t, o[1] + d[1] * t, o[2] + d[2] * t};
    return og_field(F, p);
}

/* the slab test: the interval [*t0, *t1] of o + d t in the box with *t0 >= 0, 0 when there is none; an axis with
 * d == 0 takes part through o alone (lo <= o < hi) */
static int og_slab(const double o[3], const double d[3], double* t0, double* t1)
{
    double near = 0.0, far = OG_BIG;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0) {
            if (!(o[a] >= g_grid.lo[a] && o[a] < g_grid.hi[a])) return 0;
            continue;
        }
        const double inv = 1.0 / d[a];
        const double ta = (g_grid.lo[a] - o[a]) * inv, tb = (g_grid.hi[a] - o[a]) * inv;
        if (ta != ta || tb != tb) return 0;
        const double in = ta > tb ? tb : ta, out = ta > tb ? ta : tb;
        if (in > near) near = in;
        if (out < far) far = out;
    }
    *t0 = near;
    *t1 = far;
    return near < far;
}

static inline int og_argmin3(const double v[3])
{
    int a = 0;
    if (v[1] < v[a]) a = 1;
    if (v[2] < v[a]) a = 2;
    return a;
}

/* ------------------------------------------------------------------ optical depth (no draw) */
/* planes of the DDA that the optical depth walks: voxel planes lo + k cell (nearest, k = 0 .. n), or the planes of
 * the n + 1 interpolation cells: lo, lo + (k + 0.5) cell for k = 0 .. n - 1, hi (trilinear, j = 0 .. n + 1) */
static double og_tau_plane(int a, int j)
{
    if (!g_grid.interp) return g_grid.lo[a] + (double)j * g_grid.cell[a];
    if (j <= 0) return g_grid.lo[a];
    if (j > g_grid.n[a]) return g_grid.hi[a];
    return g_grid.lo[a] + ((double)(j - 1) + 0.5) * g_grid.cell[a];
}

static double og_tau(const double o[3], const double d[3], double tmax)
{
    const og_grid* G = &g_grid;
    double t0, t1;
    if (!(tmax > 0.0) || !(G->rho_max > 0.0)) return 0.0;
    if (!og_slab(o, d, &t0, &t1)) return 0.0;
    const double tend = t1 < tmax ? t1 : tmax;
    if (!(t0 < tend)) return 0.0;
    const int tl = G->interp;
    int cell[3], dir[3], last[3];
    double next[3], inv[3];
    for (int a = 0; a < 3; ++a) {
        const double p = o[a] + d[a] * t0;
        if (tl) {  /* the interpolation cell: floor((p - lo) * inv_cell - 0.5) + 1 held to [0, n] */
            const double f = floor((p - G->lo[a]) * G->inv_cell[a] - 0.5) + 1.0;
            cell[a] = !(f >= 0.0) ? 0 : (f >= (double)G->n[a] ? G->n[a] : (int)f);
            last[a] = G->n[a];
        } else {
            cell[a] = og_voxel(a, p);
            last[a] = G->n[a] - 1;
        }
        dir[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
        inv[a] = dir[a] ? 1.0 / d[a] : 0.0;
        next[a] = dir[a] ? (og_tau_plane(a, cell[a] + (dir[a] > 0)) - o[a]) * inv[a] : OG_BIG;
    }
    double tau = 0.0, t = t0;
    double r0 = tl ? og_field_on_ray(G->rho, o, d, t) : 0.0;
    const int cap = G->n[0] + G->n[1] + G->n[2] + (tl ? 7 : 4);
    for (int k = 0; k < cap; ++k) {
        const int a = og_argmin3(next);
        const double te = next[a] < tend ? next[a] : tend;
        if (te > t) {  /* a piece the rounding left without length is passed over */
            if (tl) {  /* Simpson: exact for the cubic the field is along the ray inside a cell */
                const double tm = 0.5 * (t + te);
                const double rm = og_field_on_ray(G->rho, o, d, tm);
                const double r1 = og_field_on_ray(G->rho, o, d, te);
                tau = tau + (((r0 + 4.0 * rm) + r1) * (te - t)) * (1.0 / 6.0);
                r0 = r1;
            } else {
                const double rho = (double)G->rho[og_at(cell[0], cell[1], cell[2])];
                tau = tau + rho * (te - t);
            }
            t = te;
        }
        if (!(next[a] < tend)) break;
        cell[a] += dir[a];
        if (cell[a] < 0 || cell[a] > last[a]) break;
        next[a] = (og_tau_plane(a, cell[a] + (dir[a] > 0)) - o[a]) * inv[a];
    }
    return tau;
}

/* ------------------------------------------------------------------ tentative points */
/* the plane below super-voxel kb of an axis (kb == nb: the plane above the last one): a voxel plane, the two
 * outermost ones lo and hi themselves */
static double og_block_plane(int a, int kb)
{
    if (kb <= 0) return g_grid.lo[a];
    if (kb >= g_grid.nb[a]) return g_grid.hi[a];
    return g_grid.lo[a] + (double)(kb * g_grid.B) * g_grid.cell[a];
}

typedef struct {
    const double* o;
    const double* d;
    double tmax, sigma_t;
    double t1, t;          /* the slab's exit, the walk's position */
    uint32_t steps;        /* xi draws */
    /* local majorants: the current super-voxel, its exit axis and plane, its majorant */
    int ib[3], dir[3];
    double next[3], inv[3];
    int ax;
    double te, mu;
    /* the residual walk (estimator 15; resid != 0): the current super-voxel's minimum, the candidates' majorant is
     * mu - mn, and the control optical depth of what the walk has passed */
    int resid;
    double mn, tauc, tend;
    int flat;              /* the walk passed a block with a control and no residual (mn > 0, mr == 0) */
} og_walk;

static double og_block_mu(const og_walk* w)
{
    if (!(w->te > w->t)) return 0.0;  /* no length: passed over */
    return (double)g_grid.maj[((size_t)w->ib[2] * (size_t)g_grid.nb[1] + (size_t)w->ib[1]) * (size_t)g_grid.nb[0] + (size_t)w->ib[0]];
}

/* the block's minimum, read where og_block_mu reads the majorant */
static double og_block_mn(const og_walk* w)
{
    if (!(w->te > w->t)) return 0.0;
    return (double)g_grid.ctl[((size_t)w->ib[2] * (size_t)g_grid.nb[1] + (size_t)w->ib[1]) * (size_t)g_grid.nb[0] + (size_t)w->ib[0]];
}

/* 0: the walk draws nothing and ends as "none" (rho_max == 0, or no slab interval) */
static int og_walk_begin(og_walk* w, const double o[3], const double d[3], double tmax, double sigma_t)
{
    double t0;
    w->o = o;
    w->d = d;
    w->tmax = tmax;
    w->sigma_t = sigma_t;
    w->steps = 0;
    w->resid = 0;
    w->flat = 0;
    w->tauc = 0.0;
    if (!(g_grid.rho_max > 0.0)) return 0;
    if (!og_slab(o, d, &t0, &w->t1)) return 0;
    w->t = t0;
    w->tend = w->t1 < tmax ? w->t1 : tmax;
    if (g_grid.B >= 1) {
        for (int a = 0; a < 3; ++a) {
            w->ib[a] = og_voxel(a, o[a] + d[a] * t0) / g_grid.B;
            w->dir[a] = d[a] > 0.0 ? 1 : (d[a] < 0.0 ? -1 : 0);
            w->inv[a] = w->dir[a] ? 1.0 / d[a] : 0.0;
            w->next[a] = w->dir[a] ? (og_block_plane(a, w->ib[a] + (w->dir[a] > 0)) - o[a]) * w->inv[a] : OG_BIG;
        }
        w->ax = og_argmin3(w->next);
        w->te = w->next[w->ax];
        w->mu = og_block_mu(w);
        w->mn = og_block_mn(w);
    }
    return 1;
}

/* the next tentative point: one draw, one step counted.  1 with the point's distance and majorant, 0 for "none".
 * The residual walk (w->resid, local majorants only) takes its candidates against mr = mu - mn -- a block where
 * !(mr > 0) has none and leaves rem untouched -- and adds to w->tauc the three pieces of the control optical depth in
 * traversal order: mn times the stretch up to a block's exit plane held to tend (where it has length); up to a tentative
 * point that passed the boundary test; and up to tend where the boundary test rejects the point (where tend > t).
 * Fault 11 (orc_hetero_set_fault): the last piece is left out. */
static int og_walk_next(og_walk* w, orc_ctx* c, double* tc_out, double* mu_out)
{
    const og_grid* G = &g_grid;
    if (G->B < 1) {  /* the global majorant */
        w->t = w->t + (-M_LOG(1 - xi(c)) / (G->rho_max * w->sigma_t));
        w->steps++;
        if (w->t > w->tmax || w->t >= w->t1 || w->t != w->t) return 0;
        *tc_out = w->t;
        *mu_out = G->rho_max;
        return 1;
    }
    double rem = -M_LOG(1 - xi(c));  /* the optical depth still to cover */
    w->steps++;
    const int max_cross = G->nb[0] + G->nb[1] + G->nb[2] + 4;
    for (int k = 0; k < max_cross; ++k) {
        if (w->te > w->t) {
            const double m = w->resid ? w->mu - w->mn : w->mu;
            if (m > 0.0) {  /* an empty super-voxel is skipped: rem untouched */
                const double s = m * w->sigma_t;
                const double tc = w->t + (rem / s);
                if (tc < w->te) {
                    if (tc > w->tmax || tc >= w->t1) {
                        if (w->resid && g_hetero_fault != 11 && w->tend > w->t) w->tauc = w->tauc + w->mn * (w->tend - w->t);
                        return 0;
                    }
                    if (w->resid) w->tauc = w->tauc + w->mn * (tc - w->t);
                    *tc_out = tc;
                    *mu_out = w->mu;
                    return 1;
                }
                rem = rem - s * (w->te - w->t);
            } else if (w->resid && w->mn > 0.0) {
                w->flat = 1;
            }
            if (w->resid) {
                const double e = w->te < w->tend ? w->te : w->tend;
                if (e > w->t) w->tauc = w->tauc + w->mn * (e - w->t);
            }
            w->t = w->te;
        }
        if (!(w->te < w->t1) || w->te > w->tmax) return 0;
        w->ib[w->ax] += w->dir[w->ax];
        if (w->ib[w->ax] < 0 || w->ib[w->ax] >= G->nb[w->ax]) return 0;
        w->next[w->ax] = (og_block_plane(w->ax, w->ib[w->ax] + (w->dir[w->ax] > 0)) - w->o[w->ax]) * w->inv[w->ax];
        w->ax = og_argmin3(w->next);
        w->te = w->next[w->ax];
        w->mu = og_block_mu(w);
        w->mn = og_block_mn(w);
    }
    return 0;  /* the crossing cap */
}

/* ------------------------------------------------------------------ the three rules at a tentative point */
enum { OG_TRACK = 0, OG_RATIO = 1 };

/* OG_TRACK: the collision distance, -1 for "none", NaN for a capped track; with esum != NULL the emitting track
 * (the grid has eps): every tentative point that passed the boundary test scores (rho * eps) / mu before rho is
 * tested.  OG_RATIO: the estimate That, NaN when capped.  *steps (optional): the xi draws. */
static double og_run(int kind, const double o[3], const double d[3], double tmax, double sigma_t, orc_ctx* c,
                     uint32_t* steps, double* esum)
{
    og_walk w;
    double That = 1.0;
    if (esum) *esum = 0.0;
    if (steps) *steps = 0;
    if (!og_walk_begin(&w, o, d, tmax, sigma_t)) return kind == OG_RATIO ? 1.0 : -1.0;
    double result = (double)NAN;
    for (int k = 0; k < OG_MAX_STEPS; ++k) {
        double tc, mu;
        if (!og_walk_next(&w, c, &tc, &mu)) {
            result = kind == OG_RATIO ? That : -1.0;
            break;
        }
        const double rho = og_field_on_ray(g_grid.rho, o, d, tc);
        if (esum) {
            const double eps = og_field_on_ray(g_grid.eps, o, d, tc);
            *esum = *esum + ((rho * eps) / mu);
        }
        if (kind == OG_RATIO) {
            if (rho >= mu) {
                result = 0.0;
                break;
            }
            That = That * (1.0 - rho / mu);
        } else {
            if (rho >= mu) {  /* a certain collision: NO draw */
                result = tc;
                break;
            }
            if (xi(c) * mu < rho) {
                result = tc;
                break;
            }
        }
        w.t = tc;
    }
    if (steps) *steps = w.steps;
    return result;
}

/* ================================================================== estimators 12, 13 and 14
 * The distance decisions of the three later estimators, written from the specification (the header comments of
 * csrc/vpt_grid_eqa.h, vpt_grid_mis.h and vpt_grid_chroma.h, DESIGN.md section 4, tests/{eqa,mis,chroma}_model.py) on
 * the pieces above: og_slab, og_tau, og_field_on_ray, og_run.  The product states each decision as a chain of
 * functions that hand draws and intermediate values on; here a decision is ONE function that fills one record, the
 * light's geometry is formed once per decision, and the equi-angular pdf is the oracle's estimator-1 helper
 * (equiangular_prob, vpt_oracle.c).  FP64 without contraction, the specification's operation order. */
static double equiangular_prob(double D, double ta, double tb, double s);

/* the settings next to the grid's: estimator 13's track fraction, estimator 14's colour multipliers */
static double g_mis_q = 0.5;
static double g_col_a[3] = {1.0, 1.0, 1.0}, g_col_s[3] = {1.0, 1.0, 1.0};

enum { OG_D_SURFACE = 0, OG_D_MEDIUM = 1, OG_D_EMPTY = 2, OG_D_CAP = 3 };

/* what a decision of estimator 12 or 13 found.  Fields a branch does not reach are +0 (the probes' convention):
 * all but psurf, strategy and steps on the surface and at the cap; T at an empty point */
typedef struct {
    int kind;        /* OG_D_SURFACE; OG_D_MEDIUM; OG_D_EMPTY: a distance with rho == 0 there; OG_D_CAP: the step cap */
    int strategy;    /* 1: the distance decision ran a delta track */
    uint32_t steps;  /* that track's draws */
    double psurf;    /* the transmittance over [0, t] */
    double dist;     /* -1 on the surface, NaN at the cap */
    double pe;       /* the equi-angular pdf times 1 - psurf at dist */
    double pdf;      /* estimator 12: pe; estimator 13: the combined pdf */
    double T;        /* the transmittance over [0, dist] */
    double rho_t;    /* the density at o + d dist */
} og_decision;

/* the grid's transmittance over [0, t] of the ray: no draw */
static double og_transmittance(const double o[3], const double d[3], double t, double sigma_t)
{
    return M_EXP(sigma_t * og_tau(o, d, t) * -1.0);
}

/* the part [a, b] of [0, t] that the box holds; without a slab interval all of [0, t].
 * Fault 6 (orc_hetero_set_fault): [0, t] whatever the box is -- the reference's interval. */
static void og_eqa_interval(const double o[3], const double d[3], double t, double* a, double* b)
{
    double t0, t1;
    *a = 0.0;
    *b = t;
    if (g_hetero_fault == 6) return;
    if (!og_slab(o, d, &t0, &t1)) return;
    if (t0 > 0.0) *a = t0;
    if (!(t < t1)) *b = t1;
}

/* the light seen from the ray: its distance D from the ray's line, the foot of the perpendicular proj, and the angles
 * of the interval's two ends (equiangular_params2's operations with a in 0.0's place and b in tMax's) */
typedef struct { double D, proj, ta, tb; } og_eqa_light;

static og_eqa_light og_eqa_see(const double o[3], const double d[3], const double lp[3], double a, double b)
{
    og_eqa_light g;
    const v3 dv = vsub(vload(lp), vload(o)), rd = vload(d);
    const double dvn = sqrt(vdot(dv, dv));
    g.proj = vdot(dv, rd) / vdot(rd, rd);
    g.D = sqrt(dvn * dvn - g.proj * g.proj);
    g.ta = M_ATAN2(a - g.proj, g.D);
    g.tb = M_ATAN2(b - g.proj, g.D);
    return g;
}

/* the density of the distance whose offset from the foot is s, times the medium branch's probability */
static double og_eqa_density(const og_eqa_light* g, double s, double psurf)
{
    return equiangular_prob(g->D, g->ta, g->tb, s) * (1 - psurf);
}

/* a decision's medium side once the distance is known: the density there, and T where there is medium */
static void og_decision_point(og_decision* r, const double o[3], const double d[3], double sigma_t)
{
    r->rho_t = og_field_on_ray(g_grid.rho, o, d, r->dist);
    r->kind = r->rho_t == 0.0 ? OG_D_EMPTY : OG_D_MEDIUM;
    if (r->kind == OG_D_MEDIUM) r->T = og_transmittance(o, d, r->dist, sigma_t);
}

/* estimator 12: the draw x, then the coin against psurf; the distance is equi-angular in [a, b] toward lp */
static og_decision og_decide_eqa(orc_ctx* c, const double o[3], const double d[3], double t, const double lp[3], double sigma_t)
{
    og_decision r;
    double a, b;
    memset(&r, 0, sizeof r);
    r.dist = -1.0;
    og_eqa_interval(o, d, t, &a, &b);
    const double x = xi(c);
    r.psurf = og_transmittance(o, d, t, sigma_t);
    if (xi(c) < r.psurf) return r;
    const og_eqa_light g = og_eqa_see(o, d, lp, a, b);
    const double s = g.D * M_TAN((1 - x) * g.ta + x * g.tb);
    r.pe = og_eqa_density(&g, s, r.psurf);
    r.pdf = r.pe;
    r.dist = s + g.proj;
    og_decision_point(&r, o, d, sigma_t);
    return r;
}

/* estimator 13: the draw x, the coin, and where the coin is below q a delta track's draws.  The coin less q over
 * 1 - q is estimator 12's coin.  The pdf of a medium distance combines both strategies' densities there:
 * q sigma_t rho T + (1 - q) pe.  Fault 7: the track's density without T. */
static og_decision og_decide_mis(orc_ctx* c, const double o[3], const double d[3], double t, const double lp[3], double sigma_t,
                                 double q)
{
    og_decision r;
    double a, b;
    memset(&r, 0, sizeof r);
    r.dist = -1.0;
    og_eqa_interval(o, d, t, &a, &b);
    const double x = xi(c);
    r.psurf = og_transmittance(o, d, t, sigma_t);
    const double coin = xi(c);
    r.strategy = coin < q;
    if (r.strategy) {
        const double tc = og_run(OG_TRACK, o, d, t, sigma_t, c, &r.steps, NULL);
        if (tc != tc) {
            r.kind = OG_D_CAP;
            r.dist = tc;
            return r;
        }
        if (tc < 0) return r;
        const og_eqa_light g = og_eqa_see(o, d, lp, a, b);
        r.dist = tc;
        r.pe = og_eqa_density(&g, tc - g.proj, r.psurf);
    } else {
        if ((coin - q) / (1 - q) < r.psurf) return r;
        const og_eqa_light g = og_eqa_see(o, d, lp, a, b);
        const double s = g.D * M_TAN((1 - x) * g.ta + x * g.tb);
        r.pe = og_eqa_density(&g, s, r.psurf);
        r.dist = s + g.proj;
    }
    og_decision_point(&r, o, d, sigma_t);
    const double pff = g_hetero_fault == 7 ? sigma_t * r.rho_t : sigma_t * r.rho_t * r.T;
    r.pdf = q * pff + (1 - q) * r.pe;
    return r;
}

/* ------------------------------------------------------------------ estimator 14: the chromatic medium */
typedef struct og_chroma_s {
    double ss[3], st[3];  /* per unit density and channel: scattering, extinction = absorption + scattering */
    int grey;             /* the three extinctions are one number */
} og_chroma;

static og_chroma og_chroma_of(const double sa[3], const double ss[3])
{
    og_chroma k;
    for (int i = 0; i < 3; ++i) {
        k.ss[i] = ss[i];
        k.st[i] = sa[i] + ss[i];
    }
    k.grey = k.st[0] == k.st[1] && k.st[1] == k.st[2];
    return k;
}

/* the hero channel: uniform from one draw, channel 0 without a draw under grey extinction */
static int og_chroma_hero(const og_chroma* k, orc_ctx* c)
{
    if (k->grey) return 0;
    const int h = (int)(xi(c) * 3);
    return h > 2 ? 2 : h;
}

/* the balance heuristic over the three hero choices behind the optical depth tau, from e_k = exp(-(st_k tau - min)):
 * collision != 0: w_k = ss_k e_k over the mean of st_j e_j (under grey extinction that mean is st itself, exactly);
 * else ws_k = e_k over the mean of e_j */
static v3 og_chroma_weight(const og_chroma* k, double tau, int collision)
{
    double xk[3], e[3];
    for (int i = 0; i < 3; ++i) xk[i] = k->st[i] * tau;
    double mn = xk[0] < xk[1] ? xk[0] : xk[1];
    mn = mn < xk[2] ? mn : xk[2];
    for (int i = 0; i < 3; ++i) e[i] = M_EXP((xk[i] - mn) * -1.0);
    if (!collision) {
        const double den = ((e[0] + e[1]) + e[2]) / 3.0;
        return V3(e[0] / den, e[1] / den, e[2] / den);
    }
    const double den = k->grey ? k->st[0] : ((k->st[0] * e[0] + k->st[1] * e[1]) + k->st[2] * e[2]) / 3.0;
    return V3((k->ss[0] * e[0]) / den, (k->ss[1] * e[1]) / den, (k->ss[2] * e[2]) / den);
}

/* every channel's transmittance over a segment of optical depth tau */
static v3 og_chroma_T(const og_chroma* k, double tau)
{
    return V3(M_EXP(k->st[0] * tau * -1.0), M_EXP(k->st[1] * tau * -1.0), M_EXP(k->st[2] * tau * -1.0));
}

/* ================================================================== estimators 15 and 16
 * Their walkers, written from the specification (the header comments of csrc/vpt_grid.h, "Residual ratio tracking", and of
 * csrc/vpt_grid_spectral.h) on the pieces above.  The product restates the local-majorant DDA in
 * every walker; here all three consume the tentative points of og_walk_begin / og_walk_next, the residual walk through
 * that generator's resid mode, the two spectral walkers under the bounding extinction in sigma_t's place. */

/* residual ratio tracking over [0, tmax] (local majorants: g_grid.B >= 1): the estimate of the transmittance, the control
 * optical depth in *tauc and the draws in *steps (optional).  Without a slab interval, or on an empty grid, 1.0 with no
 * draw and tauc = +0.  At a tentative point: rho >= mu returns +0.0; else the weight 1 - (rho - mn) / mr is multiplied in
 * only where rho > mn.  "None" returns That * exp(-sigma_t tauc), a capped walk NaN.
 * Fault 12 (orc_hetero_set_fault): the weight is taken against mu, 1 - (rho - mn) / mu. */
static double og_residual(const double o[3], const double d[3], double tmax, double sigma_t, orc_ctx* c, uint32_t* steps,
                          double* tauc)
{
    og_walk w;
    double That = 1.0;
    if (steps) *steps = 0;
    *tauc = 0.0;
    if (!og_walk_begin(&w, o, d, tmax, sigma_t)) return 1.0;
    w.resid = 1;
    double result = (double)NAN;
    for (int k = 0; k < OG_MAX_STEPS; ++k) {
        double tc, mu;
        if (!og_walk_next(&w, c, &tc, &mu)) {
            result = That * M_EXP(sigma_t * w.tauc * -1.0);
            if (w.tauc > 0.0 && That != 1.0) c->ext[ORC_EXT_RESID_BOTH]++;
            break;
        }
        const double rho = og_field_on_ray(g_grid.rho, o, d, tc);
        if (rho >= mu) {
            result = 0.0;
            break;
        }
        if (rho > w.mn) That = That * (1.0 - (rho - w.mn) / (g_hetero_fault == 12 ? mu : mu - w.mn));
        w.t = tc;
    }
    if (w.flat) c->ext[ORC_EXT_RESID_FLAT]++;
    if (steps) *steps = w.steps;
    *tauc = w.tauc;
    return result;
}

/* estimator 16's launch constants beside the medium's coefficients: the bounding extinction sb (the largest channel's),
 * f_k = st_k / sb (the largest channel's is x / x == 1.0), the collision's albedo alb_k = ss_k / st_k */
typedef struct og_spectral_s {
    og_chroma m;
    double sb, f[3], alb[3];
} og_spectral;

static og_spectral og_spectral_of(const og_chroma* m)
{
    og_spectral k;
    k.m = *m;
    k.sb = m->st[0] > m->st[1] ? m->st[0] : m->st[1];
    k.sb = k.sb > m->st[2] ? k.sb : m->st[2];
    for (int i = 0; i < 3; ++i) {
        k.f[i] = m->st[i] / k.sb;
        k.alb[i] = m->ss[i] / m->st[i];
    }
    return k;
}

/* chromatic ratio tracking over [0, tmax]: ratio tracking's walk under sb with a T per channel, from (1, 1, 1).  At a
 * tentative point with rho >= mu every T_k takes 1 - f_k and the walk ends only if all three are 0.0 (the largest channel is
 * from there on; under grey extinction all are, at once); else T_k takes 1 - f_k (rho / mu).  "None" returns T as it stands,
 * the cap NaN in every channel.
 * Fault 18 (orc_hetero_set_fault): (0, 0, 0) at the first rho >= mu, as the scalar walker returns. */
static v3 og_spectral_ratio(const og_spectral* k, const double o[3], const double d[3], double tmax, orc_ctx* c, uint32_t* steps)
{
    og_walk w;
    double T[3] = {1.0, 1.0, 1.0};
    int went_on = 0;
    if (steps) *steps = 0;
    if (!og_walk_begin(&w, o, d, tmax, k->sb)) return V3(1.0, 1.0, 1.0);
    int capped = 1;
    for (int n = 0; n < OG_MAX_STEPS; ++n) {
        double tc, mu;
        if (!og_walk_next(&w, c, &tc, &mu)) {
            capped = 0;
            break;
        }
        const double rho = og_field_on_ray(g_grid.rho, o, d, tc);
        if (rho >= mu) {
            if (g_hetero_fault == 18) T[0] = T[1] = T[2] = 0.0;
            for (int i = 0; i < 3; ++i) T[i] = T[i] * (1.0 - k->f[i]);
            if (T[0] == 0.0 && T[1] == 0.0 && T[2] == 0.0) {
                capped = 0;
                break;
            }
            went_on = 1;
        } else {
            const double q = rho / mu;
            for (int i = 0; i < 3; ++i) T[i] = T[i] * (1.0 - k->f[i] * q);
        }
        w.t = tc;
    }
    if (went_on) c->ext[ORC_EXT_RATIO_WENT_ON]++;
    if (steps) *steps = w.steps;
    if (capped) return V3((double)NAN, (double)NAN, (double)NAN);
    return V3(T[0], T[1], T[2]);
}

/* the spectral track over [0, tmax] for a path that carries beta: the delta track's walk under sb with a weight W per
 * channel, from (1, 1, 1).  At a tentative point the channels' real and null fractions r_k = f_k q and n_k = 1 - r_k
 * (q = rho / mu, 1.0 at rho >= mu) are averaged with the weights h_k = |beta_k| W_k -- (1, 1, 1) where their sum is not
 * finite or not positive -- into a_r and a_n; a_n == 0.0 is a real collision without a draw, else one draw decides, real
 * iff xi (a_r + a_n) < a_r; W_k takes r_k (c / a_r) or n_k (c / a_n).  The distance, -1 for "none" (W is then the
 * surface's weight), NaN for a capped track.  Under grey extinction the scalar track under st[0], W = (1, 1, 1).
 * Fault 17 (orc_hetero_set_fault): h_k = W_k, without |beta_k|. */
static double og_spectral_track(const og_spectral* k, const double beta[3], const double o[3], const double d[3], double tmax,
                                orc_ctx* c, uint32_t* steps, double W[3])
{
    og_walk w;
    W[0] = W[1] = W[2] = 1.0;
    if (k->m.grey) return og_run(OG_TRACK, o, d, tmax, k->m.st[0], c, steps, NULL);
    if (steps) *steps = 0;
    if (!og_walk_begin(&w, o, d, tmax, k->sb)) return -1.0;
    double result = (double)NAN;
    for (int n = 0; n < OG_MAX_STEPS; ++n) {
        double tc, mu, r[3], nn[3], h[3];
        if (!og_walk_next(&w, c, &tc, &mu)) {
            result = -1.0;
            break;
        }
        const double rho = og_field_on_ray(g_grid.rho, o, d, tc);
        const double q = rho >= mu ? 1.0 : rho / mu;
        for (int i = 0; i < 3; ++i) {
            r[i] = k->f[i] * q;
            nn[i] = 1.0 - r[i];
            h[i] = g_hetero_fault == 17 ? W[i] : fabs(beta[i]) * W[i];
        }
        const double hs = (h[0] + h[1]) + h[2];
        if (!(hs > 0.0) || !isfinite(hs)) h[0] = h[1] = h[2] = 1.0;
        const double a_r = (h[0] * r[0] + h[1] * r[1]) + h[2] * r[2];
        const double a_n = (h[0] * nn[0] + h[1] * nn[1]) + h[2] * nn[2];
        const double cc = a_r + a_n;
        int real = 1;
        if (a_n == 0.0) c->ext[ORC_EXT_NO_DRAW]++;
        else real = xi(c) * cc < a_r;
        if (real) {
            const double g = cc / a_r;
            for (int i = 0; i < 3; ++i) W[i] = W[i] * (r[i] * g);
            result = tc;
            break;
        }
        const double g = cc / a_n;
        for (int i = 0; i < 3; ++i) W[i] = W[i] * (nn[i] * g);
        w.t = tc;
    }
    if (steps) *steps = w.steps;
    return result;
}

#endif
