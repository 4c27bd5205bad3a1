/*
 * vpt_host.cpp -- host-only part of libvpt: reference defaults, errors, PPM output.
 *
 * Default scene/camera/medium: include/Sphere.cpp:11-22, src/rt.cpp:752-759, src/rt.cpp:794.
 * PPM writer: src/rt.cpp:812-820 with the clamp of src/rt.cpp:803 and toDisplayValue of
 * include/mathUtilities.h:43-45; byte-identical output ("P3\n%d %d\n255\n", then "%d %d %d "
 * per pixel, no trailing newline).  The reference formats serially with fprintf; here the
 * pixels are converted and formatted in parallel (std::thread) and written with one fwrite
 * (a 4096^2 P3 file is ~150 MB).
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include <thread>

#include "vpt_accum.h"
#include "vpt_grid.h"
#include "vpt_grid_build.h"
#include "vpt_grid_eqa.h"
#include "vpt_grid_mis.h"
#include "vpt_grid_chroma.h"
#include "vpt_grid_spectral.h"
#include "vpt_internal.h"
#include "vpt_rng.h"

static thread_local std::string g_err;

int vpt_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

void vpt_clear_error(void) { g_err.clear(); }

/* what is said of the first bad voxel of an emission grid */
int vpt_int_emission_bad(double value, size_t voxel, const char* who)
{
    return vpt_fail(VPT_E_INVALID, "%s: emission value %g at voxel %zu (finite and >= 0)", who, value, voxel);
}

/* an emission grid and its colour (rgb may be NULL: the voxels only) */
int vpt_int_emission_check(const float* eps, size_t nv, const double rgb[3], const char* who)
{
    if (rgb)
        for (int c = 0; c < 3; ++c)
            if (!(rgb[c] >= 0.0 && rgb[c] - rgb[c] == 0.0))
                return vpt_fail(VPT_E_INVALID, "%s: rgb[%d] = %g (finite and >= 0)", who, c, rgb[c]);
    for (size_t i = 0; i < nv; ++i)
        if (!(eps[i] >= 0.0f && eps[i] - eps[i] == 0.0f))
            return vpt_int_emission_bad((double)eps[i], i, who);
    return VPT_OK;
}

/* vpt_grid_bad (csrc/vpt_grid.h) as a status with its message */
int vpt_int_grid_check(const vpt_grid_desc* desc, const float* density, const char* who)
{
    if (!desc || !density) return vpt_fail(VPT_E_INVALID, "%s: NULL grid", who);
    const int32_t n[3] = {desc->nx, desc->ny, desc->nz};
    return vpt_int_grid_verdict(desc, vpt_grid_bad(n, desc->lo, desc->hi, density), who);
}

/* a verdict of vpt_grid_bad on desc's grid as a status with its message */
int vpt_int_grid_verdict(const vpt_grid_desc* desc, int verdict, const char* who)
{
    switch (verdict) {
    case 1: return vpt_fail(VPT_E_INVALID, "%s: grid %d x %d x %d (each dimension >= 1, at most 2^27 voxels)", who,
                            desc->nx, desc->ny, desc->nz);
    case 2: return vpt_fail(VPT_E_INVALID, "%s: the box must be finite with hi > lo", who);
    case 3: return vpt_fail(VPT_E_INVALID, "%s: densities must be finite and >= 0", who);
    }
    return VPT_OK;
}

/* The pool kernel's camera table (PoolParams::cam_oc): oc = o - centre and |oc|^2 of n spheres whose centres
 * are `stride` doubles apart, with the operations and the order of Sphere::intersect (include/Sphere.h:28-30;
 * scene_intersect_grouped's first loop, march_origin_init on the device).  This unit is compiled with
 * -ffp-contract=off: every product and sum below is rounded on its own, as on the device. */
void vpt_int_cam_table(const double* o, const double* centre, size_t stride, int n, double (*oc)[4])
{
    for (int i = 0; i < n; ++i, centre += stride) {
        const double ocx = o[0] - centre[0], ocy = o[1] - centre[1], ocz = o[2] - centre[2];
        oc[i][0] = ocx;
        oc[i][1] = ocy;
        oc[i][2] = ocz;
        oc[i][3] = ocx * ocx + ocy * ocy + ocz * ocz;
    }
}

extern "C" {

/* debug: vpt_int_cam_table for a scene's spheres and a camera origin; out holds 4 n doubles */
int vpt_debug_cam_table(const vpt_sphere* spheres, int n, const double* o, double* out)
{
    if (!spheres || !o || !out || n < 0 || n > VPT_MAX_SPHERES) return vpt_fail(VPT_E_INVALID, "vpt_debug_cam_table: bad arguments");
    vpt_int_cam_table(o, spheres[0].p, sizeof(vpt_sphere) / sizeof(double), n, (double (*)[4])out);
    return VPT_OK;
}

const char* vpt_last_error(void) { return g_err.c_str(); }
int vpt_abi_version(void) { return VPT_ABI_VERSION; }

uint64_t vpt_stream_state(uint64_t seed, uint64_t pixel_idx, uint64_t sample)
{
    return vpt_stream_start(seed, pixel_idx, sample);
}

void vpt_default_params(vpt_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->width = 1024;
    p->height = 768;
    p->spp = 16;
    p->fb_format = VPT_FB_F32;
    p->medium.sigma_a = 0.001;
    p->medium.sigma_s = 0.009;
    p->medium.hg_g = 0.0;
    p->medium.max_depth = 0;
    p->medium.estimator = VPT_FREE_FLIGHT;
    p->medium.march_step = 0.1;  /* rayMarching3's step and light at src/rt.cpp:791 */
    p->medium.march_light = 7;
    p->seed = 0x5EED0001ull;
    /* Ray camera(Point(0, 11.2, 214), Vector(0, -0.042612, -1).normalize()) */
    double dx = 0, dy = -0.042612, dz = -1;
    double inv = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
    p->camera.o[0] = 0; p->camera.o[1] = 11.2; p->camera.o[2] = 214;
    p->camera.d[0] = dx * inv; p->camera.d[1] = dy * inv; p->camera.d[2] = dz * inv;
    p->fov_scale = 0.5095;
    p->band_rows = p->height;
    p->band_stride = 1;
    p->band_offset = 0;
}

static void set_sphere(vpt_sphere* s, double r, double px, double py, double pz, double cr, double cg, double cb,
                       double lr, double lg, double lb, int mat, const double* eta, const double* kappa, double alpha)
{
    memset(s, 0, sizeof *s);
    s->r = r;
    s->p[0] = px; s->p[1] = py; s->p[2] = pz;
    s->c[0] = cr; s->c[1] = cg; s->c[2] = cb;
    s->radiance[0] = lr; s->radiance[1] = lg; s->radiance[2] = lb;
    s->material = mat;
    if (eta) memcpy(s->eta, eta, sizeof s->eta);
    if (kappa) memcpy(s->kappa, kappa, sizeof s->kappa);
    s->alpha = alpha;
}

int vpt_default_scene(vpt_sphere* out, int cap)
{
    vpt_sphere s[10];
    static const double al_eta[3] = {1.66058, 0.88143, 0.521467};   /* aluminium */
    static const double al_kappa[3] = {9.2282, 6.27077, 4.83803};
    set_sphere(&s[0], 1e5, -1e5 - 49, 0, 0, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0);            /* left wall */
    set_sphere(&s[1], 1e5, 1e5 + 49, 0, 0, .0, .0, .5, 0, 0, 0, 0, 0, 0, 0);             /* right wall */
    set_sphere(&s[2], 1e5, 0, 0, -1e5 - 81.6, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0);          /* back wall */
    set_sphere(&s[3], 1e5, 0, -1e5 - 40.8, 0, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0);          /* floor */
    set_sphere(&s[4], 1e5, 0, 1e5 + 40.8, 0, .5, .5, .5, 0, 0, 0, 0, 0, 0, 0);           /* ceiling */
    set_sphere(&s[5], 16.5, -23, -24.3, -34.6, 0, 0, 0, 0, 0, 0, 1, al_eta, al_kappa, 0.09); /* metal */
    set_sphere(&s[6], 16.5, 23, -24.3, -3.6, .0, .0, .9, 0, 0, 0, 0, 0, 0, 0);           /* blue */
    set_sphere(&s[7], 2, 0, 24.3, -35, 0, 0, 0, 100, 100, 0, 0, 0, 0, 0);                /* light */
    set_sphere(&s[8], 0, -23, 24.3, 0, 0, 0, 0, 6000, 0, 0, 0, 0, 0, 0);                 /* point light */
    set_sphere(&s[9], 2, 23, 24.3, 35, 0, 0, 0, 75, 75, 60, 0, 0, 0, 0);                 /* light */
    if (out) {
        int n = cap < 10 ? cap : 10;
        if (n > 0) memcpy(out, s, sizeof(vpt_sphere) * (size_t)n);
    }
    return 10;
}

int vpt_shard_rows(const vpt_params* p)
{
    if (!p || p->height <= 0 || p->band_rows <= 0 || p->band_stride <= 0 || p->band_offset < 0 ||
        p->band_offset >= p->band_stride)
        return 0;
    int nb = (p->height + p->band_rows - 1) / p->band_rows;
    int rows = 0;
    for (int b = p->band_offset; b < nb; b += p->band_stride) {
        int r0 = b * p->band_rows;
        int r1 = r0 + p->band_rows;
        if (r1 > p->height) r1 = p->height;
        rows += r1 - r0;
    }
    return rows;
}

/* ---- the accumulator's statistic and policy on host arrays (csrc/vpt_accum.h) ---- */
int vpt_accum_stat_host(const double* csum, int m, int64_t npix, int chunk, double lum_floor, double* sum, double* s12,
                        double* err)
{
    vpt_clear_error();
    if (!csum || m < 0 || npix < 0 || chunk <= 0) return vpt_fail(VPT_E_INVALID, "vpt_accum_stat_host: bad arguments");
    if (!(lum_floor >= 0 && lum_floor - lum_floor == 0.0))
        return vpt_fail(VPT_E_INVALID, "vpt_accum_stat_host: lum_floor must be finite and >= 0");
    const double cfloor = (double)chunk * lum_floor;
    for (int64_t p = 0; p < npix; ++p) {
        vpt_accum_px a = {{0.0, 0.0, 0.0}, 0.0, 0.0};
        for (int k = 0; k < m; ++k) {
            const double* c = csum + ((int64_t)k * npix + p) * 3;
            vpt_accum_level(&a, c[0], c[1], c[2]);
        }
        if (sum) memcpy(sum + 3 * p, a.sum, sizeof a.sum);
        if (s12) {
            s12[2 * p] = a.s1;
            s12[2 * p + 1] = a.s2;
        }
        if (err) err[p] = vpt_accum_err(a.s1, a.s2, m, cfloor);
    }
    return VPT_OK;
}

int vpt_accum_select_host(const int32_t* tile_levels, const double* tile_err, int n_tiles, const vpt_refine* r,
                          int max_levels, int32_t* active)
{
    vpt_clear_error();
    if (!tile_levels || !tile_err || !r || !active || n_tiles < 0 || max_levels < 0)
        return vpt_fail(VPT_E_INVALID, "vpt_accum_select_host: bad arguments");
    switch (vpt_accum_refine_bad(r->target, r->lum_floor, r->min_levels, r->levels_per_pass)) {
    case 1: return vpt_fail(VPT_E_INVALID, "vpt_accum_select_host: target and lum_floor must be finite and >= 0");
    case 2: return vpt_fail(VPT_E_INVALID, "vpt_accum_select_host: min_levels must be >= 2");
    case 3: return vpt_fail(VPT_E_INVALID, "vpt_accum_select_host: levels_per_pass must be > 0");
    }
    int k = 0;
    for (int t = 0; t < n_tiles; ++t)
        if (vpt_accum_active(tile_levels[t], tile_err[t], r->min_levels, max_levels, r->target)) active[k++] = t;
    return k;
}

/* ---- the density grid's walkers on host arrays (csrc/vpt_grid.h) ---- */
/* the host probes' grid: the view, with its majorant grid (in `maj`) where block >= 1 */
static void probe_view(vpt_grid_view* G, std::vector<float>& maj, const vpt_grid_desc* desc, const float* density, int block,
                       int interp)
{
    const int32_t dims[3] = {desc->nx, desc->ny, desc->nz};
    vpt_grid_view_init(G, dims, desc->lo, desc->hi, density, density);
    G->interp = interp;
    if (block) {
        int32_t nb[3];
        vpt_grid_majorant_counts(dims, block, nb);
        maj.resize((size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2]);
        if (interp) vpt_grid_majorant_build_tl(dims, block, density, maj.data());
        else vpt_grid_majorant_build(dims, block, density, maj.data());
        vpt_grid_view_set_majorant(G, block, maj.data());
    }
}

/* the host probes' refusals of a majorant block below min_block (0, or the residual probe's 1: its control grid is per
 * super-voxel) and of an interpolation mode that does not exist */
static int probe_block_interp_check(const char* who, int block, int min_block, int interp)
{
    if (block < min_block)
        return min_block ? vpt_fail(VPT_E_INVALID, "%s: block %d (>= 1: the control grid is per super-voxel)", who, block)
                         : vpt_fail(VPT_E_INVALID, "%s: block %d (0 = the global majorant, else >= 1)", who, block);
    if (interp != VPT_GRID_NEAREST && interp != VPT_GRID_TRILINEAR)
        return vpt_fail(VPT_E_INVALID, "%s: interp %d (0 = nearest, 1 = trilinear)", who, interp);
    return VPT_OK;
}

/* the per-channel coefficients of the chromatic probes: finite, >= 0, and an extinction st[k] = sa[k] + ss[k] > 0 */
static int probe_channels_check(const char* who, const double sa[3], const double ss[3], double st[3])
{
    for (int k = 0; k < 3; ++k) {
        if (!(sa[k] >= 0.0 && sa[k] - sa[k] == 0.0 && ss[k] >= 0.0 && ss[k] - ss[k] == 0.0))  /* a NaN fails both */
            return vpt_fail(VPT_E_INVALID, "%s: channel %d: sa %g, ss %g (finite, >= 0)", who, k, sa[k], ss[k]);
        st[k] = sa[k] + ss[k];
        if (!(st[k] > 0.0)) return vpt_fail(VPT_E_INVALID, "%s: channel %d has no extinction", who, k);
    }
    return VPT_OK;
}

static int grid_probe_host(const char* who, const vpt_grid_desc* desc, const float* density, int block, int interp,
                           double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* tau,
                           double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    vpt_clear_error();
    if (!rays || !tmax || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        uint32_t ns = 0;
        if (tau) tau[i] = interp ? vpt_grid_tau_tl(&G, rays[i].o, rays[i].d, tmax[i]) : vpt_grid_tau(&G, rays[i].o, rays[i].d, tmax[i]);
        const double tc = block ? vpt_grid_track_lm_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns)
                                : vpt_grid_track_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns);
        if (t_coll) t_coll[i] = tc;
        if (states_out) states_out[i] = X;
        if (steps) steps[i] = ns;
    }
    return VPT_OK;
}

int vpt_grid_emission_probe_host(const vpt_grid_desc* desc, const float* density, const float* eps, int block, int interp,
                                 double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states, int n,
                                 double* t_coll, double* esum, uint64_t* states_out, uint32_t* steps)
{
    const char* who = "vpt_grid_emission_probe_host";
    vpt_clear_error();
    if (!rays || !tmax || !states || !eps || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    rc = vpt_int_emission_check(eps, (size_t)desc->nx * (size_t)desc->ny * (size_t)desc->nz, nullptr, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    G.emit = eps;
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        uint32_t ns = 0;
        double es = 0.0;
        const double tc = block ? vpt_grid_track_lm_em_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns, &es)
                                : vpt_grid_track_em_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns, &es);
        if (t_coll) t_coll[i] = tc;
        if (esum) esum[i] = es;
        if (states_out) states_out[i] = X;
        if (steps) steps[i] = ns;
    }
    return VPT_OK;
}

static int grid_ratio_probe_host(const char* who, const vpt_grid_desc* desc, const float* density, int block, int interp,
                                 double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states, int n,
                                 double* that, uint64_t* states_out, uint32_t* steps)
{
    vpt_clear_error();
    if (!rays || !tmax || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        uint32_t ns = 0;
        const double T = block ? vpt_grid_ratio_lm_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns)
                               : vpt_grid_ratio_m(&G, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns);
        if (that) that[i] = T;
        if (states_out) states_out[i] = X;
        if (steps) steps[i] = ns;
    }
    return VPT_OK;
}

int vpt_grid_residual_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                                 const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                                 double* tauc, uint64_t* states_out, uint32_t* steps)
{
    const char* who = "vpt_grid_residual_probe_host";
    vpt_clear_error();
    if (!rays || !tmax || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 1, interp);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    /* the view with the majorant allocation as the context keeps it: the maxima, and behind them the minima */
    const int32_t dims[3] = {desc->nx, desc->ny, desc->nz};
    vpt_grid_view G;
    vpt_grid_view_init(&G, dims, desc->lo, desc->hi, density, density);
    G.interp = interp;
    int32_t nb[3];
    vpt_grid_majorant_counts(dims, block, nb);
    std::vector<float> maj(2 * (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2]);
    vpt_grid_majorant_control_build(dims, block, interp, density, maj.data());
    vpt_grid_view_set_majorant(&G, block, maj.data());
    const float* ctl = vpt_grid_control_of(&G);
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        uint32_t ns = 0;
        double tc = 0.0;
        const double T = vpt_grid_residual_lm_m(&G, ctl, interp, rays[i].o, rays[i].d, tmax[i], sigma_t, &X, &ns, &tc);
        if (that) that[i] = T;
        if (tauc) tauc[i] = tc;
        if (states_out) states_out[i] = X;
        if (steps) steps[i] = ns;
    }
    return VPT_OK;
}

/* how the two probes of the majorant build open: the dimensions and the box are checked, the voxels are not (the builds
 * are compared on every input) */
static int majorant_probe_open(const char* who, const vpt_grid_desc* desc, const float* density, int block, int interp,
                               const float* out, const double* rho_max)
{
    vpt_clear_error();
    if (!desc || !density) return vpt_fail(VPT_E_INVALID, "%s: NULL grid", who);
    if (!out || !rho_max) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 1, interp);
    if (rc) return rc;
    const int32_t n[3] = {desc->nx, desc->ny, desc->nz};
    return vpt_int_grid_verdict(desc, vpt_grid_bad(n, desc->lo, desc->hi, nullptr), who);
}

int vpt_grid_majorant_scatter_host(const vpt_grid_desc* desc, const float* density, int block, int interp, float* out,
                                   double* rho_max)
{
    if (int rc = majorant_probe_open("vpt_grid_majorant_scatter_host", desc, density, block, interp, out, rho_max)) return rc;
    const int32_t n[3] = {desc->nx, desc->ny, desc->nz};
    vpt_grid_view G;
    vpt_grid_view_init(&G, n, desc->lo, desc->hi, density, density);
    *rho_max = G.rho_max;
    vpt_grid_majorant_control_build(n, block, interp, density, out);
    return VPT_OK;
}

int vpt_grid_majorant_gather_host(const vpt_grid_desc* desc, const float* density, int block, int interp, float* out,
                                  double* rho_max)
{
    if (int rc = majorant_probe_open("vpt_grid_majorant_gather_host", desc, density, block, interp, out, rho_max)) return rc;
    const int32_t n[3] = {desc->nx, desc->ny, desc->nz};
    int32_t nb[3];
    vpt_grid_majorant_counts(n, block, nb);
    const size_t nbv = (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2], nsx = (size_t)n[2] * (size_t)n[1] * (size_t)nb[0];
    std::vector<float> sx(2 * nsx);
    float* sxmax = sx.data();
    float* sxmin = sxmax + nsx;
    vpt_gb_acc A, R;
    vpt_gb_acc_init(&R);  /* rho_max: the maximum of the rows' maxima under the build's rule */
    for (int64_t r = 0; r < (int64_t)n[2] * n[1]; ++r) {  /* pass X */
        vpt_gb_scan_x(density + r * n[0], 0, n[0] - 1, 0, 1, &A);
        vpt_gb_acc_step(&R, A.mx, A.mn, r);
        for (int32_t bx = 0; bx < nb[0]; ++bx) {
            int32_t x0, x1;
            vpt_gb_range(n[0], block, interp, bx, &x0, &x1);
            vpt_gb_scan_x(density + r * n[0], x0, x1, 0, 1, &A);
            sxmax[r * nb[0] + bx] = A.mx;
            sxmin[r * nb[0] + bx] = A.mn;
        }
    }
    *rho_max = (double)R.mx;
    for (int32_t bz = 0; bz < nb[2]; ++bz)  /* pass YZ */
        for (int32_t by = 0; by < nb[1]; ++by)
            for (int32_t bx = 0; bx < nb[0]; ++bx) {
                int32_t z0, z1, y0, y1;
                vpt_gb_range(n[2], block, interp, bz, &z0, &z1);
                vpt_gb_range(n[1], block, interp, by, &y0, &y1);
                vpt_gb_scan_yz(sxmax, sxmin, n[1], nb[0], bx, z0, z1, y0, y1, 0, 1, &A);
                const size_t o = ((size_t)bz * (size_t)nb[1] + (size_t)by) * (size_t)nb[0] + (size_t)bx;
                out[o] = A.mx;
                out[nbv + o] = A.mn;
            }
    return VPT_OK;
}

int vpt_grid_probe_host(const vpt_grid_desc* desc, const float* density, double sigma_t, const vpt_ray* rays,
                        const double* tmax, const uint64_t* states, int n, double* tau, double* t_coll,
                        uint64_t* states_out)
{
    return grid_probe_host("vpt_grid_probe_host", desc, density, 0, 0, sigma_t, rays, tmax, states, n, tau, t_coll, states_out,
                           nullptr);
}

int vpt_grid_probe_host_lm(const vpt_grid_desc* desc, const float* density, int block, double sigma_t, const vpt_ray* rays,
                           const double* tmax, const uint64_t* states, int n, double* tau, double* t_coll,
                           uint64_t* states_out, uint32_t* steps)
{
    return grid_probe_host("vpt_grid_probe_host_lm", desc, density, block, 0, sigma_t, rays, tmax, states, n, tau, t_coll,
                           states_out, steps);
}

int vpt_grid_probe_host_ex(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                           const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* tau,
                           double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    return grid_probe_host("vpt_grid_probe_host_ex", desc, density, block, interp, sigma_t, rays, tmax, states, n, tau, t_coll,
                           states_out, steps);
}

int vpt_grid_ratio_probe_host(const vpt_grid_desc* desc, const float* density, int block, double sigma_t,
                              const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                              uint64_t* states_out, uint32_t* steps)
{
    return grid_ratio_probe_host("vpt_grid_ratio_probe_host", desc, density, block, 0, sigma_t, rays, tmax, states, n, that,
                                 states_out, steps);
}

int vpt_grid_ratio_probe_host_ex(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                                 const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                                 uint64_t* states_out, uint32_t* steps)
{
    return grid_ratio_probe_host("vpt_grid_ratio_probe_host_ex", desc, density, block, interp, sigma_t, rays, tmax, states, n,
                                 that, states_out, steps);
}

int vpt_grid_eqa_probe_host(const vpt_grid_desc* desc, const float* density, int interp, double sigma_t, const vpt_ray* rays,
                            const double* tmax, const double* light, const uint64_t* states, int n, double* psurf, double* dist,
                            double* pdf, double* T, double* rho_t, uint64_t* states_out)
{
    const char* who = "vpt_grid_eqa_probe_host";
    vpt_clear_error();
    if (!rays || !tmax || !light || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, 0, 0, interp);  /* no block: nothing tracks */
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, 0, interp);
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        double ps, ds, pf, tr, rt;
        vpt_grid_eqa_one(&G, interp, sigma_t, rays[i].o, rays[i].d, tmax[i], light + 3 * (size_t)i, &X, &ps, &ds, &pf, &tr, &rt);
        if (psurf) psurf[i] = ps;
        if (dist) dist[i] = ds;
        if (pdf) pdf[i] = pf;
        if (T) T[i] = tr;
        if (rho_t) rho_t[i] = rt;
        if (states_out) states_out[i] = X;
    }
    return VPT_OK;
}

int vpt_grid_mis_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t, double q,
                            const vpt_ray* rays, const double* tmax, const double* light, const uint64_t* states, int n,
                            double* psurf, int32_t* strategy, double* dist, double* pdf, double* pe, double* T, double* rho_t,
                            uint32_t* steps, uint64_t* states_out)
{
    const char* who = "vpt_grid_mis_probe_host";
    vpt_clear_error();
    if (!rays || !tmax || !light || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    if (rc) return rc;
    if (!(q >= 0.0 && q <= 1.0)) return vpt_fail(VPT_E_INVALID, "%s: q %g (finite, in [0, 1])", who, q);
    rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        double ps, ds, pf, pq, tr, rt;
        int sg = 0;
        uint32_t ns = 0;
        vpt_grid_mis_one(&G, interp, block != 0, sigma_t, q, rays[i].o, rays[i].d, tmax[i], light + 3 * (size_t)i, &X, &ps, &sg,
                         &ds, &pf, &pq, &tr, &rt, &ns);
        if (psurf) psurf[i] = ps;
        if (strategy) strategy[i] = sg;
        if (dist) dist[i] = ds;
        if (pdf) pdf[i] = pf;
        if (pe) pe[i] = pq;
        if (T) T[i] = tr;
        if (rho_t) rho_t[i] = rt;
        if (steps) steps[i] = ns;
        if (states_out) states_out[i] = X;
    }
    return VPT_OK;
}

int vpt_grid_chroma_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, const double sa[3],
                               const double ss[3], const vpt_ray* rays, const double* tmax, const uint64_t* states, int n,
                               int32_t* hero, double* t_coll, double* tau, double* w, uint32_t* steps, uint64_t* states_out)
{
    const char* who = "vpt_grid_chroma_probe_host";
    vpt_clear_error();
    if (!sa || !ss || !rays || !tmax || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    double st[3];
    if (!rc) rc = probe_channels_check(who, sa, ss, st);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    const size_t nn = (size_t)n;
    for (int i = 0; i < n; ++i) {
        uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
        double tc, ta, wk[3];
        int h = 0;
        uint32_t ns = 0;
        vpt_grid_chroma_one(&G, interp, block != 0, ss, st, rays[i].o, rays[i].d, tmax[i], &X, &h, &tc, &ta, wk, &ns);
        if (hero) hero[i] = h;
        if (t_coll) t_coll[i] = tc;
        if (tau) tau[i] = ta;
        if (w)
            for (int k = 0; k < 3; ++k) w[(size_t)k * nn + i] = wk[k];
        if (steps) steps[i] = ns;
        if (states_out) states_out[i] = X;
    }
    return VPT_OK;
}

int vpt_grid_spectral_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, const double sa[3],
                                 const double ss[3], const vpt_ray* rays, const double* tmax, const double* beta,
                                 const uint64_t* states, int n, double* t_coll, double* w, uint32_t* steps,
                                 uint64_t* states_out, double* T, uint32_t* ratio_steps, uint64_t* ratio_states_out)
{
    const char* who = "vpt_grid_spectral_probe_host";
    vpt_clear_error();
    if (!sa || !ss || !rays || !tmax || !states || n < 0) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    int rc = probe_block_interp_check(who, block, 0, interp);
    double st[3];
    if (!rc) rc = probe_channels_check(who, sa, ss, st);
    if (!rc) rc = vpt_int_grid_check(desc, density, who);
    if (rc) return rc;
    vpt_grid_view G;
    std::vector<float> maj;
    probe_view(&G, maj, desc, density, block, interp);
    const vpt_spectral_consts kc = vpt_grid_spectral_consts(ss, st);
    const double ones[3] = {1.0, 1.0, 1.0};
    const size_t nn = (size_t)n;
    for (int i = 0; i < n; ++i) {
        double tc, wk[3], Tk[3];
        uint32_t ns = 0, nr = 0;
        uint64_t Xt = 0, Xr = 0;
        vpt_grid_spectral_one(&G, interp, block != 0, &kc, beta ? beta + 3 * (size_t)i : ones, rays[i].o, rays[i].d, tmax[i],
                              states[i] & 0xFFFFFFFFFFFFull, &tc, wk, &ns, &Xt, Tk, &nr, &Xr);
        if (t_coll) t_coll[i] = tc;
        if (w)
            for (int k = 0; k < 3; ++k) w[(size_t)k * nn + i] = wk[k];
        if (steps) steps[i] = ns;
        if (states_out) states_out[i] = Xt;
        if (T)
            for (int k = 0; k < 3; ++k) T[(size_t)k * nn + i] = Tk[k];
        if (ratio_steps) ratio_steps[i] = nr;
        if (ratio_states_out) ratio_states_out[i] = Xr;
    }
    return VPT_OK;
}

/* ---- PPM ---- */
static inline double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
static inline int to_display(double x) { return (int)(pow(clamp01(x), 1.0 / 2.2) * 255 + .5); }

static inline char* put_int(char* p, int v)
{
    /* "%d" for the values toDisplayValue can produce (0..255; NaN inputs give INT_MIN) */
    if (v >= 0 && v < 1000) {
        if (v >= 100) *p++ = (char)('0' + v / 100);
        if (v >= 10) *p++ = (char)('0' + (v / 10) % 10);
        *p++ = (char)('0' + v % 10);
        return p;
    }
    return p + sprintf(p, "%d", v);
}

int64_t vpt_encode_ppm(const void* rgb, int fb_format, int w, int h, char* buf, int64_t cap)
{
    vpt_clear_error();
    if (!rgb || w <= 0 || h <= 0 || (fb_format != VPT_FB_F32 && fb_format != VPT_FB_F64))
        return vpt_fail(VPT_E_INVALID, "vpt_encode_ppm: bad arguments");
    const int64_t npix = (int64_t)w * h;
    char header[64];
    int hl = snprintf(header, sizeof header, "P3\n%d %d\n%d\n", w, h, 255);
    unsigned hc = std::thread::hardware_concurrency();
    int nthreads = (int)(hc == 0 ? 1 : (hc > 16 ? 16 : hc));
    if (npix < 65536) nthreads = 1;
    const int64_t chunk = (npix + nthreads - 1) / nthreads;
    std::vector<std::vector<char>> parts((size_t)nthreads);
    std::vector<int64_t> lens((size_t)nthreads, 0);
    auto work = [&](int t) {
        int64_t p0 = t * chunk, p1 = p0 + chunk < npix ? p0 + chunk : npix;
        if (p0 >= p1) return;
        std::vector<char>& v = parts[(size_t)t];
        v.resize((size_t)(p1 - p0) * 3 * 12);
        char* q = v.data();
        for (int64_t p = p0; p < p1; ++p) {
            for (int c = 0; c < 3; ++c) {
                double x = fb_format == VPT_FB_F32 ? (double)((const float*)rgb)[3 * p + c]
                                                   : ((const double*)rgb)[3 * p + c];
                q = put_int(q, to_display(clamp01(x)));
                *q++ = ' ';
            }
        }
        lens[(size_t)t] = q - v.data();
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    int64_t total = hl;
    for (int t = 0; t < nthreads; ++t) total += lens[(size_t)t];
    if (!buf) return total;
    if (cap < total) return vpt_fail(VPT_E_INVALID, "vpt_encode_ppm: buffer too small (%lld < %lld)", (long long)cap,
                                     (long long)total);
    memcpy(buf, header, (size_t)hl);
    int64_t off = hl;
    for (int t = 0; t < nthreads; ++t) {
        if (lens[(size_t)t]) memcpy(buf + off, parts[(size_t)t].data(), (size_t)lens[(size_t)t]);
        off += lens[(size_t)t];
    }
    return total;
}

int vpt_write_ppm(const char* path, const void* rgb, int fb_format, int w, int h)
{
    int64_t n = vpt_encode_ppm(rgb, fb_format, w, h, NULL, 0);
    if (n < 0) return (int)n;
    std::vector<char> buf((size_t)n);
    if (vpt_encode_ppm(rgb, fb_format, w, h, buf.data(), n) != n) return VPT_E_INVALID;
    FILE* f = path ? fopen(path, "w") : NULL;
    if (!f) return vpt_fail(VPT_E_IO, "vpt_write_ppm: cannot open '%s'", path ? path : "(null)");
    size_t wr = fwrite(buf.data(), 1, (size_t)n, f);
    int rc = fclose(f);
    if (wr != (size_t)n || rc != 0) return vpt_fail(VPT_E_IO, "vpt_write_ppm: short write to '%s'", path);
    return VPT_OK;
}

}  // extern "C"
