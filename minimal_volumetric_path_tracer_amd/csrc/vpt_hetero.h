/*
 * vpt_hetero.h -- estimator 10 (VPT_HETERO_FREE): the control flow of iterativeVPTracerFree (estimator 0,
 * include/vptShadeMethods.h:1263-1340) in a heterogeneous medium, the density grid of vpt_grid.h.  An
 * extension: the reference has no counterpart.  Draw for draw estimator 0, with two substitutions:
 *   - freeFlightSample becomes delta tracking: a collision is a medium event at t; "none" with a hit is a
 *     surface event; "none" without a hit ends the path with no contribution (the ray left into vacuum);
 *   - every transmittance factor estimator 0 reaches becomes the grid's over the same segment: Trs to the
 *     picked light's centre, MISv2's per-light factor, the point-light factor of freeSingleScattering and the
 *     factor over tdist along the sampled cone direction (the TP policy of vpt_device.h's helpers).
 * Material-3 spheres keep their multipleT treatment; hg_g and max_depth act as in estimator 0.
 * No branch of estimator 0 depends on a transmittance value, so on a uniform rho == 1 grid that contains
 * every path this estimator walks estimator 0's paths with the same draws and differs only in the rounding
 * of tau (tests/test_gpu_hetero.py).  The steps are the generic (MK = -1, LT = -1) statements of
 * decide / surface_event / medium_event<0>: the tuned instantiations of the pool kernel are not touched.
 * Local majorants (vpt_grid.h, vpt_set_grid_majorant_block): where the grid has a majorant grid the track is
 * vpt_grid_track_lm, else vpt_grid_track.  The choice is the template parameter LM of hetero_decide,
 * trace_hetero and every kernel of estimator 10, made on the host at launch from the context's view, so the
 * LM = false instantiations are the kernels as they were before local majorants existed.
 * Trilinear interpolation (vpt_grid.h, vpt_set_grid_interpolation): the template parameter TL beside LM, chosen on the
 * host in the same way from the view's interp word; the walkers and the optical depth take it as a constant, so
 * there is no test of the mode in a loop.  The TL = true kernels are instantiated in vpt_hetero_tl.hip, a code object
 * of their own, and the TL = false ones stay in vpt_hetero.hip as they were.
 * Emission (vpt_grid.h, vpt_set_emission_grid): the template parameter EM, chosen on the host where the context holds an
 * emission grid.  hetero_decide's track becomes the emitting one, and after the track, before its result is classified,
 *   p.L = p.L + (rgb * p.beta) * (((sigma_a / sigma_t) * esum) * (1 / continueprob))
 * in exactly this order, at every depth (the medium has no next-event estimation, so a collision at any depth sees it;
 * continueprob = 0.6 is the roulette's factor, which precedes decide at every depth).  sigma_a / sigma_t turns
 * E[esum] = sigma_t int T rho eps into the source term's integral sigma_a int T rho eps.  Emission takes no draw and
 * changes no branch: paths, draw counts and end states are those of EM = false.  A camera ray that ends on a light adds
 * the light's radiance to p.L, so the emission scored on that segment survives.  The colour travels with the emission
 * grid: the four doubles in front of the voxels (rgb and a pad word; VPT_EMIT_HEAD below).  The EM = true kernels are
 * instantiated in vpt_hetero_em.hip and vpt_hetero_em_tl.hip; the EM = false kernels copy and keep the fields in front of
 * `emit` (vpt_grid_fields, which every walker but the emitting ones takes), so they load and hold what they did before.
 */
#ifndef VPT_HETERO_H
#define VPT_HETERO_H

#include <stddef.h>

#include <type_traits>

#include "vpt_device.h"

#define VPT_GRID_EXP lm_exp
#define VPT_GRID_LOG lm_log
#include "vpt_grid.h"

namespace vpt {

/* the emission grid on the device: VPT_EMIT_HEAD doubles -- rgb, then a pad word -- and behind them the voxels that
 * vpt_grid_view.emit points to */
#define VPT_EMIT_HEAD 4

/* what a policy with an emission grid holds beside the view: the colour, read once from in front of the voxels */
struct GridColour {
    dv3 rgb;
};
struct GridNoColour {};

/* the grid's transmittance as the TP policy of mis_v2 / single_scattering (vpt_device.h TrHom); TL: the trilinear
 * field (GridTr is the nearest one).  EM: with the emission grid -- the policy then holds the whole view and the colour;
 * without it the fields alone (vpt_grid.h vpt_grid_fields), the object these kernels held before the view had `emit` */
template <bool TL, bool EM = false>
struct GridTrT : std::conditional_t<EM, GridColour, GridNoColour> {
    static constexpr bool hom = false;
    static constexpr bool draws = false;
    std::conditional_t<EM, vpt_grid_view, vpt_grid_fields> G;
    /* the context's view from device memory.  Without local majorants only the fields the global-majorant
     * walkers read are copied (everything before `maj`): block, nb and maj stay unset and nothing reads them, so
     * the LM = false kernels load what they loaded before local majorants existed */
    template <bool LM>
    __device__ __forceinline__ static GridTrT load(const vpt_grid_view* __restrict__ g)
    {
        GridTrT tp;
        if (LM || EM) tp.G = *g;
        else __builtin_memcpy(&tp.G, g, offsetof(vpt_grid_fields, maj));
        if constexpr (EM) {
            const double* c = (const double*)tp.G.emit - VPT_EMIT_HEAD;
            tp.rgb = mk(c[0], c[1], c[2]);
        }
        return tp;
    }
    __device__ __forceinline__ double along(dv3 o, dv3 d, double dist, double sigma_t) const
    {
        const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
        return TL ? vpt_grid_transmittance_tl(&G, oo, dd, dist, sigma_t) : vpt_grid_transmittance(&G, oo, dd, dist, sigma_t);
    }
    /* a to b: the distance and the unit direction formed as transmitance() and nrm() form them */
    __device__ __forceinline__ double between(dv3 a, dv3 b, double sigma_t) const
    {
        const dv3 aux = sub(b, a);
        const double dist = vm_sqrt(dot(aux, aux));
        if (!(dist > 0)) return lm_exp(sigma_t * 0.0 * -1.0);
        return along(a, nrm(aux), dist, sigma_t);
    }
};
using GridTr = GridTrT<false>;

/* estimator 11's policy: every factor is a ratio-tracking estimate (vpt_grid.h) over the same segment, drawn from
 * the sample's own stream where GridTr evaluates the factor -- a policy with draws == true takes the sampler first.
 * A zero-length segment is 1.0 without a draw, as vpt_grid_tau's is exp(-0).  LM: the grid has a majorant grid; TL: the
 * trilinear field; EM: with the emission grid, as in GridTrT (the shadow rays stay transmittance only). */
template <bool LM, bool TL = false, bool EM = false>
struct GridRatioTr : std::conditional_t<EM, GridColour, GridNoColour> {
    static constexpr bool hom = false;
    static constexpr bool draws = true;
    std::conditional_t<EM, vpt_grid_view, vpt_grid_fields> G;
    template <bool LM_>
    __device__ __forceinline__ static GridRatioTr load(const vpt_grid_view* __restrict__ g)
    {
        static_assert(LM_ == LM, "the policy's LM is the kernel's");
        GridRatioTr tp;
        if (LM || EM) tp.G = *g;
        else __builtin_memcpy(&tp.G, g, offsetof(vpt_grid_fields, maj));
        if constexpr (EM) {
            const double* c = (const double*)tp.G.emit - VPT_EMIT_HEAD;
            tp.rgb = mk(c[0], c[1], c[2]);
        }
        return tp;
    }
    template <bool COUNT>
    __device__ __forceinline__ double along(Sampler<COUNT>& smp, dv3 o, dv3 d, double dist, double sigma_t) const
    {
        if (!(dist > 0)) return lm_exp(sigma_t * 0.0 * -1.0);
        const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
        return LM ? vpt_grid_ratio_lm_m(&G, TL, oo, dd, dist, sigma_t, &smp.X, (uint32_t*)nullptr)
                  : vpt_grid_ratio_m(&G, TL, oo, dd, dist, sigma_t, &smp.X, (uint32_t*)nullptr);
    }
    template <bool COUNT>
    __device__ __forceinline__ double between(Sampler<COUNT>& smp, dv3 a, dv3 b, double sigma_t) const
    {
        const dv3 aux = sub(b, a);
        const double dist = vm_sqrt(dot(aux, aux));
        if (!(dist > 0)) return lm_exp(sigma_t * 0.0 * -1.0);
        return along(smp, a, nrm(aux), dist, sigma_t);
    }
};

/* measurement only (vpt_debug_hetero_steps): delta-tracking calls and their tentative steps */
struct HeteroStats {
    unsigned long long tracks, steps;
};

/* decide<0> with delta tracking in freeFlightSample's place; EM: the emitting track and its contribution (header comment) */
template <bool COUNT, bool LM = false, bool TL = false, class TP = GridTrT<TL>, bool EM = false>
VPT_DEV int hetero_decide(const DevScene* __restrict__ S, const TP& tp, Sampler<COUNT>& smp, Path& p, Event& e,
                          const Medium& m, HeteroStats* hs = nullptr)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    int id = 0;
    double t = 0.0;
    const bool hit = scene_intersect_grouped<VPT_DECIDE_GROUP>(S, smp, p.o, p.d, t, id);
    if (!hit) t = VPT_MAXFLOAT;
    e.t = t;
    e.id = id;
    const int count = S->n_emit;
    if (VPT_UNLIKELY(count == 0)) return EV_END;
    e.src = emit_pick(S, (int)(smp.next() * count), count);
    const double oo[3] = {p.o.x, p.o.y, p.o.z}, dd[3] = {p.d.x, p.d.y, p.d.z};
    uint32_t nsteps = 0;
    double tc;
    if constexpr (EM) {
        const double continueprob = 0.6;
        double esum;
        tc = LM ? vpt_grid_track_lm_em_m(&tp.G, TL, oo, dd, t, sigma_t, &smp.X, hs ? &nsteps : (uint32_t*)nullptr, &esum)
                : vpt_grid_track_em_m(&tp.G, TL, oo, dd, t, sigma_t, &smp.X, hs ? &nsteps : (uint32_t*)nullptr, &esum);
        p.L = add(p.L, scl(mul(tp.rgb, p.beta), (((m.sigma_a / sigma_t) * esum) * (1 / continueprob))));
    } else {
        tc = LM ? vpt_grid_track_lm_m(&tp.G, TL, oo, dd, t, sigma_t, &smp.X, hs ? &nsteps : (uint32_t*)nullptr)
                : vpt_grid_track_m(&tp.G, TL, oo, dd, t, sigma_t, &smp.X, hs ? &nsteps : (uint32_t*)nullptr);
    }
    if (hs) {
        hs->tracks += 1;
        hs->steps += nsteps;
    }
    if (VPT_UNLIKELY(tc != tc)) {  /* the step cap: NaN, like trace_ray_marching's */
        p.L = mk(tc, tc, tc);
        return EV_END;
    }
    if (tc >= 0) {
        e.dist = tc;
        return EV_MED;
    }
    if (!hit) return EV_END;  /* left the medium into vacuum */
    if (sph_flag(S->m_emitter, id)) {  /* the path ends on a light; only a camera ray sees it */
        if (p.depth == 0) {
            if constexpr (EM) p.L = add(p.L, mul(sph_rad(S, id), p.beta));  /* the segment's emission stays */
            else p.L = mul(sph_rad(S, id), p.beta);
        }
        return EV_END;
    }
    return EV_SURF;
}

/* surface_event<0> (MK = -1, PT = -1) */
template <bool COUNT, class TP>
VPT_DEV void hetero_surface(const DevScene* __restrict__ S, const TP& tp, Sampler<COUNT>& smp, Path& p,
                            const Event& e, const Medium& m)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const int id = e.id, src = e.src;
    const dv3 xs = add(p.o, scl(p.d, e.t));
    const dv3 nx = nrm(sub(xs, sph_p(S, id)));
    const double probSource = 1.0 / S->n_emit;
    const double alpha = S->sph[id].alpha;
    double Trs;
    if constexpr (TP::draws) Trs = tp.between(smp, xs, sph_p(S, src), sigma_t);
    else Trs = tp.between(xs, sph_p(S, src), sigma_t);
    const dv3 Ldp = scl(scl(p_light<COUNT>(S, smp, id, xs, nx, p.d, src, alpha), Trs), (1 / probSource));
    const dv3 Ld = mis_v2<COUNT, -1, true, TP>(S, smp, id, xs, nx, p.d, alpha, sigma_t, tp);
    p.L = add(p.L, scl(mul(add(Ldp, Ld), p.beta), (1 / continueprob)));
    dv3 wi = mk(0, 0, 0);
    double pdf = 0;
    const dv3 fs = bdsf<COUNT>(S, smp, wi, p.d, nx, pdf, id);
    wi = nrm(wi);
    const double cosine = dot(nx, wi);
    p.beta = scl(scl(scl(mul(p.beta, fs), (1 / continueprob)), cosine), (1 / pdf));
    p.o = xs;
    p.d = wi;
    p.depth++;
}

/* medium_event<0> (LT = -1): freeSingleScattering toward the picked light, the phase continuation; the
 * local albedo rho sigma_s / (rho sigma_t) is medium_tail's sigma_s / sigma_t */
template <bool COUNT, class TP>
VPT_DEV void hetero_medium(const DevScene* __restrict__ S, const TP& tp, Sampler<COUNT>& smp, Path& p,
                           const Event& e, const Medium& m)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const double probSource = 1.0 / S->n_emit;
    const bool zero_ok = p.beta.x - p.beta.x == 0 && p.beta.y - p.beta.y == 0 && p.beta.z - p.beta.z == 0;
    const dv3 Ld = single_scattering<COUNT, -1, TP>(S, smp, xt, p.d, e.src, sigma_t, false, m.sigma_s, 1.0, probSource,
                                                        zero_ok, tp);
    medium_tail<0, COUNT>(smp, p, Ld, 1.0, e.pdf, xt, m, true);
}

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_hetero) */
template <bool COUNT, bool LM = false, bool TL = false, bool EM = false>
__device__ static dv3 trace_hetero(const DevScene* __restrict__ S, const GridTrT<TL, EM>& tp, Sampler<COUNT>& smp, dv3 o, dv3 d,
                                   const Medium& m, HeteroStats* hs = nullptr)
{
    Path p;
    p.o = o;
    p.d = d;
    p.beta = mk(1, 1, 1);
    p.L = mk(0, 0, 0);
    p.depth = 0;
    Event e;
    e.pdf = 0;
    while (continue_path(smp, p, m)) {
        const int ev = hetero_decide<COUNT, LM, TL, GridTrT<TL, EM>, EM>(S, tp, smp, p, e, m, hs);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_surface(S, tp, smp, p, e, m);
        else hetero_medium(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the same for estimator 11 (render_kernel_simple_ratio).  Restated, not a shared template: estimator 10's function
 * above is an out-of-line function of its kernels, and its name and code are to stay what they were */
template <bool COUNT, bool LM = false, bool TL = false, bool EM = false>
__device__ static dv3 trace_hetero(const DevScene* __restrict__ S, const GridRatioTr<LM, TL, EM>& tp, Sampler<COUNT>& smp, dv3 o,
                                   dv3 d, const Medium& m, HeteroStats* hs = nullptr)
{
    Path p;
    p.o = o;
    p.d = d;
    p.beta = mk(1, 1, 1);
    p.L = mk(0, 0, 0);
    p.depth = 0;
    Event e;
    e.pdf = 0;
    while (continue_path(smp, p, m)) {
        const int ev = hetero_decide<COUNT, LM, TL, GridRatioTr<LM, TL, EM>, EM>(S, tp, smp, p, e, m, hs);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_surface(S, tp, smp, p, e, m);
        else hetero_medium(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the three steps as the persistent-wave loop (vpt_wave.h) calls them, on the kernel's view of the grid */
template <bool LM, bool TL = false, class TP = GridTrT<TL>, bool EM = false>
struct HeteroSteps {
    TP tp;
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return hetero_decide<COUNT, LM, TL, TP, EM>(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void surface(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                            const Medium& m) const
    {
        hetero_surface(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void medium(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                           const Medium& m) const
    {
        hetero_medium(S, tp, smp, p, e, m);
    }
};

struct KParams;  /* a render's launch parameters (vpt_render_simple.h) */

/* estimator 14's and 16's per-channel coefficients per unit density, launch constants (vpt_hetero_chroma.h) */
struct ChromaCoef {
    double ss[3], st[3];
};

}  // namespace vpt

/* What the estimators' launches differ in on the host, in one argument: each launch reads what its estimator takes */
struct vpt_hetero_args {
    bool lm;                    /* the grid behind the view has a majorant grid (the kernel's LM instantiation);
                                 * estimator 12, where nothing tracks, ignores it */
    double q;                   /* estimator 13: the context's track fraction */
    vpt::ChromaCoef c;          /* estimators 14 and 16: the launch's coefficients */
    unsigned long long* stats;  /* estimator 10's per-sample call: vpt_debug_hetero_steps' two counters, else NULL */
};

/* What a code object of the density-grid estimators exports: its launches.  One table per unit -- vpt_hetero.hip's four
 * are the values of (TL, EM), nearest or trilinear lookup (the view's interp word) without or with the emission grid;
 * estimator 12's to 16's units the two values of TL -- and the caller picks the table in one place (vpt_kernels.hip
 * hetero_unit).  A probe the unit does not hold is NULL. */
struct vpt_hetero_unit {
    /* the persistent-wave render kernel of the unit's estimator (K.est where it holds two), enqueued on `stream` (the
     * caller owns the queue word K.queue and has zeroed it in stream order) */
    int (*launch)(int device, const vpt::KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream);
    /* the unit's one-lane-per-pixel kernel of K.est (render_kernel_simple_<unit>) for the same render; counting iff K.counters
     * (vpt_count_work's device counters) is set */
    int (*simple_launch)(const vpt::KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream);
    /* the per-sample call of estimator est and, below, the probes on device arrays, default stream (the caller reads
     * hipGetLastError); steps: a probe's per-ray tentative steps, else NULL; light: 3 doubles per ray */
    void (*trace_launch)(int est, const vpt_ray* rays, const uint64_t* states, int n, const vpt::Medium& m, const DevScene* S,
                         const vpt_grid_view* grid, const vpt_hetero_args& a, double* out, uint64_t* out_states);
    /* the two grid probes: vpt_hetero.hip's EM = false units' */
    void (*grid_probe_launch)(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays, const double* tmax,
                              const uint64_t* states, int n, double* tau, double* t_coll, uint64_t* states_out,
                              uint32_t* steps);
    void (*grid_ratio_probe_launch)(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays,
                                    const double* tmax, const uint64_t* states, int n, double* that, uint64_t* states_out,
                                    uint32_t* steps);
    /* the emitting track's probe: vpt_hetero.hip's EM = true units' */
    void (*grid_emission_probe_launch)(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays,
                                       const double* tmax, const uint64_t* states, int n, double* t_coll, double* esum,
                                       uint64_t* states_out, uint32_t* steps);
    /* estimator 12's */
    void (*grid_eqa_probe_launch)(const vpt_grid_view* grid, double sigma_t, const vpt_ray* rays, const double* tmax,
                                  const double* light, const uint64_t* states, int n, double* psurf, double* dist, double* pdf,
                                  double* T, double* rho_t, uint64_t* states_out);
    /* estimator 13's; res: six arrays of n doubles, one behind the other (psurf, dist, pdf, pe, T, rho_t) */
    void (*grid_mis_probe_launch)(const vpt_grid_view* grid, bool lm, double sigma_t, double q, const vpt_ray* rays,
                                  const double* tmax, const double* light, const uint64_t* states, int n, double* res,
                                  int32_t* strategy, uint32_t* steps, uint64_t* states_out);
    /* estimator 14's; res: five arrays of n doubles, one behind the other (t_coll, tau, w[0], w[1], w[2]) */
    void (*grid_chroma_probe_launch)(const vpt_grid_view* grid, bool lm, const vpt::ChromaCoef& c, const vpt_ray* rays,
                                     const double* tmax, const uint64_t* states, int n, double* res, int32_t* hero,
                                     uint32_t* steps, uint64_t* states_out);
    /* estimator 15's (vpt_grid.h: vpt_grid_residual_lm_m); the view holds a majorant grid */
    void (*grid_residual_probe_launch)(const vpt_grid_view* grid, double sigma_t, const vpt_ray* rays, const double* tmax,
                                       const uint64_t* states, int n, double* that, double* tauc, uint64_t* states_out,
                                       uint32_t* steps);
    /* estimator 16's two walkers (vpt_grid_spectral.h); beta: 3 doubles per ray or NULL; res: four arrays of n doubles, one
     * behind the other (t_coll, w[0], w[1], w[2]); T: three arrays of n doubles */
    void (*grid_spectral_track_probe_launch)(const vpt_grid_view* grid, bool lm, const vpt::ChromaCoef& c, const vpt_ray* rays,
                                             const double* tmax, const double* beta, const uint64_t* states, int n, double* res,
                                             uint32_t* steps, uint64_t* states_out);
    void (*grid_spectral_ratio_probe_launch)(const vpt_grid_view* grid, bool lm, const vpt::ChromaCoef& c, const vpt_ray* rays,
                                             const double* tmax, const uint64_t* states, int n, double* T, uint32_t* steps,
                                             uint64_t* states_out);
};
extern const vpt_hetero_unit vpt_int_hetero_unit;            /* vpt_hetero.hip: TL = false, EM = false */
extern const vpt_hetero_unit vpt_int_hetero_unit_tl;         /* vpt_hetero_tl.hip: TL = true, the view's interp == 1 */
extern const vpt_hetero_unit vpt_int_hetero_unit_em;         /* vpt_hetero_em.hip: EM = true */
extern const vpt_hetero_unit vpt_int_hetero_unit_em_tl;      /* vpt_hetero_em_tl.hip: both */
extern const vpt_hetero_unit vpt_int_hetero_eqa_unit;        /* vpt_hetero_eqa.hip, and _tl: vpt_hetero_eqa_tl.hip */
extern const vpt_hetero_unit vpt_int_hetero_eqa_unit_tl;
extern const vpt_hetero_unit vpt_int_hetero_mis_unit;        /* vpt_hetero_mis.hip, vpt_hetero_mis_tl.hip */
extern const vpt_hetero_unit vpt_int_hetero_mis_unit_tl;
extern const vpt_hetero_unit vpt_int_hetero_chroma_unit;     /* vpt_hetero_chroma.hip, vpt_hetero_chroma_tl.hip */
extern const vpt_hetero_unit vpt_int_hetero_chroma_unit_tl;
extern const vpt_hetero_unit vpt_int_hetero_residual_unit;   /* vpt_hetero_residual.hip, vpt_hetero_residual_tl.hip */
extern const vpt_hetero_unit vpt_int_hetero_residual_unit_tl;
extern const vpt_hetero_unit vpt_int_hetero_spectral_unit;   /* vpt_hetero_spectral.hip, vpt_hetero_spectral_tl.hip */
extern const vpt_hetero_unit vpt_int_hetero_spectral_unit_tl;

#endif
