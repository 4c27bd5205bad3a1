/*
 * vpt_hetero_residual.h -- estimator 15 (VPT_HETERO_RESIDUAL): estimator 11 (VPT_HETERO_RATIO, vpt_hetero.h) statement for
 * statement, with every transmittance factor a residual ratio-tracking estimate over the block minima (vpt_grid.h:
 * vpt_grid_residual_lm_m) where estimator 11 takes a ratio-tracking one.  An extension: the reference has no counterpart.
 * The steps are vpt_hetero.h's hetero_decide / hetero_surface / hetero_medium on the policy below; the delta track of
 * hetero_decide is the local-majorant one (LM = true always: the estimator needs a majorant block, and B >= max(n) is the
 * global control).  No emission (EM = false): the emitting track under a control density is not worked out.
 *
 * The control grid lies behind the majorants of the view's majorant allocation (vpt_grid_control_of); the policy takes
 * that pointer from the view when it is loaded and keeps it as a member of its own, because the LDS prologue repoints
 * G.maj afterwards (vpt_hetero_lds.h: stage_grid_control_lds, which repoints this pointer too where it stages the minima).
 *
 * VPT_RESIDUAL_NOINLINE: 1 calls the walker as one out-of-line device function from every factor site; 0 (the default)
 * inlines it at each.  DESIGN.md section 4 ("Residual ratio tracking") has the registers and the times of both.
 */
#ifndef VPT_HETERO_RESIDUAL_H
#define VPT_HETERO_RESIDUAL_H

#include "vpt_hetero.h"

#ifndef VPT_RESIDUAL_NOINLINE
#define VPT_RESIDUAL_NOINLINE 0
#endif

namespace vpt {

#if VPT_RESIDUAL_NOINLINE
/* the walker out of line: one copy per unit, called from every factor site (the control optical depth is not needed there) */
template <bool TL>
__device__ __noinline__ static double residual_walk(const vpt_grid_fields* G, const float* ctl, const double* o, const double* d,
                                                    double dist, double sigma_t, uint64_t* X)
{
    double tauc;
    return vpt_grid_residual_lm_m(G, ctl, TL, o, d, dist, sigma_t, X, (uint32_t*)nullptr, &tauc);
}
#endif

/* estimator 15's policy: GridRatioTr<true, TL> with the residual walker and the control grid's pointer */
template <bool TL>
struct GridResidualTr : GridNoColour {
    static constexpr bool hom = false;
    static constexpr bool draws = true;
    vpt_grid_fields G;
    const float* ctl;  /* the block minima: behind the majorants in global memory, or staged in LDS */
    template <bool LM_>
    __device__ __forceinline__ static GridResidualTr load(const vpt_grid_view* __restrict__ g)
    {
        static_assert(LM_, "estimator 15 walks a majorant grid");
        GridResidualTr tp;
        tp.G = *g;
        tp.ctl = vpt_grid_control_of(&tp.G);
        return tp;
    }
    template <bool COUNT>
    __device__ __forceinline__ double along(Sampler<COUNT>& smp, dv3 o, dv3 d, double dist, double sigma_t) const
    {
        if (!(dist > 0)) return lm_exp(sigma_t * 0.0 * -1.0);
        const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
#if VPT_RESIDUAL_NOINLINE
        return residual_walk<TL>(&G, ctl, oo, dd, dist, sigma_t, &smp.X);
#else
        double tauc;
        return vpt_grid_residual_lm_m(&G, ctl, TL, oo, dd, dist, sigma_t, &smp.X, (uint32_t*)nullptr, &tauc);
#endif
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

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_residual): vpt_hetero.h's trace_hetero on this policy */
template <bool COUNT, bool TL>
__device__ static dv3 trace_hetero_residual(const DevScene* __restrict__ S, const GridResidualTr<TL>& tp, Sampler<COUNT>& smp,
                                            dv3 o, dv3 d, const Medium& m)
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
        const int ev = hetero_decide<COUNT, true, TL, GridResidualTr<TL>, false>(S, tp, smp, p, e, m);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_surface(S, tp, smp, p, e, m);
        else hetero_medium(S, tp, smp, p, e, m);
    }
    return p.L;
}

}  // namespace vpt

#endif
