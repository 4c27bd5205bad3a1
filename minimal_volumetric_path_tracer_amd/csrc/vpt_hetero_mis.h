/*
 * vpt_hetero_mis.h -- estimator 13 (VPT_HETERO_MIS): estimator 12 (vpt_hetero_eqa.h) with its distance decision replaced
 * by the one-sample combination of vpt_grid_mis.h -- with probability q (vpt_set_hetero_mis_fraction, the context's
 * track fraction) the scattering distance comes from a delta track, as in estimator 10, else from the equi-angular
 * distribution toward the picked light, and either way the vertex is weighted by the balance heuristic's combined pdf
 * q sigma_t rho T + (1 - q) (1 - psurf) p_eq.  An extension: the reference has no counterpart.
 *   - the draws of a decision: intersection, light pick, the equi-angular draw x, the coin c, then the track's draws
 *     where c < q; the coin decides the strategy and, rescaled, is estimator 12's surface coin;
 *   - the surface branch and the rule for an empty sampled point (rho == 0 ends the path with no draw and no
 *     contribution) are estimator 12's; the track's step cap gives a NaN radiance, estimator 10's rule;
 *   - the surface step is hetero_eqa_surface as it is; the medium step is hetero_eqa_medium on the combined pdf, with the
 *     transmittance over [0, dist] that the decision already walked carried in e.t instead of walked again (the density
 *     at the sampled point is looked up again, which is deterministic and gives the same bits);
 *   - the majorant block is honoured as estimator 10 honours it (the template parameter LM); with an emission grid
 *     the host refuses the estimator.
 * q == 0 is estimator 12 bit for bit and draw for draw; q == 1 samples every distance by delta tracking.
 * The track fraction travels in the steps object (HeteroMisSteps) and is a kernel argument of this estimator's kernels
 * alone: KParams, Event and Medium keep their layouts.
 * The kernels live in vpt_hetero_mis.hip (nearest) and vpt_hetero_mis_tl.hip (trilinear), code objects of their own.
 */
#ifndef VPT_HETERO_MIS_H
#define VPT_HETERO_MIS_H

#include "vpt_hetero_eqa.h"
#include "vpt_grid_mis.h"

namespace vpt {

/* hetero_eqa_decide with the decision of vpt_grid_mis.h in place of its coin and distance.  A medium event leaves the
 * distance in e.dist, the combined pdf in e.pdf and the transmittance over [0, dist] in e.t */
template <bool COUNT, bool LM, bool TL>
VPT_DEV int hetero_mis_decide(const DevScene* __restrict__ S, const GridTrT<TL>& tp, double q, Sampler<COUNT>& smp, Path& p,
                              Event& e, const Medium& m)
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
    double a, b;
    vpt_grid_eqa_interval(&tp.G, oo, dd, t, &a, &b);
    const double x = smp.next();  /* the equi-angular draw, taken under either strategy as estimator 12 takes it */
    const double psurf = tp.along(p.o, p.d, t, sigma_t);
    const double c = smp.next();
    const dv3 lp = sph_p(S, e.src);
    const double ll[3] = {lp.x, lp.y, lp.z};
    int strategy;
    double pe = 0.0;
    const int ev = vpt_grid_mis_distance(&tp.G, TL, LM, sigma_t, q, oo, dd, t, ll, a, b, x, psurf, c, &smp.X, &strategy,
                                         &e.dist, &pe, (uint32_t*)nullptr);
    if (VPT_UNLIKELY(ev == VPT_MIS_CAP)) {  /* the step cap: NaN, as hetero_decide's */
        p.L = mk(e.dist, e.dist, e.dist);
        return EV_END;
    }
    if (ev == VPT_MIS_SURFACE) {
        if (!hit) return EV_END;  /* left the medium into vacuum */
        if (sph_flag(S->m_emitter, id)) {  /* the path ends on a light; only a camera ray sees it */
            if (p.depth == 0) p.L = mul(sph_rad(S, id), p.beta);
            return EV_END;
        }
        return EV_SURF;
    }
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const double rho_t = vpt_grid_lookup(&tp.G, TL, xt.x, xt.y, xt.z);
    if (rho_t == 0) return EV_END;  /* no medium at the sampled point: the throughput would be exactly zero */
    const double T = tp.along(p.o, p.d, e.dist, sigma_t);
    e.pdf = vpt_grid_mis_pdf(q, sigma_t, rho_t, T, pe);
    e.t = T;
    return EV_MED;
}

/* hetero_eqa_medium at the point hetero_mis_decide sampled, statement for statement, but that T comes with the event
 * (e.t) and rho is looked up again at xt, the point decide formed in the same way */
template <bool COUNT, bool TL>
VPT_DEV void hetero_mis_medium(const DevScene* __restrict__ S, const GridTrT<TL>& tp, Sampler<COUNT>& smp, Path& p,
                               const Event& e, const Medium& m)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const double ss = m.sigma_s * vpt_grid_lookup(&tp.G, TL, xt.x, xt.y, xt.z);
    const double T = e.t;
    const double probSource = 1.0 / S->n_emit;
    const bool zero_ok = p.beta.x - p.beta.x == 0 && p.beta.y - p.beta.y == 0 && p.beta.z - p.beta.z == 0 &&
                         (1 / e.pdf) - (1 / e.pdf) == 0;
    const dv3 Ld = single_scattering<COUNT, -1, GridTrT<TL>>(S, smp, xt, p.d, e.src, sigma_t, true, ss, T, probSource, zero_ok,
                                                             tp);
    Medium ml = m;
    ml.sigma_s = ss;
    medium_tail<1, COUNT>(smp, p, Ld, T, e.pdf, xt, ml, true);
}

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_mis) */
template <bool COUNT, bool LM, bool TL>
__device__ static dv3 trace_hetero_mis(const DevScene* __restrict__ S, const GridTrT<TL>& tp, double q, Sampler<COUNT>& smp,
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
        const int ev = hetero_mis_decide<COUNT, LM, TL>(S, tp, q, smp, p, e, m);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_eqa_surface(S, tp, smp, p, e, m);
        else hetero_mis_medium<COUNT, TL>(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the three steps as the persistent-wave loop (vpt_wave.h) calls them, on the kernel's view of the grid and the
 * context's track fraction */
template <bool LM, bool TL>
struct HeteroMisSteps {
    GridTrT<TL> tp;
    double q;
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return hetero_mis_decide<COUNT, LM, TL>(S, tp, q, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void surface(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                            const Medium& m) const
    {
        hetero_eqa_surface(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void medium(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                           const Medium& m) const
    {
        hetero_mis_medium<COUNT, TL>(S, tp, smp, p, e, m);
    }
};

}  // namespace vpt

#endif
