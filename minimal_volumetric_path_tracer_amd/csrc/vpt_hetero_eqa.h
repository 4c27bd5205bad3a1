/*
 * vpt_hetero_eqa.h -- estimator 12 (VPT_HETERO_EQUIANGULAR): the control flow of MISVPTTracerRecursive (estimator 1,
 * include/vptShadeMethods.h:1345-1481; decide<1> / surface_event<1> / medium_event<1> of vpt_device.h) in the density
 * grid of vpt_grid.h.  An extension: the reference has no counterpart.  Draw for draw estimator 1, with these
 * substitutions (vpt_grid_eqa.h has the arithmetic):
 *   - the equi-angular interval [0, t] becomes the part of it the box holds, [a, b];
 *   - psurf = exp(-sigma_t t) becomes the grid's transmittance over [0, t], and the equi-angular pdf's factor
 *     1 - psurf with it; a ray that chose the surface and hit nothing ends its path (it left into vacuum, estimator
 *     10's rule); a light seen by the camera ray scores rad * beta;
 *   - at the sampled point xt the scattering coefficient is sigma_s rho(xt): a point with rho == 0 ends the path with
 *     no draw and no contribution (its throughput would be exactly zero); else single scattering and the
 *     continuation take sigma_s rho(xt) in sigma_s's place and the grid's transmittance over [0, dist] as T;
 *   - every other transmittance factor (Trs, MISv2's per-light factor, the point-light factor, the factor over tdist)
 *     is the grid's over the same segment: the policy GridTrT<TL> of vpt_hetero.h, deterministic, no draws.
 * Nothing tracks: the majorant block is accepted and ignored, and there are no null collisions.  With an emission
 * grid the host refuses the estimator (emission is scored on a delta track, which this estimator does not run).
 * On a uniform rho grid that contains every path this estimator walks estimator 1's paths at (rho sigma_a,
 * rho sigma_s) with the same draws and differs only in the rounding of tau (tests/test_gpu_hetero_eqa.py).
 * The steps are the generic (MK = -1, LT = -1) statements of estimator 1's; the surface step is restated
 * because hetero_surface (vpt_hetero.h) updates the radiance in estimator 0's order of operations.
 * The kernels live in vpt_hetero_eqa.hip (nearest) and vpt_hetero_eqa_tl.hip (trilinear), code objects of their own.
 */
#ifndef VPT_HETERO_EQA_H
#define VPT_HETERO_EQA_H

#include "vpt_hetero.h"

#define VPT_GRID_ATAN2 lm_atan2
#define VPT_GRID_TAN lm_tan
#define VPT_GRID_SQRT vm_sqrt
#define VPT_GRID_FABS vm_fabs
#include "vpt_grid_eqa.h"

namespace vpt {

/* decide<1> in the grid.  A medium event leaves the equi-angular distance in e.dist, its pdf times 1 - psurf in
 * e.pdf and -- the surface distance has no reader there -- the density at the sampled point in e.t */
template <bool COUNT, bool TL>
VPT_DEV int hetero_eqa_decide(const DevScene* __restrict__ S, const GridTrT<TL>& tp, Sampler<COUNT>& smp, Path& p, Event& e,
                              const Medium& m)
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
    const double x = smp.next();  /* equiAngularParams2's draw, taken on either branch as estimator 1 takes it */
    const double psurf = tp.along(p.o, p.d, t, sigma_t);
    if (smp.next() < psurf) {
        if (!hit) return EV_END;  /* left the medium into vacuum */
        if (sph_flag(S->m_emitter, id)) {  /* the path ends on a light; only a camera ray sees it */
            if (p.depth == 0) p.L = mul(sph_rad(S, id), p.beta);
            return EV_END;
        }
        return EV_SURF;
    }
    const dv3 lp = sph_p(S, e.src);
    const double ll[3] = {lp.x, lp.y, lp.z};
    e.dist = vpt_grid_eqa_distance(oo, dd, ll, a, b, x, psurf, &e.pdf);
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const double rho_t = vpt_grid_lookup(&tp.G, TL, xt.x, xt.y, xt.z);
    if (rho_t == 0) return EV_END;  /* no medium at the sampled point: the throughput would be exactly zero */
    e.t = rho_t;
    return EV_MED;
}

/* surface_event<1> (MK = -1, PT = -1): hetero_surface but for the radiance update, which is estimator 1's */
template <bool COUNT, class TP>
VPT_DEV void hetero_eqa_surface(const DevScene* __restrict__ S, const TP& tp, Sampler<COUNT>& smp, Path& p, const Event& e,
                                const Medium& m)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const int id = e.id, src = e.src;
    const dv3 xs = add(p.o, scl(p.d, e.t));
    const dv3 nx = nrm(sub(xs, sph_p(S, id)));
    const double probSource = 1.0 / S->n_emit;
    const double alpha = S->sph[id].alpha;
    const double Trs = tp.between(xs, sph_p(S, src), sigma_t);
    const dv3 Ldp = scl(scl(p_light<COUNT>(S, smp, id, xs, nx, p.d, src, alpha), Trs), (1 / probSource));
    const dv3 Ld = mis_v2<COUNT, -1, true, TP>(S, smp, id, xs, nx, p.d, alpha, sigma_t, tp);
    p.L = add(p.L, mul(p.beta, scl(add(Ldp, Ld), (1 / continueprob))));
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

/* medium_event<1> (LT = -1) at the point hetero_eqa_decide sampled: singleScattering toward the picked light with
 * the local sigma_s rho and the grid's transmittance to xt, then medium_tail<1> on the same two */
template <bool COUNT, class TP>
VPT_DEV void hetero_eqa_medium(const DevScene* __restrict__ S, const TP& tp, Sampler<COUNT>& smp, Path& p, const Event& e,
                               const Medium& m)
{
    const double sigma_t = m.sigma_a + m.sigma_s;
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const double ss = m.sigma_s * e.t;  /* e.t: rho at xt */
    const double T = tp.along(p.o, p.d, e.dist, sigma_t);
    const double probSource = 1.0 / S->n_emit;
    const bool zero_ok = p.beta.x - p.beta.x == 0 && p.beta.y - p.beta.y == 0 && p.beta.z - p.beta.z == 0 &&
                         (1 / e.pdf) - (1 / e.pdf) == 0;
    const dv3 Ld = single_scattering<COUNT, -1, TP>(S, smp, xt, p.d, e.src, sigma_t, true, ss, T, probSource, zero_ok, tp);
    Medium ml = m;
    ml.sigma_s = ss;
    medium_tail<1, COUNT>(smp, p, Ld, T, e.pdf, xt, ml, true);
}

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_eqa) */
template <bool COUNT, bool TL>
__device__ static dv3 trace_hetero_eqa(const DevScene* __restrict__ S, const GridTrT<TL>& tp, Sampler<COUNT>& smp, dv3 o, dv3 d,
                                       const Medium& m)
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
        const int ev = hetero_eqa_decide<COUNT, TL>(S, tp, smp, p, e, m);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_eqa_surface(S, tp, smp, p, e, m);
        else hetero_eqa_medium(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the three steps as the persistent-wave loop (vpt_wave.h) calls them, on the kernel's view of the grid */
template <bool TL>
struct HeteroEqaSteps {
    GridTrT<TL> tp;
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return hetero_eqa_decide<COUNT, TL>(S, tp, smp, p, e, m);
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
        hetero_eqa_medium(S, tp, smp, p, e, m);
    }
};

}  // namespace vpt

#endif
