/*
 * vpt_hetero_spectral.h -- estimator 16 (VPT_HETERO_SPECTRAL): estimator 11 (VPT_HETERO_RATIO, vpt_hetero.h) in the chromatic
 * medium of estimator 14 (vpt_hetero_chroma.h: the context's medium colour, ChromaCoef), by spectral tracking
 * (vpt_grid_spectral.h).  An extension: the reference has no counterpart.  Estimator 11 statement for statement, with:
 *   - decide: the delta track is the spectral one under the largest channel's extinction sb; it takes p.beta and returns
 *     the weight W per channel, and decide multiplies it in at once, p.beta = p.beta * W, before the result is classified
 *     (a collision, a surface and the camera ray that ends on a light all carry it; at the step cap p.L is NaN as before).
 *     So Event keeps its layout and the events read nothing new;
 *   - a medium event: the albedo vector alb[k] = ss[k] / st[k] stands where medium_tail<0> has sigma_s / sigma_t, in
 *     estimator 14's statements:
 *       p.L = p.L + ((Ld * p.beta) * alb) * (1 / continueprob);   p.beta = (p.beta * alb) * (1 / continueprob)
 *   - every transmittance factor -- Trs to the picked light's centre, MISv2's per-light factor, the point-light factor
 *     and the factor over tdist along the cone direction -- is the vector T of chromatic ratio tracking over the segment,
 *     drawn from the sample's own stream (the policy GridSpectralTr: draws == true and vec == true in vpt_device.h's
 *     helpers), multiplied in componentwise where estimator 11 scales by its scalar.
 * No walk of the grid's optical depth is left: the cost follows the majorant optical depth under sb.
 * With equal st[k] (the default multipliers among them) the track is estimator 10's with W = 1.0, the ratio walk is
 * estimator 11's in every channel (vpt_grid_spectral.h says why), alb is ss[k] / st and a componentwise product with three
 * equal factors is the scalar product: the estimator is then estimator 11 bit for bit and draw for draw.  The majorant
 * block is honoured (LM) and both lookups exist (TL); with an emission grid and in the accumulator the host refuses the
 * estimator.  The coefficients are a kernel argument, as estimator 14's are; the kernels live in vpt_hetero_spectral.hip
 * (nearest) and vpt_hetero_spectral_tl.hip (trilinear), code objects of their own.
 */
#ifndef VPT_HETERO_SPECTRAL_H
#define VPT_HETERO_SPECTRAL_H

#include "vpt_hetero.h"
#include "vpt_grid_spectral.h"

namespace vpt {

/* estimator 16's policy: GridRatioTr<LM, TL> with a dv3 in the scalar's place.  The helpers' sigma_t argument is not
 * read: the policy holds the coefficients and the launch constants formed from them */
template <bool LM, bool TL>
struct GridSpectralTr {
    static constexpr bool hom = false;
    static constexpr bool draws = true;
    static constexpr bool vec = true;
    vpt_grid_fields G;
    ChromaCoef c;
    vpt_spectral_consts k;
    template <bool LM_>
    __device__ __forceinline__ static GridSpectralTr load(const vpt_grid_view* __restrict__ g, const ChromaCoef& c)
    {
        static_assert(LM_ == LM, "the policy's LM is the kernel's");
        GridSpectralTr tp;
        if (LM) tp.G = *g;
        else __builtin_memcpy(&tp.G, g, offsetof(vpt_grid_fields, maj));
        tp.c = c;
        tp.k = vpt_grid_spectral_consts(c.ss, c.st);
        return tp;
    }
    template <bool COUNT>
    __device__ __forceinline__ dv3 along(Sampler<COUNT>& smp, dv3 o, dv3 d, double dist, double) const
    {
        if (!(dist > 0)) return mk(1.0, 1.0, 1.0);
        const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
        double T[3];
        vpt_grid_spectral_ratio(&G, TL, LM, &k, oo, dd, dist, &smp.X, (uint32_t*)nullptr, T);
        return mk(T[0], T[1], T[2]);
    }
    template <bool COUNT>
    __device__ __forceinline__ dv3 between(Sampler<COUNT>& smp, dv3 a, dv3 b, double sigma_t) const
    {
        const dv3 aux = sub(b, a);
        const double dist = vm_sqrt(dot(aux, aux));
        if (!(dist > 0)) return mk(1.0, 1.0, 1.0);
        return along(smp, a, nrm(aux), dist, sigma_t);
    }
};

/* hetero_decide (EM = false) with the spectral track and its weight */
template <bool COUNT, bool LM, bool TL>
VPT_DEV int hetero_spectral_decide(const DevScene* __restrict__ S, const GridSpectralTr<LM, TL>& tp, Sampler<COUNT>& smp, Path& p,
                                   Event& e, const Medium& m)
{
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
    const double bb[3] = {p.beta.x, p.beta.y, p.beta.z};
    double W[3];
    const double tc = vpt_grid_spectral_track(&tp.G, TL, LM, &tp.k, bb, oo, dd, t, &smp.X, (uint32_t*)nullptr, W);
    if (VPT_UNLIKELY(tc != tc)) {  /* the step cap: NaN, as hetero_decide's */
        p.L = mk(tc, tc, tc);
        return EV_END;
    }
    if (!tp.k.grey) p.beta = mul(p.beta, mk(W[0], W[1], W[2]));  /* grey: W is 1.0 */
    if (tc >= 0) {
        e.dist = tc;
        return EV_MED;
    }
    if (!hit) return EV_END;  /* left the medium into vacuum */
    if (sph_flag(S->m_emitter, id)) {  /* the path ends on a light; only a camera ray sees it */
        if (p.depth == 0) p.L = mul(sph_rad(S, id), p.beta);
        return EV_END;
    }
    return EV_SURF;
}

/* hetero_surface with the vector factor Trs (the weight of "none" is in p.beta already) */
template <bool COUNT, bool LM, bool TL>
VPT_DEV void hetero_spectral_surface(const DevScene* __restrict__ S, const GridSpectralTr<LM, TL>& tp, Sampler<COUNT>& smp, Path& p,
                                     const Event& e, const Medium& m)
{
    using TP = GridSpectralTr<LM, TL>;
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const int id = e.id, src = e.src;
    const dv3 xs = add(p.o, scl(p.d, e.t));
    const dv3 nx = nrm(sub(xs, sph_p(S, id)));
    const double probSource = 1.0 / S->n_emit;
    const double alpha = S->sph[id].alpha;
    const dv3 Trs = tp.between(smp, xs, sph_p(S, src), sigma_t);
    const dv3 Ldp = scl(mul(p_light<COUNT>(S, smp, id, xs, nx, p.d, src, alpha), Trs), (1 / probSource));
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

/* hetero_medium with medium_tail<0> restated on the albedo vector, as hetero_chroma_medium restates it on w */
template <bool COUNT, bool LM, bool TL>
VPT_DEV void hetero_spectral_medium(const DevScene* __restrict__ S, const GridSpectralTr<LM, TL>& tp, Sampler<COUNT>& smp, Path& p,
                                    const Event& e, const Medium& m)
{
    using TP = GridSpectralTr<LM, TL>;
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    const dv3 w = mk(tp.k.alb[0], tp.k.alb[1], tp.k.alb[2]);
    const double probSource = 1.0 / S->n_emit;
    const bool zero_ok = p.beta.x - p.beta.x == 0 && p.beta.y - p.beta.y == 0 && p.beta.z - p.beta.z == 0;
    const dv3 Ld = single_scattering<COUNT, -1, TP>(S, smp, xt, p.d, e.src, sigma_t, false, m.sigma_s, 1.0, probSource, zero_ok,
                                                    tp);
    p.L = add(p.L, scl(mul(mul(Ld, p.beta), w), (1 / continueprob)));
    const dv3 wi = phase_sample(smp, p.d);
    p.beta = scl(mul(p.beta, w), (1 / continueprob));
    p.d = wi;
    p.o = xt;
    p.depth++;
}

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_spectral) */
template <bool COUNT, bool LM, bool TL>
__device__ static dv3 trace_hetero_spectral(const DevScene* __restrict__ S, const GridSpectralTr<LM, TL>& tp, Sampler<COUNT>& smp,
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
        const int ev = hetero_spectral_decide<COUNT, LM, TL>(S, tp, smp, p, e, m);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_spectral_surface<COUNT, LM, TL>(S, tp, smp, p, e, m);
        else hetero_spectral_medium<COUNT, LM, TL>(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the three steps as the persistent-wave loop (vpt_wave.h) calls them, on the kernel's view of the grid and the launch's
 * coefficients */
template <bool LM, bool TL>
struct HeteroSpectralSteps {
    GridSpectralTr<LM, TL> tp;
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return hetero_spectral_decide<COUNT, LM, TL>(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void surface(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                            const Medium& m) const
    {
        hetero_spectral_surface<COUNT, LM, TL>(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void medium(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                           const Medium& m) const
    {
        hetero_spectral_medium<COUNT, LM, TL>(S, tp, smp, p, e, m);
    }
};

}  // namespace vpt

#endif
