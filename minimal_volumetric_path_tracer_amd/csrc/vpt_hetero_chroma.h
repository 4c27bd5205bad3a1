/*
 * vpt_hetero_chroma.h -- estimator 14 (VPT_HETERO_CHROMATIC): estimator 10 (vpt_hetero.h) in a medium whose absorption
 * and scattering depend on the colour channel.  The context's medium colour (vpt_set_medium_colour) multiplies the
 * medium's sigma_a and sigma_s per channel: sa[k] = sigma_a * ca[k], ss[k] = sigma_s * cs[k], st[k] = sa[k] + ss[k], formed
 * on the host once per launch (ChromaCoef).  An extension: the reference has no counterpart.  Estimator 10 statement
 * for statement, with the substitutions of vpt_grid_chroma.h:
 *   - decide: after the light pick one draw picks the hero channel h (none where the three st[k] are equal), and the
 *     delta track runs under st[h];
 *   - a medium event at distance t: tau over [0, t] is walked once, and the vector w of vpt_grid_chroma_w stands where
 *     medium_tail<0> has the albedo sigma_s / sigma_t:
 *       p.L = p.L + ((Ld * p.beta) * w) * (1 / continueprob);   p.beta = (p.beta * w) * (1 / continueprob)
 *   - a surface event at e.t, and the camera ray that ends on a light: tau over [0, e.t] is walked once, first
 *     p.beta = p.beta * ws (vpt_grid_chroma_ws), then estimator 10's statements;
 *   - every transmittance factor -- Trs to the picked light's centre, MISv2's per-light factor, the point-light factor
 *     and the factor over tdist along the cone direction -- is the vector T of vpt_grid_chroma_T from one walk of the
 *     segment (the policy GridChromaTr, vec == true in vpt_device.h's helpers), multiplied in componentwise where
 *     estimator 10 scales by its scalar.
 * The walks are taken in the events and not in decide, so Event keeps its layout.  With equal st[k] (the default
 * multipliers among them) no hero draw is taken, w is (ss[k] / st) and ws is 1.0 in every channel, and a componentwise
 * product with three equal factors is the scalar product: the estimator is then estimator 10 bit for bit and draw for
 * draw, and with equal ss[k] as well in every channel.  The majorant block is honoured (LM) and both lookups exist (TL);
 * with an emission grid and in the accumulator the host refuses the estimator.
 * The coefficients travel in the steps object and are a kernel argument of this estimator's kernels alone: KParams,
 * Event and Medium keep their layouts.  The kernels live in vpt_hetero_chroma.hip (nearest) and vpt_hetero_chroma_tl.hip
 * (trilinear), code objects of their own.
 */
#ifndef VPT_HETERO_CHROMA_H
#define VPT_HETERO_CHROMA_H

#include "vpt_hetero.h"
#include "vpt_grid_chroma.h"

namespace vpt {

/* the grid's transmittance per channel as the TP policy of mis_v2 / single_scattering: GridTrT with a dv3 in the
 * scalar's place.  The helpers' sigma_t argument is not read: the policy holds the three extinctions */
template <bool TL>
struct GridChromaTr {
    static constexpr bool hom = false;
    static constexpr bool draws = false;
    static constexpr bool vec = true;
    vpt_grid_fields G;
    ChromaCoef c;
    template <bool LM>
    __device__ __forceinline__ static GridChromaTr load(const vpt_grid_view* __restrict__ g, const ChromaCoef& c)
    {
        GridChromaTr tp;
        if (LM) tp.G = *g;
        else __builtin_memcpy(&tp.G, g, offsetof(vpt_grid_fields, maj));
        tp.c = c;
        return tp;
    }
    __device__ __forceinline__ dv3 of_tau(double tau) const
    {
        double T[3];
        vpt_grid_chroma_T(c.st, tau, T);
        return mk(T[0], T[1], T[2]);
    }
    __device__ __forceinline__ double tau(dv3 o, dv3 d, double dist) const
    {
        const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
        return vpt_grid_chroma_tau(&G, TL, oo, dd, dist);
    }
    __device__ __forceinline__ dv3 along(dv3 o, dv3 d, double dist, double) const { return of_tau(tau(o, d, dist)); }
    /* a to b: the distance and the unit direction formed as GridTrT::between forms them */
    __device__ __forceinline__ dv3 between(dv3 a, dv3 b, double sigma_t) const
    {
        const dv3 aux = sub(b, a);
        const double dist = vm_sqrt(dot(aux, aux));
        if (!(dist > 0)) return of_tau(0.0);
        return along(a, nrm(aux), dist, sigma_t);
    }
};

/* hetero_decide (EM = false) with the hero draw in front of the track */
template <bool COUNT, bool LM, bool TL>
VPT_DEV int hetero_chroma_decide(const DevScene* __restrict__ S, const GridChromaTr<TL>& tp, Sampler<COUNT>& smp, Path& p,
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
    const int h = vpt_grid_chroma_hero(tp.c.st, &smp.X);
    const double tc = vpt_grid_chroma_track(&tp.G, TL, LM, oo, dd, t, vpt_grid_chroma_pick(tp.c.st, h), &smp.X, (uint32_t*)nullptr);
    if (VPT_UNLIKELY(tc != tc)) {  /* the step cap: NaN, as hetero_decide's */
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
            double ws[3];
            vpt_grid_chroma_ws(tp.c.st, tp.tau(p.o, p.d, t), ws);
            p.beta = mul(p.beta, mk(ws[0], ws[1], ws[2]));
            p.L = mul(sph_rad(S, id), p.beta);
        }
        return EV_END;
    }
    return EV_SURF;
}

/* hetero_surface behind the weight of "none" over [0, e.t] */
template <bool COUNT, bool TL>
VPT_DEV void hetero_chroma_surface(const DevScene* __restrict__ S, const GridChromaTr<TL>& tp, Sampler<COUNT>& smp, Path& p,
                                   const Event& e, const Medium& m)
{
    using TP = GridChromaTr<TL>;
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const int id = e.id, src = e.src;
    double ws[3];
    vpt_grid_chroma_ws(tp.c.st, tp.tau(p.o, p.d, e.t), ws);
    p.beta = mul(p.beta, mk(ws[0], ws[1], ws[2]));
    const dv3 xs = add(p.o, scl(p.d, e.t));
    const dv3 nx = nrm(sub(xs, sph_p(S, id)));
    const double probSource = 1.0 / S->n_emit;
    const double alpha = S->sph[id].alpha;
    const dv3 Trs = tp.between(xs, sph_p(S, src), sigma_t);
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

/* hetero_medium with medium_tail<0> restated on the vector w in the albedo's place */
template <bool COUNT, bool TL>
VPT_DEV void hetero_chroma_medium(const DevScene* __restrict__ S, const GridChromaTr<TL>& tp, Sampler<COUNT>& smp, Path& p,
                                  const Event& e, const Medium& m)
{
    using TP = GridChromaTr<TL>;
    const double sigma_t = m.sigma_a + m.sigma_s;
    const double continueprob = 0.6;
    const dv3 xt = add(p.o, scl(p.d, e.dist));
    double wk[3];
    vpt_grid_chroma_w(tp.c.ss, tp.c.st, tp.tau(p.o, p.d, e.dist), wk);
    const dv3 w = mk(wk[0], wk[1], wk[2]);
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

/* one camera sample, sequentially (vpt_trace_batch, render_kernel_simple_chroma) */
template <bool COUNT, bool LM, bool TL>
__device__ static dv3 trace_hetero_chroma(const DevScene* __restrict__ S, const GridChromaTr<TL>& tp, Sampler<COUNT>& smp, dv3 o,
                                          dv3 d, const Medium& m)
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
        const int ev = hetero_chroma_decide<COUNT, LM, TL>(S, tp, smp, p, e, m);
        if (ev == EV_END) break;
        if (ev == EV_SURF) hetero_chroma_surface<COUNT, TL>(S, tp, smp, p, e, m);
        else hetero_chroma_medium<COUNT, TL>(S, tp, smp, p, e, m);
    }
    return p.L;
}

/* the three steps as the persistent-wave loop (vpt_wave.h) calls them, on the kernel's view of the grid and the launch's
 * coefficients */
template <bool LM, bool TL>
struct HeteroChromaSteps {
    GridChromaTr<TL> tp;
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return hetero_chroma_decide<COUNT, LM, TL>(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void surface(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                            const Medium& m) const
    {
        hetero_chroma_surface<COUNT, TL>(S, tp, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void medium(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                           const Medium& m) const
    {
        hetero_chroma_medium<COUNT, TL>(S, tp, smp, p, e, m);
    }
};

}  // namespace vpt

#endif
