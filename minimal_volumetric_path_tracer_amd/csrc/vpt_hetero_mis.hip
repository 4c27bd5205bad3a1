/*
 * vpt_hetero_mis.hip -- the kernels of estimator 13 (VPT_HETERO_MIS, vpt_hetero_mis.h) in a translation unit of their
 * own, as vpt_hetero_eqa.hip is for estimator 12: the code objects of the other estimators stay what they were.
 *
 * hetero_mis_kernel: the persistent-wave loop of vpt_wave.h on estimator 13's steps (HeteroMisSteps).  A lane owns one
 * pixel and runs that pixel's samples strictly in order, so the image is render_kernel_simple_mis's bit for bit.  The
 * prologue that stages a grid of at most 64 KiB in LDS, and with local majorants the majorant grid in what the density
 * left of the budget, is stage_grid_lds (vpt_hetero_lds.h), every density-grid kernel's.
 *
 * The track fraction q is a kernel argument of every kernel here (KParams keeps its layout).  render_kernel_simple_mis
 * (one lane per pixel) and the per-sample kernel are thin: each hands a lambda on trace_hetero_mis, which captures q, to the
 * one body every density-grid unit shares (vpt_hetero_simple.h).
 *
 * Trilinear interpolation: the unit instantiates one value of TL, VPT_HETERO_TL.  Compiled as it stands (0) it holds the
 * nearest-lookup kernels and exports their launches as the table vpt_int_hetero_mis_unit (vpt_hetero.h);
 * vpt_hetero_mis_tl.hip includes this file with VPT_HETERO_TL = 1 and exports vpt_int_hetero_mis_unit_tl.  The launches
 * are static; their host side is vpt_hetero_launch.h's, shared with the other density-grid units.
 */
#include <hip/hip_runtime.h>

#include "vpt_wave.h"
#include "vpt_hetero_mis.h"
#include "vpt_hetero_simple.h"
#include "vpt_hetero_lds.h"
#include "vpt_hetero_launch.h"

namespace vpt {

template <bool COUNT, int FB, bool LM, bool TL>
__global__ __launch_bounds__(256, 2) void hetero_mis_kernel(KParams P, const DevScene* __restrict__ S, double q)
{
    using TP = GridTrT<TL>;
    /* the view lives in the steps object from the start (vpt_hetero_lds.h says why) */
    HeteroMisSteps<LM, TL> st{TP::template load<LM>(P.grid), q};
    stage_grid_lds<LM>(st.tp.G);
    wave_render<HeteroMisSteps<LM, TL>, COUNT, FB>(P, S, st);
}

}  // namespace vpt

using namespace vpt;

namespace {

constexpr bool TLU = VPT_HETERO_TL != 0;  /* the unit's value of TL */

/* render_kernel_simple (vpt_render_simple.h) for estimator 13: hetero_simple_render on trace_hetero_mis */
template <bool COUNT, int FB, bool LM, bool TL>
__global__ __launch_bounds__(256) void render_kernel_simple_mis(KParams P, const DevScene* __restrict__ S, double q)
{
    const GridTrT<TL> tp = GridTrT<TL>::template load<LM>(P.grid);
    hetero_simple_render<COUNT, FB>(P, [&](Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) {
        return trace_hetero_mis<COUNT, LM, TL>(S, tp, q, smp, o, dir, m);
    });
}

/* estimator 13's per-sample call (vpt_hetero_mis.h) */
template <bool LM, bool TL>
__global__ __launch_bounds__(256) void trace_batch_hetero_mis_kernel(const vpt_ray* __restrict__ rays,
                                                                     const uint64_t* __restrict__ states, int n, Medium m,
                                                                     const DevScene* __restrict__ S,
                                                                     const vpt_grid_view* __restrict__ grid, double q,
                                                                     double* out, uint64_t* out_states)
{
    hetero_trace_one(blockIdx.x * blockDim.x + threadIdx.x, rays, states, n, m, out, out_states,
                     [&](Sampler<false>& smp, dv3 o, dv3 d, const Medium& m) {
                         return trace_hetero_mis<false, LM, TL>(S, GridTrT<TL>::template load<LM>(grid), q, smp, o, d, m);
                     });
}

/* one combined decision per lane (vpt_grid_mis.h: vpt_grid_mis_one; vpt_grid_mis_probe).  res: six arrays of n doubles,
 * one behind the other */
template <bool LM, bool TL>
__global__ __launch_bounds__(256) void grid_mis_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t, double q,
                                                             const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                             const double* __restrict__ light,
                                                             const uint64_t* __restrict__ states, int n, double* res,
                                                             int32_t* strategy, uint32_t* steps, uint64_t* states_out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_fields G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    const double lp[3] = {light[3 * i], light[3 * i + 1], light[3 * i + 2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    double ps, ds, pf, pe, tr, rt;
    int sg = 0;
    uint32_t ns = 0;
    vpt_grid_mis_one(&G, TL, LM, sigma_t, q, o, d, tmax[i], lp, &X, &ps, &sg, &ds, &pf, &pe, &tr, &rt, &ns);
    const size_t nn = (size_t)n;
    res[i] = ps;
    res[nn + i] = ds;
    res[2 * nn + i] = pf;
    res[3 * nn + i] = pe;
    res[4 * nn + i] = tr;
    res[5 * nn + i] = rt;
    strategy[i] = sg;
    steps[i] = ns;
    states_out[i] = X;
}

}  // namespace

/* the unit's launches, the slots of vpt_hetero_unit (vpt_hetero.h); estimator 13 takes lm and the track fraction */
static void trace_launch(int, const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                         const vpt_grid_view* grid, const vpt_hetero_args& a, double* out, uint64_t* out_states)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        trace_batch_hetero_mis_kernel<decltype(lmc)::value, TLU><<<g, b>>>(rays, states, n, m, S, grid, a.q, out, out_states);
    }, a.lm);
}

static void grid_mis_probe_launch(const vpt_grid_view* grid, bool lm, double sigma_t, double q, const vpt_ray* rays,
                                  const double* tmax, const double* light, const uint64_t* states, int n, double* res,
                                  int32_t* strategy, uint32_t* steps, uint64_t* states_out)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        grid_mis_probe_kernel<decltype(lmc)::value, TLU><<<g, b>>>(grid, sigma_t, q, rays, tmax, light, states, n, res, strategy, steps, states_out);
    }, lm);
}

static int simple_launch(const KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream)
{
    return with_flags([&](auto lmc, auto count, auto f32) {
        return vpt_simple_launch(render_kernel_simple_mis<decltype(count)::value, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU>,
                                 K, S, stream, a.q);
    }, a.lm, K.counters != nullptr, K.fb == VPT_FB_F32);
}

static int launch(int device, const KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream)
{
    return with_flags([&](auto lmc, auto f32) {
        return vpt_persistent_launch(hetero_mis_kernel<false, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU>,
                                     "hetero_mis_kernel", device, K, S, stream, a.q);
    }, a.lm, K.fb == VPT_FB_F32);
}

/* what the unit exports.  Host pass only: a const object with a constant initialiser is emitted for the device as well,
 * and these are host functions */
#if !defined(__HIP_DEVICE_COMPILE__)
const vpt_hetero_unit VPT_HX(vpt_int_hetero_mis_unit) = {launch, simple_launch, trace_launch, nullptr, nullptr, nullptr, nullptr, grid_mis_probe_launch};
#endif
