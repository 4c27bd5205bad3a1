/*
 * vpt_hetero_eqa.hip -- the kernels of estimator 12 (VPT_HETERO_EQUIANGULAR, vpt_hetero_eqa.h) in a translation unit of
 * their own, as vpt_hetero.hip is for estimators 10 and 11: the code objects of those stay what they were.
 *
 * hetero_eqa_kernel: the persistent-wave loop of vpt_wave.h on estimator 12's steps (HeteroEqaSteps).  A lane owns one
 * pixel and runs that pixel's samples strictly in order, so the image is render_kernel_simple_eqa's bit for bit.  The
 * prologue that stages a grid of at most 64 KiB in LDS is stage_grid_lds (vpt_hetero_lds.h) with LM = false: there is
 * no majorant grid to stage, because nothing tracks.
 *
 * render_kernel_simple_eqa (one lane per pixel) and the per-sample kernel are thin: each hands a lambda on trace_hetero_eqa
 * to the one body every density-grid unit shares (vpt_hetero_simple.h).
 *
 * Trilinear interpolation: the unit instantiates one value of TL, VPT_HETERO_TL.  Compiled as it stands (0) it holds the
 * nearest-lookup kernels and exports their launches as the table vpt_int_hetero_eqa_unit (vpt_hetero.h);
 * vpt_hetero_eqa_tl.hip includes this file with VPT_HETERO_TL = 1 and exports vpt_int_hetero_eqa_unit_tl.  The launches
 * are static; their host side is vpt_hetero_launch.h's, shared with the other density-grid units.
 */
#include <hip/hip_runtime.h>

#include "vpt_wave.h"
#include "vpt_hetero_eqa.h"
#include "vpt_hetero_simple.h"
#include "vpt_hetero_lds.h"
#include "vpt_hetero_launch.h"

namespace vpt {

template <bool COUNT, int FB, bool TL>
__global__ __launch_bounds__(256, 2) void hetero_eqa_kernel(KParams P, const DevScene* __restrict__ S)
{
    using TP = GridTrT<TL>;
    /* the view lives in the steps object from the start (vpt_hetero_lds.h says why) */
    HeteroEqaSteps<TL> st{TP::template load<false>(P.grid)};
    stage_grid_lds<false>(st.tp.G);
    wave_render<HeteroEqaSteps<TL>, COUNT, FB>(P, S, st);
}

}  // namespace vpt

using namespace vpt;

namespace {

constexpr bool TLU = VPT_HETERO_TL != 0;  /* the unit's value of TL */

/* render_kernel_simple (vpt_render_simple.h) for estimator 12: hetero_simple_render on trace_hetero_eqa */
template <bool COUNT, int FB, bool TL>
__global__ __launch_bounds__(256) void render_kernel_simple_eqa(KParams P, const DevScene* __restrict__ S)
{
    const GridTrT<TL> tp = GridTrT<TL>::template load<false>(P.grid);
    hetero_simple_render<COUNT, FB>(P, [&](Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) {
        return trace_hetero_eqa<COUNT, TL>(S, tp, smp, o, dir, m);
    });
}

/* estimator 12's per-sample call (vpt_hetero_eqa.h) */
template <bool TL>
__global__ __launch_bounds__(256) void trace_batch_hetero_eqa_kernel(const vpt_ray* __restrict__ rays,
                                                                     const uint64_t* __restrict__ states, int n, Medium m,
                                                                     const DevScene* __restrict__ S,
                                                                     const vpt_grid_view* __restrict__ grid, double* out,
                                                                     uint64_t* out_states)
{
    hetero_trace_one(blockIdx.x * blockDim.x + threadIdx.x, rays, states, n, m, out, out_states,
                     [&](Sampler<false>& smp, dv3 o, dv3 d, const Medium& m) {
                         return trace_hetero_eqa<false, TL>(S, GridTrT<TL>::template load<false>(grid), smp, o, d, m);
                     });
}

/* one equi-angular decision per lane (vpt_grid_eqa.h: vpt_grid_eqa_one; vpt_grid_eqa_probe) */
template <bool TL>
__global__ __launch_bounds__(256) void grid_eqa_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                             const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                             const double* __restrict__ light,
                                                             const uint64_t* __restrict__ states, int n, double* psurf,
                                                             double* dist, double* pdf, double* T, double* rho_t,
                                                             uint64_t* states_out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_fields G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    const double lp[3] = {light[3 * i], light[3 * i + 1], light[3 * i + 2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    double ps, ds, pf, tr, rt;
    vpt_grid_eqa_one(&G, TL, sigma_t, o, d, tmax[i], lp, &X, &ps, &ds, &pf, &tr, &rt);
    psurf[i] = ps;
    dist[i] = ds;
    pdf[i] = pf;
    T[i] = tr;
    rho_t[i] = rt;
    states_out[i] = X;
}

}  // namespace

/* the unit's launches, the slots of vpt_hetero_unit (vpt_hetero.h); estimator 12 takes nothing of vpt_hetero_args */
static void trace_launch(int, const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                         const vpt_grid_view* grid, const vpt_hetero_args&, double* out, uint64_t* out_states)
{
    trace_batch_hetero_eqa_kernel<TLU><<<vpt_ray_grid(n), dim3(256)>>>(rays, states, n, m, S, grid, out, out_states);
}

static void grid_eqa_probe_launch(const vpt_grid_view* grid, double sigma_t, const vpt_ray* rays, const double* tmax,
                                  const double* light, const uint64_t* states, int n, double* psurf, double* dist,
                                  double* pdf, double* T, double* rho_t, uint64_t* states_out)
{
    grid_eqa_probe_kernel<TLU><<<vpt_ray_grid(n), dim3(256)>>>(grid, sigma_t, rays, tmax, light, states, n, psurf, dist, pdf,
                                                                T, rho_t, states_out);
}

static int simple_launch(const KParams& K, const DevScene* S, const vpt_hetero_args&, void* stream)
{
    return with_flags([&](auto count, auto f32) {
        return vpt_simple_launch(render_kernel_simple_eqa<decltype(count)::value, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, TLU>,
                                 K, S, stream);
    }, K.counters != nullptr, K.fb == VPT_FB_F32);
}

static int launch(int device, const KParams& K, const DevScene* S, const vpt_hetero_args&, void* stream)
{
    return with_flags([&](auto f32) {
        return vpt_persistent_launch(hetero_eqa_kernel<false, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, TLU>,
                                     "hetero_eqa_kernel", device, K, S, stream);
    }, K.fb == VPT_FB_F32);
}

/* what the unit exports.  Host pass only: a const object with a constant initialiser is emitted for the device as well,
 * and these are host functions */
#if !defined(__HIP_DEVICE_COMPILE__)
const vpt_hetero_unit VPT_HX(vpt_int_hetero_eqa_unit) = {launch, simple_launch, trace_launch, nullptr, nullptr, nullptr, grid_eqa_probe_launch};
#endif
