/*
 * vpt_hetero_residual.hip -- the kernels of estimator 15 (VPT_HETERO_RESIDUAL, vpt_hetero_residual.h) in a translation unit
 * of their own, as vpt_hetero_eqa.hip is for estimator 12: the code objects of the other estimators stay what they were.
 *
 * hetero_residual_kernel: the persistent-wave loop of vpt_wave.h on vpt_hetero.h's steps (HeteroSteps) with estimator 15's
 * policy.  A lane owns one pixel and runs that pixel's samples strictly in order, so the image is render_kernel_simple_residual's
 * bit for bit.  The prologue is stage_grid_control_lds (vpt_hetero_lds.h): stage_grid_lds's budget with the control grid
 * beside the majorants where the 64 KiB hold all three arrays.  The probe kernel runs the same prologue, so the probe's
 * bit-for-bit comparison with the host covers the staged and the global-memory reads.
 *
 * render_kernel_simple_residual (one lane per pixel) and the per-sample kernel are thin: each hands a lambda on
 * trace_hetero_residual to the one body every density-grid unit shares (vpt_hetero_simple.h).
 *
 * Trilinear interpolation: the unit instantiates one value of TL, VPT_HETERO_TL.  Compiled as it stands (0) it holds the
 * nearest-lookup kernels and exports their launches as the table vpt_int_hetero_residual_unit (vpt_hetero.h);
 * vpt_hetero_residual_tl.hip includes this file with VPT_HETERO_TL = 1 and exports vpt_int_hetero_residual_unit_tl.  The
 * launches are static; their host side is vpt_hetero_launch.h's, shared with the other density-grid units.
 */
#include <hip/hip_runtime.h>

#include "vpt_wave.h"
#include "vpt_hetero_residual.h"
#include "vpt_hetero_simple.h"
#include "vpt_hetero_lds.h"
#include "vpt_hetero_launch.h"

namespace vpt {

template <bool COUNT, int FB, bool TL>
__global__ __launch_bounds__(256, 2) void hetero_residual_kernel(KParams P, const DevScene* __restrict__ S)
{
    using TP = GridResidualTr<TL>;
    /* the view lives in the steps object from the start (vpt_hetero_lds.h says why) */
    HeteroSteps<true, TL, TP, false> st{TP::template load<true>(P.grid)};
    stage_grid_control_lds(st.tp.G, st.tp.ctl);
    wave_render<HeteroSteps<true, TL, TP, false>, COUNT, FB>(P, S, st);
}

}  // namespace vpt

using namespace vpt;

namespace {

constexpr bool TLU = VPT_HETERO_TL != 0;  /* the unit's value of TL */

/* render_kernel_simple (vpt_render_simple.h) for estimator 15: hetero_simple_render on trace_hetero_residual */
template <bool COUNT, int FB, bool TL>
__global__ __launch_bounds__(256) void render_kernel_simple_residual(KParams P, const DevScene* __restrict__ S)
{
    const GridResidualTr<TL> tp = GridResidualTr<TL>::template load<true>(P.grid);
    hetero_simple_render<COUNT, FB>(P, [&](Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) {
        return trace_hetero_residual<COUNT, TL>(S, tp, smp, o, dir, m);
    });
}

/* estimator 15's per-sample call (vpt_hetero_residual.h) */
template <bool TL>
__global__ __launch_bounds__(256) void trace_batch_hetero_residual_kernel(const vpt_ray* __restrict__ rays,
                                                                          const uint64_t* __restrict__ states, int n, Medium m,
                                                                          const DevScene* __restrict__ S,
                                                                          const vpt_grid_view* __restrict__ grid, double* out,
                                                                          uint64_t* out_states)
{
    hetero_trace_one(blockIdx.x * blockDim.x + threadIdx.x, rays, states, n, m, out, out_states,
                     [&](Sampler<false>& smp, dv3 o, dv3 d, const Medium& m) {
                         return trace_hetero_residual<false, TL>(S, GridResidualTr<TL>::template load<true>(grid), smp, o, d, m);
                     });
}

/* the residual walker (vpt_grid.h), one ray per lane (vpt_grid_residual_probe), behind the render kernel's prologue: every
 * lane of the workgroup stages, then the lanes past n leave */
template <bool TL>
__global__ __launch_bounds__(256) void grid_residual_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                                  const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                                  const uint64_t* __restrict__ states, int n, double* that,
                                                                  double* tauc, uint64_t* states_out, uint32_t* steps)
{
    GridResidualTr<TL> tp = GridResidualTr<TL>::template load<true>(grid);
    stage_grid_control_lds(tp.G, tp.ctl);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    uint32_t ns = 0;
    double tc = 0.0;
    that[i] = vpt_grid_residual_lm_m(&tp.G, tp.ctl, TL, o, d, tmax[i], sigma_t, &X, &ns, &tc);
    tauc[i] = tc;
    states_out[i] = X;
    if (steps) steps[i] = ns;
}

}  // namespace

/* the unit's launches, the slots of vpt_hetero_unit (vpt_hetero.h); estimator 15 takes nothing of vpt_hetero_args: the
 * caller has checked that the view holds a majorant grid */
static void trace_launch(int, const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                         const vpt_grid_view* grid, const vpt_hetero_args&, double* out, uint64_t* out_states)
{
    trace_batch_hetero_residual_kernel<TLU><<<vpt_ray_grid(n), dim3(256)>>>(rays, states, n, m, S, grid, out, out_states);
}

static void grid_residual_probe_launch(const vpt_grid_view* grid, double sigma_t, const vpt_ray* rays, const double* tmax,
                                       const uint64_t* states, int n, double* that, double* tauc, uint64_t* states_out,
                                       uint32_t* steps)
{
    grid_residual_probe_kernel<TLU><<<vpt_ray_grid(n), dim3(256)>>>(grid, sigma_t, rays, tmax, states, n, that, tauc, states_out,
                                                                     steps);
}

static int simple_launch(const KParams& K, const DevScene* S, const vpt_hetero_args&, void* stream)
{
    return with_flags([&](auto count, auto f32) {
        return vpt_simple_launch(render_kernel_simple_residual<decltype(count)::value, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, TLU>,
                                 K, S, stream);
    }, K.counters != nullptr, K.fb == VPT_FB_F32);
}

static int launch(int device, const KParams& K, const DevScene* S, const vpt_hetero_args&, void* stream)
{
    return with_flags([&](auto f32) {
        return vpt_persistent_launch(hetero_residual_kernel<false, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, TLU>,
                                     "hetero_residual_kernel", device, K, S, stream);
    }, K.fb == VPT_FB_F32);
}

/* what the unit exports.  Host pass only: a const object with a constant initialiser is emitted for the device as well,
 * and these are host functions */
#if !defined(__HIP_DEVICE_COMPILE__)
const vpt_hetero_unit VPT_HX(vpt_int_hetero_residual_unit) = {launch,  simple_launch, trace_launch, nullptr, nullptr, nullptr,
                                                              nullptr, nullptr,       nullptr,      grid_residual_probe_launch};
#endif
