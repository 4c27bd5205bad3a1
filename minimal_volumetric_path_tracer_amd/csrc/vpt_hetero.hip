/*
 * vpt_hetero.hip -- the render kernels of estimator 10 (VPT_HETERO_FREE, vpt_hetero.h) and of estimator 11
 * (VPT_HETERO_RATIO: the same kernels on the ratio-tracking policy, chosen on the host as LM is) in a translation unit
 * of its own, as vpt_pool_mis.hip is for the north-star kernel: the hot loop here is null-collision
 * stepping through a voxel grid, latency-bound and divergent, not ray/sphere arithmetic, and the unit can
 * take compile flags of its own.
 *
 * hetero_kernel: the persistent-wave loop of vpt_wave.h on estimator 10's steps (HeteroSteps, vpt_hetero.h).  A
 * lane owns one pixel and runs that pixel's samples strictly in order (acc = L + acc, then * (1 / (double)spp)),
 * so the image is render_kernel_simple_hetero's bit for bit.  What the kernel adds to the loop is the prologue
 * that stages the grid in LDS (stage_grid_lds, vpt_hetero_lds.h: one function for every density-grid kernel).
 *
 * render_kernel_simple_hetero / _ratio (one lane per pixel) and the two per-sample kernels are thin: each loads its policy
 * and hands a lambda on trace_hetero to the one body every density-grid unit shares (vpt_hetero_simple.h).
 *
 * Density reads: a grid of at most 64 KiB (16 384 voxels) is staged in LDS once per workgroup
 * (VPT_HETERO_LDS, on by default); a larger one is read from global memory, where the L2 holds the grids of
 * the tests and of the timing.  -DVPT_HETERO_LDS=0 reads every grid from global memory.  DESIGN.md section 4
 * has both timings (LDS won on the 16^3 grids by several times the run-to-run spread).  The 64 KiB do not lower
 * the occupancy: the registers already hold it at two workgroups per CU.
 *
 * Trilinear interpolation: every kernel here takes the template parameter TL (vpt_hetero.h) and the unit instantiates
 * one value of it, VPT_HETERO_TL.  Compiled as it stands (0) the unit holds the nearest-lookup kernels and exports their
 * launches as the table vpt_int_hetero_unit (vpt_hetero.h); vpt_hetero_tl.hip includes this file with VPT_HETERO_TL = 1
 * and exports vpt_int_hetero_unit_tl, so the trilinear kernels are a code object of their own and this unit's stays what
 * it was.  The LDS prologue serves both lookups as it is.
 *
 * Emission: the template parameter EM (vpt_hetero.h) in the same way, VPT_HETERO_EM.  vpt_hetero_em.hip and
 * vpt_hetero_em_tl.hip include this file with VPT_HETERO_EM = 1 and export vpt_int_hetero_unit_em and _em_tl (the
 * emitting track's probe in place of the two grid probes), two more code objects; this unit's kernels and the
 * trilinear unit's stay what they were.  The emission grid is read from global memory: the LDS prologue stages the
 * density and the majorants as before.
 *
 * The launches at the end of the file are static and reach the caller through that table alone; what a launch does on
 * the host (flags to template arguments, the persistent-wave grid, the one-lane-per-pixel grid) is vpt_hetero_launch.h's.
 */
#include <hip/hip_runtime.h>

#include "vpt_wave.h"
#include "vpt_hetero.h"
#include "vpt_hetero_simple.h"
#include "vpt_hetero_lds.h"
#include "vpt_hetero_launch.h"

#ifndef VPT_HETERO_EM
#define VPT_HETERO_EM 0
#endif
#if VPT_HETERO_EM  /* the emission units' suffixes: vpt_hetero_lds.h's VPT_HX knows the interpolation alone */
#undef VPT_HX
#if VPT_HETERO_TL
#define VPT_HX(name) name##_em_tl
#else
#define VPT_HX(name) name##_em
#endif
#endif

namespace vpt {

template <bool COUNT, int FB, bool LM, bool TL, bool EM = false>
__global__ __launch_bounds__(256, 2) void hetero_kernel(KParams P, const DevScene* __restrict__ S)
{
    using TP = GridTrT<TL, EM>;
    /* the view lives in the steps object from the start (vpt_hetero_lds.h says why) */
    HeteroSteps<LM, TL, TP, EM> st{TP::template load<LM>(P.grid)};
    stage_grid_lds<LM>(st.tp.G);
    wave_render<HeteroSteps<LM, TL, TP, EM>, COUNT, FB>(P, S, st);
}

/* estimator 11 (VPT_HETERO_RATIO): hetero_kernel on the ratio-tracking policy.  A kernel of its own, three lines as it
 * is: with estimator 10's kernel calling a common body template its code moves (commuted v_mul_f64 operands, swapped
 * v_add_f64 pairs, up to three instructions more or fewer), and that kernel is to stay what it was */
template <bool COUNT, int FB, bool LM, bool TL, bool EM = false>
__global__ __launch_bounds__(256, 2) void hetero_ratio_kernel(KParams P, const DevScene* __restrict__ S)
{
    using TP = GridRatioTr<LM, TL, EM>;
    HeteroSteps<LM, TL, TP, EM> st{TP::template load<LM>(P.grid)};
    stage_grid_lds<LM>(st.tp.G);
    wave_render<HeteroSteps<LM, TL, TP, EM>, COUNT, FB>(P, S, st);
}

}  // namespace vpt

using namespace vpt;

namespace {

constexpr bool TLU = VPT_HETERO_TL != 0;  /* the unit's value of TL */
constexpr bool EMU = VPT_HETERO_EM != 0;  /* and of EM */

/* render_kernel_simple (vpt_render_simple.h) for estimator 10: hetero_simple_render on trace_hetero */
template <bool COUNT, int FB, bool LM, bool TL, bool EM>
__global__ __launch_bounds__(256) void render_kernel_simple_hetero(KParams P, const DevScene* __restrict__ S)
{
    const GridTrT<TL, EM> tp = GridTrT<TL, EM>::template load<LM>(P.grid);
    hetero_simple_render<COUNT, FB>(P, [&](Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) {
        return trace_hetero<COUNT, LM, TL>(S, tp, smp, o, dir, m);
    });
}

/* and for estimator 11: the same on the ratio-tracking policy */
template <bool COUNT, int FB, bool LM, bool TL, bool EM>
__global__ __launch_bounds__(256) void render_kernel_simple_ratio(KParams P, const DevScene* __restrict__ S)
{
    const GridRatioTr<LM, TL, EM> tp = GridRatioTr<LM, TL, EM>::template load<LM>(P.grid);
    hetero_simple_render<COUNT, FB>(P, [&](Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) {
        return trace_hetero<COUNT, LM, TL>(S, tp, smp, o, dir, m);
    });
}

/* estimator 10's per-sample call (vpt_hetero.h); stats: vpt_debug_hetero_steps' two counters, else NULL */
template <bool LM, bool TL, bool EM = false>
__global__ __launch_bounds__(256) void trace_batch_hetero_kernel(const vpt_ray* __restrict__ rays,
                                                                 const uint64_t* __restrict__ states, int n, Medium m,
                                                                 const DevScene* __restrict__ S,
                                                                 const vpt_grid_view* __restrict__ grid, double* out,
                                                                 uint64_t* out_states, unsigned long long* stats)
{
    hetero_trace_one(blockIdx.x * blockDim.x + threadIdx.x, rays, states, n, m, out, out_states,
                     [&](Sampler<false>& smp, dv3 o, dv3 d, const Medium& m) {
                         HeteroStats hs{0, 0};
                         const dv3 L = trace_hetero<false, LM, TL>(S, GridTrT<TL, EM>::template load<LM>(grid), smp, o, d, m,
                                                                   stats ? &hs : nullptr);
                         if (stats) {
                             atomicAdd(&stats[0], hs.tracks);
                             atomicAdd(&stats[1], hs.steps);
                         }
                         return L;
                     });
}

/* estimator 11's per-sample call: the same on the ratio-tracking policy (no step statistics) */
template <bool LM, bool TL, bool EM = false>
__global__ __launch_bounds__(256) void trace_batch_hetero_ratio_kernel(const vpt_ray* __restrict__ rays,
                                                                       const uint64_t* __restrict__ states, int n, Medium m,
                                                                       const DevScene* __restrict__ S,
                                                                       const vpt_grid_view* __restrict__ grid, double* out,
                                                                       uint64_t* out_states)
{
    hetero_trace_one(blockIdx.x * blockDim.x + threadIdx.x, rays, states, n, m, out, out_states,
                     [&](Sampler<false>& smp, dv3 o, dv3 d, const Medium& m) {
                         return trace_hetero<false, LM, TL>(S, GridRatioTr<LM, TL, EM>::template load<LM>(grid), smp, o, d, m);
                     });
}

/* the density grid's walkers (vpt_grid.h), one ray per lane (vpt_grid_probe, vpt_grid_probe_lm) */
template <bool LM, bool TL>
__global__ __launch_bounds__(256) void grid_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                         const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                         const uint64_t* __restrict__ states, int n, double* tau,
                                                         double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_fields G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    tau[i] = TL ? vpt_grid_tau_tl(&G, o, d, tmax[i]) : vpt_grid_tau(&G, o, d, tmax[i]);
    uint32_t ns = 0;
    t_coll[i] = LM ? vpt_grid_track_lm_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns)
                   : vpt_grid_track_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns);
    states_out[i] = X;
    if (steps) steps[i] = ns;
}

/* the ratio-tracking walkers (vpt_grid.h), one ray per lane (vpt_grid_ratio_probe) */
template <bool LM, bool TL>
__global__ __launch_bounds__(256) void grid_ratio_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                               const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                               const uint64_t* __restrict__ states, int n, double* that,
                                                               uint64_t* states_out, uint32_t* steps)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_fields G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    uint32_t ns = 0;
    that[i] = LM ? vpt_grid_ratio_lm_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns)
                 : vpt_grid_ratio_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns);
    states_out[i] = X;
    if (steps) steps[i] = ns;
}

#if VPT_HETERO_EM
/* the emitting tracks (vpt_grid.h), one ray per lane (vpt_grid_emission_probe) */
template <bool LM, bool TL>
__global__ __launch_bounds__(256) void grid_emission_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                                  const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                                  const uint64_t* __restrict__ states, int n, double* t_coll,
                                                                  double* esum, uint64_t* states_out, uint32_t* steps)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_view G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    uint32_t ns = 0;
    double es = 0.0;
    t_coll[i] = LM ? vpt_grid_track_lm_em_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns, &es)
                   : vpt_grid_track_em_m(&G, TL, o, d, tmax[i], sigma_t, &X, &ns, &es);
    esum[i] = es;
    states_out[i] = X;
    if (steps) steps[i] = ns;
}
#endif

}  // namespace

/* the unit's launches, the slots of vpt_hetero_unit (vpt_hetero.h says what each does).  Estimator 11's stand at the end
 * of the unit (below): the kernels are instantiated in the order of their first use, and estimator 10's keep the places
 * -- and with them the label numbers -- they had */
static void ratio_trace_launch(const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                               const vpt_grid_view* grid, bool lm, double* out, uint64_t* out_states);
static int ratio_simple_launch(const KParams& K, const DevScene* S, bool lm, void* stream);
static int ratio_launch(int device, const KParams& K, const DevScene* S, bool lm, void* stream);

static void trace_launch(int est, const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                         const vpt_grid_view* grid, const vpt_hetero_args& a, double* out, uint64_t* out_states)
{
    if (est == VPT_HETERO_RATIO) return ratio_trace_launch(rays, states, n, m, S, grid, a.lm, out, out_states);
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        trace_batch_hetero_kernel<decltype(lmc)::value, TLU, EMU><<<g, b>>>(rays, states, n, m, S, grid, out, out_states, a.stats);
    }, a.lm);
}

#if VPT_HETERO_EM
static void grid_emission_probe_launch(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays,
                                       const double* tmax, const uint64_t* states, int n, double* t_coll, double* esum,
                                       uint64_t* states_out, uint32_t* steps)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        grid_emission_probe_kernel<decltype(lmc)::value, TLU><<<g, b>>>(grid, sigma_t, rays, tmax, states, n, t_coll, esum, states_out, steps);
    }, lm);
}
#else
static void grid_probe_launch(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays, const double* tmax,
                              const uint64_t* states, int n, double* tau, double* t_coll, uint64_t* states_out,
                              uint32_t* steps)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        grid_probe_kernel<decltype(lmc)::value, TLU><<<g, b>>>(grid, sigma_t, rays, tmax, states, n, tau, t_coll, states_out, steps);
    }, lm);
}
#endif

static int simple_launch(const KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream)
{
    if (K.est == VPT_HETERO_RATIO) return ratio_simple_launch(K, S, a.lm, stream);
    return with_flags([&](auto lmc, auto count, auto f32) {
        return vpt_simple_launch(render_kernel_simple_hetero<decltype(count)::value, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU, EMU>,
                                 K, S, stream);
    }, a.lm, K.counters != nullptr, K.fb == VPT_FB_F32);
}

static int launch(int device, const KParams& K, const DevScene* S, const vpt_hetero_args& a, void* stream)
{
    if (K.est == VPT_HETERO_RATIO) return ratio_launch(device, K, S, a.lm, stream);
    return with_flags([&](auto lmc, auto f32) {
        return vpt_persistent_launch(hetero_kernel<false, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU, EMU>,
                                     "hetero_kernel", device, K, S, stream);
    }, a.lm, K.fb == VPT_FB_F32);
}

/* ---- estimator 11 ---- */
static void ratio_trace_launch(const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                               const vpt_grid_view* grid, bool lm, double* out, uint64_t* out_states)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        trace_batch_hetero_ratio_kernel<decltype(lmc)::value, TLU, EMU><<<g, b>>>(rays, states, n, m, S, grid, out, out_states);
    }, lm);
}

#if !VPT_HETERO_EM
static void grid_ratio_probe_launch(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays,
                                    const double* tmax, const uint64_t* states, int n, double* that, uint64_t* states_out,
                                    uint32_t* steps)
{
    const dim3 g = vpt_ray_grid(n), b(256);
    with_flags([&](auto lmc) {
        grid_ratio_probe_kernel<decltype(lmc)::value, TLU><<<g, b>>>(grid, sigma_t, rays, tmax, states, n, that, states_out, steps);
    }, lm);
}
#endif

static int ratio_simple_launch(const KParams& K, const DevScene* S, bool lm, void* stream)
{
    return with_flags([&](auto lmc, auto count, auto f32) {
        return vpt_simple_launch(render_kernel_simple_ratio<decltype(count)::value, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU, EMU>,
                                 K, S, stream);
    }, lm, K.counters != nullptr, K.fb == VPT_FB_F32);
}

static int ratio_launch(int device, const KParams& K, const DevScene* S, bool lm, void* stream)
{
    return with_flags([&](auto lmc, auto f32) {
        return vpt_persistent_launch(hetero_ratio_kernel<false, decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64, decltype(lmc)::value, TLU, EMU>,
                                     "hetero_kernel", device, K, S, stream);
    }, lm, K.fb == VPT_FB_F32);
}

/* what the unit exports: its launches by slot.  Host pass only: a const object with a constant initialiser is emitted for
 * the device as well, and these are host functions */
#if defined(__HIP_DEVICE_COMPILE__)
#elif VPT_HETERO_EM
const vpt_hetero_unit VPT_HX(vpt_int_hetero_unit) = {launch, simple_launch, trace_launch, nullptr, nullptr, grid_emission_probe_launch};
#else
const vpt_hetero_unit VPT_HX(vpt_int_hetero_unit) = {launch, simple_launch, trace_launch, grid_probe_launch, grid_ratio_probe_launch};
#endif
