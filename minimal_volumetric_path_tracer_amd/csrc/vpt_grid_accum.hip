/*
 * vpt_grid_accum.hip -- the render kernels of the grid accumulator (vpt_accum_create_grid): the continuing
 * persistent-wave loop of vpt_wave_accum.h on the steps objects and policies of the estimators 10 to 16, each with the
 * LDS prologue its one-shot sibling runs (vpt_hetero_lds.h).
 *
 * One source, fourteen code objects: the Makefile compiles this file once per estimator family (VPT_GA_FAMILY) and
 * lookup (VPT_HETERO_TL, as the _tl wrappers of the render units do), and for estimators 10 and 11 without and with the
 * emission grid (VPT_HETERO_EM).  The units of the one-shot renders are not touched: their code objects stay what they
 * were.  A unit holds the LM = false and LM = true kernels (estimators 12 and 15: one kernel) and exports one launch
 * (vpt_grid_accum.h).  There are no FB or COUNT variants: the state is FP64 and the kernels do not count.
 *
 *   VPT_GA_FAMILY  kernel                       steps                                 extra argument
 *   0              grid_accum_kernel            HeteroSteps over GridTrT        (10)  --
 *                  grid_accum_ratio_kernel      HeteroSteps over GridRatioTr    (11)  --
 *   1              grid_accum_eqa_kernel        HeteroEqaSteps                  (12)  --
 *   2              grid_accum_mis_kernel        HeteroMisSteps                  (13)  the track fraction q
 *   3              grid_accum_chroma_kernel     HeteroChromaSteps               (14)  ChromaCoef
 *   4              grid_accum_residual_kernel   HeteroSteps over GridResidualTr (15)  --
 *   5              grid_accum_spectral_kernel   HeteroSpectralSteps             (16)  ChromaCoef
 */
#include <hip/hip_runtime.h>

#ifndef VPT_GA_FAMILY
#error "vpt_grid_accum.hip is compiled with -DVPT_GA_FAMILY=0..5 (csrc/Makefile)"
#endif

#include "vpt_wave_accum.h"
#if VPT_GA_FAMILY == 0
#include "vpt_hetero.h"
#elif VPT_GA_FAMILY == 1
#include "vpt_hetero_eqa.h"
#elif VPT_GA_FAMILY == 2
#include "vpt_hetero_mis.h"
#elif VPT_GA_FAMILY == 3
#include "vpt_hetero_chroma.h"
#elif VPT_GA_FAMILY == 4
#include "vpt_hetero_residual.h"
#else
#include "vpt_hetero_spectral.h"
#endif
#include "vpt_hetero_lds.h"
#include "vpt_hetero_launch.h"
#include "vpt_grid_accum.h"

#ifndef VPT_HETERO_EM
#define VPT_HETERO_EM 0
#endif
#if VPT_HETERO_EM && VPT_GA_FAMILY != 0
#error "the emission grid is estimators 10 and 11's (VPT_GA_FAMILY == 0)"
#endif
#if VPT_HETERO_EM  /* vpt_hetero_lds.h's VPT_HX knows the interpolation alone */
#undef VPT_HX
#if VPT_HETERO_TL
#define VPT_HX(name) name##_em_tl
#else
#define VPT_HX(name) name##_em
#endif
#endif

namespace vpt {

#if VPT_GA_FAMILY == 0

template <bool LM, bool TL, bool EM>
__global__ __launch_bounds__(256, 2) void grid_accum_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A)
{
    using TP = GridTrT<TL, EM>;
    /* the view lives in the steps object from the start (vpt_hetero_lds.h says why) */
    HeteroSteps<LM, TL, TP, EM> st{TP::template load<LM>(P.grid)};
    stage_grid_lds<LM>(st.tp.G);
    wave_accum(P, S, A, st);
}

template <bool LM, bool TL, bool EM>
__global__ __launch_bounds__(256, 2) void grid_accum_ratio_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A)
{
    using TP = GridRatioTr<LM, TL, EM>;
    HeteroSteps<LM, TL, TP, EM> st{TP::template load<LM>(P.grid)};
    stage_grid_lds<LM>(st.tp.G);
    wave_accum(P, S, A, st);
}

#elif VPT_GA_FAMILY == 1

template <bool TL>
__global__ __launch_bounds__(256, 2) void grid_accum_eqa_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A)
{
    using TP = GridTrT<TL>;
    HeteroEqaSteps<TL> st{TP::template load<false>(P.grid)};
    stage_grid_lds<false>(st.tp.G);
    wave_accum(P, S, A, st);
}

#elif VPT_GA_FAMILY == 2

template <bool LM, bool TL>
__global__ __launch_bounds__(256, 2) void grid_accum_mis_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A, double q)
{
    using TP = GridTrT<TL>;
    HeteroMisSteps<LM, TL> st{TP::template load<LM>(P.grid), q};
    stage_grid_lds<LM>(st.tp.G);
    wave_accum(P, S, A, st);
}

#elif VPT_GA_FAMILY == 3

template <bool LM, bool TL>
__global__ __launch_bounds__(256, 2) void grid_accum_chroma_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A,
                                                                   ChromaCoef c)
{
    using TP = GridChromaTr<TL>;
    HeteroChromaSteps<LM, TL> st{TP::template load<LM>(P.grid, c)};
    stage_grid_lds<LM>(st.tp.G);
    wave_accum(P, S, A, st);
}

#elif VPT_GA_FAMILY == 4

template <bool TL>
__global__ __launch_bounds__(256, 2) void grid_accum_residual_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A)
{
    using TP = GridResidualTr<TL>;
    HeteroSteps<true, TL, TP, false> st{TP::template load<true>(P.grid)};
    stage_grid_control_lds(st.tp.G, st.tp.ctl);
    wave_accum(P, S, A, st);
}

#else

template <bool LM, bool TL>
__global__ __launch_bounds__(256, 2) void grid_accum_spectral_kernel(KParams P, const DevScene* __restrict__ S, GridAccum A,
                                                                     ChromaCoef c)
{
    using TP = GridSpectralTr<LM, TL>;
    HeteroSpectralSteps<LM, TL> st{TP::template load<LM>(P.grid, c)};
    stage_grid_lds<LM>(st.tp.G);
    wave_accum(P, S, A, st);
}

#endif

}  // namespace vpt

using namespace vpt;

namespace {

constexpr bool TLU = VPT_HETERO_TL != 0;  /* the unit's value of TL */
#if VPT_GA_FAMILY == 0
constexpr bool EMU = VPT_HETERO_EM != 0;  /* and of EM */
#endif

/* vpt_persistent_launch (vpt_hetero_launch.h) with the clamp on the listed tiles, not the shard's: a pass over three
 * tiles is one workgroup.  x: the kernel's arguments behind (K, S, A) */
template <class Kern, class... X>
int pass_launch(Kern kern, const char* name, int device, const KParams& K, const DevScene* S, const GridAccum& A, void* stream,
                const X&... x)
{
    int blocks = 0;
    hipError_t e = vpt_resident_blocks(kern, 256, device, &blocks);
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", name, hipGetErrorString(e));
    const int need = (int)((A.n_list + 3u) / 4u);  /* 4 waves per block, one tile per wave to start */
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    kern<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(K, S, A, x...);
    e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return (int)VPT_OK;
}

}  // namespace

#if VPT_GA_FAMILY == 0
int VPT_HX(vpt_int_grid_accum_hetero)(int device, const KParams& K, const DevScene* S, const GridAccum& A,
                                      const vpt_hetero_args& a, void* stream)
{
    return with_flags([&](auto lmc, auto ratio) {
        constexpr bool LM = decltype(lmc)::value;
        if constexpr (decltype(ratio)::value)
            return pass_launch(grid_accum_ratio_kernel<LM, TLU, EMU>, "grid_accum_ratio_kernel", device, K, S, A, stream);
        else
            return pass_launch(grid_accum_kernel<LM, TLU, EMU>, "grid_accum_kernel", device, K, S, A, stream);
    }, a.lm, K.est == VPT_HETERO_RATIO);
}
#elif VPT_GA_FAMILY == 1
int VPT_HX(vpt_int_grid_accum_eqa)(int device, const KParams& K, const DevScene* S, const GridAccum& A, const vpt_hetero_args&,
                                   void* stream)
{
    return pass_launch(grid_accum_eqa_kernel<TLU>, "grid_accum_eqa_kernel", device, K, S, A, stream);
}
#elif VPT_GA_FAMILY == 2
int VPT_HX(vpt_int_grid_accum_mis)(int device, const KParams& K, const DevScene* S, const GridAccum& A, const vpt_hetero_args& a,
                                   void* stream)
{
    return with_flags([&](auto lmc) {
        return pass_launch(grid_accum_mis_kernel<decltype(lmc)::value, TLU>, "grid_accum_mis_kernel", device, K, S, A, stream, a.q);
    }, a.lm);
}
#elif VPT_GA_FAMILY == 3
int VPT_HX(vpt_int_grid_accum_chroma)(int device, const KParams& K, const DevScene* S, const GridAccum& A,
                                      const vpt_hetero_args& a, void* stream)
{
    return with_flags([&](auto lmc) {
        return pass_launch(grid_accum_chroma_kernel<decltype(lmc)::value, TLU>, "grid_accum_chroma_kernel", device, K, S, A, stream, a.c);
    }, a.lm);
}
#elif VPT_GA_FAMILY == 4
int VPT_HX(vpt_int_grid_accum_residual)(int device, const KParams& K, const DevScene* S, const GridAccum& A,
                                        const vpt_hetero_args&, void* stream)
{
    return pass_launch(grid_accum_residual_kernel<TLU>, "grid_accum_residual_kernel", device, K, S, A, stream);
}
#else
int VPT_HX(vpt_int_grid_accum_spectral)(int device, const KParams& K, const DevScene* S, const GridAccum& A,
                                        const vpt_hetero_args& a, void* stream)
{
    return with_flags([&](auto lmc) {
        return pass_launch(grid_accum_spectral_kernel<decltype(lmc)::value, TLU>, "grid_accum_spectral_kernel", device, K, S, A, stream, a.c);
    }, a.lm);
}
#endif
