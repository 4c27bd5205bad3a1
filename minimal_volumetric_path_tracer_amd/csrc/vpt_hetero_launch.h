/*
 * vpt_hetero_launch.h -- the host side of a launch, shared by the seven density-grid units (vpt_hetero.hip for estimators
 * 10 and 11, vpt_hetero_eqa.hip, vpt_hetero_mis.hip, vpt_hetero_chroma.hip, vpt_hetero_residual.hip, vpt_hetero_spectral.hip
 * for 12 to 16, and the _tl / _em units that include them) and vpt_kernels.hip.  Host code only: it names kernels and
 * launches them, and holds no __global__ or __device__ function, so including it leaves a unit's code object what it was
 * (what the units share on the device is vpt_hetero_lds.h's and vpt_hetero_simple.h's).
 */
#ifndef VPT_HETERO_LAUNCH_H
#define VPT_HETERO_LAUNCH_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "vpt_render_simple.h"
#include "vpt_internal.h"

/* run-time flags as compile-time constants: f(std::bool_constant<flag>{}...), whatever f returns */
template <class F>
static auto with_flags(F f)
{
    return f();
}
template <class F, class... Bools>
static auto with_flags(F f, bool flag, Bools... rest)
{
    if (flag) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

/* one lane per ray: the grid of the per-sample calls and the probes, in workgroups of 256 */
static inline dim3 vpt_ray_grid(int n) { return dim3((unsigned)((n + 255) / 256)); }

/* the workgroups of `threads` lanes the device holds of kern at once: occupancy x CUs, at least one per CU */
template <class Kern>
static hipError_t vpt_resident_blocks(Kern kern, int threads, int device, int* blocks)
{
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess) *blocks = (per_cu < 1 ? 1 : per_cu) * cus;
    return e;
}

/* the clamp of a persistent-wave launch (vpt_wave.h): at most one workgroup per four tiles, at least one */
static inline int vpt_wave_blocks(int blocks, const vpt::KParams& K)
{
    const int need = (K.tiles_x * K.tiles_y + 3) / 4;  /* 4 waves per block, one tile per wave to start */
    if (blocks > need) blocks = need;
    return blocks < 1 ? 1 : blocks;
}

/* a persistent-wave kernel on as many workgroups as the device holds, clamped as above; `name` stands in the message.
 * a: the kernel's arguments behind (K, S) -- none, estimator 13's track fraction, estimator 14's and 16's coefficients */
template <class Kern, class... A>
static int vpt_persistent_launch(Kern kern, const char* name, int device, const vpt::KParams& K, const DevScene* S,
                                 void* stream, const A&... a)
{
    int blocks = 0;
    hipError_t e = vpt_resident_blocks(kern, 256, device, &blocks);
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", name, hipGetErrorString(e));
    kern<<<dim3((unsigned)vpt_wave_blocks(blocks, K)), dim3(256), 0, (hipStream_t)stream>>>(K, S, a...);
    e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return (int)VPT_OK;
}

/* kern: a unit's render_kernel_simple_<unit> of K.est (the body: vpt_hetero_simple.h), one lane per pixel: counting mode
 * (K.counters != NULL) and VPT_SIMPLE_KERNEL=1; a: as above */
template <class... A>
static int vpt_simple_launch(void (*kern)(vpt::KParams, const DevScene*, A...), const vpt::KParams& K, const DevScene* S,
                             void* stream, const A&... a)
{
    dim3 grid((unsigned)((K.w + 15) / 16), (unsigned)((K.shard_rows + 15) / 16));
    kern<<<grid, dim3(256), 0, (hipStream_t)stream>>>(K, S, a...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "render_kernel_simple<%d> launch: %s", (int)K.est, hipGetErrorString(e));
    return (int)VPT_OK;
}

#endif
