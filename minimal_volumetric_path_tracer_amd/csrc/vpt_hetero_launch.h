/*
 * vpt_hetero_launch.h -- the host side of a launch, shared by the density-grid units (vpt_hetero.hip, vpt_hetero_eqa.hip
 * and the units that include them) and vpt_kernels.hip.  Host code only: it names kernels and launches them, and holds
 * no __global__ or __device__ function, so including it leaves a unit's code object what it was.
 */
#ifndef VPT_HETERO_LAUNCH_H
#define VPT_HETERO_LAUNCH_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "vpt_render_simple.h"
#include "vpt_internal.h"

/* run-time flags as compile-time constants: f(std::bool_constant<flag>{}...) */
template <class F>
static int with_flags(F f)
{
    return f();
}
template <class F, class... Bools>
static int with_flags(F f, bool flag, Bools... rest)
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

/* a persistent-wave kernel on as many workgroups as the device holds, clamped as above; `name` stands in the message */
static int vpt_persistent_launch(void (*kern)(vpt::KParams, const DevScene*), const char* name, int device,
                                 const vpt::KParams& K, const DevScene* S, void* stream)
{
    int blocks = 0;
    hipError_t e = vpt_resident_blocks(kern, 256, device, &blocks);
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", name, hipGetErrorString(e));
    kern<<<dim3((unsigned)vpt_wave_blocks(blocks, K)), dim3(256), 0, (hipStream_t)stream>>>(K, S);
    e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s launch: %s", name, hipGetErrorString(e));
    return (int)VPT_OK;
}

/* render_kernel_simple<EST> (vpt_render_simple.h), one lane per pixel: counting mode (K.counters != NULL) and
 * VPT_SIMPLE_KERNEL=1 */
template <int EST, bool LM, bool TL, bool EM>
static int vpt_simple_launch(const vpt::KParams& K, const DevScene* S, void* stream)
{
    return with_flags([&](auto count, auto f32) {
        constexpr int FB = decltype(f32)::value ? VPT_FB_F32 : VPT_FB_F64;
        dim3 grid((unsigned)((K.w + 15) / 16), (unsigned)((K.shard_rows + 15) / 16));
        render_kernel_simple<EST, decltype(count)::value, FB, LM, TL, EM><<<grid, dim3(256), 0, (hipStream_t)stream>>>(K, S);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "render_kernel_simple<%d> launch: %s", EST, hipGetErrorString(e));
        return (int)VPT_OK;
    }, K.counters != nullptr, K.fb == VPT_FB_F32);
}

#endif
