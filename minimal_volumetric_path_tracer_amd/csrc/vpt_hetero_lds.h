/*
 * vpt_hetero_lds.h -- what the persistent-wave kernels of the seven density-grid units (vpt_hetero.hip, vpt_hetero_eqa.hip,
 * vpt_hetero_mis.hip, vpt_hetero_chroma.hip, vpt_hetero_residual.hip, vpt_hetero_spectral.hip and the units that include
 * them) share on the device: the compile-time switches with their defaults, and the prologue that stages the grid in LDS.
 * Device code, unlike vpt_hetero_launch.h; the prologue is inlined into each kernel and leaves its code what it was
 * ("One LDS prologue").  The units' one-lane-per-pixel and per-sample kernels share vpt_hetero_simple.h.
 *
 * VPT_HETERO_LDS (1): a grid of at most 64 KiB (16 384 voxels) is staged in LDS once per workgroup; 0 reads every grid
 * from global memory.  VPT_HETERO_LDS_MAJ (1): with local majorants the majorant grid is staged in what the density
 * left of the budget -- all of it where the density does not fit (DESIGN.md section 4 has the timings that decided both
 * defaults).  VPT_HETERO_TL (0): the unit's value of the template parameter TL, and VPT_HX the suffix of what such a
 * unit exports.
 */
#ifndef VPT_HETERO_LDS_H
#define VPT_HETERO_LDS_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#ifndef VPT_HETERO_LDS
#define VPT_HETERO_LDS 1
#endif
#define VPT_HETERO_LDS_BYTES 65536
#ifndef VPT_HETERO_LDS_MAJ
#define VPT_HETERO_LDS_MAJ 1
#endif
#ifndef VPT_HETERO_TL
#define VPT_HETERO_TL 0
#endif
#if VPT_HETERO_TL
#define VPT_HX(name) name##_tl
#else
#define VPT_HX(name) name
#endif

namespace vpt {

/* The prologue of a persistent-wave kernel: G is the view inside the kernel's steps object, and every lane of the
 * workgroup calls this before the render loop.  The view lives in the steps object from the start: the walkers take its
 * address, so a copy made after the prologue is a second stack object (416 against 288 bytes of scratch, 9 against 4
 * spilled VGPRs in hetero_kernel).  LM: the grid has a majorant grid; estimator 12, where nothing tracks, passes false */
template <bool LM, class GV>
__device__ __forceinline__ void stage_grid_lds(GV& G)
{
#if VPT_HETERO_LDS
    __shared__ float lds_rho[VPT_HETERO_LDS_BYTES / sizeof(float)];
    const int64_t nv = (int64_t)G.n[0] * G.n[1] * G.n[2];
    if (nv <= (int64_t)(VPT_HETERO_LDS_BYTES / sizeof(float))) {  /* workgroup-uniform */
        for (int k = threadIdx.x; k < (int)nv; k += blockDim.x) lds_rho[k] = G.rho[k];
        __syncthreads();
        G.rho = lds_rho;
    }
#if VPT_HETERO_LDS_MAJ
    if (LM) {  /* the majorant grid goes into what the density left of the budget */
        const int64_t cap = (int64_t)(VPT_HETERO_LDS_BYTES / sizeof(float));
        const int64_t used = nv <= cap ? nv : 0;
        const int64_t nbv = (int64_t)G.nb[0] * G.nb[1] * G.nb[2];
        if (nbv <= cap - used) {  /* workgroup-uniform */
            for (int k = threadIdx.x; k < (int)nbv; k += blockDim.x) lds_rho[used + k] = G.maj[k];
            __syncthreads();
            G.maj = lds_rho + used;
        }
    }
#endif
#endif
}

/* The prologue of estimator 15's kernels (vpt_hetero_residual.hip), in stage_grid_lds's place: the same budget, with the
 * control grid beside the majorants.  ctl is the policy's own pointer to the block minima, taken from the view before
 * this runs (in global memory they lie directly behind the nbv majorants, vpt_grid.h, so the two arrays are one copy).
 * The density is staged where it fits, as above; the majorants and the minima go into what it left when that holds
 * both; else the majorants alone where they fit, as above, and the minima are read from global memory */
template <class GV>
__device__ __forceinline__ void stage_grid_control_lds(GV& G, const float*& ctl)
{
#if VPT_HETERO_LDS
    __shared__ float lds_rho[VPT_HETERO_LDS_BYTES / sizeof(float)];
    const int64_t cap = (int64_t)(VPT_HETERO_LDS_BYTES / sizeof(float));
    const int64_t nv = (int64_t)G.n[0] * G.n[1] * G.n[2];
    const int64_t used = nv <= cap ? nv : 0;
    if (used) {  /* workgroup-uniform, like every test below */
        for (int k = threadIdx.x; k < (int)nv; k += blockDim.x) lds_rho[k] = G.rho[k];
        G.rho = lds_rho;
    }
#if VPT_HETERO_LDS_MAJ
    const int64_t nbv = (int64_t)G.nb[0] * G.nb[1] * G.nb[2];
    if (2 * nbv <= cap - used) {
        for (int k = threadIdx.x; k < (int)(2 * nbv); k += blockDim.x) lds_rho[used + k] = G.maj[k];
        G.maj = lds_rho + used;
        ctl = lds_rho + used + nbv;
    } else if (nbv <= cap - used) {
        for (int k = threadIdx.x; k < (int)nbv; k += blockDim.x) lds_rho[used + k] = G.maj[k];
        G.maj = lds_rho + used;
    }
#endif
    __syncthreads();
#endif
}

}  // namespace vpt

#endif
