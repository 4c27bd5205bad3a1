/* vpt_internal.h -- shared host-side helpers of libvpt (not part of the ABI). */
#ifndef VPT_INTERNAL_H
#define VPT_INTERNAL_H

#include <stddef.h>

#include "../../include/vpt.h"

/* records a thread-local message for vpt_last_error() and returns `code` */
int vpt_fail(int code, const char* fmt, ...);
void vpt_clear_error(void);

/* what the progressive accumulator (vpt_accum.hip) needs of a context (vpt_kernels.hip) */
int vpt_int_device(const vpt_context* ctx);
const unsigned* vpt_int_guard_flag(const vpt_context* ctx);   /* device address of PoolParams::guard's flag */
int vpt_int_check_guard(vpt_context* ctx, const char* who);   /* after a synchronisation */
int vpt_int_check_params(const vpt_context* ctx, const vpt_params* p);  /* build_kparams' validation */
int vpt_int_pool_pass(vpt_context* ctx, const vpt_params* p, int C, int k0, int k1, const unsigned* d_tiles,
                      unsigned n_tiles, double* d_partials, unsigned* d_queue);
/* the grid accumulator's pass (estimators 10 to 16): d_nadd[i] more levels of C samples for tile d_list[i] (NULL: the
 * shard's tiles in order), continued from d_levels into d_sum / d_s12; validates as vpt_render does */
int vpt_int_grid_pass(vpt_context* ctx, const vpt_params* p, int C, const unsigned* d_list, const int* d_nadd,
                      unsigned n_tiles, const int* d_levels, double* d_sum, double* d_s12, unsigned* d_queue);
/* its tail (vpt_grid_tail.hip), after the pass in stream order: per listed tile the error at levels[tile] + d_nadd[i]
 * levels from d_s12 (cfloor = (double)C * lum_floor), into d_err[tile], and d_levels[tile] += d_nadd[i] */
int vpt_int_grid_tail(int w, int rows, int tiles_x, const unsigned* d_list, const int* d_nadd, unsigned n_tiles,
                      const double* d_s12, double cfloor, int* d_levels, double* d_err);

/* the pool kernel's camera table for origin o: (o - centre, |o - centre|^2) of n spheres, centres `stride`
 * doubles apart (vpt_host.cpp) */
void vpt_int_cam_table(const double* o, const double* centre, size_t stride, int n, double (*oc)[4]);

/* vpt_grid_bad's verdict on a grid as a vpt_status with its message (vpt_host.cpp) */
int vpt_int_grid_check(const vpt_grid_desc* desc, const float* density, const char* who);
/* a verdict of vpt_grid_bad (0 .. 3) on desc's grid as a vpt_status with vpt_int_grid_check's message (vpt_host.cpp) */
int vpt_int_grid_verdict(const vpt_grid_desc* desc, int verdict, const char* who);
/* an emission grid of nv voxels and its colour: finite and >= 0, else VPT_E_INVALID with its message (vpt_host.cpp) */
int vpt_int_emission_check(const float* eps, size_t nv, const double rgb[3], const char* who);
/* its verdict on a bad voxel: VPT_E_INVALID with the message that names the voxel and its value (vpt_host.cpp) */
int vpt_int_emission_bad(double value, size_t voxel, const char* who);

/* ---- grids from device memory (vpt_grid_build.hip); both return a hipError_t's value (0: success), enqueue on the
 * current device's default stream and return once their result is there ---- */
/* the check and the maximum of nv voxels in device memory: *vmax the largest voxel (from +0.0f under strict >, the host's
 * rho_max scan) and *bad the lowest linear index of a voxel that is NaN, negative or infinite (vpt_grid_bad's
 * predicate), -1 where there is none */
int vpt_int_grid_scan(const float* d_v, long long nv, float* vmax, long long* bad);
/* vpt_grid_majorant_control_build's 2 nbv floats (vpt_grid.h) for the voxels d_rho of an n[0] x n[1] x n[2] grid, into
 * d_out, bit for bit (vpt_grid_build.h) */
int vpt_int_grid_build(const int* n, int B, int tl, const float* d_rho, float* d_out);

#endif
