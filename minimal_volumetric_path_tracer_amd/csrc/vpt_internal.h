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
/* an emission grid of nv voxels and its colour: finite and >= 0, else VPT_E_INVALID with its message (vpt_host.cpp) */
int vpt_int_emission_check(const float* eps, size_t nv, const double rgb[3], const char* who);

#endif
