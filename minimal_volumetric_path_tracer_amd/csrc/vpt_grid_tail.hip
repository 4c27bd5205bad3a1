/*
 * vpt_grid_tail.hip -- the grid accumulator's tail kernel (vpt_accum_create_grid, vpt_accum.hip): accum_kernel's second
 * half.  It runs after the render kernel of a pass (wave_accum, vpt_wave_accum.h) in stream order, one wave per listed
 * tile and one lane per pixel: the pixels' errors at the tile's new level count (vpt_accum_err on s1, s2, which the render
 * kernel has folded), the tile's maximum in which a NaN wins, then err[tile] and levels[tile] += nadd[entry].  The render
 * kernel reads the level counts and does not write them, so a tile's count changes once per pass, here.
 *
 * A unit of its own: a kernel added to vpt_accum.hip moves the labels of resolve_kernel, and that code object is to stay
 * what it was.
 */
#include <hip/hip_runtime.h>

#include <math.h>

#include "vpt_math.h"
#define VPT_ACCUM_SQRT vm_sqrt /* the device code's correctly rounded square root */
#include "vpt_accum.h"
#include "vpt_internal.h"

namespace {

struct TailParams {
    int w, rows, tiles_x;
    unsigned n_list;
    const unsigned* list;  /* the pass's tiles */
    const int* nadd;       /* per list entry: the levels the pass added */
    const double* s12;     /* rows * w * 2 */
    double cfloor;         /* (double)C * lum_floor */
    int* levels;           /* per tile */
    double* err;           /* per tile */
};

__global__ __launch_bounds__(256) void grid_tail_kernel(TailParams A)
{
    const int lane = threadIdx.x & 63;
    const unsigned li = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (li >= A.n_list) return;  /* wave-uniform */
    const unsigned tile = A.list[li];
    const int ty = (int)(tile / (unsigned)A.tiles_x), tx = (int)(tile - (unsigned)ty * (unsigned)A.tiles_x);
    const int x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
    const bool valid = x < A.w && lr < A.rows;  /* lanes in the padding of an edge tile take no part */
    const int m = A.levels[tile] + A.nadd[li];
    double e = -(double)INFINITY;
    if (valid) {
        const size_t p = (size_t)lr * (size_t)A.w + (size_t)x;
        e = vpt_accum_err(A.s12[2 * p], A.s12[2 * p + 1], m, A.cfloor);
    }
    /* the tile's maximum (a NaN wins); the value does not depend on the order */
    for (int d = 32; d >= 1; d >>= 1) e = vpt_accum_max(e, __shfl_xor(e, d));
    if (lane == 0) {
        A.err[tile] = e;
        A.levels[tile] = m;
    }
}

}  // namespace

int vpt_int_grid_tail(int w, int rows, int tiles_x, const unsigned* d_list, const int* d_nadd, unsigned n_tiles,
                      const double* d_s12, double cfloor, int* d_levels, double* d_err)
{
    const TailParams A{w, rows, tiles_x, n_tiles, d_list, d_nadd, d_s12, cfloor, d_levels, d_err};
    grid_tail_kernel<<<dim3((n_tiles + 3u) / 4u), dim3(256), 0, nullptr>>>(A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "grid_tail_kernel launch: %s", hipGetErrorString(e));
    return VPT_OK;
}
