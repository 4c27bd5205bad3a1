/*
 * vpt_grid_build.h -- the block maxima and minima of a density grid (vpt_grid.h: local majorants, the control grid of
 * residual ratio tracking) stated per output, as a gather.  Written once and compiled for the host (vpt_host.cpp:
 * vpt_grid_majorant_gather_host) and the device (vpt_grid_build.hip), as the walkers are.
 *
 * vpt_grid_majorant_control_build (vpt_grid.h) is a scatter: it visits the voxels in ascending z, then y, then x order and
 * lets every voxel update the blocks it counts for, a maximum from +0.0f under strict >, a minimum from +INFINITY under
 * strict <.  So a block's maximum is the first voxel of its box, in that order, that no other voxel of the box exceeds
 * (or the +0.0f it started from), and its minimum the first voxel that none falls below: among values that compare equal
 * -- +0.0 and -0.0 -- the earlier one stays.  The contract here is bit identity with that build for every input.
 *
 * The box of block b of an axis of k voxels is [bB, min((b + 1)B, k) - 1], under the trilinear field widened by one voxel
 * on each side and held to [0, k - 1] (vpt_gb_range).  A box is a product of three ranges, and "the first in z, y, x
 * order among equals" is "the first z, there the first y, there the first x": the reduction is separable.  Two passes:
 *   X   per row (z, y) and block bx: the row's voxels of bx's range, ascending x          -> sx[z][y][bx], maxima and minima
 *   YZ  per block (bz, by, bx): sx[z][y][bx] over bz's and by's ranges, ascending z, then y -> the nbv maxima and, directly
 *       behind them, the nbv minima
 * each a scan from +0.0f under strict > (maxima, of voxels and then of maxima) and from +INFINITY under strict < (minima).
 *
 * A scan may be split over `step` lanes, lane `first` taking the elements first, first + step, ... of the range in ascending
 * order (the host: first 0, step 1, the whole range).  A lane's minimum comes with the position of the element it took it
 * from, and two lanes' results are combined by vpt_gb_min_join: the smaller value, and of two that compare equal the one
 * with the lower position -- so the joined result is the serial scan's bit for bit, in whatever order lanes are joined.
 * The maxima need no position: joined under strict > as well, they differ from the serial scan only where a -0.0 meets a
 * +0.0 that is not the initial one, and a scan that starts from +0.0f never takes a -0.0.
 */
#ifndef VPT_GRID_BUILD_H
#define VPT_GRID_BUILD_H

#include <math.h>
#include <stdint.h>

#include "vpt_grid.h"

/* the voxels [*i0, *i1] of block b of an axis of k voxels (header comment) */
VPT_GR void vpt_gb_range(int32_t k, int32_t B, int tl, int32_t b, int32_t* i0, int32_t* i1)
{
    const int64_t a = (int64_t)b * B, e = a + B < (int64_t)k ? a + B - 1 : (int64_t)k - 1;  /* B may be 2^31 - 1 */
    *i0 = (int32_t)(tl && a > 0 ? a - 1 : a);
    *i1 = (int32_t)(tl && e + 1 < (int64_t)k ? e + 1 : e);
}

/* a running maximum, minimum and the position the minimum was taken from (-1: none yet) */
typedef struct vpt_gb_acc {
    float mx, mn;
    int64_t at;
} vpt_gb_acc;

VPT_GR void vpt_gb_acc_init(vpt_gb_acc* A)
{
    A->mx = 0.0f;
    A->mn = INFINITY;
    A->at = -1;
}

/* one element of a scan: a candidate maximum vmax and a candidate minimum vmin at position `at` (ascending per lane) */
VPT_GR void vpt_gb_acc_step(vpt_gb_acc* A, float vmax, float vmin, int64_t at)
{
    if (vmax > A->mx) A->mx = vmax;
    if (vmin < A->mn) {
        A->mn = vmin;
        A->at = at;
    }
}

/* A joined with another lane's result (header comment) */
VPT_GR void vpt_gb_acc_join(vpt_gb_acc* A, float mx, float mn, int64_t at)
{
    if (mx > A->mx) A->mx = mx;
    if (at >= 0 && (A->at < 0 || mn < A->mn || (mn == A->mn && at < A->at))) {
        A->mn = mn;
        A->at = at;
    }
}

/* pass X: lane `first` of `step` over the voxels [i0, i1] of a row */
VPT_GR void vpt_gb_scan_x(const float* row, int32_t i0, int32_t i1, int32_t first, int32_t step, vpt_gb_acc* A)
{
    vpt_gb_acc_init(A);
    for (int64_t x = (int64_t)i0 + first; x <= (int64_t)i1; x += step) vpt_gb_acc_step(A, row[x], row[x], x - i0);
}

/* pass YZ: lane `first` of `step` over the rows (z, y), z in [z0, z1] and y in [y0, y1], in ascending z, then y order, of
 * column bx of the row maxima sxmax and the row minima sxmin (nz x ny x nbx each) */
VPT_GR void vpt_gb_scan_yz(const float* sxmax, const float* sxmin, int32_t ny, int32_t nbx, int32_t bx, int32_t z0, int32_t z1,
                           int32_t y0, int32_t y1, int64_t first, int64_t step, vpt_gb_acc* A)
{
    vpt_gb_acc_init(A);
    const int64_t ly = (int64_t)y1 - y0 + 1, len = ((int64_t)z1 - z0 + 1) * ly;
    for (int64_t k = first; k < len; k += step) {
        const int64_t z = z0 + k / ly, y = y0 + k % ly;
        const int64_t at = (z * ny + y) * nbx + bx;
        vpt_gb_acc_step(A, sxmax[at], sxmin[at], k);
    }
}

#endif
