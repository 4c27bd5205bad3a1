/*
 * vpt_accum.h -- the progressive accumulator's running statistic and refine policy.  Plain C, shared by
 * the accumulate kernel (vpt_accum.hip) and the host entry points vpt_accum_stat_host /
 * vpt_accum_select_host (vpt_host.cpp), so that the GPU and the host state it once.
 *
 * A pixel's samples arrive one chunk level at a time: level k is the sum of samples [kC, kC + C), formed
 * as acc = L + acc by the pool kernel (vpt_chunks.h, uniform layout).  Per pixel the accumulator keeps
 *   sum  the chunk sums added in level order, sum = c + sum   (reduce_kernel's add(chunk, tot))
 *   s1   the chunk luminances,                s1 = y + s1
 *   s2   their squares,                       s2 = y*y + s2
 * with y = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z.  Everything is FP64, without contraction, in exactly
 * this operation order; division and square root are the correctly rounded ones.
 *
 * After m levels the pixel's error is the standard error of the mean chunk luminance relative to the
 * mean, the mean floored at cfloor = (double)C * lum_floor (computed once on the host):
 *   m >= 2:  mean = s1 / m;  var = (s2 - s1*mean) / (m - 1), !(var > 0) -> 0;  se = sqrt(var / m);
 *            err = se / (mean > cfloor ? mean : cfloor)
 *   m <  2:  err = +inf
 * A NaN sample makes s1 and s2 NaN; var then clamps to 0 and the mean fails the floor test, so that pixel's
 * error is 0, not NaN.  A NaN error arises only as 0 / 0: a black pixel with lum_floor = 0.
 * A tile's error is the maximum over its valid pixels (a maximum does not depend on the order).  The
 * maximum is taken with vpt_accum_max below, which lets a NaN win: a tile with a NaN pixel error reports NaN.
 *
 * A tile is active for the next pass iff levels < max_levels && (levels < min_levels || err > target).
 * Written this way a NaN error makes a tile INACTIVE once it has min_levels (NaN > target is false):
 * more samples cannot repair a NaN sum, so the refine loop does not spend them.
 */
#ifndef VPT_ACCUM_H
#define VPT_ACCUM_H

#include <math.h>

/* the correctly rounded square root: sqrt() on the host, the device library's (vpt_math.h) in vpt_accum.hip */
#ifndef VPT_ACCUM_SQRT
#define VPT_ACCUM_SQRT sqrt
#endif

#ifdef __HIPCC__
#define VPT_AC __host__ __device__ static inline
#else
#define VPT_AC static inline
#endif

typedef struct {
    double sum[3];
    double s1, s2;
} vpt_accum_px;

VPT_AC double vpt_accum_lum(double cx, double cy, double cz) { return (0.2126 * cx + 0.7152 * cy) + 0.0722 * cz; }

/* one more chunk level (chunk sum c) of a pixel */
VPT_AC void vpt_accum_level(vpt_accum_px* a, double cx, double cy, double cz)
{
    const double y = vpt_accum_lum(cx, cy, cz);
    a->sum[0] = cx + a->sum[0];
    a->sum[1] = cy + a->sum[1];
    a->sum[2] = cz + a->sum[2];
    a->s1 = y + a->s1;
    a->s2 = y * y + a->s2;
}

/* the pixel's error after m levels; cfloor = (double)C * lum_floor */
VPT_AC double vpt_accum_err(double s1, double s2, int m, double cfloor)
{
    if (m < 2) return (double)INFINITY;
    const double mean = s1 / (double)m;
    double var = (s2 - s1 * mean) / (double)(m - 1);
    if (!(var > 0)) var = 0;
    const double se = VPT_ACCUM_SQRT(var / (double)m);
    const double den = mean > cfloor ? mean : cfloor;
    return se / den;
}

/* maximum in which a NaN wins (fmax would drop it) */
VPT_AC double vpt_accum_max(double a, double b) { return (a != a || a > b) ? a : b; }

VPT_AC int vpt_accum_active(int levels, double err, int min_levels, int max_levels, double target)
{
    return levels < max_levels && (levels < min_levels || err > target);
}

/* vpt_refine's fields: 0 when valid, else 1 target / lum_floor not finite or negative, 2 min_levels < 2,
 * 3 levels_per_pass <= 0 */
VPT_AC int vpt_accum_refine_bad(double target, double lum_floor, int min_levels, int levels_per_pass)
{
    if (!(target >= 0 && target - target == 0.0) || !(lum_floor >= 0 && lum_floor - lum_floor == 0.0)) return 1;
    if (min_levels < 2) return 2;
    if (levels_per_pass <= 0) return 3;
    return 0;
}

#endif
