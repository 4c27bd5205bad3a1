/*
 * vpt_render_simple.h -- a render's launch parameters (KParams) and the per-pixel helpers every render kernel but the
 * pool kernel uses (row mapping, camera ray, pixel store), for every unit; and render_kernel_simple, the one-lane-per-pixel
 * render kernel of estimators 0 to 9, which vpt_kernels.hip instantiates.  The density-grid units (estimators 10 to 16)
 * have that loop as a body of their own, hetero_simple_render (vpt_hetero_simple.h), so this header knows none of their
 * estimators and the code object of vpt_kernels.hip -- the tuned pool kernels and their placement -- stays what it was
 * before estimator 10 existed.  render_kernel_simple replaces main()'s OpenMP pixel loop (src/rt.cpp:767-805):
 * one lane owns one pixel and runs its spp camera samples (src/rt.cpp:786-798) through the estimator,
 * accumulating in FP64 in the reference's order, then writes the average (src/rt.cpp:800) once.
 */
#ifndef VPT_RENDER_SIMPLE_H
#define VPT_RENDER_SIMPLE_H

#include "vpt_device.h"

struct vpt_grid_view;  /* the density grid as the walkers see it (vpt_grid.h) */

namespace vpt {

struct KParams {
    int32_t w, h, spp, fb;
    int32_t band_rows, band_stride, band_offset, shard_rows;
    double sigma_a, sigma_s, g;
    int32_t max_depth, est;
    double march_step;             /* rayMarching3 (estimator 6) */
    int32_t march_light;
    uint64_t seed;
    double o[3], d[3], cx[3], cy[3];
    void* out;
    unsigned long long* counters;  /* counting mode: [tests, iterations] */
    unsigned* queue;               /* pixel work queue head (zeroed before each launch) */
    int32_t tiles_x, tiles_y;      /* 8x8 pixel tiles covering the shard */
    int32_t cost_surf, cost_med;   /* event scheduler weights */
    int32_t chunk;                 /* samples per partial sum (pool kernel) */
    int32_t taper;                 /* tapered chunk layout (auto mode, vpt_chunks.h) */
    const vpt_grid_view* grid;     /* estimators 10 to 16: the context's density grid (device), else NULL */
};

__host__ __device__ __forceinline__ Medium medium_of(const KParams& P)
{
    return Medium{P.sigma_a, P.sigma_s, P.g, P.max_depth, P.march_step, P.march_light};
}

/* where row lr of the shard lies in the image: the bands of band_rows rows are dealt out band_stride apart */
struct PixelRow {
    int fr, y;     /* file row, camera row */
    uint64_t idx;  /* the pixel's stream index, src/rt.cpp:773 */
};

__device__ __forceinline__ PixelRow pixel_row(const KParams& P, int x, int lr)
{
    const int k = lr / P.band_rows, r = lr - k * P.band_rows;
    const int fr = (P.band_offset + k * P.band_stride) * P.band_rows + r;
    return PixelRow{fr, P.h - 1 - fr, (uint64_t)fr * (uint64_t)P.w + (uint64_t)x};
}

/* camera ray of one sample, src/rt.cpp:787 (x draw first) */
template <bool COUNT>
__device__ __forceinline__ dv3 camera_dir(const KParams& P, Sampler<COUNT>& smp, int x, int y)
{
    const dv3 cd = mk(P.d[0], P.d[1], P.d[2]);
    const dv3 cx = mk(P.cx[0], P.cx[1], P.cx[2]), cy = mk(P.cy[0], P.cy[1], P.cy[2]);
    double jx = smp.next();
    double jy = smp.next();
    dv3 dir = add(add(scl(cx, (((double)x + jx - 0.5) / P.w - .5)), scl(cy, (((double)y + jy - 0.5) / P.h - .5))), cd);
    return nrm(dir);
}

/* the pixel's average (src/rt.cpp:800) into row lr of the shard's framebuffer */
template <int FB>
__device__ __forceinline__ void store_pixel(const KParams& P, int x, int lr, dv3 acc)
{
    acc = scl(acc, (1 / (double)P.spp));
    const size_t oi = ((size_t)lr * (size_t)P.w + (size_t)x) * 3;
    if (FB == VPT_FB_F32) {
        float* out = (float*)P.out;
        out[oi] = (float)acc.x;
        out[oi + 1] = (float)acc.y;
        out[oi + 2] = (float)acc.z;
    } else {
        double* out = (double*)P.out;
        out[oi] = acc.x;
        out[oi + 1] = acc.y;
        out[oi + 2] = acc.z;
    }
}

}  // namespace vpt

namespace {

using namespace vpt;

/* estimators 0 to 9 (the density-grid units: vpt_hetero_simple.h) */
template <int EST, bool COUNT, int FB>
__global__ __launch_bounds__(256) void render_kernel_simple(KParams P, const DevScene* __restrict__ S)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int lr = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    /* rayMarching3: every shadow ray leaves the light's centre, so oc and |oc|^2 of each sphere are
     * formed once per workgroup (round 3: 26.7 -> 32.4 Msamples/s) */
    __shared__ double march_oc[EST == 6 ? VPT_MAX_SPHERES : 1][4];
    if (EST == 6) {
        march_origin_init(S, sph_p(S, P.march_light), march_oc);
        __syncthreads();
    }
    if (x >= P.w || lr >= P.shard_rows) return;
    const PixelRow row = pixel_row(P, x, lr);
    const Medium m = medium_of(P);
    const dv3 o = mk(P.o[0], P.o[1], P.o[2]);
    dv3 acc = mk(0, 0, 0);
    uint64_t tests = 0, iters = 0, mism = 0;
    for (int i = 0; i < P.spp; ++i) {
        Sampler<COUNT> smp;
        smp.X = vpt_stream_start(P.seed, row.idx, (uint64_t)i);
        smp.g = P.g;
        smp.cnt.tests = 0;
        smp.cnt.iterations = 0;
        smp.cnt.draw_mismatch = 0;
        const dv3 dir = camera_dir(P, smp, x, row.y);
        const dv3 L = trace_sample<EST, COUNT>(S, smp, o, dir, m, EST == 6 ? march_oc : nullptr);
        acc = add(L, acc);
        if (COUNT) {
            tests += smp.cnt.tests;
            iters += smp.cnt.iterations;
            mism += smp.cnt.draw_mismatch;
        }
    }
    store_pixel<FB>(P, x, lr, acc);
    if (COUNT) {
        atomicAdd(&P.counters[0], (unsigned long long)tests);
        atomicAdd(&P.counters[1], (unsigned long long)iters);
        if (mism) atomicAdd(&P.counters[2], (unsigned long long)mism);
    }
}

}  // namespace

#endif
