/*
 * vpt_hetero_simple.h -- the two reference kernels of the density-grid units (estimators 10 to 16), each stated once as
 * a body that takes the estimator as a callable  est(Sampler<COUNT>& smp, dv3 o, dv3 dir, const Medium& m) -> dv3:
 *
 *   hetero_simple_render: render_kernel_simple's one-lane-per-pixel loop (vpt_render_simple.h says what it replaces).
 *   Every unit's render_kernel_simple_<unit> loads its policy once and calls this with a lambda on its trace_hetero*.
 *
 *   hetero_trace_one: one lane of a unit's per-sample call (vpt_trace_batch), the trace_batch_hetero*_kernel of the unit.
 *
 * These are the bit-exact reference path (VPT_SIMPLE_KERNEL=1, vpt_count_work, vpt_trace_batch): nothing times them.  The
 * loop of estimators 0 to 9 stays in vpt_render_simple.h and the persistent-wave kernels keep their own three lines
 * each: routed through a common body their code moves ("One simple loop, one per-sample body").
 */
#ifndef VPT_HETERO_SIMPLE_H
#define VPT_HETERO_SIMPLE_H

#include "vpt_render_simple.h"

namespace vpt {

/* one lane owns one pixel and runs its spp camera samples through est, accumulating in FP64 in the reference's order,
 * then writes the average once; counting mode adds the lane's totals to P.counters */
template <bool COUNT, int FB, class Est>
__device__ __forceinline__ void hetero_simple_render(const KParams& P, Est est)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int lr = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
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
        const dv3 L = est(smp, o, dir, m);
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

/* lane i of a per-sample call: the ray's sample from its 48-bit state through est, the radiance and the state behind it */
template <class Est>
__device__ __forceinline__ void hetero_trace_one(int i, const vpt_ray* __restrict__ rays, const uint64_t* __restrict__ states,
                                                 int n, const Medium& m, double* out, uint64_t* out_states, Est est)
{
    if (i >= n) return;
    Sampler<false> smp;
    smp.X = states[i] & 0xFFFFFFFFFFFFull;
    smp.g = m.g;
    const dv3 L = est(smp, ld3(rays[i].o), ld3(rays[i].d), m);
    out[3 * i] = L.x;
    out[3 * i + 1] = L.y;
    out[3 * i + 2] = L.z;
    out_states[i] = smp.X;
}

}  // namespace vpt

#endif
