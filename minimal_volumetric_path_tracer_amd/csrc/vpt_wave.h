/*
 * vpt_wave.h -- the persistent-wave render loop, shared by its kernels: the density-grid units' seven (hetero_kernel and
 * hetero_ratio_kernel in vpt_hetero.hip, hetero_eqa_kernel, hetero_mis_kernel, hetero_chroma_kernel, hetero_residual_kernel
 * and hetero_spectral_kernel in the units of estimators 12 to 16) and render_kernel (vpt_kernels.hip, the A/B path of
 * -DVPT_DEBUG_ENV=1 builds).
 *
 * Every lane owns one pixel at a time and runs that pixel's camera samples strictly in order (so the
 * per-pixel FP64 sum is the one-lane-per-pixel kernels', bit for bit), but the wave does not wait for its longest path:
 *   - path regeneration: a lane whose path ends starts its next sample at once;
 *   - a lane that finishes its pixel takes the next one from a device-wide queue (one atomic per
 *     wave, 8x8-tile order for coherent camera rays), so waves drain together at the very end;
 *   - deferred events: after the common part of an iteration (roulette, intersection, light and
 *     distance sampling) a lane holds a pending SURFACE or MEDIUM event; each round the wave runs
 *     only ONE of the two shading blocks -- the one with more lanes per unit of cost -- and the
 *     other lanes keep their event for a later round (no data moves, no divergence between the
 *     two blocks).  The image does not depend on that choice.
 *
 * Steps is the estimator: decide(S, smp, p, e, m) returns EV_END, EV_SURF or EV_MED, and surface / medium
 * (S, smp, p, e, m) run the pending event.
 */
#ifndef VPT_WAVE_H
#define VPT_WAVE_H

#include "vpt_render_simple.h"

namespace vpt {

/* the estimators 0-9 of vpt_device.h */
template <int EST>
struct EstSteps {
    template <bool COUNT>
    __device__ __forceinline__ int decide(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, Event& e,
                                          const Medium& m) const
    {
        return vpt::decide<EST>(S, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void surface(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                            const Medium& m) const
    {
        surface_event<EST>(S, smp, p, e, m);
    }
    template <bool COUNT>
    __device__ __forceinline__ void medium(const DevScene* __restrict__ S, Sampler<COUNT>& smp, Path& p, const Event& e,
                                           const Medium& m) const
    {
        medium_event<EST>(S, smp, p, e, m);
    }
};

template <class Steps, bool COUNT, int FB>
__device__ __forceinline__ void wave_render(const KParams& P, const DevScene* __restrict__ S, const Steps& st)
{
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    const Medium m = medium_of(P);
    const dv3 o0 = mk(P.o[0], P.o[1], P.o[2]);
    const unsigned npix = (unsigned)P.tiles_x * (unsigned)P.tiles_y * 64u;

    int x = 0, y = 0, lr = 0;
    uint64_t idx = 0;
    int i = 0;                 /* next sample to start */
    bool done = false, need_pixel = true, in_path = false;
    int pending = EV_END;
    dv3 acc = mk(0, 0, 0);
    Path p;
    Event e;
    e.pdf = 0;
    Sampler<COUNT> smp;
    smp.X = 0;
    smp.g = P.g;
    smp.cnt.tests = 0;
    smp.cnt.iterations = 0;
    smp.cnt.draw_mismatch = 0;

    while (true) {
        /* (1) converged: lanes without a pixel take the next ones from the queue */
        const uint64_t needm = __ballot(need_pixel && !done);
        if (needm) {
            const int leader = __ffsll((unsigned long long)needm) - 1;
            unsigned base = 0;
            if (lane == leader) base = atomicAdd(P.queue, (unsigned)__popcll(needm));
            base = __shfl(base, leader);
            if (need_pixel && !done) {
                const unsigned q = base + (unsigned)__popcll(needm & below);
                if (q >= npix) {
                    done = true;
                } else {
                    const unsigned tile = q >> 6, within = q & 63u;
                    x = (int)(tile % (unsigned)P.tiles_x) * 8 + (int)(within & 7u);
                    lr = (int)(tile / (unsigned)P.tiles_x) * 8 + (int)(within >> 3);
                    if (x < P.w && lr < P.shard_rows) {
                        const PixelRow row = pixel_row(P, x, lr);
                        y = row.y;
                        idx = row.idx;
                        i = 0;
                        acc = mk(0, 0, 0);
                        need_pixel = false;
                    }
                }
            }
        }
        if (__ballot(!done) == 0) break;

        /* (2) lanes without a pending event advance their path to the next event */
        if (!done && !need_pixel && pending == EV_END) {
            while (true) {
                if (!in_path) {
                    if (i == P.spp) {
                        store_pixel<FB>(P, x, lr, acc);
                        need_pixel = true;
                        break;
                    }
                    smp.X = vpt_stream_start(P.seed, idx, (uint64_t)i);
                    ++i;
                    p.o = o0;
                    p.d = camera_dir(P, smp, x, y);
                    p.beta = mk(1, 1, 1);
                    p.L = mk(0, 0, 0);
                    p.depth = 0;
                    in_path = true;
                }
                if (!continue_path(smp, p, m)) {
                    acc = add(p.L, acc);  /* src/rt.cpp:794 */
                    in_path = false;
                    continue;
                }
                const int ev = st.decide(S, smp, p, e, m);
                if (ev == EV_END) {
                    acc = add(p.L, acc);
                    in_path = false;
                    continue;
                }
                pending = ev;
                break;
            }
        }

        /* (3) run one shading block: the one with more pending lanes per unit of cost */
        const int ns = __popcll(__ballot(pending == EV_SURF));
        const int nm = __popcll(__ballot(pending == EV_MED));
        if (ns + nm == 0) continue;
        if (ns * P.cost_med >= nm * P.cost_surf) {
            if (pending == EV_SURF) {
                st.surface(S, smp, p, e, m);
                pending = EV_END;
            }
        } else {
            if (pending == EV_MED) {
                st.medium(S, smp, p, e, m);
                pending = EV_END;
            }
        }
    }
    if (COUNT) {
        atomicAdd(&P.counters[0], (unsigned long long)smp.cnt.tests);
        atomicAdd(&P.counters[1], (unsigned long long)smp.cnt.iterations);
    }
}

}  // namespace vpt

#endif
