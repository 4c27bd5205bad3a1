/*
 * vpt_wave_accum.h -- the persistent-wave render loop of vpt_wave.h, continued: the render kernel of the grid
 * accumulator (vpt_accum_create_grid, vpt_accum.hip), instantiated by vpt_grid_accum.hip on the steps objects of the
 * estimators 10 to 16.
 *
 * wave_render (vpt_wave.h) starts a pixel at acc = 0, i = 0, runs samples [0, spp) and stores acc / spp.  wave_accum
 * starts a pixel at acc = sum[pixel], i = k0 C, runs samples [k0 C, (k0 + n) C) and stores acc back: k0 is the level
 * count of the pixel's tile in the accumulator's state, n the number of levels this pass adds to that tile.  Path
 * regeneration, the deferred surface / medium scheduling, the tile-ordered queue and the one atomic per wave are
 * wave_render's; so is the order of the sum (acc = L + acc over the pixel's samples, strictly in order), which is why a
 * pixel with m levels is the pixel of vpt_render(spp = mC) whatever passes brought the levels.
 *
 * What differs from wave_render:
 *   - the queue index q names entry q >> 6 of the pass's tile list (GridAccum::list; NULL: every tile in order), and the
 *     per-entry count nadd[q >> 6], so tiles at different level counts and with different numbers of levels to add are
 *     one launch;
 *   - beside acc the lane keeps the chunk sum c = L + c of the current level; when the pixel's sample count reaches a
 *     multiple of C, the level's luminance y = vpt_accum_lum(c) is folded into the state in memory, s1 = y + s1 and
 *     s2 = y*y + s2 (vpt_accum_level's lines), and c starts again at zero.  s1 and s2 live in memory, not in registers:
 *     a boundary comes once per C samples, and the loop carries 6 + 1 live VGPRs more than wave_render (c and the
 *     boundary's sample index) instead of 10 + 1 ("The grid accumulator", has the resource table);
 *   - lanes in the padding of an edge tile take no pixel, as in wave_render, so they read and write no state;
 *   - the kernel does not write the tiles' level counts or errors: the tail kernel (grid_tail_kernel,
 *     vpt_grid_tail.hip) does, after this one in stream order.
 *
 * The loop is a copy of wave_render's, not a shared body: a shared body moves the code of the existing kernels
 * ("Why the persistent-wave kernels are not shared").  The copy is debt, named in DESIGN.md section 8.
 */
#ifndef VPT_WAVE_ACCUM_H
#define VPT_WAVE_ACCUM_H

#include "vpt_render_simple.h"
#include "vpt_accum.h"

namespace vpt {

/* a pass of the grid accumulator: the kernel's argument behind (KParams, scene) and before the estimator's own */
struct GridAccum {
    int32_t C;              /* samples per level */
    uint32_t n_list;        /* tiles of this pass */
    const uint32_t* list;   /* their numbers (row-major over the shard), or NULL: tiles 0 .. n_list - 1 */
    const int32_t* nadd;    /* per list entry: levels to add (> 0) */
    const int32_t* levels;  /* per tile of the shard: levels held (read only here) */
    double* sum;            /* rows * w * 3 */
    double* s12;            /* rows * w * 2 */
};

template <class Steps>
__device__ __forceinline__ void wave_accum(const KParams& P, const DevScene* __restrict__ S, const GridAccum& A, const Steps& st)
{
    constexpr bool COUNT = false;
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    const Medium m = medium_of(P);
    const dv3 o0 = mk(P.o[0], P.o[1], P.o[2]);
    const unsigned npix = A.n_list * 64u;

    int x = 0, y = 0, lr = 0;
    uint64_t idx = 0;
    int i = 0;                 /* next sample to start */
    int iend = 0;              /* the end of the pixel's range */
    int ifold = 0;             /* the end of the current level */
    bool done = false, need_pixel = true, in_path = false;
    int pending = EV_END;
    dv3 acc = mk(0, 0, 0);     /* the pixel's sum */
    dv3 c = mk(0, 0, 0);       /* the current level's */
    Path p;
    Event e;
    e.pdf = 0;
    Sampler<COUNT> smp;
    smp.X = 0;
    smp.g = P.g;
    smp.cnt.tests = 0;
    smp.cnt.iterations = 0;
    smp.cnt.draw_mismatch = 0;

    /* a path has ended: its radiance into the pixel's sum and the level's; at the level's last sample the fold */
    auto path_end = [&]() {
        acc = add(p.L, acc);  /* src/rt.cpp:794 */
        c = add(p.L, c);
        if (i == ifold) {  /* i samples of the pixel have been started, and this was the last of them */
            const size_t px = (size_t)lr * (size_t)P.w + (size_t)x;
            const double yl = vpt_accum_lum(c.x, c.y, c.z);
            A.s12[2 * px] = yl + A.s12[2 * px];
            A.s12[2 * px + 1] = yl * yl + A.s12[2 * px + 1];
            c = mk(0, 0, 0);
            ifold += A.C;
        }
        in_path = false;
    };

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
                    const unsigned li = q >> 6, within = q & 63u;
                    const unsigned tile = A.list ? A.list[li] : li;
                    x = (int)(tile % (unsigned)P.tiles_x) * 8 + (int)(within & 7u);
                    lr = (int)(tile / (unsigned)P.tiles_x) * 8 + (int)(within >> 3);
                    if (x < P.w && lr < P.shard_rows) {
                        const PixelRow row = pixel_row(P, x, lr);
                        const size_t px = (size_t)lr * (size_t)P.w + (size_t)x;
                        y = row.y;
                        idx = row.idx;
                        i = A.levels[tile] * A.C;
                        iend = i + A.nadd[li] * A.C;
                        ifold = i + A.C;
                        acc = mk(A.sum[3 * px], A.sum[3 * px + 1], A.sum[3 * px + 2]);
                        c = mk(0, 0, 0);
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
                    if (i == iend) {
                        const size_t px = (size_t)lr * (size_t)P.w + (size_t)x;
                        A.sum[3 * px] = acc.x;
                        A.sum[3 * px + 1] = acc.y;
                        A.sum[3 * px + 2] = acc.z;
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
                    path_end();
                    continue;
                }
                const int ev = st.decide(S, smp, p, e, m);
                if (ev == EV_END) {
                    path_end();
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
}

}  // namespace vpt

#endif
