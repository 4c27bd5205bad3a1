/*
 * vpt_hetero.hip -- the render kernel of estimator 10 (VPT_HETERO_FREE, vpt_hetero.h) in a translation unit
 * of its own, as vpt_pool_mis.hip is for the north-star kernel: the hot loop here is null-collision
 * stepping through a voxel grid, latency-bound and divergent, not ray/sphere arithmetic, and the unit can
 * take compile flags of its own.
 *
 * hetero_kernel: persistent waves, the scheme of vpt_kernels.hip's render_kernel.  A lane owns one pixel and
 * runs that pixel's samples strictly in order (acc = L + acc, then * (1 / (double)spp)), so the image is
 * render_kernel_simple<10>'s bit for bit; a lane regenerates a path the moment one ends, and takes its next
 * pixel from a device-wide queue in 8x8-tile order (one atomic per wave).  After decide (intersection, light
 * pick, delta tracking) a lane holds a pending surface or medium event and the wave runs one of the two
 * shading blocks per round, the one more lanes wait for.
 *
 * Density reads: a grid of at most 64 KiB (16 384 voxels) is staged in LDS once per workgroup
 * (VPT_HETERO_LDS, on by default); a larger one is read from global memory, where the L2 holds the grids of
 * the tests and of the timing.  -DVPT_HETERO_LDS=0 reads every grid from global memory.  DESIGN.md section 4
 * has both timings (LDS won on the 16^3 grids by several times the run-to-run spread).  The 64 KiB do not lower
 * the occupancy: the registers already hold it at two workgroups per CU.
 */
#include <hip/hip_runtime.h>

#include <string.h>

#include "vpt_render_simple.h"
#include "vpt_internal.h"

#ifndef VPT_HETERO_LDS
#define VPT_HETERO_LDS 1
#endif
#define VPT_HETERO_LDS_BYTES 65536
/* with local majorants: the majorant grid is staged in what the density left of the LDS budget -- all of it
 * where the density does not fit (DESIGN.md section 4 has the timing that decided the default) */
#ifndef VPT_HETERO_LDS_MAJ
#define VPT_HETERO_LDS_MAJ 1
#endif

namespace vpt {

template <bool COUNT, int FB, bool LM>
__global__ __launch_bounds__(256, 2) void hetero_kernel(HeteroParams P, Medium m, const DevScene* __restrict__ S)
{
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    const dv3 o0 = mk(P.o[0], P.o[1], P.o[2]);
    const dv3 cd = mk(P.d[0], P.d[1], P.d[2]);
    const dv3 cx = mk(P.cx[0], P.cx[1], P.cx[2]), cy = mk(P.cy[0], P.cy[1], P.cy[2]);
    const unsigned npix = (unsigned)P.tiles_x * (unsigned)P.tiles_y * 64u;
    GridTr tp = GridTr::load<LM>(P.grid);
#if VPT_HETERO_LDS
    __shared__ float lds_rho[VPT_HETERO_LDS_BYTES / sizeof(float)];
    {
        const int64_t nv = (int64_t)tp.G.n[0] * tp.G.n[1] * tp.G.n[2];
        if (nv <= (int64_t)(VPT_HETERO_LDS_BYTES / sizeof(float))) {  /* workgroup-uniform */
            for (int k = threadIdx.x; k < (int)nv; k += blockDim.x) lds_rho[k] = tp.G.rho[k];
            __syncthreads();
            tp.G.rho = lds_rho;
        }
#if VPT_HETERO_LDS_MAJ
        if (LM) {  /* the majorant grid goes into what the density left of the budget */
            const int64_t cap = (int64_t)(VPT_HETERO_LDS_BYTES / sizeof(float));
            const int64_t used = nv <= cap ? nv : 0;
            const int64_t nbv = (int64_t)tp.G.nb[0] * tp.G.nb[1] * tp.G.nb[2];
            if (nbv <= cap - used) {  /* workgroup-uniform */
                for (int k = threadIdx.x; k < (int)nbv; k += blockDim.x) lds_rho[used + k] = tp.G.maj[k];
                __syncthreads();
                tp.G.maj = lds_rho + used;
            }
        }
#endif
    }
#endif

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
    smp.g = m.g;
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
                        const int k = lr / P.band_rows, r = lr - k * P.band_rows;
                        const int fr = (P.band_offset + k * P.band_stride) * P.band_rows + r; /* file row */
                        y = P.h - 1 - fr;                                                       /* camera row */
                        idx = (uint64_t)fr * (uint64_t)P.w + (uint64_t)x;                       /* src/rt.cpp:773 */
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
                        acc = scl(acc, (1 / (double)P.spp));  /* src/rt.cpp:800 */
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
                        need_pixel = true;
                        break;
                    }
                    smp.X = vpt_stream_start(P.seed, idx, (uint64_t)i);
                    ++i;
                    /* jittered camera ray, src/rt.cpp:787, x draw first */
                    const double jx = smp.next();
                    const double jy = smp.next();
                    const dv3 dir = add(add(scl(cx, (((double)x + jx - 0.5) / P.w - .5)), scl(cy, (((double)y + jy - 0.5) / P.h - .5))), cd);
                    p.o = o0;
                    p.d = nrm(dir);
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
                const int ev = hetero_decide<COUNT, LM>(S, tp, smp, p, e, m);
                if (ev == EV_END) {
                    acc = add(p.L, acc);
                    in_path = false;
                    continue;
                }
                pending = ev;
                break;
            }
        }

        /* (3) run one shading block: the one more lanes wait for */
        const int ns = __popcll(__ballot(pending == EV_SURF));
        const int nm = __popcll(__ballot(pending == EV_MED));
        if (ns + nm == 0) continue;
        if (ns >= nm) {
            if (pending == EV_SURF) {
                hetero_surface(S, tp, smp, p, e, m);
                pending = EV_END;
            }
        } else {
            if (pending == EV_MED) {
                hetero_medium(S, tp, smp, p, e, m);
                pending = EV_END;
            }
        }
    }
}

}  // namespace vpt

using namespace vpt;

namespace {

/* estimator 10's per-sample call (vpt_hetero.h) */
template <bool LM>
__global__ __launch_bounds__(256) void trace_batch_hetero_kernel(const vpt_ray* __restrict__ rays,
                                                                 const uint64_t* __restrict__ states, int n, Medium m,
                                                                 const DevScene* __restrict__ S,
                                                                 const vpt_grid_view* __restrict__ grid, double* out,
                                                                 uint64_t* out_states, unsigned long long* stats)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler<false> smp;
    smp.X = states[i] & 0xFFFFFFFFFFFFull;
    smp.g = m.g;
    HeteroStats hs{0, 0};
    dv3 L = trace_hetero<false, LM>(S, GridTr::load<LM>(grid), smp, ld3(rays[i].o), ld3(rays[i].d), m, stats ? &hs : nullptr);
    if (stats) {  /* vpt_debug_hetero_steps */
        atomicAdd(&stats[0], hs.tracks);
        atomicAdd(&stats[1], hs.steps);
    }
    out[3 * i] = L.x;
    out[3 * i + 1] = L.y;
    out[3 * i + 2] = L.z;
    out_states[i] = smp.X;
}

/* the density grid's walkers (vpt_grid.h), one ray per lane (vpt_grid_probe, vpt_grid_probe_lm) */
template <bool LM>
__global__ __launch_bounds__(256) void grid_probe_kernel(const vpt_grid_view* __restrict__ grid, double sigma_t,
                                                         const vpt_ray* __restrict__ rays, const double* __restrict__ tmax,
                                                         const uint64_t* __restrict__ states, int n, double* tau,
                                                         double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpt_grid_view G = *grid;
    const double o[3] = {rays[i].o[0], rays[i].o[1], rays[i].o[2]}, d[3] = {rays[i].d[0], rays[i].d[1], rays[i].d[2]};
    uint64_t X = states[i] & 0xFFFFFFFFFFFFull;
    tau[i] = vpt_grid_tau(&G, o, d, tmax[i]);
    uint32_t ns = 0;
    t_coll[i] = LM ? vpt_grid_track_lm(&G, o, d, tmax[i], sigma_t, &X, &ns) : vpt_grid_track(&G, o, d, tmax[i], sigma_t, &X, &ns);
    states_out[i] = X;
    if (steps) steps[i] = ns;
}

}  // namespace

void vpt_int_hetero_trace_launch(const vpt_ray* rays, const uint64_t* states, int n, const Medium& m, const DevScene* S,
                                 const vpt_grid_view* grid, bool lm, double* out, uint64_t* out_states,
                                 unsigned long long* stats)
{
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    if (lm) trace_batch_hetero_kernel<true><<<g, b>>>(rays, states, n, m, S, grid, out, out_states, stats);
    else trace_batch_hetero_kernel<false><<<g, b>>>(rays, states, n, m, S, grid, out, out_states, stats);
}

void vpt_int_grid_probe_launch(const vpt_grid_view* grid, bool lm, double sigma_t, const vpt_ray* rays, const double* tmax,
                               const uint64_t* states, int n, double* tau, double* t_coll, uint64_t* states_out,
                               uint32_t* steps)
{
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    if (lm) grid_probe_kernel<true><<<g, b>>>(grid, sigma_t, rays, tmax, states, n, tau, t_coll, states_out, steps);
    else grid_probe_kernel<false><<<g, b>>>(grid, sigma_t, rays, tmax, states, n, tau, t_coll, states_out, steps);
}

/* render_kernel_simple<10> (vpt_render_simple.h): counting mode (counters != NULL) and VPT_SIMPLE_KERNEL=1 */
template <bool COUNT, int FB, bool LM>
static int launch_simple(const KParams& K, const DevScene* S, hipStream_t stream)
{
    dim3 grid((unsigned)((K.w + 15) / 16), (unsigned)((K.shard_rows + 15) / 16));
    render_kernel_simple<VPT_HETERO_FREE, COUNT, FB, LM><<<grid, dim3(256), 0, stream>>>(K, S);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "render_kernel_simple<10> launch: %s", hipGetErrorString(e));
    return VPT_OK;
}

int vpt_int_hetero_simple_launch(const HeteroParams& H, const Medium& m, const DevScene* S, bool lm,
                                 unsigned long long* counters, void* stream)
{
    KParams K;
    memset(&K, 0, sizeof K);
    K.w = H.w;
    K.h = H.h;
    K.spp = H.spp;
    K.fb = H.fb;
    K.band_rows = H.band_rows;
    K.band_stride = H.band_stride;
    K.band_offset = H.band_offset;
    K.shard_rows = H.shard_rows;
    K.sigma_a = m.sigma_a;
    K.sigma_s = m.sigma_s;
    K.g = m.g;
    K.max_depth = m.max_depth;
    K.est = VPT_HETERO_FREE;
    K.march_step = m.march_step;
    K.march_light = m.march_light;
    K.seed = H.seed;
    for (int i = 0; i < 3; ++i) {
        K.o[i] = H.o[i];
        K.d[i] = H.d[i];
        K.cx[i] = H.cx[i];
        K.cy[i] = H.cy[i];
    }
    K.out = H.out;
    K.counters = counters;
    K.tiles_x = H.tiles_x;
    K.tiles_y = H.tiles_y;
    K.grid = H.grid;
    hipStream_t st = (hipStream_t)stream;
    const bool f32 = H.fb == VPT_FB_F32;
    if (lm) {
        if (counters) return f32 ? launch_simple<true, VPT_FB_F32, true>(K, S, st) : launch_simple<true, VPT_FB_F64, true>(K, S, st);
        return f32 ? launch_simple<false, VPT_FB_F32, true>(K, S, st) : launch_simple<false, VPT_FB_F64, true>(K, S, st);
    }
    if (counters) return f32 ? launch_simple<true, VPT_FB_F32, false>(K, S, st) : launch_simple<true, VPT_FB_F64, false>(K, S, st);
    return f32 ? launch_simple<false, VPT_FB_F32, false>(K, S, st) : launch_simple<false, VPT_FB_F64, false>(K, S, st);
}

template <int FB, bool LM>
static int launch(int device, const HeteroParams& H, const Medium& m, const DevScene* S, hipStream_t stream)
{
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hetero_kernel<false, FB, LM>, 256, 0);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "hetero_kernel: %s", hipGetErrorString(e));
    int blocks = (per_cu < 1 ? 1 : per_cu) * cus;
    const int tiles = H.tiles_x * H.tiles_y;
    const int need = (tiles + 3) / 4;  /* 4 waves per block, one tile per wave to start */
    if (blocks > need) blocks = need;
    if (blocks < 1) blocks = 1;
    hetero_kernel<false, FB, LM><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(H, m, S);
    e = hipGetLastError();
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "hetero_kernel launch: %s", hipGetErrorString(e));
    return VPT_OK;
}

int vpt_int_hetero_launch(int device, const HeteroParams& H, const Medium& m, const DevScene* S, bool lm, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (lm) return H.fb == VPT_FB_F32 ? launch<VPT_FB_F32, true>(device, H, m, S, st) : launch<VPT_FB_F64, true>(device, H, m, S, st);
    return H.fb == VPT_FB_F32 ? launch<VPT_FB_F32, false>(device, H, m, S, st) : launch<VPT_FB_F64, false>(device, H, m, S, st);
}
