/*
 * vpt_kernels.hip -- HIP kernels (gfx950) and the device half of the C ABI (include/vpt.h).
 *
 * A render of the estimators 0-5 runs on the workgroup task pool (pool_kernel, vpt_pool.h) and reduce_kernel;
 * ray marching (6-9), counting mode and VPT_SIMPLE_KERNEL=1 run render_kernel_simple (vpt_render_simple.h), one
 * lane per pixel; the kernels of estimators 10 to 16 live in the density-grid units (vpt_hetero*.hip).  render_kernel,
 * the persistent-wave loop of vpt_wave.h, is compiled only into -DVPT_DEBUG_ENV=1 builds.  The rest are the per-sample
 * calls and the probes.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <vector>

#include "vpt_device.h"
#include "vpt_pool.h"
#include "vpt_wave.h"
#include "vpt_hetero_mis.h"
#include "vpt_hetero_chroma.h"
#include "vpt_hetero_launch.h"
#include "vpt_grid_accum.h"

/* the EST = 1 pool kernel comes from vpt_pool_mis.hip, compiled with flags of its own (VPT_MIS_TU;
 * -DVPT_MIS_TU=0 instantiates it here, as the syntax checks of tests/test_knobs.py do) */
#ifndef VPT_MIS_TU
#define VPT_MIS_TU 1
#endif
#if VPT_MIS_TU
namespace vpt {
extern template __global__ void pool_kernel<1, false>(PoolParams P0, Medium m0, const DevScene* __restrict__ S,
                                                      unsigned long long* counters, unsigned long long* stats);
extern template __global__ void pool_kernel<1, false, true>(PoolParams P0, Medium m0, const DevScene* __restrict__ S,
                                                            unsigned long long* counters, unsigned long long* stats);
}  // namespace vpt
#if VPT_SECTIONS
extern "C" int vpt_mis_sections_add(unsigned long long* out);
#endif
#endif

using namespace vpt;

namespace {

#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return vpt_fail(VPT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

/* The device arrays of one per-ray call (the per-sample calls and the probes at the end of this file).  Every step is
 * a synchronous HIP call on the default stream; the first error is kept and every later step does nothing, so a call
 * reads as a straight sequence -- alloc, up, launch, down -- and asks once, with status().  The destructor frees what
 * was allocated. */
class Staging {
public:
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging()
    {
        for (void* d : owned_) (void)hipFree(d);
    }
    /* `count` elements of T on the device, an allocation of their own; NULL after an error */
    template <class T>
    T* alloc(size_t count)
    {
        void* d = nullptr;
        if (err_ == hipSuccess) err_ = hipMalloc(&d, sizeof(T) * count);
        if (err_ == hipSuccess) owned_.push_back(d);
        return (T*)d;
    }
    /* alloc where the caller passed the optional array `host`, else NULL */
    template <class T>
    T* alloc_if(const T* host, size_t count)
    {
        return host ? alloc<T>(count) : nullptr;
    }
    template <class T>
    void up(T* dev, const T* host, size_t count)
    {
        if (err_ == hipSuccess) err_ = hipMemcpy(dev, host, sizeof(T) * count, hipMemcpyHostToDevice);
    }
    /* a result to the host; an optional output the caller left NULL is skipped */
    template <class T>
    void down(T* host, const T* dev, size_t count)
    {
        if (err_ == hipSuccess && host) err_ = hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    /* f launches the call's kernel */
    template <class F>
    void launch(F f)
    {
        if (err_ != hipSuccess) return;
        f();
        err_ = hipGetLastError();
    }
    /* VPT_OK, or VPT_E_HIP with "<who>: <hip error string>" */
    int status(const char* who) const
    {
        if (err_ != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(err_));
        return VPT_OK;
    }

private:
    std::vector<void*> owned_;
    hipError_t err_ = hipSuccess;
};

/* What every device probe of the density grid stages first, on the context's device: the rays, their stream states and
 * tmax, and the array of the states behind the walk.  The probe adds its own arrays, launches and copies down as with
 * any Staging */
struct ProbeStaging : Staging {
    size_t nn = 0;
    vpt_ray* dr = nullptr;
    uint64_t *ds = nullptr, *dso = nullptr;
    double* dtm = nullptr;
    int stage(int device, const vpt_ray* rays, const uint64_t* states, const double* tmax, int n)
    {
        HIP_OK(hipSetDevice(device));
        nn = (size_t)n;
        dr = alloc<vpt_ray>(nn);
        ds = alloc<uint64_t>(nn);
        dso = alloc<uint64_t>(nn);
        dtm = alloc<double>(nn);
        up(dr, rays, nn);
        up(ds, states, nn);
        up(dtm, tmax, nn);
        return VPT_OK;
    }
};

/* the persistent-wave loop (vpt_wave.h) on the estimators 0-9: the round-1 design, which the pool kernel
 * replaced; an A/B path of -DVPT_DEBUG_ENV=1 builds (launch_wave) */
template <int EST, bool COUNT, int FB>
__global__ __launch_bounds__(256) void render_kernel(KParams P, const DevScene* __restrict__ S)
{
    wave_render<EstSteps<EST>, COUNT, FB>(P, S, {});
}

template <int EST>
__global__ __launch_bounds__(256) void trace_batch_kernel(const vpt_ray* __restrict__ rays,
                                                          const uint64_t* __restrict__ states, int n, Medium m,
                                                          double g, const DevScene* __restrict__ S, double* out,
                                                          uint64_t* out_states)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler<false> smp;
    smp.X = states[i] & 0xFFFFFFFFFFFFull;
    smp.g = g;
    dv3 L = trace_sample<EST, false>(S, smp, ld3(rays[i].o), ld3(rays[i].d), m);
    out[3 * i] = L.x;
    out[3 * i + 1] = L.y;
    out[3 * i + 2] = L.z;
    out_states[i] = smp.X;
}

/* punctualVolumetric (include/rayMarchingMethods.h:12-31) at n points */
__global__ __launch_bounds__(256) void punctual_kernel(int idsource, const double* __restrict__ x, int n, double phase,
                                                       double sigma_t, double sigma_s, const DevScene* __restrict__ S,
                                                       double* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler<false> smp;
    smp.X = 0;
    smp.g = 0;
    const dv3 L = punctual_volumetric(S, smp, idsource, ld3(x + 3 * i), phase, sigma_t, sigma_s);
    out[3 * i] = L.x;
    out[3 * i + 1] = L.y;
    out[3 * i + 2] = L.z;
}

/* rayMarching (include/rayMarchingMethods.h:34-103) with its out-parameters, one ray per lane */
__global__ __launch_bounds__(256) void ray_marching_kernel(const vpt_ray* __restrict__ rays,
                                                           const uint64_t* __restrict__ states, int n, double sigma_t,
                                                           double sigma_s, double steps, const DevScene* __restrict__ S,
                                                           double* out, double* x_new, int* idsource,
                                                           uint64_t* out_states)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler<false> smp;
    smp.X = states[i] & 0xFFFFFFFFFFFFull;
    smp.g = 0;
    dv3 xn = ld3(x_new + 3 * i);
    int id = idsource[i];
    const dv3 L = ray_marching_explicit(S, smp, ld3(rays[i].o), ld3(rays[i].d), sigma_t, sigma_s, steps, xn, id);
    out[3 * i] = L.x;
    out[3 * i + 1] = L.y;
    out[3 * i + 2] = L.z;
    x_new[3 * i] = xn.x;
    x_new[3 * i + 1] = xn.y;
    x_new[3 * i + 2] = xn.z;
    idsource[i] = id;
    out_states[i] = smp.X;
}

__global__ void math_probe_kernel(int fn, const double* x, const double* y, double* out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = x[i], b = y[i], r = 0;
    switch (fn) {
    case 0: r = vm_sqrt(a); break;
    case 1: r = lm_exp(a); break;
    case 2: r = lm_log(a); break;
    case 3: r = lm_sin(a); break;
    case 4: r = lm_cos(a); break;
    case 5: r = lm_tan(a); break;
    case 6: r = lm_atan(a); break;
    case 7: r = lm_acos(a); break;
    case 8: r = lm_atan2(a, b); break;
    case 12: r = vm_inv_sqrt(a); break;  /* 1.0 / sqrt(a) (nrm) */
    case 10:
    case 11: {
        double sv, cv;
        lm_sincos_acos(a, &sv, &cv);
        r = fn == 10 ? sv : cv;
        break;
    }
    case 14:
    case 15:
    case 16:
    case 17: {  /* lm_dir_trig(c = a, phi = b) as the direction samplers call it (cone path when every
                 * lane of the wave has c > 0.9925): sin(acos c), cos(acos c), sin(phi), cos(phi) */
        double q[4];
        lm_dir_trig(a, b, &q[0], &q[1], &q[2], &q[3]);
        r = q[fn - 14];
        break;
    }
    case 18: {  /* a / b through one shared reciprocal of b (VPT_DIV_SHARE), unconditionally */
        double bb = b;
        __asm__ volatile("" : "+v"(bb));
        r = vm_div_by(a, vm_rcp_of(bb));
        break;
    }
    case 19: r = hemi_cosine_prob(a); break;  /* a * 1 / pi */
    case 20: {                                /* 1 / a and b / a, their bits xor'ed (inv_and_ratio) */
        double inv, q;
        inv_and_ratio(a, b, inv, q);
        r = __longlong_as_double(__double_as_longlong(inv) ^ __double_as_longlong(q));
        break;
    }
    case 21: r = vm_sqrt_isect(a); break;    /* the sphere tests' root (VPT_ISECT_CLASS) */
    case 22: r = vm_sqrt_isect_z(a); break;  /* the shadow rays' (VPT_ISECT_ZERO) */
    case 23: {  /* log in two halves as decide() takes it: the table pair loaded, other work, then the rest */
        gm_log_pair lp = gm_log_pair_of(a);
        vpt_opaque(lp.invc);
        vpt_opaque(lp.logc);
        r = gm_log_finish(a, lp);
        break;
    }
    default: r = a / b; break;
    }
    out[i] = r;
}

/* HG extension probe: phase_sample around din from each state (the two draws of the stream), and
 * phase_value toward each wl (vpt_phase_probe) */
__global__ void phase_probe_kernel(double g, double dx, double dy, double dz, const uint64_t* X, int n, double* dirs,
                                   uint64_t* Xout, const double* wl, int nw, double* vals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const dv3 din = mk(dx, dy, dz);
    if (i < n) {
        Sampler<false> smp;
        smp.X = X[i];
        smp.g = g;
        smp.cnt.tests = smp.cnt.iterations = smp.cnt.draw_mismatch = 0;
        const dv3 w = phase_sample(smp, din);
        dirs[3 * i] = w.x;
        dirs[3 * i + 1] = w.y;
        dirs[3 * i + 2] = w.z;
        Xout[i] = smp.X;
    }
    if (i < nw) vals[i] = phase_value(g, din, mk(wl[3 * i], wl[3 * i + 1], wl[3 * i + 2]));
}

bool is_finite(double v) { return v == v && v - v == 0.0; }

unsigned long long* g_pool_stats = nullptr;  /* debug statistics buffer (VPT_POOL_STATS=1) */

}  // namespace

/* Per-stream launch state: a render enqueued on one stream must not share its work queue or its
 * chunk partials with a render in flight on another stream of the same context.  Each stream
 * that renders gets its own slot (queue head + partials, grown on demand, stream-ordered), so
 * vpt_render_device may be called on several streams of one context at once. */
struct StreamSlot {
    hipStream_t stream;
    unsigned* d_queue;
    double* d_partials;      /* chunk sums of the pool kernel */
    size_t partials_bytes;
    hipEvent_t done;         /* recorded after the slot's last launch */
    unsigned long long used; /* last use (context tick), for reuse by another stream */
};
/* at most this many slots (each holds a partials buffer): a further stream takes over the least
 * recently used slot whose work has finished, or waits for the least recently used one */
constexpr int MAX_STREAM_SLOTS = 8;
constexpr int LAUNCH_LOG2_MAX = 26;  /* samples per workgroup per pool launch <= 2^26 (launch_max_units) */

struct vpt_context {
    int device;
    DevScene* d_scene;
    DevScene h_scene;
    int has_scene;
    unsigned long long* d_counters;
    unsigned* d_guard;       /* pool_kernel's argument-layout guard flag (PoolParams::guard), sticky */
    unsigned guard_bias = 0; /* vpt_debug_karg_guard */
    std::mutex mu;           /* guards slots: held from taking a slot until its launches are enqueued */
    std::vector<std::unique_ptr<StreamSlot>> slots;  /* stable addresses */
    unsigned long long tick = 0;
    int launch_log2 = LAUNCH_LOG2_MAX;  /* samples per workgroup per launch <= 2^launch_log2 (vpt_debug_set_launch_bound) */
    /* the density grid of estimator 10 (vpt_set_density_grid): its view and its voxels on the device */
    vpt_grid_view* d_grid = nullptr;
    float* d_rho = nullptr;
    int has_grid = 0;
    /* the current grid was set from device memory (vpt_set_density_grid_device): its majorant grid is rebuilt on the
     * device, from d_rho (vpt_grid_build.hip) */
    int grid_from_device = 0;
    /* local majorants (vpt_set_grid_majorant_block): the context's block size (0: off), the current grid's
     * block maxima on the device and the host's copy of its view */
    int maj_block = 0;
    float* d_maj = nullptr;
    vpt_grid_view h_grid = {};
    /* trilinear interpolation (vpt_set_grid_interpolation): the context's mode, in h_grid.interp of every grid */
    int grid_interp = 0;
    /* emission (vpt_set_emission_grid): the current grid's emission on the device -- the colour's VPT_EMIT_HEAD doubles,
     * then the voxels that h_grid.emit points to (vpt_hetero.h); NULL: none */
    double* d_emit = nullptr;
    /* estimator 13's track fraction (vpt_set_hetero_mis_fraction): the context's, whatever grid and scene it holds */
    double mis_fraction = 0.5;
    /* estimator 14's medium colour (vpt_set_medium_colour): the per-channel multipliers of sigma_a and sigma_s; the
     * context's, like the track fraction */
    double chroma_a[3] = {1.0, 1.0, 1.0}, chroma_s[3] = {1.0, 1.0, 1.0};
};

/* The stream's slot, created on first use (or taken over from an idle stream once MAX_STREAM_SLOTS
 * exist); partials grown to `pbytes` in stream order (the previous buffer is freed after the work
 * already queued on the stream).  The caller holds ctx->mu from here until its launches on the slot
 * are enqueued and slot_done() has recorded them, so no other thread can grow, free or hand over the
 * slot's buffers in between. */
static int stream_slot(vpt_context* ctx, hipStream_t stream, size_t pbytes, StreamSlot** out)
{
    StreamSlot* sl = nullptr;
    for (auto& x : ctx->slots)
        if (x->stream == stream) sl = x.get();
    if (!sl && (int)ctx->slots.size() < MAX_STREAM_SLOTS) {
        std::unique_ptr<StreamSlot> n(new StreamSlot{stream, nullptr, nullptr, 0, nullptr, 0});
        HIP_OK(hipMalloc((void**)&n->d_queue, sizeof(unsigned)));
        const hipError_t e = hipEventCreateWithFlags(&n->done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipFree(n->d_queue);
            return vpt_fail(VPT_E_HIP, "hipEventCreateWithFlags: %s", hipGetErrorString(e));
        }
        ctx->slots.push_back(std::move(n));
        sl = ctx->slots.back().get();
    }
    if (!sl) {  /* every slot belongs to another stream: take an idle one, else wait for the oldest */
        StreamSlot* idle = nullptr;
        StreamSlot* oldest = nullptr;
        for (auto& x : ctx->slots) {
            if (!oldest || x->used < oldest->used) oldest = x.get();
            if (hipEventQuery(x->done) == hipSuccess && (!idle || x->used < idle->used)) idle = x.get();
        }
        sl = idle ? idle : oldest;
        if (!idle) HIP_OK(hipEventSynchronize(sl->done));
        sl->stream = stream;  /* its buffers are no longer read by the previous stream */
    }
    if (pbytes > sl->partials_bytes) {
        if (sl->d_partials) HIP_OK(hipFreeAsync(sl->d_partials, stream));
        sl->d_partials = nullptr;
        sl->partials_bytes = 0;
        HIP_OK(hipMallocAsync((void**)&sl->d_partials, pbytes, stream));
        sl->partials_bytes = pbytes;
    }
    sl->used = ++ctx->tick;
    *out = sl;
    return VPT_OK;
}

/* after the slot's launches: its event marks when the stream is done with its buffers */
static int slot_done(StreamSlot* sl, hipStream_t stream)
{
    HIP_OK(hipEventRecord(sl->done, stream));
    return VPT_OK;
}

static int check_medium(const vpt_medium* m)
{
    if (!m) return vpt_fail(VPT_E_INVALID, "medium is NULL");
    if (!is_finite(m->sigma_a) || !is_finite(m->sigma_s) || m->sigma_a < 0 || m->sigma_s < 0)
        return vpt_fail(VPT_E_INVALID, "sigma_a/sigma_s must be finite and >= 0");
    if (!is_finite(m->hg_g) || m->hg_g <= -1.0 || m->hg_g >= 1.0) return vpt_fail(VPT_E_INVALID, "hg_g must be in (-1, 1)");
    if (m->max_depth < 0) return vpt_fail(VPT_E_INVALID, "max_depth must be >= 0");
    if (m->estimator < 0 || m->estimator >= VPT_NUM_ESTIMATORS)
        return vpt_fail(VPT_E_INVALID, "unknown estimator %d", m->estimator);
    return VPT_OK;
}

/* the launch constants of estimators 14 and 16 from the medium and the context's colour: per unit density ss[k] = sigma_s * cs[k]
 * and st[k] = sigma_a * ca[k] + ss[k] (vpt_hetero_chroma.h) */
static ChromaCoef chroma_coef(const vpt_context* ctx, double sigma_a, double sigma_s)
{
    ChromaCoef c;
    for (int k = 0; k < 3; ++k) {
        const double sa = sigma_a * ctx->chroma_a[k];
        c.ss[k] = sigma_s * ctx->chroma_s[k];
        c.st[k] = sa + c.ss[k];
    }
    return c;
}

/* the ray-marching estimators' parameters: march_step (the step of rayMarching3 / rayMarching2, the
 * segment count of rayMarchingGlobal / rayMarching) finite and > 0; march_light (6, 7) a sphere of
 * the scene; rayMarchingGlobal and rayMarching read the hard-coded sphere 5
 * (include/rayMarchingMethods.h:64,153), so the scene needs at least 6 spheres */
static int check_march(const vpt_context* ctx, const vpt_medium* m)
{
    if (m->estimator >= VPT_HETERO_FREE && m->estimator <= VPT_HETERO_SPECTRAL) {
        if (!ctx->has_grid) return vpt_fail(VPT_E_INVALID, "estimator %d needs a density grid (vpt_set_density_grid)", m->estimator);
        if (m->estimator == VPT_HETERO_CHROMATIC || m->estimator == VPT_HETERO_SPECTRAL) {
            if (ctx->h_grid.emit)  /* the emitting track's weight under a hero channel, or under spectral weights, is not worked out */
                return vpt_fail(VPT_E_UNSUPPORTED, "estimator %d does not score an emission grid (estimators 10 and 11 do)",
                                m->estimator);
            const ChromaCoef c = chroma_coef(ctx, m->sigma_a, m->sigma_s);
            for (int k = 0; k < 3; ++k)
                if (!(c.st[k] > 0))  /* the hero's track, the weights and the albedo divide by it */
                    return vpt_fail(VPT_E_INVALID, "estimator %d: channel %d has no extinction (sigma_a * absorb + sigma_s * "
                                    "scatter == 0; vpt_set_medium_colour)", m->estimator, k);
            return VPT_OK;
        }
        /* emission is scored on a delta track, which estimator 12 does not run and estimator 13 runs only in part */
        if ((m->estimator == VPT_HETERO_EQUIANGULAR || m->estimator == VPT_HETERO_MIS || m->estimator == VPT_HETERO_RESIDUAL) &&
            ctx->h_grid.emit)
            return vpt_fail(VPT_E_UNSUPPORTED, "estimator %d does not score an emission grid (estimators 10 and 11 do)",
                            m->estimator);
        if (m->estimator == VPT_HETERO_RESIDUAL && ctx->h_grid.block < 1)  /* the control grid lies behind the majorants */
            return vpt_fail(VPT_E_INVALID, "estimator %d needs a majorant block (vpt_set_grid_majorant_block; a block >= the "
                            "grid's largest dimension is the global control)", m->estimator);
        return VPT_OK;
    }
    if (m->estimator < VPT_RAY_MARCHING) return VPT_OK;
    if (!is_finite(m->march_step) || !(m->march_step > 0))
        return vpt_fail(VPT_E_INVALID, "march_step must be finite and > 0");
    if ((m->estimator == VPT_RAY_MARCHING || m->estimator == VPT_RAY_MARCHING_SA) &&
        (m->march_light < 0 || m->march_light >= ctx->h_scene.n))
        return vpt_fail(VPT_E_INVALID, "march_light %d is not a sphere of the scene (%d)", m->march_light, ctx->h_scene.n);
    if ((m->estimator == VPT_RAY_MARCHING_GLOBAL || m->estimator == VPT_RAY_MARCHING_EXPLICIT) && ctx->h_scene.n < 6)
        return vpt_fail(VPT_E_INVALID, "rayMarchingGlobal / rayMarching sample sphere 5: the scene has %d spheres",
                        ctx->h_scene.n);
    return VPT_OK;
}

static int build_kparams(const vpt_context* ctx, const vpt_params* p, void* d_out, KParams& K)
{
    if (!ctx || !p) return vpt_fail(VPT_E_INVALID, "NULL context or params");
    if (!ctx->has_scene) return vpt_fail(VPT_E_INVALID, "no scene set (vpt_set_scene)");
    if (p->width <= 0 || p->height <= 0 || p->spp <= 0) return vpt_fail(VPT_E_INVALID, "width/height/spp must be > 0");
    if ((int64_t)p->width * p->height > (int64_t)1 << 31) return vpt_fail(VPT_E_INVALID, "image too large");
    if (p->fb_format != VPT_FB_F32 && p->fb_format != VPT_FB_F64) return vpt_fail(VPT_E_INVALID, "bad fb_format");
    int rc = check_medium(&p->medium);
    if (!rc) rc = check_march(ctx, &p->medium);
    if (rc) return rc;
    if (p->band_rows <= 0 || p->band_stride <= 0 || p->band_offset < 0 || p->band_offset >= p->band_stride)
        return vpt_fail(VPT_E_INVALID, "bad band_rows/band_stride/band_offset");
    int rows = vpt_shard_rows(p);  /* 0: more shards than bands -- a legal no-op */
    const double* cd = p->camera.d;
    if (!is_finite(p->fov_scale) || !is_finite(cd[0]) || !is_finite(cd[1]) || !is_finite(cd[2]))
        return vpt_fail(VPT_E_INVALID, "bad camera");
    memset(&K, 0, sizeof K);
    K.w = p->width;
    K.h = p->height;
    K.spp = p->spp;
    K.fb = p->fb_format;
    K.band_rows = p->band_rows;
    K.band_stride = p->band_stride;
    K.band_offset = p->band_offset;
    K.shard_rows = rows;
    K.sigma_a = p->medium.sigma_a;
    K.sigma_s = p->medium.sigma_s;
    K.g = p->medium.hg_g;
    K.max_depth = p->medium.max_depth;
    K.est = p->medium.estimator;
    K.march_step = p->medium.march_step;
    K.march_light = p->medium.march_light;
    K.seed = p->seed;
    for (int i = 0; i < 3; ++i) {
        K.o[i] = p->camera.o[i];
        K.d[i] = cd[i];
    }
    /* Vector cx = Vector(w * 0.5095 / h, 0., 0.); cy = (cx % camera.d).normalize() * 0.5095
     * (src/rt.cpp:758-759), same operation order */
    K.cx[0] = p->width * p->fov_scale / p->height;
    K.cx[1] = 0.;
    K.cx[2] = 0.;
    double crx = K.cx[1] * cd[2] - K.cx[2] * cd[1];
    double cry = K.cx[2] * cd[0] - K.cx[0] * cd[2];
    double crz = K.cx[0] * cd[1] - K.cx[1] * cd[0];
    double inv = 1.0 / sqrt(crx * crx + cry * cry + crz * crz);
    K.cy[0] = crx * inv * p->fov_scale;
    K.cy[1] = cry * inv * p->fov_scale;
    K.cy[2] = crz * inv * p->fov_scale;
    K.out = d_out;
    K.grid = ctx->has_grid ? ctx->d_grid : nullptr;
    if (p->chunk_spp < 0) return vpt_fail(VPT_E_INVALID, "chunk_spp must be >= 0");
    /* auto: 32 samples per work unit (A/B at 1024^2 x 256: chunk 4 / 8 / 16 / 32 / 64 -> 3816 / 3969 /
     * 4085 / 4153 / 4129 Ms/s), the last 32 of a pixel tapered (vpt_chunks.h); spp <= 32 is then one
     * chunk, i.e. the reference's sequential sum.  An explicit chunk_spp gives uniform chunks. */
    K.chunk = p->chunk_spp > 0 ? (p->chunk_spp < p->spp ? p->chunk_spp : p->spp) : vpt_auto_chunk(p->spp);
    K.taper = p->chunk_spp == 0;
    return VPT_OK;
}

/* the pool kernel's argument-layout guard (PoolParams::guard): after a synchronised render, a raised
 * flag means a launch read its parameters from the wrong place and rendered nothing */
static int check_guard(vpt_context* ctx, const char* who)
{
    unsigned g = 0;
    HIP_OK(hipMemcpy(&g, ctx->d_guard, sizeof g, hipMemcpyDeviceToHost));
    if (g) return vpt_fail(VPT_E_INTERNAL, "%s: pool_kernel's launch parameters are not at the start of its argument "
                           "segment (VPT_P_KARG guard); the image is NaN", who);
    return VPT_OK;
}

template <typename Kern>
static int persistent_grid(vpt_context* ctx, Kern kern, int* blocks, int threads = 256)
{
    HIP_OK(vpt_resident_blocks(kern, threads, ctx->device, blocks));
    return VPT_OK;
}

/* A/B and debug switches read from the environment (VPT_SIMPLE_KERNEL, VPT_WAVE_KERNEL,
 * VPT_COST_SURF / VPT_COST_MED, VPT_POOL_STATS) exist only in builds made with -DVPT_DEBUG_ENV=1
 * (scripts/build_variant.sh); the production library ignores the environment, so a stray
 * variable cannot change the kernel or its timing. */
#ifndef VPT_DEBUG_ENV
#define VPT_DEBUG_ENV 0
#endif
static int env_int(const char* name, int dflt)
{
    if (!VPT_DEBUG_ENV) return dflt;
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

template <int EST, bool COUNT, int FB>
static int launch_wave(vpt_context* ctx, KParams K, hipStream_t stream);
template <int EST, int FB>
static int launch_pool(vpt_context* ctx, KParams K, hipStream_t stream);

/* The pool's ring positions are 32-bit counters that grow by ~3 per sample a workgroup runs, so a
 * render is split into launches of at most 2^LAUNCH_LOG2_MAX samples per workgroup: units in order
 * [unit0, unit0 + nunits), each unit one partial slot, so the split changes no value (the chunk
 * sums are per unit; reduce_kernel adds them after the last launch).  One launch holds up to
 * ~17 G samples on 256 CUs; BASELINE configs[4] (2^34 samples per GPU) takes two. */
static uint64_t launch_max_units(int blocks, int C, int log2_bound)
{
    const uint64_t m = (((uint64_t)1 << log2_bound) * (uint64_t)(blocks > 0 ? blocks : 1)) / (uint64_t)(C > 0 ? C : 1);
    return m < 1 ? 1 : m;
}

/* log2(v) when v is a power of two, else -1 (PoolParams shift fast paths) */
static int log2_exact(int64_t v)
{
    if (v <= 0 || (v & (v - 1)) != 0) return -1;
    int k = 0;
    while ((v >> k) != 1) ++k;
    return k;
}

/* VPT_SIMPLE_KERNEL=1 selects render_kernel_simple<10> for estimator 10 in every build (the production
 * library ignores the variable for estimators 0-9, env_int): the one-lane-per-pixel kernel is the new
 * kernel's reference in tests/test_gpu_hetero.py, which must be able to run it on the library as shipped */
static bool hetero_simple_kernel()
{
    const char* v = getenv("VPT_SIMPLE_KERNEL");
    return v && *v && atoi(v) != 0;
}

/* The code object that holds an estimator's kernels for a lookup (tl: trilinear) and, for estimators 10 and 11, a medium
 * without or with emission (vpt_hetero.h); estimators 12 to 16 take the lookup alone.  The one place where the settings
 * turn into a unit: every launch below goes through the table returned here.  A probe names its estimator's unit, and
 * the two grid probes exist in the units without emission only, so their callers pass em = false whatever the context
 * holds. */
static const vpt_hetero_unit& hetero_unit(int est, bool tl, bool em)
{
    switch (est) {
    case VPT_HETERO_EQUIANGULAR: return tl ? vpt_int_hetero_eqa_unit_tl : vpt_int_hetero_eqa_unit;
    case VPT_HETERO_MIS: return tl ? vpt_int_hetero_mis_unit_tl : vpt_int_hetero_mis_unit;
    case VPT_HETERO_CHROMATIC: return tl ? vpt_int_hetero_chroma_unit_tl : vpt_int_hetero_chroma_unit;
    case VPT_HETERO_RESIDUAL: return tl ? vpt_int_hetero_residual_unit_tl : vpt_int_hetero_residual_unit;
    case VPT_HETERO_SPECTRAL: return tl ? vpt_int_hetero_spectral_unit_tl : vpt_int_hetero_spectral_unit;
    default: break;  /* 10 and 11 */
    }
    if (em) return tl ? vpt_int_hetero_unit_em_tl : vpt_int_hetero_unit_em;
    return tl ? vpt_int_hetero_unit_tl : vpt_int_hetero_unit;
}
static const vpt_hetero_unit& hetero_unit(const vpt_context* ctx, int est)
{
    return hetero_unit(est, ctx->h_grid.interp != 0, ctx->h_grid.emit != nullptr);
}

/* what the context and the medium give a launch of these units (vpt_hetero_args); stats: estimator 10's per-sample call */
static vpt_hetero_args hetero_args(const vpt_context* ctx, double sigma_a, double sigma_s, unsigned long long* stats)
{
    return vpt_hetero_args{ctx->h_grid.block > 0, ctx->mis_fraction, chroma_coef(ctx, sigma_a, sigma_s), stats};
}

/* estimators 10, 11 (by K.est: hetero_kernel / hetero_ratio_kernel), 12 (hetero_eqa_kernel; the majorant block plays no
 * part), 13 (hetero_mis_kernel, with the context's track fraction), 14 (hetero_chroma_kernel, with the coefficients
 * of the context's medium colour), 15 (hetero_residual_kernel) and 16 (hetero_spectral_kernel, with the same coefficients)
 * on the stream's queue word; counting mode and VPT_SIMPLE_KERNEL=1: the unit's render_kernel_simple_<unit> (one body,
 * vpt_hetero_simple.h) */
static int launch_hetero(vpt_context* ctx, KParams K, hipStream_t stream)
{
    const vpt_hetero_unit& u = hetero_unit(ctx, K.est);
    const vpt_hetero_args a = hetero_args(ctx, K.sigma_a, K.sigma_s, nullptr);
    if (K.counters || hetero_simple_kernel()) return u.simple_launch(K, ctx->d_scene, a, stream);
    std::lock_guard<std::mutex> lock(ctx->mu);
    StreamSlot* sl = nullptr;
    int rc = stream_slot(ctx, stream, 0, &sl);
    if (rc) return rc;
    K.queue = sl->d_queue;
    HIP_OK(hipMemsetAsync(K.queue, 0, sizeof(unsigned), stream));
    rc = u.launch(ctx->device, K, ctx->d_scene, a, stream);
    if (rc) return rc;
    return slot_done(sl, stream);
}

template <int EST, bool COUNT, int FB>
static int launch_one(vpt_context* ctx, KParams K, hipStream_t stream)
{
    if constexpr (EST >= VPT_HETERO_FREE) {  /* the density-grid units' kernels (hetero_unit) */
        return launch_hetero(ctx, K, stream);
    } else {
        const DevScene* S = ctx->d_scene;
        /* counting (vpt_count_work) needs only the totals: the one-lane-per-pixel kernel, which is
         * also the A/B baseline (VPT_SIMPLE_KERNEL=1: samples in sequence per lane) */
        if (COUNT || env_int("VPT_SIMPLE_KERNEL", 0)) {
            dim3 grid((unsigned)((K.w + 15) / 16), (unsigned)((K.shard_rows + 15) / 16));
            render_kernel_simple<EST, COUNT, FB><<<grid, dim3(256), 0, stream>>>(K, S);
            HIP_OK(hipGetLastError());
            return VPT_OK;
        }
        if constexpr (!COUNT && EST <= 5) return launch_pool<EST, FB>(ctx, K, stream);
        if constexpr (EST >= 6) {  /* ray marching: one lane per pixel, samples summed in order */
            dim3 grid((unsigned)((K.w + 15) / 16), (unsigned)((K.shard_rows + 15) / 16));
            render_kernel_simple<EST, COUNT, FB><<<grid, dim3(256), 0, stream>>>(K, S);
            HIP_OK(hipGetLastError());
        }
        return VPT_OK;
    }
}

/* One pass of the pool kernel: the chunks [c0, c1) of layout `lay` for a set of 8x8 tiles -- every tile of
 * the shard in order (tile_map NULL, n_tiles = tiles_x * tiles_y) or the n_tiles tiles a device list names.
 * pool_plan fills Q and checks the bounds (no GPU call); pool_enqueue sets the buffers and launches.
 * The units of a pass are chunk-major like a whole render's, level_units = 64 n_tiles per chunk, and the
 * pass is the unit range [c0 level_units, c1 level_units) of the layout.  A tile list needs pool_kernel<EST, false, true>
 * (estimators 0 and 1; VPT_E_UNSUPPORTED otherwise). */
static int pool_plan(const KParams& K, vpt_chunk_layout lay, int c0, int c1, const unsigned* tile_map, unsigned n_tiles,
                     PoolParams& Q, uint64_t* first, uint64_t* count)
{
    if (K.w > 65535 || K.h > 65535) return vpt_fail(VPT_E_INVALID, "width and height must be < 65536");
    Q.w = K.w;
    Q.h = K.h;
    Q.spp = K.spp;
    Q.rows = K.shard_rows;
    Q.band_rows = K.band_rows;
    Q.band_stride = K.band_stride;
    Q.band_offset = K.band_offset;
    Q.tiles_x = K.tiles_x;
    Q.lay = lay;
    Q.nch = Q.lay.n;
    Q.level_units = n_tiles * 64u;
    Q.sh_lu = log2_exact((int64_t)Q.level_units);
    Q.sh_tx = log2_exact(K.tiles_x);
    Q.sh_br = log2_exact(K.band_rows);
    Q.sh_bs = log2_exact(K.band_stride);
    Q.sh_c = log2_exact(Q.lay.C);
    Q.rw = log2_exact(K.w) >= 0 ? 1.0 / K.w : 0.0;
    Q.rh = log2_exact(K.h) >= 0 ? 1.0 / K.h : 0.0;
    Q.tile_map = tile_map;
    /* the kernel adds unit0 to a unit's index in u32: the pass's last unit must fit */
    const uint64_t end = (uint64_t)n_tiles * 64u * (uint64_t)c1;
    if (end >= 0xFFFFFFFFull) return vpt_fail(VPT_E_INVALID, "too many work units (%llu)", (unsigned long long)end);
    *first = (uint64_t)n_tiles * 64u * (uint64_t)c0;
    *count = end - *first;
    Q.seed = K.seed;
    for (int i = 0; i < 3; ++i) {
        Q.o[i] = K.o[i];
        Q.d[i] = K.d[i];
        Q.cx[i] = K.cx[i];
        Q.cy[i] = K.cy[i];
    }
    return VPT_OK;
}

/* partials: where chunk 0's plane would start (a pass that holds only the chunks from c0 on passes its buffer
 * minus c0 planes; the address is only formed, never dereferenced below the buffer) */
template <int EST>
static int pool_enqueue(vpt_context* ctx, const KParams& K, PoolParams& Q, uint64_t first, uint64_t units, double* partials,
                        unsigned* queue, hipStream_t stream)
{
    const DevScene* S = ctx->d_scene;
    constexpr bool COUNT = false;
    int blocks = 0;
    Q.partials = partials;
    Q.queue = queue;
    Q.guard = ctx->d_guard;
    Q.guard_bias = ctx->guard_bias;
    /* this launch's camera and this context's scene: every render, accumulator pass and rank comes through here */
    memset(Q.cam_oc, 0, sizeof Q.cam_oc);
    vpt_int_cam_table(K.o, &ctx->h_scene.geo[0].px, sizeof(GeoSphere) / sizeof(double), ctx->h_scene.n, Q.cam_oc);
    const Medium m = medium_of(K);
    /* a pass over a tile list runs pool_kernel<EST, false, true>, which exists for the estimators 0 and 1 */
    constexpr bool HAS_TILES = EST <= 1;
    const bool tiles = Q.tile_map != nullptr;
    if (tiles && !HAS_TILES)
        return vpt_fail(VPT_E_UNSUPPORTED, "estimator %d renders whole tile sets only (tile subsets: estimators 0 and 1)", EST);
    int rc;
    if constexpr (HAS_TILES) {
        rc = tiles ? persistent_grid(ctx, pool_kernel<EST, COUNT, true>, &blocks, VPT_POOL_THREADS)
                   : persistent_grid(ctx, pool_kernel<EST, COUNT>, &blocks, VPT_POOL_THREADS);
    } else {
        rc = persistent_grid(ctx, pool_kernel<EST, COUNT>, &blocks, VPT_POOL_THREADS);
    }
    if (rc) return rc;
    const uint64_t need = (units + POOL - 1) / POOL;
    if ((uint64_t)blocks > need) blocks = (int)need;
    /* every workgroup adds UREFILL to the u32 queue once more after it runs dry */
    if (first + units + (uint64_t)blocks * (UREFILL + 1) >= 0xFFFFFFFFull)
        return vpt_fail(VPT_E_INVALID, "too many work units (%llu) for the u32 work queue", (unsigned long long)(first + units));
    /* launches of at most 2^launch_log2 samples per workgroup (launch_max_units); samples per
     * unit: at most the layout's head chunk C, and a unit above 2^LAUNCH_LOG2_MAX is refused */
    if (Q.lay.C > (1 << LAUNCH_LOG2_MAX))
        return vpt_fail(VPT_E_INVALID, "chunk of %d samples > 2^26 (the per-workgroup launch bound)", Q.lay.C);
    const uint64_t max_units = launch_max_units(blocks, Q.lay.C, ctx->launch_log2);
    unsigned long long* stats = nullptr;
    if (env_int("VPT_POOL_STATS", 0)) {  /* debug: scheduler statistics, vpt_debug_pool_stats */
        if (!g_pool_stats) HIP_OK(hipMalloc((void**)&g_pool_stats, (TL0 + 3 * TL_MAXWG) * sizeof(unsigned long long)));
        HIP_OK(hipMemsetAsync(g_pool_stats, 0, TL0 * sizeof(unsigned long long), stream));
        HIP_OK(hipMemsetAsync(g_pool_stats + TL0, 0xFF, 3 * TL_MAXWG * sizeof(unsigned long long), stream));
        stats = g_pool_stats;
    }
    for (uint64_t u0 = 0; u0 < units; u0 += max_units) {
        Q.unit0 = (unsigned)(first + u0);
        Q.nunits = (unsigned)(units - u0 < max_units ? units - u0 : max_units);
        HIP_OK(hipMemsetAsync(Q.queue, 0, sizeof(unsigned), stream));
        if constexpr (HAS_TILES) {
            if (tiles) pool_kernel<EST, COUNT, true><<<dim3((unsigned)blocks), dim3(VPT_POOL_THREADS), 0, stream>>>(Q, m, S, K.counters, stats);
            else pool_kernel<EST, COUNT><<<dim3((unsigned)blocks), dim3(VPT_POOL_THREADS), 0, stream>>>(Q, m, S, K.counters, stats);
        } else {
            pool_kernel<EST, COUNT><<<dim3((unsigned)blocks), dim3(VPT_POOL_THREADS), 0, stream>>>(Q, m, S, K.counters, stats);
        }
        HIP_OK(hipGetLastError());
    }
    return VPT_OK;
}

template <int EST, int FB>
static int launch_pool(vpt_context* ctx, KParams K, hipStream_t stream)
{
    [[maybe_unused]] constexpr bool COUNT = false;  /* the debug arm below */
    int rc;
    const bool wave = EST <= 1 && env_int("VPT_WAVE_KERNEL", 0);  /* A/B: the previous design, FF/MIS */
    if (!wave) {  /* default: workgroup task pool (vpt_pool.h) */
        PoolParams Q;
        uint64_t first = 0, units = 0;
        const vpt_chunk_layout lay = vpt_chunks(K.spp, K.chunk, K.taper);
        rc = pool_plan(K, lay, 0, lay.n, nullptr, (unsigned)K.tiles_x * (unsigned)K.tiles_y, Q, &first, &units);
        if (rc) return rc;
        const size_t pbytes = (size_t)K.shard_rows * (size_t)K.w * (size_t)Q.nch * 3 * sizeof(double);
        std::lock_guard<std::mutex> lock(ctx->mu);  /* until the launches on the slot are enqueued */
        StreamSlot* sl = nullptr;
        rc = stream_slot(ctx, stream, pbytes, &sl);
        if (rc) return rc;
        rc = pool_enqueue<EST>(ctx, K, Q, first, units, sl->d_partials, sl->d_queue, stream);
        if (rc) return rc;
        const size_t npix = (size_t)K.shard_rows * (size_t)K.w;
        reduce_kernel<FB><<<dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream>>>(Q, K.out);
        HIP_OK(hipGetLastError());
        return slot_done(sl, stream);
    }
#if VPT_DEBUG_ENV
    /* the round-1 wave scheduler (render_kernel), an A/B path of debug builds only */
    if constexpr (EST <= 1) return launch_wave<EST, COUNT, FB>(ctx, K, stream);
#endif
    return VPT_OK;
}

template <int EST, bool COUNT, int FB>
static int launch_wave(vpt_context* ctx, KParams K, hipStream_t stream)
{
    const DevScene* S = ctx->d_scene;
    int blocks = 0;
    int rc = persistent_grid(ctx, render_kernel<EST, COUNT, FB>, &blocks);
    if (rc) return rc;
    blocks = vpt_wave_blocks(blocks, K);
    std::lock_guard<std::mutex> lock(ctx->mu);
    StreamSlot* sl = nullptr;
    rc = stream_slot(ctx, stream, 0, &sl);
    if (rc) return rc;
    K.queue = sl->d_queue;
    HIP_OK(hipMemsetAsync(K.queue, 0, sizeof(unsigned), stream));
    render_kernel<EST, COUNT, FB><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(K, S);
    HIP_OK(hipGetLastError());
    return slot_done(sl, stream);
}

template <bool COUNT>
static int launch_render(vpt_context* ctx, KParams K, hipStream_t stream)
{
    if (K.shard_rows == 0) return VPT_OK;
    K.tiles_x = (K.w + 7) / 8;
    K.tiles_y = (K.shard_rows + 7) / 8;
    K.cost_surf = env_int("VPT_COST_SURF", 1);
    K.cost_med = env_int("VPT_COST_MED", 1);
#define VPT_LAUNCH_EST(E)                                                              \
    case E:                                                                            \
        if (K.fb == VPT_FB_F32) return launch_one<E, COUNT, VPT_FB_F32>(ctx, K, stream); \
        return launch_one<E, COUNT, VPT_FB_F64>(ctx, K, stream);
    switch (K.est) {
        VPT_LAUNCH_EST(0)
        VPT_LAUNCH_EST(1)
        VPT_LAUNCH_EST(2)
        VPT_LAUNCH_EST(3)
        VPT_LAUNCH_EST(4)
        VPT_LAUNCH_EST(5)
        VPT_LAUNCH_EST(6)
        VPT_LAUNCH_EST(7)
        VPT_LAUNCH_EST(8)
        VPT_LAUNCH_EST(9)
        VPT_LAUNCH_EST(10)
        VPT_LAUNCH_EST(11)
        VPT_LAUNCH_EST(12)
        VPT_LAUNCH_EST(13)
        VPT_LAUNCH_EST(14)
        VPT_LAUNCH_EST(15)
        VPT_LAUNCH_EST(16)
    }
#undef VPT_LAUNCH_EST
    return vpt_fail(VPT_E_INVALID, "unknown estimator %d", K.est);
}

/* ---- for the progressive accumulator (vpt_accum.hip; declared in vpt_internal.h) ---- */
int vpt_int_device(const vpt_context* ctx) { return ctx->device; }
const unsigned* vpt_int_guard_flag(const vpt_context* ctx) { return ctx->d_guard; }
int vpt_int_check_guard(vpt_context* ctx, const char* who) { return check_guard(ctx, who); }

int vpt_int_check_params(const vpt_context* ctx, const vpt_params* p)
{
    KParams K;
    return build_kparams(ctx, p, (void*)1, K);
}

/* chunk levels [k0, k1) of the uniform layout with chunk C, for the n_tiles tiles d_tiles lists (NULL: all
 * tiles_x * tiles_y tiles of p's shard), into d_partials, which holds the planes of those levels only (level k0
 * first).  Enqueued on the default stream; the caller owns the buffers and synchronises. */
int vpt_int_pool_pass(vpt_context* ctx, const vpt_params* p, int C, int k0, int k1, const unsigned* d_tiles,
                      unsigned n_tiles, double* d_partials, unsigned* d_queue)
{
    KParams K;
    int rc = build_kparams(ctx, p, (void*)1, K);
    if (rc) return rc;
    if (K.est > 5) return vpt_fail(VPT_E_UNSUPPORTED, "estimator %d does not run on the pool kernel", K.est);
    if (C <= 0 || k0 < 0 || k1 <= k0 || (int64_t)k1 * C > 0x7FFFFFFF || n_tiles == 0 || K.shard_rows == 0)
        return vpt_fail(VPT_E_INVALID, "bad pass (levels [%d, %d) of %d samples, %u tiles)", k0, k1, C, n_tiles);
    K.tiles_x = (K.w + 7) / 8;
    K.tiles_y = (K.shard_rows + 7) / 8;
    K.spp = k1 * C;
    K.chunk = C;
    K.taper = 0;
    PoolParams Q;
    uint64_t first = 0, units = 0;
    rc = pool_plan(K, vpt_chunks(K.spp, C, 0), k0, k1, d_tiles, n_tiles, Q, &first, &units);
    if (rc) return rc;
    const size_t plane = (size_t)K.shard_rows * (size_t)K.w * 3;
    double* base = (double*)((uintptr_t)d_partials - (uintptr_t)k0 * plane * sizeof(double));
    switch (K.est) {
    case 0: return pool_enqueue<0>(ctx, K, Q, first, units, base, d_queue, nullptr);
    case 1: return pool_enqueue<1>(ctx, K, Q, first, units, base, d_queue, nullptr);
    case 2: return pool_enqueue<2>(ctx, K, Q, first, units, base, d_queue, nullptr);
    case 3: return pool_enqueue<3>(ctx, K, Q, first, units, base, d_queue, nullptr);
    case 4: return pool_enqueue<4>(ctx, K, Q, first, units, base, d_queue, nullptr);
    default: return pool_enqueue<5>(ctx, K, Q, first, units, base, d_queue, nullptr);
    }
}

/* The code object that holds the grid accumulator's render kernel for an estimator, a lookup and, for estimators 10 and
 * 11, a medium without or with emission (vpt_grid_accum.hip): hetero_unit()'s choice for the continuing loop */
static vpt_grid_accum_launch* grid_accum_unit(int est, bool tl, bool em)
{
    switch (est) {
    case VPT_HETERO_EQUIANGULAR: return tl ? vpt_int_grid_accum_eqa_tl : vpt_int_grid_accum_eqa;
    case VPT_HETERO_MIS: return tl ? vpt_int_grid_accum_mis_tl : vpt_int_grid_accum_mis;
    case VPT_HETERO_CHROMATIC: return tl ? vpt_int_grid_accum_chroma_tl : vpt_int_grid_accum_chroma;
    case VPT_HETERO_RESIDUAL: return tl ? vpt_int_grid_accum_residual_tl : vpt_int_grid_accum_residual;
    case VPT_HETERO_SPECTRAL: return tl ? vpt_int_grid_accum_spectral_tl : vpt_int_grid_accum_spectral;
    default: break;  /* 10 and 11 */
    }
    if (em) return tl ? vpt_int_grid_accum_hetero_em_tl : vpt_int_grid_accum_hetero_em;
    return tl ? vpt_int_grid_accum_hetero_tl : vpt_int_grid_accum_hetero;
}

/* One pass of the grid accumulator (estimators 10 to 16): d_nadd[i] further levels of C samples for tile d_list[i]
 * (d_list NULL: the shard's tiles in order, n_tiles of them), from the level counts d_levels holds, into d_sum and
 * d_s12 (vpt_wave_accum.h).  Validates as a render does, so a grid that was cleared or a setting that no longer suits
 * the estimator fails here with the render's status before anything is enqueued.  One launch on the default stream;
 * the caller owns the buffers and synchronises. */
int vpt_int_grid_pass(vpt_context* ctx, const vpt_params* p, int C, const unsigned* d_list, const int* d_nadd,
                      unsigned n_tiles, const int* d_levels, double* d_sum, double* d_s12, unsigned* d_queue)
{
    KParams K;
    int rc = build_kparams(ctx, p, (void*)1, K);
    if (rc) return rc;
    if (K.est < VPT_HETERO_FREE) return vpt_fail(VPT_E_UNSUPPORTED, "estimator %d has no grid pass", K.est);
    K.tiles_x = (K.w + 7) / 8;
    K.tiles_y = (K.shard_rows + 7) / 8;
    if (C <= 0 || n_tiles == 0 || n_tiles > (unsigned)K.tiles_x * (unsigned)K.tiles_y || K.shard_rows == 0 ||
        (uint64_t)n_tiles * 64u >= 0xF0000000ull)  /* the u32 queue: every lane adds itself once more after it runs dry */
        return vpt_fail(VPT_E_INVALID, "bad grid pass (%u tiles, levels of %d samples)", n_tiles, C);
    K.cost_surf = env_int("VPT_COST_SURF", 1);
    K.cost_med = env_int("VPT_COST_MED", 1);
    K.out = nullptr;
    K.queue = d_queue;
    GridAccum A;
    A.C = C;
    A.n_list = n_tiles;
    A.list = d_list;
    A.nadd = d_nadd;
    A.levels = d_levels;
    A.sum = d_sum;
    A.s12 = d_s12;
    HIP_OK(hipMemsetAsync(d_queue, 0, sizeof(unsigned), nullptr));
    return grid_accum_unit(K.est, ctx->h_grid.interp != 0, ctx->h_grid.emit != nullptr)(
        ctx->device, K, ctx->d_scene, A, hetero_args(ctx, K.sigma_a, K.sigma_s, nullptr), nullptr);
}

extern "C" {

int vpt_context_create(int device, vpt_context** out)
{
    vpt_clear_error();
    if (!out) return vpt_fail(VPT_E_INVALID, "vpt_context_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return vpt_fail(VPT_E_INVALID, "vpt_context_create: device %d of %d", device, ndev);
    HIP_OK(hipSetDevice(device));
    vpt_context* c = new vpt_context();
    memset(&c->h_scene, 0, sizeof c->h_scene);
    c->device = device;
    c->has_scene = 0;
    c->d_scene = nullptr;
    c->d_counters = nullptr;
    c->d_guard = nullptr;
    hipError_t e = hipMalloc((void**)&c->d_scene, sizeof(DevScene));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_counters, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_guard, sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(c->d_guard, 0, sizeof(unsigned));
    if (e != hipSuccess) {
        vpt_context_destroy(c);
        return vpt_fail(VPT_E_HIP, "vpt_context_create: hipMalloc: %s", hipGetErrorString(e));
    }
    *out = c;
    return VPT_OK;
}

void vpt_context_destroy(vpt_context* ctx)
{
    if (!ctx) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(ctx->device);
    if (ctx->d_scene) (void)hipFree(ctx->d_scene);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->d_guard) (void)hipFree(ctx->d_guard);
    if (ctx->d_grid) (void)hipFree(ctx->d_grid);
    if (ctx->d_rho) (void)hipFree(ctx->d_rho);
    if (ctx->d_maj) (void)hipFree(ctx->d_maj);
    if (ctx->d_emit) (void)hipFree(ctx->d_emit);
    for (auto& sl : ctx->slots) {
        if (sl->done) (void)hipEventSynchronize(sl->done);
        if (sl->d_partials) (void)hipFree(sl->d_partials);
        if (sl->d_queue) (void)hipFree(sl->d_queue);
        if (sl->done) (void)hipEventDestroy(sl->done);
    }
    (void)hipSetDevice(prev);
    delete ctx;
}

int vpt_set_scene(vpt_context* ctx, const vpt_sphere* s, int n)
{
    vpt_clear_error();
    if (!ctx || !s) return vpt_fail(VPT_E_INVALID, "vpt_set_scene: NULL argument");
    if (n < 1) return vpt_fail(VPT_E_INVALID, "vpt_set_scene: empty scene");
    if (n > VPT_MAX_SPHERES) return vpt_fail(VPT_E_TOO_MANY, "vpt_set_scene: %d spheres > %d", n, VPT_MAX_SPHERES);
    DevScene h;
    memset(&h, 0, sizeof h);
    h.n = n;
    for (int i = 0; i < n; ++i) {
        const vpt_sphere& q = s[i];
        if (q.material < 0 || q.material > 3)
            return vpt_fail(VPT_E_UNSUPPORTED, "vpt_set_scene: sphere %d material %d", i, q.material);
        const double* vals[6] = {q.p, q.c, q.radiance, q.eta, q.kappa, nullptr};
        bool ok = is_finite(q.r) && q.r >= 0 && is_finite(q.alpha);
        for (int a = 0; a < 5; ++a)
            for (int c = 0; c < 3; ++c) ok = ok && is_finite(vals[a][c]);
        if (!ok) return vpt_fail(VPT_E_INVALID, "vpt_set_scene: sphere %d has a non-finite or negative field", i);
        h.sph[i] = q;
        h.geo[i].px = q.p[0];
        h.geo[i].py = q.p[1];
        h.geo[i].pz = q.p[2];
        h.geo[i].r2 = q.r * q.r;
        h.geo[i].mat3 = q.material == 3;
        h.geo[i].emitter = (q.radiance[0] > 0 || q.radiance[1] > 0 || q.radiance[2] > 0);
        h.geo[i].skey = q.material == 0 ? 0 : q.material == 1 ? 2 : 3;
        h.geo[i].point = q.r == 0;
        if (h.geo[i].emitter) h.emit[h.n_emit++] = i;
        const uint64_t bit = 1ull << i;
        if (h.geo[i].emitter) h.m_emitter |= bit;
        if (h.geo[i].point) h.m_point |= bit;
        if (h.geo[i].mat3) h.m_mat3 |= bit;
        if (h.geo[i].skey & 1) h.m_skey1 |= bit;
        if (h.geo[i].skey & 2) h.m_skey2 |= bit;
        if (q.r > 0 && q.radiance[0] > 0) h.mis_light[h.n_mis++] = i;
        if (q.material == 3) h.n_mat3++;
    }
    h.n_non3 = n - h.n_mat3;
    vpt_erand48_jump(2 * h.n_mis + 5, &h.kp_sa, &h.kp_sc);
    h.emit_all_radiance = 1;
    for (int i = 0; i < n; ++i)
        if (!h.geo[i].emitter && (s[i].radiance[0] != 0 || s[i].radiance[1] != 0 || s[i].radiance[2] != 0))
            h.emit_all_radiance = 0;
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipMemcpy(ctx->d_scene, &h, sizeof h, hipMemcpyHostToDevice));
    ctx->h_scene = h;
    ctx->has_scene = 1;
    return VPT_OK;
}

/* the block maxima of `density` (host) for block size B >= 1 on the device (*d_maj, the caller frees) and in
 * the view; the dilated maxima where the view's field is trilinear (vpt_grid.h).  Directly behind them, in the same
 * allocation, the block minima: estimator 15's control grid (vpt_grid_control_of), built whenever the maxima are */
static hipError_t majorant_upload(vpt_grid_view* G, int B, const float* density, float** d_maj)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(G->n, B, nb);
    std::vector<float> maj(2 * (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2]);
    vpt_grid_majorant_control_build(G->n, B, G->interp, density, maj.data());
    hipError_t e = hipMalloc((void**)d_maj, maj.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(*d_maj, maj.data(), maj.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) vpt_grid_view_set_majorant(G, B, *d_maj);
    return e;
}

int vpt_set_density_grid(vpt_context* ctx, const vpt_grid_desc* desc, const float* density)
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "vpt_set_density_grid: NULL context");
    HIP_OK(hipSetDevice(ctx->device));
    if (!desc) {  /* clear */
        HIP_OK(hipDeviceSynchronize());
        if (ctx->d_rho) (void)hipFree(ctx->d_rho);
        if (ctx->d_maj) (void)hipFree(ctx->d_maj);
        if (ctx->d_emit) (void)hipFree(ctx->d_emit);
        ctx->d_rho = nullptr;
        ctx->d_maj = nullptr;
        ctx->d_emit = nullptr;  /* the emission grid goes with the grid whose dimensions it has */
        ctx->h_grid.emit = nullptr;
        ctx->has_grid = 0;  /* maj_block and grid_interp stay: the next grid gets its majorant grid and its mode */
        ctx->grid_from_device = 0;
        return VPT_OK;
    }
    int rc = vpt_int_grid_check(desc, density, "vpt_set_density_grid");
    if (rc) return rc;
    const int32_t dims[3] = {desc->nx, desc->ny, desc->nz};
    const size_t bytes = (size_t)desc->nx * (size_t)desc->ny * (size_t)desc->nz * sizeof(float);
    float* d_rho = nullptr;
    HIP_OK(hipMalloc((void**)&d_rho, bytes));
    vpt_grid_view G;
    vpt_grid_view_init(&G, dims, desc->lo, desc->hi, density, d_rho);  /* the majorant: scanned on the host */
    G.interp = ctx->grid_interp;
    hipError_t e = hipMemcpy(d_rho, density, bytes, hipMemcpyHostToDevice);
    float* d_maj = nullptr;
    if (e == hipSuccess && ctx->maj_block) e = majorant_upload(&G, ctx->maj_block, density, &d_maj);
    if (e == hipSuccess && !ctx->d_grid) e = hipMalloc((void**)&ctx->d_grid, sizeof(vpt_grid_view));
    if (e == hipSuccess) e = hipDeviceSynchronize();  /* nothing in flight reads the previous grid */
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d_rho);
        if (d_maj) (void)hipFree(d_maj);
        return vpt_fail(VPT_E_HIP, "vpt_set_density_grid: %s", hipGetErrorString(e));
    }
    if (ctx->d_rho) (void)hipFree(ctx->d_rho);
    if (ctx->d_maj) (void)hipFree(ctx->d_maj);
    if (ctx->d_emit) (void)hipFree(ctx->d_emit);  /* the previous grid's emission: G.emit is NULL */
    ctx->d_rho = d_rho;
    ctx->d_maj = d_maj;
    ctx->d_emit = nullptr;
    ctx->h_grid = G;
    ctx->has_grid = 1;
    ctx->grid_from_device = 0;
    return VPT_OK;
}

/* majorant_upload for a grid set from device memory: the same 2 nbv floats, built on the device from the context's copy
 * of the voxels (vpt_grid_build.hip) */
static hipError_t majorant_build_device(vpt_grid_view* G, int B, const float* d_rho, float** d_maj)
{
    int32_t nb[3];
    vpt_grid_majorant_counts(G->n, B, nb);
    hipError_t e = hipMalloc((void**)d_maj, 2 * (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2] * sizeof(float));
    if (e == hipSuccess) e = (hipError_t)vpt_int_grid_build(G->n, B, G->interp, d_rho, *d_maj);
    if (e == hipSuccess) vpt_grid_view_set_majorant(G, B, *d_maj);
    return e;
}

/* `bytes` bytes at p are device memory of the context's device, inside one allocation: what the _device entry points ask
 * of a pointer before any kernel or copy touches it */
static int device_pointer_check(const vpt_context* ctx, const void* p, size_t bytes, const char* who, const char* what)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    hipError_t e = hipPointerGetAttributes(&at, p);
    void* base = nullptr;
    size_t size = 0;
    if (e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ctx->device)
        e = hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p);
    else if (e == hipSuccess)
        e = hipErrorInvalidValue;
    if (e == hipSuccess && (const char*)p + bytes > (const char*)base + size) e = hipErrorInvalidValue;
    if (e != hipSuccess) {
        (void)hipGetLastError();  /* a pointer HIP does not know leaves its error behind */
        return vpt_fail(VPT_E_INVALID, "%s: %s is not %zu bytes of device memory on device %d", who, what, bytes, ctx->device);
    }
    return VPT_OK;
}

int vpt_set_density_grid_device(vpt_context* ctx, const vpt_grid_desc* desc, const float* d_density, void* stream)
{
    const char* who = "vpt_set_density_grid_device";
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "%s: NULL context", who);
    if (!desc || !d_density) return vpt_fail(VPT_E_INVALID, "%s: NULL grid", who);
    const int32_t dims[3] = {desc->nx, desc->ny, desc->nz};
    int rc = vpt_int_grid_verdict(desc, vpt_grid_bad(dims, desc->lo, desc->hi, nullptr), who);
    if (rc) return rc;
    const long long nv = (long long)desc->nx * desc->ny * desc->nz;
    const size_t bytes = (size_t)nv * sizeof(float);
    HIP_OK(hipSetDevice(ctx->device));
    rc = device_pointer_check(ctx, d_density, bytes, who, "d_density");
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));  /* the producer has written the voxels */
    float* d_rho = nullptr;
    HIP_OK(hipMalloc((void**)&d_rho, bytes));
    /* the context's own copy first: what is checked is what is kept, whatever the caller does with its tensor */
    hipError_t e = hipMemcpy(d_rho, d_density, bytes, hipMemcpyDeviceToDevice);
    float mx = 0.0f;
    long long bad = -1;
    if (e == hipSuccess) e = (hipError_t)vpt_int_grid_scan(d_rho, nv, &mx, &bad);
    if (e == hipSuccess && bad >= 0) {
        (void)hipFree(d_rho);
        return vpt_int_grid_verdict(desc, 3, who);
    }
    vpt_grid_view G;
    vpt_grid_view_fill(&G, dims, desc->lo, desc->hi, mx, d_rho);
    G.interp = ctx->grid_interp;
    float* d_maj = nullptr;
    if (e == hipSuccess && ctx->maj_block) e = majorant_build_device(&G, ctx->maj_block, d_rho, &d_maj);
    if (e == hipSuccess && !ctx->d_grid) e = hipMalloc((void**)&ctx->d_grid, sizeof(vpt_grid_view));
    if (e == hipSuccess) e = hipDeviceSynchronize();  /* nothing in flight reads the previous grid */
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d_rho);
        if (d_maj) (void)hipFree(d_maj);
        return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (ctx->d_rho) (void)hipFree(ctx->d_rho);
    if (ctx->d_maj) (void)hipFree(ctx->d_maj);
    if (ctx->d_emit) (void)hipFree(ctx->d_emit);  /* the previous grid's emission: G.emit is NULL */
    ctx->d_rho = d_rho;
    ctx->d_maj = d_maj;
    ctx->d_emit = nullptr;
    ctx->h_grid = G;
    ctx->has_grid = 1;
    ctx->grid_from_device = 1;
    return VPT_OK;
}

int vpt_set_emission_grid_device(vpt_context* ctx, const float* d_eps, const double rgb[3], void* stream)
{
    const char* who = "vpt_set_emission_grid_device";
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "%s: NULL context", who);
    if (!d_eps) return vpt_fail(VPT_E_INVALID, "%s: NULL grid", who);  /* clearing stays with vpt_set_emission_grid */
    if (!rgb) return vpt_fail(VPT_E_INVALID, "%s: rgb is NULL", who);
    if (!ctx->has_grid) return vpt_fail(VPT_E_INVALID, "%s: no density grid set (vpt_set_density_grid)", who);
    int rc = vpt_int_emission_check(nullptr, 0, rgb, who);  /* the colour; the voxels below */
    if (rc) return rc;
    vpt_grid_view G = ctx->h_grid;
    const long long nv = (long long)G.n[0] * G.n[1] * G.n[2];
    const size_t bytes = (size_t)nv * sizeof(float);
    HIP_OK(hipSetDevice(ctx->device));
    rc = device_pointer_check(ctx, d_eps, bytes, who, "d_eps");
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    const double head[VPT_EMIT_HEAD] = {rgb[0], rgb[1], rgb[2], 0.0};
    double* d_emit = nullptr;
    HIP_OK(hipMalloc((void**)&d_emit, sizeof head + bytes));
    float* d_vox = (float*)(d_emit + VPT_EMIT_HEAD);
    hipError_t e = hipMemcpy(d_emit, head, sizeof head, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_vox, d_eps, bytes, hipMemcpyDeviceToDevice);
    float mx = 0.0f, at_bad = 0.0f;
    long long bad = -1;
    if (e == hipSuccess) e = (hipError_t)vpt_int_grid_scan(d_vox, nv, &mx, &bad);
    if (e == hipSuccess && bad >= 0) e = hipMemcpy(&at_bad, d_vox + bad, sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && bad >= 0) {
        (void)hipFree(d_emit);
        return vpt_int_emission_bad((double)at_bad, (size_t)bad, who);
    }
    G.emit = d_vox;
    if (e == hipSuccess) e = hipDeviceSynchronize();  /* nothing in flight reads the view or the previous emission grid */
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d_emit);
        return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (ctx->d_emit) (void)hipFree(ctx->d_emit);
    ctx->d_emit = d_emit;
    ctx->h_grid = G;
    return VPT_OK;
}

int vpt_get_grid_majorants(vpt_context* ctx, float* maxima, float* minima, size_t nbv, int32_t nb[3], double* rho_max)
{
    const char* who = "vpt_get_grid_majorants";
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "%s: NULL context", who);
    if (!nb || !rho_max) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    if (!ctx->has_grid) return vpt_fail(VPT_E_INVALID, "%s: no density grid set (vpt_set_density_grid)", who);
    const vpt_grid_view& G = ctx->h_grid;
    for (int a = 0; a < 3; ++a) nb[a] = G.nb[a];
    *rho_max = G.rho_max;
    if (!G.block) return VPT_OK;
    const size_t need = (size_t)G.nb[0] * (size_t)G.nb[1] * (size_t)G.nb[2];
    if (nbv < need) return vpt_fail(VPT_E_INVALID, "%s: room for %zu blocks, the majorant grid has %zu", who, nbv, need);
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipDeviceSynchronize());
    if (maxima) HIP_OK(hipMemcpy(maxima, ctx->d_maj, need * sizeof(float), hipMemcpyDeviceToHost));
    if (minima) HIP_OK(hipMemcpy(minima, ctx->d_maj + need, need * sizeof(float), hipMemcpyDeviceToHost));
    return VPT_OK;
}

int vpt_set_emission_grid(vpt_context* ctx, const float* eps, const double rgb[3])
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "vpt_set_emission_grid: NULL context");
    if (!ctx->has_grid) return vpt_fail(VPT_E_INVALID, "vpt_set_emission_grid: no density grid set (vpt_set_density_grid)");
    vpt_grid_view G = ctx->h_grid;
    double* d_emit = nullptr;
    HIP_OK(hipSetDevice(ctx->device));
    if (eps) {
        if (!rgb) return vpt_fail(VPT_E_INVALID, "vpt_set_emission_grid: rgb is NULL");
        const size_t nv = (size_t)G.n[0] * (size_t)G.n[1] * (size_t)G.n[2];
        int rc = vpt_int_emission_check(eps, nv, rgb, "vpt_set_emission_grid");
        if (rc) return rc;
        const double head[VPT_EMIT_HEAD] = {rgb[0], rgb[1], rgb[2], 0.0};
        HIP_OK(hipMalloc((void**)&d_emit, sizeof head + nv * sizeof(float)));
        hipError_t e = hipMemcpy(d_emit, head, sizeof head, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_emit + VPT_EMIT_HEAD, eps, nv * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d_emit);
            return vpt_fail(VPT_E_HIP, "vpt_set_emission_grid: %s", hipGetErrorString(e));
        }
        G.emit = (const float*)(d_emit + VPT_EMIT_HEAD);
    } else {
        G.emit = nullptr;
    }
    hipError_t e = hipDeviceSynchronize();  /* nothing in flight reads the view or the previous emission grid */
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d_emit) (void)hipFree(d_emit);
        return vpt_fail(VPT_E_HIP, "vpt_set_emission_grid: %s", hipGetErrorString(e));
    }
    if (ctx->d_emit) (void)hipFree(ctx->d_emit);
    ctx->d_emit = d_emit;
    ctx->h_grid = G;
    return VPT_OK;
}

int vpt_set_grid_majorant_block(vpt_context* ctx, int block)
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "vpt_set_grid_majorant_block: NULL context");
    if (block < 0) return vpt_fail(VPT_E_INVALID, "vpt_set_grid_majorant_block: block %d (0 = off, else >= 1 voxels per axis)", block);
    if (!ctx->has_grid) {  /* applied when a grid is set */
        ctx->maj_block = block;
        return VPT_OK;
    }
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipDeviceSynchronize());  /* nothing in flight reads the view or the previous majorant grid */
    vpt_grid_view G = ctx->h_grid;
    float* d_maj = nullptr;
    hipError_t e = hipSuccess;
    if (block && ctx->grid_from_device) {  /* built where the voxels are */
        e = majorant_build_device(&G, block, ctx->d_rho, &d_maj);
    } else if (block) {  /* the block maxima are scanned on the host, from the device's copy of the voxels */
        const size_t nv = (size_t)G.n[0] * (size_t)G.n[1] * (size_t)G.n[2];
        std::vector<float> rho(nv);
        e = hipMemcpy(rho.data(), ctx->d_rho, nv * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = majorant_upload(&G, block, rho.data(), &d_maj);
    } else {
        vpt_grid_view_set_majorant(&G, 0, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d_maj) (void)hipFree(d_maj);
        return vpt_fail(VPT_E_HIP, "vpt_set_grid_majorant_block: %s", hipGetErrorString(e));
    }
    if (ctx->d_maj) (void)hipFree(ctx->d_maj);
    ctx->d_maj = d_maj;
    ctx->h_grid = G;
    ctx->maj_block = block;
    return VPT_OK;
}

int vpt_set_hetero_mis_fraction(vpt_context* ctx, double q)
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "vpt_set_hetero_mis_fraction: NULL context");
    if (!(q >= 0.0 && q <= 1.0))  /* a NaN fails both */
        return vpt_fail(VPT_E_INVALID, "vpt_set_hetero_mis_fraction: q %g (finite, in [0, 1])", q);
    ctx->mis_fraction = q;  /* a kernel argument of the next launch: nothing in flight reads it */
    return VPT_OK;
}

int vpt_set_medium_colour(vpt_context* ctx, const double absorb[3], const double scatter[3])
{
    vpt_clear_error();
    if (!ctx || !absorb || !scatter) return vpt_fail(VPT_E_INVALID, "vpt_set_medium_colour: NULL argument");
    for (int k = 0; k < 3; ++k)
        if (!is_finite(absorb[k]) || !is_finite(scatter[k]) || absorb[k] < 0 || scatter[k] < 0)
            return vpt_fail(VPT_E_INVALID, "vpt_set_medium_colour: channel %d: absorb %g, scatter %g (finite, >= 0)", k,
                            absorb[k], scatter[k]);
    for (int k = 0; k < 3; ++k) {  /* kernel arguments of the next launch: nothing in flight reads them */
        ctx->chroma_a[k] = absorb[k];
        ctx->chroma_s[k] = scatter[k];
    }
    return VPT_OK;
}

int vpt_set_grid_interpolation(vpt_context* ctx, int mode)
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "vpt_set_grid_interpolation: NULL context");
    if (mode != VPT_GRID_NEAREST && mode != VPT_GRID_TRILINEAR)
        return vpt_fail(VPT_E_INVALID, "vpt_set_grid_interpolation: mode %d (0 = nearest, 1 = trilinear)", mode);
    if (!ctx->has_grid || ctx->h_grid.interp == mode) {  /* applied when a grid is set */
        ctx->grid_interp = mode;
        return VPT_OK;
    }
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipDeviceSynchronize());  /* nothing in flight reads the view or the previous majorant grid */
    vpt_grid_view G = ctx->h_grid;
    G.interp = mode;
    float* d_maj = nullptr;
    hipError_t e = hipSuccess;
    if (G.block && ctx->grid_from_device) {  /* the majorant grid follows the mode: built where the voxels are */
        e = majorant_build_device(&G, G.block, ctx->d_rho, &d_maj);
    } else if (G.block) {  /* the majorant grid follows the mode: rebuilt from the device's copy of the voxels */
        const size_t nv = (size_t)G.n[0] * (size_t)G.n[1] * (size_t)G.n[2];
        std::vector<float> rho(nv);
        e = hipMemcpy(rho.data(), ctx->d_rho, nv * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = majorant_upload(&G, G.block, rho.data(), &d_maj);
    }
    if (e == hipSuccess) e = hipMemcpy(ctx->d_grid, &G, sizeof G, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d_maj) (void)hipFree(d_maj);
        return vpt_fail(VPT_E_HIP, "vpt_set_grid_interpolation: %s", hipGetErrorString(e));
    }
    if (G.block) {
        if (ctx->d_maj) (void)hipFree(ctx->d_maj);
        ctx->d_maj = d_maj;
    }
    ctx->h_grid = G;
    ctx->grid_interp = mode;
    return VPT_OK;
}

/* how every device probe of the density grid opens; args_ok: the context and the entry point's arrays are there */
static int grid_probe_open(const vpt_context* ctx, const char* who, bool args_ok)
{
    vpt_clear_error();
    if (!args_ok) return vpt_fail(VPT_E_INVALID, "%s: bad arguments", who);
    if (!ctx->has_grid) return vpt_fail(VPT_E_INVALID, "%s: no density grid set (vpt_set_density_grid)", who);
    return VPT_OK;
}

/* the chromatic probes' coefficients (chroma_coef), or the refusal of a medium they cannot walk */
static int probe_chroma_coef(const vpt_context* ctx, const char* who, double sigma_a, double sigma_s, ChromaCoef* cc)
{
    if (!is_finite(sigma_a) || !is_finite(sigma_s) || sigma_a < 0 || sigma_s < 0)
        return vpt_fail(VPT_E_INVALID, "%s: sigma_a/sigma_s must be finite and >= 0", who);
    *cc = chroma_coef(ctx, sigma_a, sigma_s);
    for (int k = 0; k < 3; ++k)
        if (!(cc->st[k] > 0)) return vpt_fail(VPT_E_INVALID, "%s: channel %d has no extinction", who, k);
    return VPT_OK;
}

/* vpt_grid_probe (lm false: the global-majorant track whatever the context's setting) and vpt_grid_probe_lm */
static int grid_probe(vpt_context* ctx, bool lm, double sigma_t, const vpt_ray* rays, const double* tmax,
                      const uint64_t* states, int n, double* tau, double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    const char* who = lm ? "vpt_grid_probe_lm" : "vpt_grid_probe";
    if (int rc = grid_probe_open(ctx, who, ctx && rays && tmax && states && tau && t_coll && states_out && n >= 0)) return rc;
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double *dtau = st.alloc<double>(nn), *dtc = st.alloc<double>(nn);
    uint32_t* dst = st.alloc_if(steps, nn);
    /* the existing probe keeps its global-majorant behaviour: a copy of the view without the majorant grid */
    const vpt_grid_view* dview = ctx->d_grid;
    if (!lm && ctx->h_grid.block > 0) {
        vpt_grid_view G = ctx->h_grid;
        vpt_grid_view_set_majorant(&G, 0, nullptr);
        vpt_grid_view* dplain = st.alloc<vpt_grid_view>(1);
        st.up(dplain, &G, 1);
        dview = dplain;
    }
    st.launch([&] {
        hetero_unit(VPT_HETERO_FREE, ctx->h_grid.interp != 0, false)
            .grid_probe_launch(dview, lm && ctx->h_grid.block > 0, sigma_t, st.dr, st.dtm, st.ds, n, dtau, dtc, st.dso, dst);
    });
    st.down(tau, dtau, nn);
    st.down(t_coll, dtc, nn);
    st.down(states_out, st.dso, nn);
    st.down(steps, dst, nn);
    return st.status(who);
}

int vpt_grid_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                   int n, double* tau, double* t_coll, uint64_t* states_out)
{
    return grid_probe(ctx, false, sigma_t, rays, tmax, states, n, tau, t_coll, states_out, nullptr);
}

int vpt_grid_probe_lm(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                      int n, double* tau, double* t_coll, uint64_t* states_out, uint32_t* steps)
{
    return grid_probe(ctx, true, sigma_t, rays, tmax, states, n, tau, t_coll, states_out, steps);
}

int vpt_grid_ratio_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax,
                         const uint64_t* states, int n, double* that, uint64_t* states_out, uint32_t* steps)
{
    if (int rc = grid_probe_open(ctx, "vpt_grid_ratio_probe", ctx && rays && tmax && states && that && states_out && n >= 0))
        return rc;
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double* dth = st.alloc<double>(nn);
    uint32_t* dst = st.alloc_if(steps, nn);
    st.launch([&] {
        hetero_unit(VPT_HETERO_RATIO, ctx->h_grid.interp != 0, false)
            .grid_ratio_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, sigma_t, st.dr, st.dtm, st.ds, n, dth, st.dso, dst);
    });
    st.down(that, dth, nn);
    st.down(states_out, st.dso, nn);
    st.down(steps, dst, nn);
    return st.status("vpt_grid_ratio_probe");
}

int vpt_grid_eqa_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const double* light,
                       const uint64_t* states, int n, double* psurf, double* dist, double* pdf, double* T, double* rho_t,
                       uint64_t* states_out)
{
    if (int rc = grid_probe_open(ctx, "vpt_grid_eqa_probe",
                                 ctx && rays && tmax && light && states && psurf && dist && pdf && T && rho_t && states_out &&
                                     n >= 0))
        return rc;
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double* dl = st.alloc<double>(3 * nn);
    double* dres = st.alloc<double>(5 * nn);  /* the five result arrays, one behind the other */
    st.up(dl, light, 3 * nn);
    st.launch([&] {
        hetero_unit(ctx, VPT_HETERO_EQUIANGULAR)
            .grid_eqa_probe_launch(ctx->d_grid, sigma_t, st.dr, st.dtm, dl, st.ds, n, dres, dres + nn, dres + 2 * nn, dres + 3 * nn,
                                   dres + 4 * nn, st.dso);
    });
    double* const res[5] = {psurf, dist, pdf, T, rho_t};
    for (int k = 0; k < 5; ++k) st.down(res[k], dres + (size_t)k * nn, nn);
    st.down(states_out, st.dso, nn);
    return st.status("vpt_grid_eqa_probe");
}

int vpt_grid_mis_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const double* light,
                       const uint64_t* states, int n, double* psurf, int32_t* strategy, double* dist, double* pdf, double* pe,
                       double* T, double* rho_t, uint32_t* steps, uint64_t* states_out)
{
    if (int rc = grid_probe_open(ctx, "vpt_grid_mis_probe",
                                 ctx && rays && tmax && light && states && psurf && strategy && dist && pdf && pe && T && rho_t &&
                                     steps && states_out && n >= 0))
        return rc;
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double* dl = st.alloc<double>(3 * nn);
    double* dres = st.alloc<double>(6 * nn);  /* the six result arrays of doubles, one behind the other */
    int32_t* dsg = st.alloc<int32_t>(nn);
    uint32_t* dst = st.alloc<uint32_t>(nn);
    st.up(dl, light, 3 * nn);
    st.launch([&] {
        hetero_unit(ctx, VPT_HETERO_MIS)
            .grid_mis_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, sigma_t, ctx->mis_fraction, st.dr, st.dtm, dl, st.ds, n,
                                   dres, dsg, dst, st.dso);
    });
    double* const res[6] = {psurf, dist, pdf, pe, T, rho_t};
    for (int k = 0; k < 6; ++k) st.down(res[k], dres + (size_t)k * nn, nn);
    st.down(strategy, dsg, nn);
    st.down(steps, dst, nn);
    st.down(states_out, st.dso, nn);
    return st.status("vpt_grid_mis_probe");
}

int vpt_grid_chroma_probe(vpt_context* ctx, double sigma_a, double sigma_s, const vpt_ray* rays, const double* tmax,
                          const uint64_t* states, int n, int32_t* hero, double* t_coll, double* tau, double* w, uint32_t* steps,
                          uint64_t* states_out)
{
    const char* who = "vpt_grid_chroma_probe";
    ChromaCoef cc;
    int rc = grid_probe_open(ctx, who,
                             ctx && rays && tmax && states && hero && t_coll && tau && w && steps && states_out && n >= 0);
    if (!rc) rc = probe_chroma_coef(ctx, who, sigma_a, sigma_s, &cc);
    if (rc || n == 0) return rc;
    ProbeStaging st;
    rc = st.stage(ctx->device, rays, states, tmax, n);
    if (rc) return rc;
    const size_t nn = st.nn;
    double* dres = st.alloc<double>(5 * nn);  /* t_coll, tau and the three weights, one array behind the other */
    int32_t* dh = st.alloc<int32_t>(nn);
    uint32_t* dst = st.alloc<uint32_t>(nn);
    st.launch([&] {
        hetero_unit(ctx, VPT_HETERO_CHROMATIC)
            .grid_chroma_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, cc, st.dr, st.dtm, st.ds, n, dres, dh, dst, st.dso);
    });
    st.down(t_coll, dres, nn);
    st.down(tau, dres + nn, nn);
    st.down(w, dres + 2 * nn, 3 * nn);  /* w[c * n + i] */
    st.down(hero, dh, nn);
    st.down(steps, dst, nn);
    st.down(states_out, st.dso, nn);
    return st.status(who);
}

int vpt_grid_spectral_probe(vpt_context* ctx, double sigma_a, double sigma_s, const vpt_ray* rays, const double* tmax,
                            const double* beta, const uint64_t* states, int n, double* t_coll, double* w, uint32_t* steps,
                            uint64_t* states_out, double* T, uint32_t* ratio_steps, uint64_t* ratio_states_out)
{
    const char* who = "vpt_grid_spectral_probe";
    ChromaCoef cc;
    int rc = grid_probe_open(ctx, who,
                             ctx && rays && tmax && states && t_coll && w && steps && states_out && T && ratio_steps &&
                                 ratio_states_out && n >= 0);
    if (!rc) rc = probe_chroma_coef(ctx, who, sigma_a, sigma_s, &cc);
    if (rc || n == 0) return rc;
    ProbeStaging st;
    rc = st.stage(ctx->device, rays, states, tmax, n);
    if (rc) return rc;
    const size_t nn = st.nn;
    uint64_t* dro = st.alloc<uint64_t>(nn);
    double* db = beta ? st.alloc<double>(3 * nn) : nullptr;
    double* dres = st.alloc<double>(4 * nn);  /* t_coll and the three weights, one array behind the other */
    double* dT = st.alloc<double>(3 * nn);
    uint32_t *dst = st.alloc<uint32_t>(nn), *drs = st.alloc<uint32_t>(nn);
    if (beta) st.up(db, beta, 3 * nn);
    st.launch([&] {
        const vpt_hetero_unit& u = hetero_unit(ctx, VPT_HETERO_SPECTRAL);
        u.grid_spectral_track_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, cc, st.dr, st.dtm, db, st.ds, n, dres, dst, st.dso);
        u.grid_spectral_ratio_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, cc, st.dr, st.dtm, st.ds, n, dT, drs, dro);
    });
    st.down(t_coll, dres, nn);
    st.down(w, dres + nn, 3 * nn);  /* w[c * n + i] */
    st.down(steps, dst, nn);
    st.down(states_out, st.dso, nn);
    st.down(T, dT, 3 * nn);  /* T[c * n + i] */
    st.down(ratio_steps, drs, nn);
    st.down(ratio_states_out, dro, nn);
    return st.status(who);
}

int vpt_grid_residual_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                            int n, double* that, double* tauc, uint64_t* states_out, uint32_t* steps)
{
    if (int rc = grid_probe_open(ctx, "vpt_grid_residual_probe",
                                 ctx && rays && tmax && states && that && tauc && states_out && n >= 0))
        return rc;
    if (ctx->h_grid.block < 1)
        return vpt_fail(VPT_E_INVALID, "vpt_grid_residual_probe: no majorant block set (vpt_set_grid_majorant_block)");
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double *dth = st.alloc<double>(nn), *dtc = st.alloc<double>(nn);
    uint32_t* dst = st.alloc_if(steps, nn);
    st.launch([&] {
        hetero_unit(ctx, VPT_HETERO_RESIDUAL)
            .grid_residual_probe_launch(ctx->d_grid, sigma_t, st.dr, st.dtm, st.ds, n, dth, dtc, st.dso, dst);
    });
    st.down(that, dth, nn);
    st.down(tauc, dtc, nn);
    st.down(states_out, st.dso, nn);
    st.down(steps, dst, nn);
    return st.status("vpt_grid_residual_probe");
}

int vpt_grid_emission_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                            int n, double* t_coll, double* esum, uint64_t* states_out, uint32_t* steps)
{
    vpt_clear_error();
    if (!ctx || !rays || !tmax || !states || !t_coll || !esum || !states_out || n < 0)
        return vpt_fail(VPT_E_INVALID, "vpt_grid_emission_probe: bad arguments");
    if (!ctx->has_grid || !ctx->h_grid.emit)
        return vpt_fail(VPT_E_INVALID, "vpt_grid_emission_probe: no emission grid set (vpt_set_emission_grid)");
    if (n == 0) return VPT_OK;
    ProbeStaging st;
    if (int rc = st.stage(ctx->device, rays, states, tmax, n)) return rc;
    const size_t nn = st.nn;
    double *dtc = st.alloc<double>(nn), *des = st.alloc<double>(nn);
    uint32_t* dst = st.alloc_if(steps, nn);
    st.launch([&] {
        hetero_unit(VPT_HETERO_FREE, ctx->h_grid.interp != 0, true)
            .grid_emission_probe_launch(ctx->d_grid, ctx->h_grid.block > 0, sigma_t, st.dr, st.dtm, st.ds, n, dtc, des, st.dso,
                                        dst);
    });
    st.down(t_coll, dtc, nn);
    st.down(esum, des, nn);
    st.down(states_out, st.dso, nn);
    st.down(steps, dst, nn);
    return st.status("vpt_grid_emission_probe");
}

int vpt_render_device(vpt_context* ctx, const vpt_params* p, void* d_out, void* stream)
{
    vpt_clear_error();
    if (!d_out) return vpt_fail(VPT_E_INVALID, "vpt_render_device: d_out is NULL");
    KParams K;
    int rc = build_kparams(ctx, p, d_out, K);
    if (rc) return rc;
    HIP_OK(hipSetDevice(ctx->device));
    return launch_render<false>(ctx, K, (hipStream_t)stream);
}

int vpt_render(vpt_context* ctx, const vpt_params* p, void* h_out)
{
    vpt_clear_error();
    if (!h_out) return vpt_fail(VPT_E_INVALID, "vpt_render: h_out is NULL");
    KParams K;
    int rc = build_kparams(ctx, p, (void*)1, K);
    if (rc) return rc;
    HIP_OK(hipSetDevice(ctx->device));
    size_t bytes = (size_t)K.shard_rows * (size_t)K.w * 3 * (K.fb == VPT_FB_F32 ? sizeof(float) : sizeof(double));
    if (bytes == 0) return VPT_OK;
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, bytes));
    K.out = d;
    rc = launch_render<false>(ctx, K, nullptr);
    hipError_t e = rc ? hipSuccess : hipMemcpy(h_out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "vpt_render: %s", hipGetErrorString(e));
    return check_guard(ctx, "vpt_render");
}

int vpt_count_work(vpt_context* ctx, const vpt_params* p, uint64_t* tests, uint64_t* iterations)
{
    vpt_clear_error();
    KParams K;
    int rc = build_kparams(ctx, p, (void*)1, K);
    if (rc) return rc;
    HIP_OK(hipSetDevice(ctx->device));
    size_t bytes = (size_t)K.shard_rows * (size_t)K.w * 3 * (K.fb == VPT_FB_F32 ? sizeof(float) : sizeof(double));
    if (bytes == 0) {
        if (tests) *tests = 0;
        if (iterations) *iterations = 0;
        return VPT_OK;
    }
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, bytes));
    K.out = d;
    K.counters = ctx->d_counters;
    unsigned long long hc[3] = {0, 0, 0};
    hipError_t e = hipMemset(ctx->d_counters, 0, sizeof hc);
    if (e == hipSuccess) {
        rc = launch_render<true>(ctx, K, nullptr);
        if (!rc) e = hipMemcpy(hc, ctx->d_counters, sizeof hc, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "vpt_count_work: %s", hipGetErrorString(e));
    if (hc[2])  /* the kill-predicting rings would lose bit-exactness on this scene (vpt_pool.h) */
        return vpt_fail(VPT_E_INTERNAL, "vpt_count_work: %llu events drew a different number of samples than the "
                        "kill prediction assumes", (unsigned long long)hc[2]);
    if (tests) *tests = hc[0];
    if (iterations) *iterations = hc[1];
    return VPT_OK;
}

/* stats: vpt_debug_hetero_steps' two device counters (estimator 10), else NULL */
static int trace_batch(vpt_context* ctx, const vpt_medium* m, const vpt_ray* rays, const uint64_t* states, int n,
                       double* out_rgb, uint64_t* out_states, unsigned long long* stats);

int vpt_trace_batch(vpt_context* ctx, const vpt_medium* m, const vpt_ray* rays, const uint64_t* states, int n,
                    double* out_rgb, uint64_t* out_states)
{
    return trace_batch(ctx, m, rays, states, n, out_rgb, out_states, nullptr);
}

}  // extern "C"

static int trace_batch(vpt_context* ctx, const vpt_medium* m, const vpt_ray* rays, const uint64_t* states, int n,
                       double* out_rgb, uint64_t* out_states, unsigned long long* stats)
{
    vpt_clear_error();
    if (!ctx || !rays || !states || !out_rgb || n < 0) return vpt_fail(VPT_E_INVALID, "vpt_trace_batch: bad arguments");
    if (!ctx->has_scene) return vpt_fail(VPT_E_INVALID, "no scene set (vpt_set_scene)");
    int rc = check_medium(m);
    if (!rc) rc = check_march(ctx, m);
    if (rc) return rc;
    if (n == 0) return VPT_OK;
    HIP_OK(hipSetDevice(ctx->device));
    Staging st;
    const size_t nn = (size_t)n;
    vpt_ray* dr = st.alloc<vpt_ray>(nn);
    uint64_t *ds = st.alloc<uint64_t>(nn), *dso = st.alloc<uint64_t>(nn);
    double* dout = st.alloc<double>(3 * nn);
    st.up(dr, rays, nn);
    st.up(ds, states, nn);
    st.launch([&] {
        Medium mm{m->sigma_a, m->sigma_s, m->hg_g, m->max_depth, m->march_step, m->march_light};
        const dim3 grid = vpt_ray_grid(n), block(256);
        switch (m->estimator) {
        case 0: trace_batch_kernel<0><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 1: trace_batch_kernel<1><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 2: trace_batch_kernel<2><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 3: trace_batch_kernel<3><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 4: trace_batch_kernel<4><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 5: trace_batch_kernel<5><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 6: trace_batch_kernel<6><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 7: trace_batch_kernel<7><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case 8: trace_batch_kernel<8><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        case VPT_HETERO_FREE:
        case VPT_HETERO_RATIO:
        case VPT_HETERO_EQUIANGULAR:
        case VPT_HETERO_MIS:
        case VPT_HETERO_CHROMATIC:
        case VPT_HETERO_RESIDUAL:
        case VPT_HETERO_SPECTRAL:
            hetero_unit(ctx, m->estimator).trace_launch(m->estimator, dr, ds, n, mm, ctx->d_scene, ctx->d_grid,
                                                        hetero_args(ctx, m->sigma_a, m->sigma_s, stats), dout, dso);
            break;
        default: trace_batch_kernel<9><<<grid, block>>>(dr, ds, n, mm, m->hg_g, ctx->d_scene, dout, dso); break;
        }
    });
    st.down(out_rgb, dout, 3 * nn);
    st.down(out_states, dso, nn);
    return st.status("vpt_trace_batch");
}

extern "C" {

int vpt_punctual_volumetric(vpt_context* ctx, int idsource, const double* x, int n, double phase, double sigma_t,
                            double sigma_s, double* out_rgb)
{
    vpt_clear_error();
    if (!ctx || !x || !out_rgb || n < 0) return vpt_fail(VPT_E_INVALID, "vpt_punctual_volumetric: bad arguments");
    if (!ctx->has_scene) return vpt_fail(VPT_E_INVALID, "no scene set (vpt_set_scene)");
    if (idsource < 0 || idsource >= ctx->h_scene.n)
        return vpt_fail(VPT_E_INVALID, "idsource %d is not a sphere of the scene (%d)", idsource, ctx->h_scene.n);
    if (n == 0) return VPT_OK;
    HIP_OK(hipSetDevice(ctx->device));
    Staging st;
    const size_t nn = (size_t)n;
    double *dx = st.alloc<double>(3 * nn), *dout = st.alloc<double>(3 * nn);
    st.up(dx, x, 3 * nn);
    st.launch([&] {
        punctual_kernel<<<vpt_ray_grid(n), dim3(256)>>>(idsource, dx, n, phase, sigma_t, sigma_s, ctx->d_scene, dout);
    });
    st.down(out_rgb, dout, 3 * nn);
    return st.status("vpt_punctual_volumetric");
}

int vpt_ray_marching_batch(vpt_context* ctx, double sigma_t, double sigma_s, double steps, const vpt_ray* rays,
                           const uint64_t* states, int n, double* out_rgb, double* x_new, int32_t* idsource,
                           uint64_t* out_states)
{
    vpt_clear_error();
    if (!ctx || !rays || !states || !out_rgb || !x_new || !idsource || n < 0)
        return vpt_fail(VPT_E_INVALID, "vpt_ray_marching_batch: bad arguments");
    if (!ctx->has_scene) return vpt_fail(VPT_E_INVALID, "no scene set (vpt_set_scene)");
    if (ctx->h_scene.n < 6) return vpt_fail(VPT_E_INVALID, "rayMarching samples sphere 5: the scene has %d spheres", ctx->h_scene.n);
    if (!is_finite(steps) || !(steps > 0)) return vpt_fail(VPT_E_INVALID, "steps must be finite and > 0");
    if (n == 0) return VPT_OK;
    HIP_OK(hipSetDevice(ctx->device));
    Staging st;
    const size_t nn = (size_t)n;
    vpt_ray* dr = st.alloc<vpt_ray>(nn);
    uint64_t *ds = st.alloc<uint64_t>(nn), *dso = st.alloc<uint64_t>(nn);
    double *dout = st.alloc<double>(3 * nn), *dxn = st.alloc<double>(3 * nn);
    int32_t* did = st.alloc<int32_t>(nn);
    st.up(dr, rays, nn);
    st.up(ds, states, nn);
    st.up(dxn, x_new, 3 * nn);
    st.up(did, idsource, nn);
    st.launch([&] {
        ray_marching_kernel<<<vpt_ray_grid(n), dim3(256)>>>(dr, ds, n, sigma_t, sigma_s, steps, ctx->d_scene, dout, dxn, did, dso);
    });
    st.down(out_rgb, dout, 3 * nn);
    st.down(x_new, dxn, 3 * nn);
    st.down(idsource, did, nn);
    st.down(out_states, dso, nn);
    return st.status("vpt_ray_marching_batch");
}

int vpt_math_probe(vpt_context* ctx, int fn, const double* x, const double* y, double* out, int n)
{
    vpt_clear_error();
    if (!ctx || !x || !y || !out || n < 0) return vpt_fail(VPT_E_INVALID, "vpt_math_probe: bad arguments");
    if (n == 0) return VPT_OK;
    HIP_OK(hipSetDevice(ctx->device));
    Staging st;
    const size_t nn = (size_t)n;
    double *dx = st.alloc<double>(nn), *dy = st.alloc<double>(nn), *dout = st.alloc<double>(nn);
    st.up(dx, x, nn);
    st.up(dy, y, nn);
    st.launch([&] { math_probe_kernel<<<vpt_ray_grid(n), dim3(256)>>>(fn, dx, dy, dout, n); });
    st.down(out, dout, nn);
    return st.status("vpt_math_probe");
}

int vpt_phase_probe(vpt_context* ctx, double g, const double din[3], const uint64_t* states, int n, double* dirs,
                    uint64_t* states_out, const double* wl, int nw, double* values)
{
    vpt_clear_error();
    if (!ctx || !din || n < 0 || nw < 0 || (n > 0 && (!states || !dirs || !states_out)) || (nw > 0 && (!wl || !values)))
        return vpt_fail(VPT_E_INVALID, "vpt_phase_probe: bad arguments");
    if (!is_finite(g) || g <= -1.0 || g >= 1.0) return vpt_fail(VPT_E_INVALID, "vpt_phase_probe: g must be in (-1, 1)");
    const int m = n > nw ? n : nw;
    if (m == 0) return VPT_OK;
    HIP_OK(hipSetDevice(ctx->device));
    Staging st;
    const size_t n1 = (size_t)(n > 0 ? n : 1), w1 = (size_t)(nw > 0 ? nw : 1);
    uint64_t *dX = st.alloc<uint64_t>(n1), *dXo = st.alloc<uint64_t>(n1);
    double *dd = st.alloc<double>(3 * n1), *dw = st.alloc<double>(3 * w1), *dv = st.alloc<double>(w1);
    if (n > 0) st.up(dX, states, (size_t)n);
    if (nw > 0) st.up(dw, wl, 3 * (size_t)nw);
    st.launch([&] {
        phase_probe_kernel<<<vpt_ray_grid(m), dim3(256)>>>(g, din[0], din[1], din[2], dX, n, dd, dXo, dw, nw, dv);
    });
    if (n > 0) st.down(dirs, dd, 3 * (size_t)n);
    if (n > 0) st.down(states_out, dXo, (size_t)n);
    if (nw > 0) st.down(values, dv, (size_t)nw);
    return st.status("vpt_phase_probe");
}

}  // extern "C"

/* Debug (not part of include/vpt.h): scheduler statistics of the last pool launch made with
 * VPT_POOL_STATS=1 -- NSTATS counters, layout in vpt_pool.h. */
extern "C" int vpt_debug_pool_stats(unsigned long long* out)
{
    if (!g_pool_stats || !out) return VPT_E_INVALID;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, g_pool_stats, NSTATS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return VPT_OK;
}

/* measurement (not part of include/vpt.h; scripts/hetero_time.py): vpt_trace_batch for estimator 10 that also
 * counts the delta-tracking calls of the batch and their tentative steps */
extern "C" int vpt_debug_hetero_steps(vpt_context* ctx, const vpt_medium* m, const vpt_ray* rays, const uint64_t* states,
                                      int n, double* out_rgb, uint64_t* tracks, uint64_t* steps)
{
    if (!ctx || !m || m->estimator != VPT_HETERO_FREE || !tracks || !steps)
        return vpt_fail(VPT_E_INVALID, "vpt_debug_hetero_steps: bad arguments");
    HIP_OK(hipSetDevice(ctx->device));
    unsigned long long hc[2] = {0, 0};
    HIP_OK(hipMemset(ctx->d_counters, 0, sizeof hc));
    const int rc = trace_batch(ctx, m, rays, states, n, out_rgb, nullptr, ctx->d_counters);
    if (rc) return rc;
    HIP_OK(hipMemcpy(hc, ctx->d_counters, sizeof hc, hipMemcpyDeviceToHost));
    *tracks = hc[0];
    *steps = hc[1];
    return VPT_OK;
}

/* debug: the section timers of builds made with -DVPT_SECTIONS=1 (vpt_device.h), 3 x SECT_N
 * counters (cycles, entries, active lanes) accumulated since the last call; returns VPT_E_INVALID otherwise */
extern "C" int vpt_debug_sections(unsigned long long* out)
{
#if VPT_SECTIONS
    if (!out) return VPT_E_INVALID;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpyFromSymbol(out, HIP_SYMBOL(vpt::g_vpt_sect), 3 * vpt::SECT_N * sizeof(unsigned long long)));
    static const unsigned long long zero[3 * vpt::SECT_N] = {};
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(vpt::g_vpt_sect), zero, sizeof(zero)));
#if VPT_MIS_TU
    if (vpt_mis_sections_add(out)) return vpt_fail(VPT_E_HIP, "section timers of the EST = 1 unit");
#endif
    return VPT_OK;
#else
    (void)out;
    return VPT_E_INVALID;
#endif
}

/* debug: the per-workgroup timeline of the last VPT_POOL_STATS launch (vpt_pool.h TL0), 3 x TL_MAXWG */
extern "C" int vpt_debug_pool_timeline(unsigned long long* out)
{
    if (!g_pool_stats || !out) return VPT_E_INVALID;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, g_pool_stats + TL0, 3 * TL_MAXWG * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return VPT_OK;
}

/* debug: the per-launch bound of ctx's pool renders lowered to 2^log2 samples per workgroup (0..26; 26 =
 * the production bound), so that a small render takes the multi-launch path that BASELINE configs[4]
 * (2^34 samples per GPU) takes in production (tests/test_gpu_parity.py).  Returns VPT_E_INVALID
 * outside 0..26. */
extern "C" int vpt_debug_set_launch_bound(vpt_context* ctx, int log2)
{
    if (!ctx || log2 < 0 || log2 > LAUNCH_LOG2_MAX) return vpt_fail(VPT_E_INVALID, "launch bound 2^%d outside 2^0..2^26", log2);
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->launch_log2 = log2;
    return VPT_OK;
}

/* debug, host only (no GPU): the launches a pool render of p's shard makes on `blocks` workgroups with the
 * bound 2^log2 -- the same units (tiles of 8 x 8 pixels x chunks, vpt_chunks.h) and the same split as
 * launch_pool.  Writes up to cap (unit0, nunits) pairs; returns the number of launches, or < 0. */
/* debug: task slots per workgroup pool of this build (vpt_pool.h POOL) */
extern "C" int vpt_debug_pool_tasks(void) { return POOL; }


extern "C" int64_t vpt_debug_launch_plan(const vpt_params* p, int blocks, int log2, uint64_t* unit0, uint64_t* nunits,
                                         int64_t cap)
{
    if (!p || blocks < 1 || log2 < 0 || log2 > LAUNCH_LOG2_MAX || p->spp <= 0 || p->width <= 0 || p->chunk_spp < 0)
        return VPT_E_INVALID;
    const int rows = vpt_shard_rows(p);
    const int chunk = p->chunk_spp > 0 ? (p->chunk_spp < p->spp ? p->chunk_spp : p->spp) : vpt_auto_chunk(p->spp);
    const vpt_chunk_layout lay = vpt_chunks(p->spp, chunk, p->chunk_spp == 0);
    const uint64_t units = (uint64_t)((p->width + 7) / 8) * (uint64_t)((rows + 7) / 8) * 64u * (uint64_t)lay.n;
    /* launch_pool's clamp: no more workgroups than the units fill (one pool of POOL tasks each) */
    const uint64_t need = (units + POOL - 1) / POOL;
    if ((uint64_t)blocks > need) blocks = (int)need;
    const uint64_t max_units = launch_max_units(blocks, lay.C, log2);
    int64_t k = 0;
    for (uint64_t u0 = 0; u0 < units; u0 += max_units, ++k) {
        if (k < cap && unit0 && nunits) {
            unit0[k] = u0;
            nunits[k] = units - u0 < max_units ? units - u0 : max_units;
        }
    }
    return k;
}

/* Test hooks of two internal checks (tests/test_gpu_parity.py), each undone by passing 0:
 * vpt_debug_karg_guard: bias != 0 makes pool_kernel's argument-layout guard fail (and clears the sticky
 * flag when 0), so vpt_render must return VPT_E_INTERNAL;
 * vpt_debug_kill_jump: the kill prediction's surface jump (DevScene::kp_sa, kp_sc) set to `draws` draws
 * instead of 2 n_mis + 5, so vpt_count_work's draw-count check must fail (0: the scene's own). */
extern "C" int vpt_debug_karg_guard(vpt_context* ctx, unsigned bias)
{
    vpt_clear_error();
    if (!ctx) return vpt_fail(VPT_E_INVALID, "NULL context");
    HIP_OK(hipSetDevice(ctx->device));
    ctx->guard_bias = bias;
    if (bias == 0) HIP_OK(hipMemset(ctx->d_guard, 0, sizeof(unsigned)));
    return VPT_OK;
}
extern "C" int vpt_debug_kill_jump(vpt_context* ctx, int draws)
{
    vpt_clear_error();
    if (!ctx || !ctx->has_scene) return vpt_fail(VPT_E_INVALID, "NULL context or no scene");
    if (draws < 0) return vpt_fail(VPT_E_INVALID, "draws must be >= 0");
    DevScene& h = ctx->h_scene;
    vpt_erand48_jump(draws > 0 ? draws : 2 * h.n_mis + 5, &h.kp_sa, &h.kp_sc);
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipMemcpy(ctx->d_scene, &h, sizeof h, hipMemcpyHostToDevice));
    return VPT_OK;
}
