/*
 * vpt_accum.hip -- the progressive accumulator (vpt_accum_* of include/vpt.h): kernels and device half.
 *
 * Data: per pixel of the shard sum[3] and (s1, s2) in FP64, per 8x8 tile a level count and an error, and a
 * partial-sum buffer that holds the chunk levels of ONE pass (levels x rows x w x 24 B) instead of all of a
 * render's.  A pass renders `n` further levels [k0, k0 + n) for a list of tiles with the pool kernel
 * (vpt_int_pool_pass: the uniform layout's unit range of those levels, PoolParams::tile_map for the list),
 * then accum_kernel folds the partials into the state in level order and evaluates the tiles' errors
 * (vpt_accum.h).  Tiles of one call may stand at different level counts; they are passed in groups of equal
 * (k0, n), one after the other on the default stream, so the groups share the partial buffer.
 *
 * Bitwise bar: level k of a pixel is samples [kC, kC + C) of its own erand48 streams, summed as acc = L + acc by
 * the same pool kernel a one-shot render runs; accum_kernel adds the levels as sum = c + sum, reduce_kernel's
 * order, and resolve_kernel scales by 1 / (double)(levels * C), reduce_kernel's 1 / (double)spp.  A pixel with
 * m levels is therefore the pixel of vpt_render(spp = mC, chunk_spp = C), whatever passes brought the levels.
 *
 * The grid accumulator (vpt_accum_create_grid; estimators 10 to 16, the density-grid estimators) is the same handle with
 * another way of bringing the levels and a contract of its own.  Those estimators render with the persistent-wave loop,
 * where one lane owns a pixel and sums its samples strictly in order; a pass continues that loop (wave_accum,
 * vpt_wave_accum.h; vpt_int_grid_pass) from the state, so there is no partial buffer and no fold.  For a pixel that
 * holds m levels:
 *   sum     is acc = L + acc over samples 0 .. mC - 1 of its stream, in order, starting from zero, whatever calls, tile
 *           lists and groups brought the levels; resolve_kernel scales by 1 / (double)(mC), as store_pixel does, so the
 *           pixel is the pixel of vpt_render(spp = mC), bit for bit, in FP64 and FP32.  C does not change the image;
 *   s1, s2  are as above: level k contributes y = vpt_accum_lum(c_k), c_k the sum of samples [kC, kC + C) formed as
 *           c = L + c from zero, folded as s1 = y + s1, s2 = y*y + s2 (vpt_accum_level's lines).  sum is NOT the sum of
 *           the c_k here: only the statistic sees the chunks;
 *   errors and policy (vpt_accum_err, the tile maximum in which a NaN wins, vpt_accum_active, the refine loop and its
 *           report) are vpt_accum.h's, unchanged.
 * A pass is one launch of the render kernel for all listed tiles -- each at its own level count, each with its own
 * number of levels to add -- and then grid_tail_kernel (vpt_grid_tail.hip, a unit of its own so that this one's code
 * object stays what it was), which evaluates the tiles' errors and advances their level counts (the render kernel does
 * not write them).  Every pass validates the parameters as vpt_render does: when the
 * grid was cleared, or a setting no longer suits the estimator, the pass fails with the render's status and changes no
 * state.  The scene, the grid and its settings (block, interpolation, emission, medium colour, track fraction) must stay
 * as they are while the accumulator holds samples.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "vpt_math.h"
#define VPT_ACCUM_SQRT vm_sqrt /* the device code's correctly rounded square root */
#include "vpt_accum.h"
#include "vpt_chunks.h"
#include "vpt_internal.h"

#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return vpt_fail(VPT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

namespace {

struct AccumParams {
    int w, rows, tiles_x;
    int nlev;                 /* levels of this pass (0: only re-evaluate the errors) */
    unsigned n_list;
    const unsigned* list;     /* the pass's tiles */
    const double* partials;   /* nlev planes of rows * w * 3 */
    double* sum;              /* rows * w * 3 */
    double* s12;              /* rows * w * 2 */
    int* levels;              /* per tile */
    double* err;              /* per tile */
    const unsigned* guard;    /* PoolParams::guard's flag */
    double cfloor;            /* (double)C * lum_floor */
};

/* one wave per 8x8 tile of the list, one lane per pixel */
__global__ __launch_bounds__(256) void accum_kernel(AccumParams A)
{
    const int lane = threadIdx.x & 63;
    const unsigned li = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (li >= A.n_list) return;  /* wave-uniform */
    const unsigned tile = A.list[li];
    const int ty = (int)(tile / (unsigned)A.tiles_x), tx = (int)(tile - (unsigned)ty * (unsigned)A.tiles_x);
    const int x = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
    const bool valid = x < A.w && lr < A.rows;  /* lanes in the padding of an edge tile take no part */
    const int m = A.levels[tile] + A.nlev;
    const bool poison = *(volatile const unsigned*)A.guard != 0;  /* the pool launch rendered nothing */
    double e = -(double)INFINITY;
    if (valid) {
        const size_t p = (size_t)lr * (size_t)A.w + (size_t)x;
        const size_t plane = (size_t)A.rows * (size_t)A.w * 3;
        vpt_accum_px a;
        a.sum[0] = A.sum[3 * p];
        a.sum[1] = A.sum[3 * p + 1];
        a.sum[2] = A.sum[3 * p + 2];
        a.s1 = A.s12[2 * p];
        a.s2 = A.s12[2 * p + 1];
        const double* q = A.partials + 3 * p;
        for (int k = 0; k < A.nlev; ++k) vpt_accum_level(&a, q[k * plane], q[k * plane + 1], q[k * plane + 2]);
        e = vpt_accum_err(a.s1, a.s2, m, A.cfloor);
        if (poison) {
            const double n = __builtin_nan("");
            a.sum[0] = a.sum[1] = a.sum[2] = a.s1 = a.s2 = e = n;
        }
        if (A.nlev > 0 || poison) {
            A.sum[3 * p] = a.sum[0];
            A.sum[3 * p + 1] = a.sum[1];
            A.sum[3 * p + 2] = a.sum[2];
            A.s12[2 * p] = a.s1;
            A.s12[2 * p + 1] = a.s2;
        }
    }
    /* the tile's maximum (a NaN wins); the value does not depend on the order */
    for (int d = 32; d >= 1; d >>= 1) e = vpt_accum_max(e, __shfl_xor(e, d));
    if (lane == 0) {
        A.err[tile] = e;
        A.levels[tile] = m;
    }
}

struct ResolveParams {
    int w, rows, tiles_x, C;
    const double* sum;
    const int* levels;
    void* out;
};

/* reduce_kernel's scl(tot, 1 / (double)spp) with spp = levels * C of the pixel's tile */
template <int FB>
__global__ __launch_bounds__(256) void resolve_kernel(ResolveParams R)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t npix = (size_t)R.rows * (size_t)R.w;
    if (p >= npix) return;
    const int lr = (int)(p / (size_t)R.w), x = (int)(p - (size_t)lr * (size_t)R.w);
    const int lv = R.levels[(size_t)(lr >> 3) * (size_t)R.tiles_x + (size_t)(x >> 3)];
    double r[3] = {0.0, 0.0, 0.0};
    if (lv > 0) {
        const double s = 1 / (double)((int64_t)lv * R.C);
        for (int c = 0; c < 3; ++c) r[c] = R.sum[3 * p + c] * s;
    }
    if (FB == VPT_FB_F32) {
        float* o = (float*)R.out;
        for (int c = 0; c < 3; ++c) o[3 * p + c] = (float)r[c];
    } else {
        double* o = (double*)R.out;
        for (int c = 0; c < 3; ++c) o[3 * p + c] = r[c];
    }
}

}  // namespace

struct vpt_accum {
    vpt_context* ctx;
    int device;  /* ctx's, kept so that destroying the accumulator does not need the context */
    bool grid;   /* vpt_accum_create_grid's: passes continue the persistent-wave loop (no partial buffer) */
    vpt_params p;
    int C, max_levels, rows, w, tiles_x, tiles_y, ntiles;
    double lum_floor;
    double* d_sum;
    double* d_s12;
    int* d_levels;
    double* d_err;
    unsigned* d_list;
    int* d_nadd;  /* the grid accumulator's per-entry counts of a pass */
    unsigned* d_queue;
    double* d_partials;
    size_t partials_bytes;
    std::vector<int32_t> levels;   /* host mirrors, refreshed after every pass */
    std::vector<double> err;
    std::vector<int32_t> valid_px; /* valid pixels per tile (sample counts of the report) */
};

namespace {

size_t npix_of(const vpt_accum* a) { return (size_t)a->rows * (size_t)a->w; }

int download_tiles(vpt_accum* a)
{
    HIP_OK(hipMemcpy(a->levels.data(), a->d_levels, sizeof(int32_t) * (size_t)a->ntiles, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(a->err.data(), a->d_err, sizeof(double) * (size_t)a->ntiles, hipMemcpyDeviceToHost));
    return VPT_OK;
}

int launch_accum(vpt_accum* a, const unsigned* d_list, unsigned n_list, int nlev)
{
    AccumParams A;
    A.w = a->w;
    A.rows = a->rows;
    A.tiles_x = a->tiles_x;
    A.nlev = nlev;
    A.n_list = n_list;
    A.list = d_list;
    A.partials = a->d_partials;
    A.sum = a->d_sum;
    A.s12 = a->d_s12;
    A.levels = a->d_levels;
    A.err = a->d_err;
    A.guard = vpt_int_guard_flag(a->ctx);
    A.cfloor = (double)a->C * a->lum_floor;
    accum_kernel<<<dim3((n_list + 3u) / 4u), dim3(256), 0, nullptr>>>(A);
    HIP_OK(hipGetLastError());
    return VPT_OK;
}

/* add_pass for the grid accumulator, the list sorted (ord): the list and the per-entry counts go up, ONE launch of the
 * render kernel serves every entry, the tail kernel follows.  Validated first, so a failing pass changes no state */
int grid_pass(vpt_accum* a, const std::vector<int32_t>& list, const std::vector<int32_t>& nadd, const std::vector<size_t>& ord,
              const char* who)
{
    int rc = vpt_int_check_params(a->ctx, &a->p);
    if (rc) return rc;
    const unsigned n = (unsigned)ord.size();
    std::vector<unsigned> h_list(n);
    std::vector<int32_t> h_nadd(n);
    for (size_t i = 0; i < ord.size(); ++i) {
        h_list[i] = (unsigned)list[ord[i]];
        h_nadd[i] = nadd[ord[i]];
    }
    HIP_OK(hipMemcpy(a->d_list, h_list.data(), sizeof(unsigned) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(a->d_nadd, h_nadd.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
    rc = vpt_int_grid_pass(a->ctx, &a->p, a->C, a->d_list, a->d_nadd, n, a->d_levels, a->d_sum, a->d_s12, a->d_queue);
    if (!rc) {
        rc = vpt_int_grid_tail(a->w, a->rows, a->tiles_x, a->d_list, a->d_nadd, n, a->d_s12, (double)a->C * a->lum_floor,
                               a->d_levels, a->d_err);
    }
    const hipError_t e = hipDeviceSynchronize();
    if (rc) return rc;
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return download_tiles(a);
}

/* nadd[i] more levels for tile list[i] (validated by the caller: in range, no duplicates, within the cap,
 * nadd > 0).  Groups of equal (level count, nadd), each: pool pass, then accum_kernel.  Synchronises, refreshes
 * the host mirrors and checks the pool kernel's guard. */
int add_pass(vpt_accum* a, const std::vector<int32_t>& list, const std::vector<int32_t>& nadd, const char* who)
{
    if (list.empty()) return VPT_OK;
    HIP_OK(hipSetDevice(vpt_int_device(a->ctx)));
    std::vector<size_t> ord(list.size());
    for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
    /* by (level count, levels to add), tiles ascending within a group */
    std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
        const int lx = a->levels[(size_t)list[x]], ly = a->levels[(size_t)list[y]];
        if (lx != ly) return lx < ly;
        if (nadd[x] != nadd[y]) return nadd[x] < nadd[y];
        return list[x] < list[y];
    });
    if (a->grid) return grid_pass(a, list, nadd, ord, who);
    if (a->p.medium.estimator > 1) {
        /* the pool kernel's tile-list variant exists for the estimators 0 and 1 (vpt_pool.h): the others take
         * whole-set passes only, i.e. every tile, from one level count, by one number of levels */
        const size_t lo = ord.front(), hi = ord.back();
        if (list.size() != (size_t)a->ntiles || a->levels[(size_t)list[lo]] != a->levels[(size_t)list[hi]] ||
            nadd[lo] != nadd[hi])
            return vpt_fail(VPT_E_UNSUPPORTED, "%s: estimator %d accumulates whole tile sets only (tile subsets: "
                            "estimators 0 and 1)", who, a->p.medium.estimator);
    }
    std::vector<unsigned> h_list(list.size());
    int most = 0;
    for (size_t i = 0; i < ord.size(); ++i) {
        h_list[i] = (unsigned)list[ord[i]];
        most = std::max(most, (int)nadd[ord[i]]);
    }
    const size_t need = npix_of(a) * 3 * sizeof(double) * (size_t)most;
    if (need > a->partials_bytes) {
        if (a->d_partials) HIP_OK(hipFree(a->d_partials));
        a->d_partials = nullptr;
        a->partials_bytes = 0;
        HIP_OK(hipMalloc((void**)&a->d_partials, need));
        a->partials_bytes = need;
    }
    HIP_OK(hipMemcpy(a->d_list, h_list.data(), sizeof(unsigned) * h_list.size(), hipMemcpyHostToDevice));
    int rc = VPT_OK;
    for (size_t g0 = 0; g0 < ord.size() && !rc;) {
        const int k0 = a->levels[(size_t)h_list[g0]], n = nadd[ord[g0]];
        size_t g1 = g0 + 1;
        while (g1 < ord.size() && a->levels[(size_t)h_list[g1]] == k0 && nadd[ord[g1]] == n) ++g1;
        const unsigned cnt = (unsigned)(g1 - g0);
        /* every tile in order needs no indirection: the whole-image pass of a plain progressive render */
        const bool all = cnt == (unsigned)a->ntiles;
        rc = vpt_int_pool_pass(a->ctx, &a->p, a->C, k0, k0 + n, all ? nullptr : a->d_list + g0, cnt, a->d_partials,
                               a->d_queue);
        if (!rc) rc = launch_accum(a, a->d_list + g0, cnt, n);
        g0 = g1;
    }
    const hipError_t e = hipDeviceSynchronize();
    if (rc) return rc;
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    rc = download_tiles(a);
    if (rc) return rc;
    return vpt_int_check_guard(a->ctx, who);
}

int check_refine(const vpt_refine* r, const char* who)
{
    if (!r) return vpt_fail(VPT_E_INVALID, "%s: NULL refine parameters", who);
    switch (vpt_accum_refine_bad(r->target, r->lum_floor, r->min_levels, r->levels_per_pass)) {
    case 1: return vpt_fail(VPT_E_INVALID, "%s: target and lum_floor must be finite and >= 0", who);
    case 2: return vpt_fail(VPT_E_INVALID, "%s: min_levels must be >= 2 (one level has no variance)", who);
    case 3: return vpt_fail(VPT_E_INVALID, "%s: levels_per_pass must be > 0", who);
    }
    return VPT_OK;
}

int select_active(const int32_t* levels, const double* err, int n, const vpt_refine* r, int max_levels, int32_t* active)
{
    int k = 0;
    for (int t = 0; t < n; ++t)
        if (vpt_accum_active(levels[t], err[t], r->min_levels, max_levels, r->target)) active[k++] = t;
    return k;
}

template <int FB>
int launch_resolve(vpt_accum* a, void* d_out, hipStream_t stream)
{
    ResolveParams R{a->w, a->rows, a->tiles_x, a->C, a->d_sum, a->d_levels, d_out};
    resolve_kernel<FB><<<dim3((unsigned)((npix_of(a) + 255) / 256)), dim3(256), 0, stream>>>(R);
    HIP_OK(hipGetLastError());
    return VPT_OK;
}

}  // namespace

/* both constructors: the parameters against the context as vpt_render checks them, then the estimator's kind */
static int accum_create(vpt_context* ctx, const vpt_params* p, vpt_accum** out, bool grid, const char* who)
{
    vpt_clear_error();
    if (!out) return vpt_fail(VPT_E_INVALID, "%s: out is NULL", who);
    *out = nullptr;
    int rc = vpt_int_check_params(ctx, p);
    if (rc) return rc;
    if (!grid && p->medium.estimator > 5)
        return vpt_fail(VPT_E_UNSUPPORTED, "vpt_accum_create: estimator %d has no chunks (estimators 0-5 accumulate)",
                        p->medium.estimator);
    if (grid && p->medium.estimator < VPT_HETERO_FREE)
        return vpt_fail(VPT_E_INVALID, "vpt_accum_create_grid: estimator %d is not a density-grid estimator (10-16); "
                        "estimators 0-5 accumulate with vpt_accum_create", p->medium.estimator);
    const int C = p->chunk_spp > 0 ? p->chunk_spp : (p->spp < 32 ? p->spp : 32);
    if (p->spp % C != 0)
        return vpt_fail(VPT_E_INVALID, "%s: spp %d (the cap) is not a multiple of the chunk %d", who, p->spp, C);
    const int rows = vpt_shard_rows(p);
    if (rows <= 0) return vpt_fail(VPT_E_INVALID, "%s: the shard has no rows", who);
    if (p->width > 65535 || p->height > 65535) return vpt_fail(VPT_E_INVALID, "width and height must be < 65536");
    HIP_OK(hipSetDevice(vpt_int_device(ctx)));
    vpt_accum* a = new vpt_accum();
    a->ctx = ctx;
    a->device = vpt_int_device(ctx);
    a->grid = grid;
    a->p = *p;
    a->C = C;
    a->max_levels = p->spp / C;
    a->rows = rows;
    a->w = p->width;
    a->tiles_x = (p->width + 7) / 8;
    a->tiles_y = (rows + 7) / 8;
    a->ntiles = a->tiles_x * a->tiles_y;
    a->lum_floor = 0.01;
    a->d_sum = a->d_s12 = a->d_err = a->d_partials = nullptr;
    a->d_levels = a->d_nadd = nullptr;
    a->d_list = a->d_queue = nullptr;
    a->partials_bytes = 0;
    a->levels.assign((size_t)a->ntiles, 0);
    a->err.assign((size_t)a->ntiles, (double)INFINITY);
    a->valid_px.resize((size_t)a->ntiles);
    for (int t = 0; t < a->ntiles; ++t) {
        const int tx = t % a->tiles_x, ty = t / a->tiles_x;
        a->valid_px[(size_t)t] = std::min(8, a->w - tx * 8) * std::min(8, rows - ty * 8);
    }
    const size_t npix = npix_of(a), nt = (size_t)a->ntiles;
    hipError_t e = hipMalloc((void**)&a->d_sum, npix * 3 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&a->d_s12, npix * 2 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&a->d_levels, nt * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&a->d_err, nt * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&a->d_list, nt * sizeof(unsigned));
    if (e == hipSuccess && grid) e = hipMalloc((void**)&a->d_nadd, nt * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&a->d_queue, sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(a->d_sum, 0, npix * 3 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a->d_s12, 0, npix * 2 * sizeof(double));
    if (e == hipSuccess) e = hipMemset(a->d_levels, 0, nt * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(a->d_err, a->err.data(), nt * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        vpt_accum_destroy(a);
        return vpt_fail(VPT_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    *out = a;
    return VPT_OK;
}

extern "C" {

int vpt_accum_create(vpt_context* ctx, const vpt_params* p, vpt_accum** out)
{
    return accum_create(ctx, p, out, false, "vpt_accum_create");
}

int vpt_accum_create_grid(vpt_context* ctx, const vpt_params* p, vpt_accum** out)
{
    return accum_create(ctx, p, out, true, "vpt_accum_create_grid");
}

void vpt_accum_destroy(vpt_accum* a)
{
    if (!a) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(a->device);
    (void)hipDeviceSynchronize();
    if (a->d_sum) (void)hipFree(a->d_sum);
    if (a->d_s12) (void)hipFree(a->d_s12);
    if (a->d_levels) (void)hipFree(a->d_levels);
    if (a->d_err) (void)hipFree(a->d_err);
    if (a->d_list) (void)hipFree(a->d_list);
    if (a->d_nadd) (void)hipFree(a->d_nadd);
    if (a->d_queue) (void)hipFree(a->d_queue);
    if (a->d_partials) (void)hipFree(a->d_partials);
    (void)hipSetDevice(prev);
    delete a;
}

int vpt_accum_tiles(const vpt_accum* a, int* tiles_x, int* tiles_y, int* chunk, int* max_levels)
{
    vpt_clear_error();
    if (!a) return vpt_fail(VPT_E_INVALID, "vpt_accum_tiles: NULL accumulator");
    if (tiles_x) *tiles_x = a->tiles_x;
    if (tiles_y) *tiles_y = a->tiles_y;
    if (chunk) *chunk = a->C;
    if (max_levels) *max_levels = a->max_levels;
    return VPT_OK;
}

int vpt_accum_add(vpt_accum* a, int levels, const int32_t* tiles, int n_tiles)
{
    vpt_clear_error();
    if (!a) return vpt_fail(VPT_E_INVALID, "vpt_accum_add: NULL accumulator");
    if (levels <= 0) return vpt_fail(VPT_E_INVALID, "vpt_accum_add: levels must be > 0");
    std::vector<int32_t> list;
    if (!tiles) {
        list.resize((size_t)a->ntiles);
        for (int t = 0; t < a->ntiles; ++t) list[(size_t)t] = t;
    } else {
        if (n_tiles < 0 || n_tiles > a->ntiles)
            return vpt_fail(VPT_E_INVALID, "vpt_accum_add: %d tiles listed, the accumulator has %d", n_tiles, a->ntiles);
        std::vector<char> seen((size_t)a->ntiles, 0);
        for (int i = 0; i < n_tiles; ++i) {
            const int32_t t = tiles[i];
            if (t < 0 || t >= a->ntiles) return vpt_fail(VPT_E_INVALID, "vpt_accum_add: tile %d outside [0, %d)", t, a->ntiles);
            if (seen[(size_t)t]) return vpt_fail(VPT_E_INVALID, "vpt_accum_add: tile %d is listed twice", t);
            seen[(size_t)t] = 1;
        }
        list.assign(tiles, tiles + n_tiles);
    }
    for (int32_t t : list)
        if (a->levels[(size_t)t] > a->max_levels - levels)
            return vpt_fail(VPT_E_INVALID, "vpt_accum_add: tile %d has %d levels, %d more would pass the cap of %d", t,
                            a->levels[(size_t)t], levels, a->max_levels);
    return add_pass(a, list, std::vector<int32_t>(list.size(), levels), "vpt_accum_add");
}

int vpt_accum_refine(vpt_accum* a, const vpt_refine* r, vpt_refine_report* report)
{
    vpt_clear_error();
    if (!a) return vpt_fail(VPT_E_INVALID, "vpt_accum_refine: NULL accumulator");
    int rc = check_refine(r, "vpt_accum_refine");
    if (rc) return rc;
    HIP_OK(hipSetDevice(vpt_int_device(a->ctx)));
    if (r->lum_floor != a->lum_floor) {  /* the errors held were taken against another floor: evaluate them again */
        a->lum_floor = r->lum_floor;
        std::vector<unsigned> ident((size_t)a->ntiles);
        for (int t = 0; t < a->ntiles; ++t) ident[(size_t)t] = (unsigned)t;
        HIP_OK(hipMemcpy(a->d_list, ident.data(), sizeof(unsigned) * ident.size(), hipMemcpyHostToDevice));
        rc = launch_accum(a, a->d_list, (unsigned)a->ntiles, 0);
        if (rc) return rc;
        HIP_OK(hipDeviceSynchronize());
        rc = download_tiles(a);
        if (rc) return rc;
    }
    int passes = 0;
    uint64_t samples = 0;
    std::vector<int32_t> active((size_t)a->ntiles), nadd;
    while (true) {
        const int n = select_active(a->levels.data(), a->err.data(), a->ntiles, r, a->max_levels, active.data());
        if (n == 0) break;
        std::vector<int32_t> list(active.begin(), active.begin() + n);
        nadd.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            nadd[(size_t)i] = std::min(r->levels_per_pass, a->max_levels - a->levels[(size_t)list[(size_t)i]]);
            samples += (uint64_t)a->valid_px[(size_t)list[(size_t)i]] * (uint64_t)nadd[(size_t)i] * (uint64_t)a->C;
        }
        rc = add_pass(a, list, nadd, "vpt_accum_refine");
        if (rc) return rc;
        ++passes;
    }
    if (report) {
        report->passes = passes;
        report->tiles_converged = report->tiles_capped = 0;
        report->samples = samples;
        double me = -(double)INFINITY;
        for (int t = 0; t < a->ntiles; ++t) {
            if (a->err[(size_t)t] > r->target) report->tiles_capped++;
            else report->tiles_converged++;
            me = vpt_accum_max(me, a->err[(size_t)t]);
        }
        report->max_err = me;
    }
    return VPT_OK;
}

int vpt_accum_resolve_device(vpt_accum* a, int fb_format, void* d_out, void* stream)
{
    vpt_clear_error();
    if (!a || !d_out) return vpt_fail(VPT_E_INVALID, "vpt_accum_resolve_device: NULL argument");
    if (fb_format != VPT_FB_F32 && fb_format != VPT_FB_F64) return vpt_fail(VPT_E_INVALID, "bad fb_format");
    HIP_OK(hipSetDevice(vpt_int_device(a->ctx)));
    if (fb_format == VPT_FB_F32) return launch_resolve<VPT_FB_F32>(a, d_out, (hipStream_t)stream);
    return launch_resolve<VPT_FB_F64>(a, d_out, (hipStream_t)stream);
}

int vpt_accum_resolve(vpt_accum* a, int fb_format, void* h_out)
{
    vpt_clear_error();
    if (!a || !h_out) return vpt_fail(VPT_E_INVALID, "vpt_accum_resolve: NULL argument");
    if (fb_format != VPT_FB_F32 && fb_format != VPT_FB_F64) return vpt_fail(VPT_E_INVALID, "bad fb_format");
    HIP_OK(hipSetDevice(vpt_int_device(a->ctx)));
    const size_t bytes = npix_of(a) * 3 * (fb_format == VPT_FB_F32 ? sizeof(float) : sizeof(double));
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, bytes));
    int rc = vpt_accum_resolve_device(a, fb_format, d, nullptr);
    const hipError_t e = rc ? hipSuccess : hipMemcpy(h_out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return vpt_fail(VPT_E_HIP, "vpt_accum_resolve: %s", hipGetErrorString(e));
    return VPT_OK;
}

int vpt_accum_read(vpt_accum* a, double* sum, double* s12, int32_t* tile_levels, double* tile_err)
{
    vpt_clear_error();
    if (!a) return vpt_fail(VPT_E_INVALID, "vpt_accum_read: NULL accumulator");
    HIP_OK(hipSetDevice(vpt_int_device(a->ctx)));
    const size_t npix = npix_of(a), nt = (size_t)a->ntiles;
    if (sum) HIP_OK(hipMemcpy(sum, a->d_sum, npix * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (s12) HIP_OK(hipMemcpy(s12, a->d_s12, npix * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (tile_levels) HIP_OK(hipMemcpy(tile_levels, a->d_levels, nt * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tile_err) HIP_OK(hipMemcpy(tile_err, a->d_err, nt * sizeof(double), hipMemcpyDeviceToHost));
    return VPT_OK;
}

}  // extern "C"
