/*
 * vpt_grid_build.hip -- grids from device memory (vpt_set_density_grid_device, vpt_set_emission_grid_device): what the host
 * entry points do in host loops, as kernels over the context's own copy of the voxels.
 *
 * grid_scan_kernel: vpt_grid_bad's voxel predicate and vpt_grid_view_init's maximum in one streaming pass.  A lane reads
 * 16 bytes at a time from the first 16-byte boundary on (the up to three voxels in front of it and behind the last full
 * quad are read one by one), keeps a running maximum (from +0.0f under strict >) and the lowest index of a bad voxel; the
 * wave reduces by shuffles, the workgroup through LDS, and every workgroup stores its pair into its own entry of a slab,
 * which the host finishes.  No atomics and no hand-off between workgroups: the result does not depend on arrival order.  The
 * maximum of valid voxels is +0.0 or positive, so its bits do not depend on the order of the compares either.
 *
 * grid_build_kernel<false>, grid_build_kernel<true>: the passes X and YZ of vpt_grid_build.h.  An output is reduced by a group of W
 * adjacent lanes, W a power of two <= 64 chosen per launch: in pass X the smallest that covers a block's range (so a wave
 * reads one contiguous stretch of a row), in pass YZ 1 where a row of outputs fills a wave (the lanes run along bx and
 * every load is contiguous) and more where it does not (few, large blocks).  Lane l of a group scans elements l, l + W, ...
 * in ascending order and the group joins by vpt_gb_acc_join, lowest position first among equals: the serial scan's bits.
 * Scratch: pass X's 2 nz ny nbx floats.  Linear indices are 64-bit.
 *
 * A unit of its own, and no other unit includes vpt_grid_build.h: the other code objects stay what they are.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <vector>

#include "vpt_grid_build.h"
#include "vpt_internal.h"

namespace {

struct ScanEntry {  /* one workgroup's result */
    float mx;
    int32_t pad_;
    long long bad;  /* LLONG_MAX: none */
};
constexpr long long NO_BAD = 0x7FFFFFFFFFFFFFFFll;

struct ScanAcc {
    float mx;
    long long bad;
    __device__ void take(float v, long long i)
    {
        if (!(v >= 0.0f && v - v == 0.0f) && i < bad) bad = i;  /* vpt_grid_bad's predicate */
        if (v > mx) mx = v;
    }
    __device__ void join(float omx, long long obad)
    {
        if (omx > mx) mx = omx;
        if (obad < bad) bad = obad;
    }
};

/* v[0 .. head) one by one, then nquad float4 from v + head (16-byte aligned), then the voxels behind them */
__global__ __launch_bounds__(256) void grid_scan_kernel(const float* __restrict__ v, long long nv, int head, long long nquad,
                                                        ScanEntry* __restrict__ slab)
{
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, nthreads = (long long)gridDim.x * 256;
    ScanAcc A{0.0f, NO_BAD};
    if (gid < head) A.take(v[gid], gid);
    const float4* q = (const float4*)(v + head);
    for (long long i = gid; i < nquad; i += nthreads) {
        const float4 w = q[i];
        const long long at = head + 4 * i;
        A.take(w.x, at);
        A.take(w.y, at + 1);
        A.take(w.z, at + 2);
        A.take(w.w, at + 3);
    }
    const long long tail = head + 4 * nquad + gid;
    if (gid < 4 && tail < nv) A.take(v[tail], tail);
    for (int d = 32; d >= 1; d >>= 1) A.join(__shfl_xor(A.mx, d), __shfl_xor(A.bad, d));
    __shared__ float s_mx[4];
    __shared__ long long s_bad[4];
    if ((threadIdx.x & 63) == 0) {
        s_mx[threadIdx.x >> 6] = A.mx;
        s_bad[threadIdx.x >> 6] = A.bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) A.join(s_mx[w], s_bad[w]);
        slab[blockIdx.x] = ScanEntry{A.mx, 0, A.bad};
    }
}

struct BuildParams {
    int32_t n[3], nb[3];
    int32_t B, tl;
    int32_t w;              /* lanes per output: a power of two <= 64 */
    long long total;        /* outputs of the pass */
    const float* rho;       /* pass X reads it */
    float *sxmax, *sxmin;   /* pass X writes, pass YZ reads: n[2] x n[1] x nb[0] each */
    float *omax, *omin;     /* pass YZ writes: the nbv maxima and the nbv minima behind them */
};

/* a group's lanes joined: afterwards every lane of the group holds the serial scan's result */
__device__ void group_join(vpt_gb_acc* A, int w)
{
    for (int d = w >> 1; d >= 1; d >>= 1) {
        const float mx = __shfl_xor(A->mx, d), mn = __shfl_xor(A->mn, d);
        const long long at = __shfl_xor((long long)A->at, d);
        vpt_gb_acc_join(A, mx, mn, (int64_t)at);
    }
}

/* the passes' common loop: output o for the group of P.w lanes that `lane` is in, wave-uniform trip counts (every lane
 * of a wave takes part in every shuffle; a group without an output scans nothing) */
template <bool YZ>
__global__ __launch_bounds__(256) void grid_build_kernel(BuildParams P)
{
    const int w = P.w, sub = (int)(threadIdx.x & (unsigned)(w - 1));
    const long long per_wave = 64 / w, per_grid = (long long)gridDim.x * 4 * per_wave;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long in_wave = (threadIdx.x & 63) / w;
    for (long long base = wave * per_wave; base < P.total; base += per_grid) {
        const long long o = base + in_wave;
        const bool on = o < P.total;
        vpt_gb_acc A;
        vpt_gb_acc_init(&A);
        if (on) {
            if (YZ) {
                const long long plane = (long long)P.nb[0] * P.nb[1];
                const int32_t bz = (int32_t)(o / plane), by = (int32_t)((o - bz * plane) / P.nb[0]);
                const int32_t bx = (int32_t)(o - bz * plane - (long long)by * P.nb[0]);
                int32_t z0, z1, y0, y1;
                vpt_gb_range(P.n[2], P.B, P.tl, bz, &z0, &z1);
                vpt_gb_range(P.n[1], P.B, P.tl, by, &y0, &y1);
                vpt_gb_scan_yz(P.sxmax, P.sxmin, P.n[1], P.nb[0], bx, z0, z1, y0, y1, sub, w, &A);
            } else {
                const long long r = o / P.nb[0];
                const int32_t bx = (int32_t)(o - r * P.nb[0]);
                int32_t x0, x1;
                vpt_gb_range(P.n[0], P.B, P.tl, bx, &x0, &x1);
                vpt_gb_scan_x(P.rho + r * P.n[0], x0, x1, sub, w, &A);
            }
        }
        group_join(&A, w);
        if (on && sub == 0) {
            (YZ ? P.omax : P.sxmax)[o] = A.mx;
            (YZ ? P.omin : P.sxmin)[o] = A.mn;
        }
    }
}

int pow2_ceil(long long v, int cap)
{
    int w = 1;
    while (w < cap && w < v) w <<= 1;
    return w;
}

/* the workgroups of a streaming launch over `waves` waves of work: eight per CU at most (the rest by grid stride) */
hipError_t launch_blocks(long long waves, unsigned* blocks)
{
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const long long cap = (long long)(cus > 0 ? cus : 1) * 8, want = (waves + 3) / 4;
    *blocks = (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
    return hipSuccess;
}

}  // namespace

int vpt_int_grid_scan(const float* d_v, long long nv, float* vmax, long long* bad)
{
    const int mis = (int)(((uintptr_t)d_v & 15u) / 4u);  /* d_v is a float's address */
    const int head = (int)((4 - mis) % 4 < nv ? (4 - mis) % 4 : nv);
    const long long nquad = (nv - head) / 4;
    unsigned blocks = 1;
    hipError_t e = launch_blocks((nquad + 63) / 64, &blocks);
    if (e != hipSuccess) return (int)e;
    ScanEntry* d_slab = nullptr;
    e = hipMalloc((void**)&d_slab, sizeof(ScanEntry) * blocks);
    if (e != hipSuccess) return (int)e;
    std::vector<ScanEntry> slab(blocks);
    grid_scan_kernel<<<dim3(blocks), dim3(256), 0, nullptr>>>(d_v, nv, head, nquad, d_slab);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(slab.data(), d_slab, sizeof(ScanEntry) * blocks, hipMemcpyDeviceToHost);
    (void)hipFree(d_slab);
    if (e != hipSuccess) return (int)e;
    float mx = 0.0f;
    long long b = NO_BAD;
    for (const ScanEntry& s : slab) {
        if (s.mx > mx) mx = s.mx;
        if (s.bad < b) b = s.bad;
    }
    *vmax = mx;
    *bad = b == NO_BAD ? -1 : b;
    return (int)hipSuccess;
}

int vpt_int_grid_build(const int* n, int B, int tl, const float* d_rho, float* d_out)
{
    BuildParams P = {};
    for (int a = 0; a < 3; ++a) P.n[a] = n[a];
    vpt_grid_majorant_counts(P.n, B, P.nb);
    P.B = B;
    P.tl = tl ? 1 : 0;
    const long long nbv = (long long)P.nb[0] * P.nb[1] * P.nb[2], nsx = (long long)P.n[2] * P.n[1] * P.nb[0];
    float* d_sx = nullptr;
    hipError_t e = hipMalloc((void**)&d_sx, sizeof(float) * 2 * (size_t)nsx);
    if (e != hipSuccess) return (int)e;
    P.rho = d_rho;
    P.sxmax = d_sx;
    P.sxmin = d_sx + nsx;
    P.omax = d_out;
    P.omin = d_out + nbv;
    unsigned blocks = 1;
    /* pass X: a group covers a block's range, B voxels and the dilation's two */
    long long len[3];  /* the longest range of an axis */
    for (int a = 0; a < 3; ++a) len[a] = (long long)B + 2 * P.tl < P.n[a] ? (long long)B + 2 * P.tl : P.n[a];
    P.w = pow2_ceil(len[0], 64);
    P.total = nsx;
    e = launch_blocks((nsx + 64 / P.w - 1) / (64 / P.w), &blocks);
    if (e == hipSuccess) {
        grid_build_kernel<false><<<dim3(blocks), dim3(256), 0, nullptr>>>(P);
        e = hipGetLastError();
    }
    /* pass YZ: one lane per output where a row of outputs fills a wave, else what is left of the wave per output, up to
     * the rows a block gathers */
    P.w = pow2_ceil(len[1] * len[2], 64 / pow2_ceil(P.nb[0], 64));
    P.total = nbv;
    if (e == hipSuccess) e = launch_blocks((nbv + 64 / P.w - 1) / (64 / P.w), &blocks);
    if (e == hipSuccess) {
        grid_build_kernel<true><<<dim3(blocks), dim3(256), 0, nullptr>>>(P);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    (void)hipFree(d_sx);
    return (int)e;
}
