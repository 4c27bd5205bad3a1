/*
 * vpt.h -- C ABI of the MI355X volumetric path tracer (libvpt.so).
 *
 * Drop-in boundary for the hot path of gabo99cas/minimal_volumetric_path_tracer.  The reference
 * has no FFI; its hot path is one C++ call per camera sample,
 *     Color iterativeVPTracerFree(const Ray&, double sigma_a, double sigma_s)   vptShadeMethods.h:1263
 *     Color MISVPTTracerRecursive(const Ray&, double, double, int depth)        vptShadeMethods.h:1345
 * made from main()'s OpenMP pixel loop (src/rt.cpp:767-805) with the scene in a global
 * std::vector<Sphere> (include/Sphere.h:49) and the RNG in a global erand48 state
 * (include/Vector.h:38).  A GPU cannot be fed one sample per call, so the boundary is lifted to
 * the pixel loop (vpt_render*), with the per-sample call kept as a batch entry
 * (vpt_trace_batch).  Implicit globals become explicit arguments; no global state remains.
 *
 * Plain C: fixed-width scalars and pointers only.  All functions return VPT_OK (0) or a
 * negative vpt_status; vpt_last_error() gives a thread-local message for the last failure.
 */
#ifndef VPT_H
#define VPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPT_ABI_VERSION 3

typedef enum {
    VPT_OK = 0,
    VPT_E_INVALID = -1,        /* bad argument (null pointer, size, NaN parameter ...) */
    VPT_E_TOO_MANY = -2,       /* more spheres than VPT_MAX_SPHERES */
    VPT_E_NO_EMITTER = -3,     /* reserved */
    VPT_E_UNSUPPORTED = -4,    /* material id outside {0,1,2,3}; an estimator the accumulator cannot serve */
    VPT_E_HIP = -5,            /* HIP runtime error (message in vpt_last_error) */
    VPT_E_IO = -6,             /* file could not be written */
    VPT_E_INTERNAL = -7        /* an internal invariant failed (message in vpt_last_error) */
} vpt_status;

#define VPT_MAX_SPHERES 64

/* Byte-identical to the reference's Sphere (include/Sphere.h:12-21; 144 B, offsets r 0, p 8,
 * c 32, radiance 56, material 80, eta 88, kappa 112, alpha 136), so spheres.data() of a
 * reference build can be passed as is.  material: 0 Lambert, 1 microfacet conductor, 2 smooth
 * dielectric (eta 1.5), 3 "volumetric" (only seen by the shadow-ray transmittance).  A sphere
 * is an emitter when any radiance channel is > 0; r == 0 makes it a point light. */
typedef struct vpt_sphere {
    double r;
    double p[3];
    double c[3];
    double radiance[3];
    int32_t material;
    int32_t reserved_;
    double eta[3];
    double kappa[3];
    double alpha;
} vpt_sphere;

/* Reference Ray (include/Ray.h:10-15): origin and direction (callers normalise). */
typedef struct vpt_ray {
    double o[3];
    double d[3];
} vpt_ray;

typedef enum {
    VPT_FREE_FLIGHT = 0,           /* iterativeVPTracerFree, vptShadeMethods.h:1263 (main's estimator) */
    VPT_MIS_EQUIANGULAR = 1,       /* MISVPTTracerRecursive, vptShadeMethods.h:1345 */
    VPT_EXPLICIT_FREE = 2,         /* explicitVPTracerRecursiveFree, vptShadeMethods.h:1153 */
    VPT_IMPLICIT_FREE = 3,         /* implicitVPTracerRecursiveFree, vptShadeMethods.h:940 */
    VPT_EXPLICIT_EQUIANGULAR = 4,  /* explicitVPTracerRecursive, vptShadeMethods.h:1014 */
    VPT_SURFACE_PT = 5,            /* iterativePathTracer, shadeMethods.h:104: surface-only path tracing (the
                                    * commented alternative at src/rt.cpp:793); sigma_a, sigma_s, hg_g and
                                    * max_depth are ignored; rendered by the task-pool kernel like 0-4
                                    * (chunk_spp applies) */
    VPT_RAY_MARCHING = 6,          /* rayMarching3, rayMarchingMethods.h:330: constant-step marching toward the
                                    * light march_light (the commented alternative at src/rt.cpp:791, which
                                    * passes sigma_a 0.001, sigma_s 0.0125, step 0.1, light 7); draws nothing
                                    * beyond the camera jitter; samples summed in the reference's order */
    VPT_RAY_MARCHING_SA = 7,       /* rayMarching2, rayMarchingMethods.h:262: steps of march_step toward sphere
                                    * march_light by solid-angle sampling, plus a hit light's radiance */
    VPT_RAY_MARCHING_GLOBAL = 8,   /* rayMarchingGlobal, rayMarchingMethods.h:106: 10 diffuse bounces, each
                                    * marched by rayMarching in march_step segments (a count), toward the
                                    * hard-coded sphere 5 (scenes need >= 6 spheres) */
    VPT_RAY_MARCHING_EXPLICIT = 9, /* rayMarching, rayMarchingMethods.h:34: the Color it returns for the camera
                                    * ray with sigma_t = sigma_a + sigma_s, steps = march_step (a count),
                                    * light = sphere 5; its out-parameters: vpt_ray_marching_batch */
    VPT_HETERO_FREE = 10,          /* extension: iterativeVPTracerFree's control flow in a heterogeneous medium, the
                                    * density grid of vpt_set_density_grid (VPT_E_INVALID without one): delta
                                    * tracking for freeFlightSample, the grid's transmittance for every
                                    * transmittance factor; sigma_a, sigma_s are per unit density; a ray that
                                    * leaves the grid without a hit ends its path; rendered by a kernel of its own
                                    * (chunk_spp is ignored, as for 6-9); csrc/vpt_grid.h, csrc/vpt_hetero.h */
    VPT_HETERO_RATIO = 11,         /* extension: VPT_HETERO_FREE statement for statement, with every transmittance
                                    * factor a ratio-tracking estimate over the same segment, drawn from the
                                    * sample's own stream where estimator 10 evaluates the factor (a factor it skips
                                    * as an exact zero and a zero-length segment draw nothing): the same
                                    * expectation, other draws, a cost that follows the majorant optical depth and
                                    * not the grid's resolution; honours vpt_set_grid_majorant_block; not in the
                                    * accumulator (VPT_E_UNSUPPORTED) */
    VPT_HETERO_EQUIANGULAR = 12,   /* extension: MISVPTTracerRecursive's control flow in the density grid
                                    * (VPT_E_INVALID without one): the scattering distance is sampled equi-angularly
                                    * toward the picked light inside the part of [0, t] the box holds, the surface
                                    * probability and every transmittance factor are the grid's exact ones, and the
                                    * local sigma_s rho scales the scattering vertex -- no tracking, no majorant (the
                                    * majorant block is accepted and ignored), no null collisions; the same
                                    * expectation as estimator 10 without the 1 / d^2 noise of a vertex near a point
                                    * light; nearest and trilinear fields; with an emission grid and in the
                                    * accumulator VPT_E_UNSUPPORTED; csrc/vpt_grid_eqa.h, csrc/vpt_hetero_eqa.h */
    VPT_HETERO_MIS = 13,           /* extension: VPT_HETERO_EQUIANGULAR with its distance decision replaced by the
                                    * one-sample combination of two strategies under the balance heuristic: with
                                    * probability q (vpt_set_hetero_mis_fraction, default 0.5) the scattering distance
                                    * is a delta track's, as in estimator 10 (the majorant block is honoured), else the
                                    * equi-angular one, and the vertex is weighted by the combined pdf
                                    * q sigma_t rho T + (1 - q) (1 - psurf) p_eq -- a weight bounded by
                                    * (sigma_s / sigma_t) / q and by estimator 12's / (1 - q) at once; the same
                                    * expectation as estimators 10 and 12; q = 0 is estimator 12 bit for bit, q = 1
                                    * samples every distance by tracking; with an emission grid and in the accumulator
                                    * VPT_E_UNSUPPORTED; csrc/vpt_grid_mis.h, csrc/vpt_hetero_mis.h */
    VPT_HETERO_CHROMATIC = 14,     /* extension: VPT_HETERO_FREE in a chromatic medium -- the context's medium colour
                                    * (vpt_set_medium_colour) multiplies sigma_a and sigma_s per colour channel.  One
                                    * draw per decision picks a hero channel whose extinction drives the delta track
                                    * (the majorant block is honoured), and collisions, surfaces and every
                                    * transmittance factor are weighted per channel by the balance heuristic over the
                                    * three hero choices, evaluated exactly from the grid's optical depth: weights
                                    * bounded by 3 ss_c / st_c and by 3.  With equal extinctions in the three channels
                                    * (the default colour among them) no hero draw is taken and the paths are
                                    * estimator 10's draw for draw; with the default colour the image is estimator
                                    * 10's bit for bit.  A channel without extinction is VPT_E_INVALID; with an
                                    * emission grid and in the accumulator VPT_E_UNSUPPORTED; csrc/vpt_grid_chroma.h,
                                    * csrc/vpt_hetero_chroma.h */
    VPT_HETERO_RESIDUAL = 15,      /* extension: VPT_HETERO_RATIO statement for statement, with every transmittance
                                    * factor a residual ratio-tracking estimate: per super-voxel of the majorant block
                                    * the minimum density is a control under the field, its part exp(-sigma_t mn len) of
                                    * the transmittance is taken analytically, and only rho - mn is tracked against the
                                    * residual majorant mu - mn -- fewer draws, weights nearer 1, zero variance where a
                                    * block is uniform; the same expectation as estimators 10 and 11.  With an all-zero
                                    * control grid it is estimator 11 bit for bit.  Needs a majorant block
                                    * (vpt_set_grid_majorant_block; block 0 -> VPT_E_INVALID; a block >= the largest
                                    * dimension is the global control); nearest and trilinear fields; with an emission
                                    * grid and in the accumulator VPT_E_UNSUPPORTED; csrc/vpt_grid.h,
                                    * csrc/vpt_hetero_residual.h */
    VPT_HETERO_SPECTRAL = 16       /* extension: VPT_HETERO_RATIO in the chromatic medium of VPT_HETERO_CHROMATIC (the
                                    * context's medium colour, vpt_set_medium_colour) by spectral tracking: every
                                    * decision tracks once under the largest channel's extinction and carries a weight
                                    * per channel (the history-aware average variant: the weights of a path that
                                    * carries (1, 1, 1) sum to 3 and none exceeds 3), and every transmittance factor is
                                    * a chromatic ratio-tracking estimate, three products from one walk.  No walk of the
                                    * grid's optical depth is left, so the cost follows the majorant optical depth and
                                    * not the resolution.  The same expectation per channel as estimator 14.  With
                                    * equal extinctions in the three channels (the default colour among them) it is
                                    * estimator 11 bit for bit.  The majorant block is honoured; nearest and trilinear
                                    * fields.  A channel without extinction is VPT_E_INVALID; with an emission grid and
                                    * in the accumulator VPT_E_UNSUPPORTED; csrc/vpt_grid_spectral.h,
                                    * csrc/vpt_hetero_spectral.h */
} vpt_estimator;
#define VPT_NUM_ESTIMATORS 17

typedef enum {
    VPT_FB_F32 = 0,            /* framebuffer: 3 x float per pixel */
    VPT_FB_F64 = 1             /* framebuffer: 3 x double per pixel */
} vpt_fb_format;

/* Homogeneous medium + estimator (src/rt.cpp:794 passes sigma_a = 0.001, sigma_s = 0.009). */
typedef struct vpt_medium {
    double sigma_a;
    double sigma_s;
    double hg_g;               /* extension: Henyey-Greenstein g; 0 = the reference's isotropic phase */
    int32_t max_depth;         /* extension: max path vertices; 0 = unbounded (Russian roulette only) */
    int32_t estimator;         /* vpt_estimator */
    double march_step;         /* ray marching (6-9): step length (6, 7) or number of segments (8, 9); > 0,
                                * default 0.1 */
    int32_t march_light;       /* VPT_RAY_MARCHING, VPT_RAY_MARCHING_SA: index of the light sphere (default 7) */
    int32_t reserved_;
} vpt_medium;

/* One image (or one shard of an image): main() of src/rt.cpp:744-830 made explicit. */
typedef struct vpt_params {
    int32_t width, height;     /* src/rt.cpp:752 (1024 x 768) */
    int32_t spp;               /* src/rt.cpp:784 (argv[1]) */
    int32_t fb_format;         /* vpt_fb_format */
    vpt_medium medium;
    uint64_t seed;             /* image seed; every (pixel, sample) owns an erand48 stream */
    vpt_ray camera;            /* src/rt.cpp:755: o = (0, 11.2, 214), d = norm(0, -0.042612, -1) */
    double fov_scale;          /* src/rt.cpp:758-759: 0.5095 */
    /* Row sharding in FILE order (file row = h-1-y, src/rt.cpp:773).  File rows are cut into
     * bands of band_rows; this call renders bands band_offset, band_offset + band_stride, ...
     * and writes them compactly, in increasing file-row order.  Whole image: band_rows = height,
     * band_stride = 1, band_offset = 0 (vpt_default_params). */
    int32_t band_rows, band_stride, band_offset;
    /* Samples per partial sum (build extension).  A pixel's samples are summed sequentially inside
     * a chunk exactly as the reference sums a pixel (src/rt.cpp:794), and the chunk sums are then
     * added in chunk order; chunk_spp == 1 or >= spp is the reference's own sequential order.
     * Chunks are the GPU's unit of work.  chunk_spp > 0: uniform chunks of chunk_spp samples;
     * 0 = auto: chunks of min(spp, 32), the last 64 samples in shrinking chunks (22, 14, 10, ...,
     * 1; layout in csrc/vpt_chunks.h) so that a launch ends on short units.  spp <= 32 is one
     * chunk either way. */
    int32_t chunk_spp;
} vpt_params;

/* Fills the reference defaults: 1024x768, spp 16, free-flight, sigma 0.001/0.009, camera and
 * fov of src/rt.cpp:752-759, seed 0x5EED0001, float32 framebuffer, whole image. */
void vpt_default_params(vpt_params* p);

/* The reference scene (include/Sphere.cpp:11-22): writes min(cap, 10) spheres, returns 10. */
int vpt_default_scene(vpt_sphere* out, int cap);

/* Number of file rows a params' shard covers (output holds rows * width pixels). */
int vpt_shard_rows(const vpt_params* p);

/* ---- context: one device, one scene ---- */
typedef struct vpt_context vpt_context;

int vpt_context_create(int device, vpt_context** out);
void vpt_context_destroy(vpt_context* ctx);
/* Copies the scene to the device (replaces the reference's global `spheres`). */
int vpt_set_scene(vpt_context* ctx, const vpt_sphere* spheres, int n);

/* ---- heterogeneous medium (estimators VPT_HETERO_FREE, VPT_HETERO_RATIO) ----
 * nx x ny x nz float32 voxels of density rho >= 0 (finite), x fastest, piecewise constant inside the world box
 * [lo, hi]; rho = 0 outside.  The medium's coefficients are rho(x) sigma_a and rho(x) sigma_s. */
typedef struct vpt_grid_desc {
    int32_t nx, ny, nz, reserved_;
    double lo[3], hi[3];
} vpt_grid_desc;
/* Copies the grid to the device (synchronous); desc NULL clears it.  The grid persists across vpt_set_scene and
 * must not change while a render is in flight.  A dimension < 1, hi <= lo, a NaN, negative or infinite density
 * or more than 2^27 voxels -> VPT_E_INVALID (the previous grid stays). */
int vpt_set_density_grid(vpt_context* ctx, const vpt_grid_desc* desc, const float* density);
/* Local majorants for the delta tracking of estimators VPT_HETERO_FREE and VPT_HETERO_RATIO (and the ratio tracking
 * of the latter; csrc/vpt_grid.h; VPT_HETERO_RESIDUAL needs them, and reads the block minima built beside them): the voxels are grouped
 * into cubic super-voxels of `block` voxels per axis, each with the maximum density of its voxels, and a track
 * steps with the majorant of the super-voxel it is in (empty ones are skipped).  Fewer null collisions on sparse
 * fields; the same estimator in distribution, other draws.  block 0 (the default) turns it off: the single
 * global majorant, every value as before.  block >= max(nx, ny, nz) is one super-voxel and reproduces block 0
 * bit for bit; block < 0 -> VPT_E_INVALID.  The setting belongs to the context: it is applied to the current
 * grid at once (synchronous), to every later vpt_set_density_grid, and survives a clear. */
int vpt_set_grid_majorant_block(vpt_context* ctx, int block);
/* How estimators VPT_HETERO_FREE and VPT_HETERO_RATIO read the density between the voxel centres (csrc/vpt_grid.h).
 * VPT_GRID_NEAREST (the default): piecewise constant per voxel, every value as before.  VPT_GRID_TRILINEAR: the
 * values sit at the voxel centres and are interpolated trilinearly in FP64, clamped (not faded) at the border of the
 * box and zero outside it; the optical depth stays deterministic and exact (Simpson's rule on the interpolation
 * cells), the tracks take the same draws in the same places, and local majorants are taken over each super-voxel
 * dilated by one voxel, so block 1 is no longer free of null collisions.  A uniform grid renders as with
 * VPT_GRID_NEAREST.  The setting belongs to the context: it is applied to the current grid at once (synchronous), to
 * every later vpt_set_density_grid, and survives a clear.  Any other mode -> VPT_E_INVALID, nothing changes. */
typedef enum { VPT_GRID_NEAREST = 0, VPT_GRID_TRILINEAR = 1 } vpt_grid_interp;
int vpt_set_grid_interpolation(vpt_context* ctx, int mode);
/* Volumetric emission for estimators VPT_HETERO_FREE and VPT_HETERO_RATIO (csrc/vpt_grid.h, csrc/vpt_hetero.h): an
 * emission grid eps of the density grid's nx x ny x nz float32 values (finite, >= 0; the same box, layout and lookup --
 * nearest or trilinear -- as the density) and a colour rgb (finite, >= 0).  The medium's source term is
 * sigma_a rho(x) eps(x) rgb, radiance per unit length: Kirchhoff's form, so where the medium does not absorb (sigma_a = 0
 * or rho = 0) it does not glow.  Scored by the collision estimator on every tentative collision of the delta track, at
 * every depth, without a random draw: paths, draw counts and end states are those of the same render without emission.
 * Copied to the device (synchronous); eps NULL clears it (rgb is ignored).  Without a density grid, or with a NaN,
 * negative or infinite eps or rgb value -> VPT_E_INVALID, nothing changes.  The emission grid belongs to the density
 * grid: setting or clearing that one clears it; vpt_set_grid_majorant_block and vpt_set_grid_interpolation leave it in
 * place.  vpt_trace_batch, vpt_render*, vpt_count_work honour it; the progressive accumulator supports neither estimator. */
int vpt_set_emission_grid(vpt_context* ctx, const float* eps, const double rgb[3]);
/* Grids from device memory: vpt_set_density_grid and vpt_set_emission_grid for voxels that already lie on the context's
 * device (a simulation step, a learned field, a frame of an animated cloud), without a host round trip.  d_density / d_eps:
 * nx x ny x nz float32 in device memory of the context's device, x fastest; `stream` (a hipStream_t, NULL = the default
 * stream) is the stream on which their producer wrote them: the call waits for it and is then synchronous, as the host
 * calls are.  The voxels are COPIED, device to device, into the context's own allocation, so the caller's buffer may be
 * freed or overwritten once the call has returned; lifetimes, ownership and "must not change while a render is in flight"
 * are those of the host calls.  The check of the voxels, the maximum and the block maxima and minima are kernels
 * (csrc/vpt_grid_build.hip) with the host's rules -- among voxels that compare equal (+0.0 and -0.0) the one first in z, y,
 * x order stays -- so a grid set either way is the same afterwards, bit for bit: every estimator, probe, vpt_count_work
 * and both accumulators work without knowing.  The context remembers where the grid came from: for a grid set from
 * device memory vpt_set_grid_majorant_block and vpt_set_grid_interpolation rebuild on the device too, and no voxel
 * crosses to the host.
 * Before anything reads the pointer it is checked (hipPointerGetAttributes, hipMemGetAddressRange): not device memory of
 * the context's device, or not that many bytes of one allocation -> VPT_E_INVALID.  A NULL context, descriptor or pointer
 * -> VPT_E_INVALID before any GPU call ("... NULL context", "... NULL grid"): clearing stays with
 * vpt_set_density_grid(ctx, NULL, NULL) and vpt_set_emission_grid(ctx, NULL, NULL).  Bad dimensions, a bad box or a bad
 * voxel -> VPT_E_INVALID with the host call's message under this function's name (for emission: the lowest bad voxel and
 * its value); the previous grid, its emission and all settings stay. */
int vpt_set_density_grid_device(vpt_context* ctx, const vpt_grid_desc* desc, const float* d_density, void* stream);
int vpt_set_emission_grid_device(vpt_context* ctx, const float* d_eps, const double rgb[3], void* stream);
/* The majorant grid as the kernels read it, for a grid set either way: the nb[0] x nb[1] x nb[2] block maxima (x fastest)
 * into maxima and the block minima into minima (either may be NULL), each with room for nbv floats.  Always fills nb and
 * rho_max.  With block 0 there is no majorant grid: VPT_OK, nb = {0, 0, 0}, nothing copied.  nbv smaller than the grid's
 * block count, or no density grid -> VPT_E_INVALID. */
int vpt_get_grid_majorants(vpt_context* ctx, float* maxima, float* minima, size_t nbv, int32_t nb[3], double* rho_max);

/* Renders into a DEVICE buffer on `stream` (a hipStream_t, NULL = default stream); returns
 * after enqueueing.  d_out: vpt_shard_rows(p) * width * 3 elements of fb_format, the
 * per-pixel average BEFORE the clamp of src/rt.cpp:803.  Renders on different streams of one
 * context may be in flight together: each stream gets its own work queue and partial-sum
 * buffer (stream-ordered, grown on demand); calls on one stream run in order.  The scene must
 * not change (vpt_set_scene) while a render that uses it is in flight. */
int vpt_render_device(vpt_context* ctx, const vpt_params* p, void* d_out, void* stream);

/* Same, synchronous, host output buffer. */
int vpt_render(vpt_context* ctx, const vpt_params* p, void* h_out);

/* ---- several GPUs of one process ----
 * One image rendered by devices 0 .. n_gpus-1 of this process (replaces the OpenMP pixel loop of
 * src/rt.cpp:767-805 on a multi-GPU node without a launcher).  Device g renders the file-row
 * bands g, g + n_gpus, ... (band_rows of `p` when it cuts the image, else 16 rows; p itself must
 * describe the whole image: band_stride 1, band_offset 0); the strips are gathered to device 0
 * over RCCL (one communicator per device, ncclCommInitAll; grouped ncclSend/ncclRecv) and
 * written to h_out in file order.  Bit-identical to vpt_render for any n_gpus.  Synchronous.
 * vpt_multi_* keep the contexts, streams, communicators and buffers between images. */
typedef struct vpt_multi vpt_multi;
int vpt_multi_create(int n_gpus, vpt_multi** out);
int vpt_multi_set_scene(vpt_multi* m, const vpt_sphere* spheres, int n);
/* vpt_set_density_grid on every context of the handle */
int vpt_multi_set_density_grid(vpt_multi* m, const vpt_grid_desc* desc, const float* density);
/* vpt_set_grid_majorant_block on every context of the handle */
int vpt_multi_set_grid_majorant_block(vpt_multi* m, int block);
/* vpt_set_grid_interpolation on every context of the handle */
int vpt_multi_set_grid_interpolation(vpt_multi* m, int mode);
/* vpt_set_emission_grid on every context of the handle */
int vpt_multi_set_emission_grid(vpt_multi* m, const float* eps, const double rgb[3]);
int vpt_multi_render(vpt_multi* m, const vpt_params* p, void* h_out);
void vpt_multi_destroy(vpt_multi* m);
/* one-shot: create, set the scene, render, destroy */
int vpt_render_multi(const vpt_sphere* spheres, int n, const vpt_params* p, int n_gpus, void* h_out);

/* ---- progressive accumulator: a render that can be continued, with a per-tile error ----
 * An accumulator holds, per pixel of p's shard, the sum of the samples received so far and a running
 * noise statistic (csrc/vpt_accum.h), and per 8x8 tile (row-major over the shard, tiles_x per row) a level
 * count and an error.  Samples arrive in chunk levels of C samples: level k of a pixel is its samples
 * [kC, kC + C), so a pixel that holds m levels -- through any sequence of vpt_accum_add / vpt_accum_refine
 * calls -- resolves to the bits of vpt_render(spp = mC, chunk_spp = C) for that pixel.
 * p->spp is the cap (most samples a pixel may receive), a multiple of C; C = p->chunk_spp, or min(32, spp)
 * when that is 0; estimators 0-5 (6-9 have no chunks: VPT_E_UNSUPPORTED); band_* are honoured, so a shard
 * can be accumulated.  The partial-sum buffer holds only the levels of one pass.
 * All calls are synchronous except vpt_accum_resolve_device.  The context must outlive the accumulator, and
 * its scene must not change (vpt_set_scene) while an accumulator holds samples: that is the caller's error
 * and is not detected.  One accumulator is used by one thread at a time. */
typedef struct vpt_accum vpt_accum;

int vpt_accum_create(vpt_context* ctx, const vpt_params* p, vpt_accum** out);
/* The accumulator of the density-grid estimators (10-16), which vpt_accum_create refuses because they have no chunked
 * sum: the same handle and the same calls below, with a contract of its own.  These estimators sum a pixel's samples
 * strictly in order, and a pass continues that sum from the state.  For a pixel that holds m levels:
 *   sum     is acc = L + acc over samples 0 .. mC - 1 of its stream, in order, from zero, whatever calls, tile lists and
 *           groups brought the levels; the resolve scales by 1 / (double)(mC).  So the pixel is the pixel of
 *           vpt_render(spp = mC), bit for bit, in FP64 and FP32; C does not change the image, it is the granularity of a
 *           level and of the error statistic;
 *   s1, s2  are as above: level k contributes y = lum(c_k), c_k the sum of samples [kC, kC + C) formed as c = L + c from
 *           zero; s1 = y + s1, s2 = y*y + s2.  sum is not the sum of the c_k here: only the statistic sees the chunks;
 *   errors, the active rule, vpt_accum_refine and its report are the ones below, unchanged.
 * C = p->chunk_spp, or min(32, spp) when that is 0; p->spp, the cap, is a multiple of C.  Returns what vpt_render returns
 * for the same parameters and context (no grid, estimator 15 without a majorant block, a channel without extinction:
 * VPT_E_INVALID; an emission grid under estimators 12-16: VPT_E_UNSUPPORTED); an estimator below 10 is VPT_E_INVALID
 * (vpt_accum_create is theirs).  Tile subsets are served for all seven estimators, and tiles at different level counts
 * are one launch.  Every pass validates again: after vpt_clear_density_grid, or a setting that makes the estimator
 * invalid, vpt_accum_add / vpt_accum_refine fail with the render's status and change no state.  The scene, the grid and
 * its settings (majorant block, interpolation, emission, medium colour, track fraction) must not change while the
 * accumulator holds samples: as for the scene above, that is the caller's error and is not detected. */
int vpt_accum_create_grid(vpt_context* ctx, const vpt_params* p, vpt_accum** out);
void vpt_accum_destroy(vpt_accum* a);
/* the tile grid, the chunk size C and the cap in levels (any pointer may be NULL) */
int vpt_accum_tiles(const vpt_accum* a, int* tiles_x, int* tiles_y, int* chunk, int* max_levels);

/* `levels` more chunk levels for the n_tiles listed tiles (tiles NULL = all): indices in [0, tiles_x *
 * tiles_y), no duplicates, any order.  A tile that would pass max_levels, a duplicate or an index out of
 * range -> VPT_E_INVALID, and nothing is rendered.  A list that is not the whole tile set needs estimator 0 or 1
 * (the tile-list variant of the pool kernel exists for these two): VPT_E_UNSUPPORTED otherwise, also from
 * vpt_accum_refine once its active set is a subset (the passes made until then stay). */
int vpt_accum_add(vpt_accum* a, int levels, const int32_t* tiles, int n_tiles);

/* Adaptive refinement.  A tile is active iff levels < max_levels && (levels < min_levels || err > target);
 * a NaN error therefore retires a tile once it has min_levels.  lum_floor: the mean luminance below which
 * the error is taken relative to lum_floor instead (0.01 by default; it also becomes the floor of later
 * vpt_accum_add calls).  min_levels >= 2 (one level has no variance). */
typedef struct vpt_refine {
    double target, lum_floor;
    int32_t min_levels, levels_per_pass;
} vpt_refine;
typedef struct vpt_refine_report {
    int32_t passes;            /* passes this call made */
    int32_t tiles_converged;   /* tiles whose error is not above target */
    int32_t tiles_capped;      /* tiles stopped by max_levels with an error above target */
    uint64_t samples;          /* camera samples this call rendered (valid pixels x levels x C) */
    double max_err;            /* largest tile error at the end (NaN if any tile's is NaN) */
} vpt_refine_report;
/* repeats vpt_accum_add (levels_per_pass levels, fewer where the cap is nearer) on the active tiles until
 * none is active; report may be NULL */
int vpt_accum_refine(vpt_accum* a, const vpt_refine* r, vpt_refine_report* report);

/* The image so far: per pixel sum * (1 / (double)(levels * C)) with its tile's level count, 0 for a tile
 * without samples; vpt_shard_rows * width * 3 elements of fb_format, file order. */
int vpt_accum_resolve(vpt_accum* a, int fb_format, void* h_out);
/* enqueues the resolve on `stream` (NULL = default stream) and returns; the caller synchronises that
 * stream before reading d_out */
int vpt_accum_resolve_device(vpt_accum* a, int fb_format, void* d_out, void* stream);

/* state download, any pointer may be NULL: sum[rows*w*3], s12[rows*w*2] (s1, s2 per pixel),
 * tile_levels[tiles], tile_err[tiles] (+inf below two levels) */
int vpt_accum_read(vpt_accum* a, double* sum, double* s12, int32_t* tile_levels, double* tile_err);

/* csrc/vpt_accum.h on host arrays (no GPU needed): the chunk sums csum[m][npix][3] of m levels -> per pixel
 * sum[3], s12[2] and err (any output may be NULL); chunk = C */
int vpt_accum_stat_host(const double* csum, int m, int64_t npix, int chunk, double lum_floor, double* sum, double* s12,
                        double* err);
/* the refine policy on host arrays (no GPU needed): returns the number of active tiles and writes their
 * ascending indices to active (n_tiles entries), or a negative vpt_status */
int vpt_accum_select_host(const int32_t* tile_levels, const double* tile_err, int n_tiles, const vpt_refine* r,
                          int max_levels, int32_t* active);

/* The per-sample call itself, batched: rays[i] with erand48 start state states[i] (low 48
 * bits) through the estimator of `m`; out_rgb[3i..3i+2] = the Color the reference returns,
 * out_states[i] (optional) = the erand48 state afterwards.  Host pointers; synchronous. */
int vpt_trace_batch(vpt_context* ctx, const vpt_medium* m, const vpt_ray* rays, const uint64_t* states, int n,
                    double* out_rgb, uint64_t* out_states);

/* punctualVolumetric(idsource, x, phase, sigma_t, sigma_s) (include/rayMarchingMethods.h:12-31; no
 * caller in the reference) at the n points x[3i..3i+2]: visibilityVPT from sphere idsource's centre,
 * radiance / distance^2 * phase * multipleT * sigma_s.  Host arrays; synchronous. */
int vpt_punctual_volumetric(vpt_context* ctx, int idsource, const double* x, int n, double phase, double sigma_t,
                            double sigma_s, double* out_rgb);

/* rayMarching(r, sigma_t, sigma_s, steps, x_new, idsource) (include/rayMarchingMethods.h:34-103) for
 * rays[i] with erand48 start state states[i]: out_rgb = the Color; x_new[3i..] and idsource[i] are
 * in/out like the reference's reference parameters (set to the first hit, unchanged on a miss);
 * out_states optional.  Needs >= 6 spheres (sphere 5 is hard-coded).  Host arrays; synchronous. */
int vpt_ray_marching_batch(vpt_context* ctx, double sigma_t, double sigma_s, double steps, const vpt_ray* rays,
                           const uint64_t* states, int n, double* out_rgb, double* x_new, int32_t* idsource,
                           uint64_t* out_states);

/* Counting mode: ray-sphere tests (Sphere::intersect calls, include/Sphere.h:27) the render
 * of `p` performs in the REFERENCE algorithm (shortcuts of this build count what they skip),
 * plus estimator loop iterations.  Synchronous. */
int vpt_count_work(vpt_context* ctx, const vpt_params* p, uint64_t* tests, uint64_t* iterations);

/* Start state of one sample's erand48 stream (host-side statement of the device spec). */
uint64_t vpt_stream_state(uint64_t seed, uint64_t pixel_idx, uint64_t sample);

/* Evaluates the device math library on the GPU: fn 0 sqrt, 1 exp, 2 log, 3 sin, 4 cos, 5 tan,
 * 6 atan, 7 acos, 8 atan2(x, y), 9 x / y, 10 / 11 sin / cos of acos(x), 12 1 / sqrt(x) (the
 * normalisation's reciprocal).  Host arrays, synchronous (parity tests). */
int vpt_math_probe(vpt_context* ctx, int fn, const double* x, const double* y, double* out, int n);

/* Henyey-Greenstein phase extension (the north-star's HG g; the reference has only the isotropic
 * phase, include/vptSamplingFunctions.h:34-47 and include/volumetricBasicFunctions.h:59-62, which
 * g == 0 reproduces bit for bit).  For each of the n erand48 states: the direction the medium event
 * samples around the propagation direction din (two draws), and the state after them; for each of
 * the nw directions wl: the phase value the NEE weights with (mu = din . wl).  Host arrays,
 * synchronous (property tests). */
int vpt_phase_probe(vpt_context* ctx, double g, const double din[3], const uint64_t* states, int n, double* dirs,
                    uint64_t* states_out, const double* wl, int nw, double* values);

/* The majorant build on the host, on a grid given directly (no GPU needed): for block >= 1 and interp (vpt_grid_interp)
 * the nbv = nb[0] nb[1] nb[2] block maxima of `density` and behind them the nbv block minima into out (2 nbv floats,
 * nb[a] = ceil(n[a] / block)), and the largest voxel into rho_max.  vpt_grid_majorant_scatter_host is the build of
 * vpt_set_density_grid (csrc/vpt_grid.h: every voxel updates the blocks it counts for), vpt_grid_majorant_gather_host
 * the statement per output that the device builder runs (csrc/vpt_grid_build.h); the two agree bit for bit on every
 * input.  The dimensions and the box are checked, the voxels are not. */
int vpt_grid_majorant_scatter_host(const vpt_grid_desc* desc, const float* density, int block, int interp, float* out,
                                   double* rho_max);
int vpt_grid_majorant_gather_host(const vpt_grid_desc* desc, const float* density, int block, int interp, float* out,
                                  double* rho_max);
/* Density-grid probe (csrc/vpt_grid.h) on the GPU, in the style of vpt_phase_probe: for each of the n rays
 * (unit directions) with surface distance tmax[i] and erand48 state states[i]: tau[i] = the optical depth of
 * the context's grid over t in [0, tmax[i]] (no draw), t_coll[i] = the delta-tracking result for sigma_t (-1:
 * none, NaN: the 2^22-step cap), states_out[i] = the state after the track.  Host arrays, synchronous. */
int vpt_grid_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                   int n, double* tau, double* t_coll, uint64_t* states_out);
/* the same code compiled for the host, on a grid given directly (no GPU needed) */
int vpt_grid_probe_host(const vpt_grid_desc* desc, const float* density, double sigma_t, const vpt_ray* rays,
                        const double* tmax, const uint64_t* states, int n, double* tau, double* t_coll,
                        uint64_t* states_out);
/* The two probes above always track with the global majorant.  vpt_grid_probe_lm honours the context's
 * vpt_set_grid_majorant_block setting and vpt_grid_probe_host_lm takes the block size (0: the global majorant,
 * < 0 -> VPT_E_INVALID); steps (may be NULL): per ray the tentative steps of the track, one per draw of a free
 * path (csrc/vpt_grid.h). */
int vpt_grid_probe_lm(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                      int n, double* tau, double* t_coll, uint64_t* states_out, uint32_t* steps);
int vpt_grid_probe_host_lm(const vpt_grid_desc* desc, const float* density, int block, double sigma_t, const vpt_ray* rays,
                           const double* tmax, const uint64_t* states, int n, double* tau, double* t_coll,
                           uint64_t* states_out, uint32_t* steps);
/* Ratio-tracking probe (csrc/vpt_grid.h: vpt_grid_ratio, vpt_grid_ratio_lm; estimator VPT_HETERO_RATIO's
 * transmittance): that[i] = the estimate of exp(-sigma_t tau) over t in [0, tmax[i]] from states[i] (in [0, 1];
 * NaN: the 2^22-step cap), states_out[i] = the state after it, steps[i] (may be NULL) = its draws.  The GPU probe
 * honours the context's vpt_set_grid_majorant_block setting; the host probe takes the block size (0: the global
 * majorant, < 0 -> VPT_E_INVALID).  Host arrays, synchronous. */
int vpt_grid_ratio_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax,
                         const uint64_t* states, int n, double* that, uint64_t* states_out, uint32_t* steps);
int vpt_grid_ratio_probe_host(const vpt_grid_desc* desc, const float* density, int block, double sigma_t,
                              const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                              uint64_t* states_out, uint32_t* steps);
/* The three GPU probes above honour the context's vpt_set_grid_interpolation setting (the default is nearest).  The
 * host probes with an explicit mode (a vpt_grid_interp; any other value -> VPT_E_INVALID): vpt_grid_probe_host_lm and
 * vpt_grid_ratio_probe_host are these with interp = VPT_GRID_NEAREST. */
int vpt_grid_probe_host_ex(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                           const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* tau,
                           double* t_coll, uint64_t* states_out, uint32_t* steps);
int vpt_grid_ratio_probe_host_ex(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                                 const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                                 uint64_t* states_out, uint32_t* steps);
/* Residual ratio-tracking probe (csrc/vpt_grid.h: vpt_grid_residual_lm_m; estimator VPT_HETERO_RESIDUAL's transmittance):
 * that[i] = the estimate of exp(-sigma_t tau) over t in [0, tmax[i]] from states[i] (in [0, exp(-sigma_t tauc[i])]; NaN:
 * the 2^22-step cap), tauc[i] = the control optical depth the walk took analytically (the block minima integrated over
 * the part of the segment inside the box; up to the tentative point where that[i] is +0), states_out[i] = the state after
 * it, steps[i] (may be NULL) = its draws.  The GPU probe reads the context's grid, majorant block and interpolation:
 * without a grid or with block 0 -> VPT_E_INVALID.  The host probe takes them as arguments: block < 1, a bad grid or a bad
 * mode -> VPT_E_INVALID.  Host arrays, synchronous. */
int vpt_grid_residual_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                            int n, double* that, double* tauc, uint64_t* states_out, uint32_t* steps);
int vpt_grid_residual_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t,
                                 const vpt_ray* rays, const double* tmax, const uint64_t* states, int n, double* that,
                                 double* tauc, uint64_t* states_out, uint32_t* steps);

/* Emission probe (csrc/vpt_grid.h: vpt_grid_track_em_m, vpt_grid_track_lm_em_m): the delta track of vpt_grid_probe_lm from
 * states[i] over t in [0, tmax[i]] with the collision estimator of the emission grid: t_coll[i], states_out[i] and steps[i]
 * (may be NULL) are that probe's bit for bit, esum[i] = the sum of rho eps / mu over the track's tentative collisions, whose
 * expectation is sigma_t times the integral of T rho eps along the tracked segment.  The GPU probe reads the context's
 * emission grid (VPT_E_INVALID without one) and honours its majorant block and interpolation; the host probe takes the
 * density, eps (both nx x ny x nz), the block size and the mode.  Host arrays, synchronous. */
int vpt_grid_emission_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states,
                            int n, double* t_coll, double* esum, uint64_t* states_out, uint32_t* steps);
int vpt_grid_emission_probe_host(const vpt_grid_desc* desc, const float* density, const float* eps, int block, int interp,
                                 double sigma_t, const vpt_ray* rays, const double* tmax, const uint64_t* states, int n,
                                 double* t_coll, double* esum, uint64_t* states_out, uint32_t* steps);

/* Equi-angular probe (csrc/vpt_grid_eqa.h: vpt_grid_eqa_one; one distance decision of estimator
 * VPT_HETERO_EQUIANGULAR).  For each of the n rays (unit directions) with surface distance tmax[i], light position
 * light[3 i .. 3 i + 2] and erand48 state states[i]: psurf[i] = the grid's transmittance over [0, tmax[i]] for sigma_t;
 * two draws, always -- the equi-angular draw, then the coin; coin < psurf is the surface branch: dist[i] = -1 and
 * pdf[i] = T[i] = rho_t[i] = +0.  Else dist[i] = the equi-angular distance toward the light inside the part of
 * [0, tmax[i]] the box holds, pdf[i] = its density times 1 - psurf[i], rho_t[i] = the density at o + d dist[i] and T[i] =
 * the transmittance over [0, dist[i]] (+0 where rho_t[i] == 0: the path ends there).  states_out[i] = the state after
 * the two draws.  The GPU probe reads the context's grid and interpolation (VPT_E_INVALID without a grid); the host
 * probe takes the density and the mode (a vpt_grid_interp).  Host arrays, synchronous. */
int vpt_grid_eqa_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const double* light,
                       const uint64_t* states, int n, double* psurf, double* dist, double* pdf, double* T, double* rho_t,
                       uint64_t* states_out);
int vpt_grid_eqa_probe_host(const vpt_grid_desc* desc, const float* density, int interp, double sigma_t, const vpt_ray* rays,
                            const double* tmax, const double* light, const uint64_t* states, int n, double* psurf, double* dist,
                            double* pdf, double* T, double* rho_t, uint64_t* states_out);

/* The track fraction q of estimator VPT_HETERO_MIS: the probability that a distance decision runs a delta track and not
 * the equi-angular strategy.  Finite and in [0, 1], else VPT_E_INVALID and the previous value stays; the default is 0.5.
 * Belongs to the context, like the majorant block: it needs no grid and survives grid and scene changes.  Takes effect
 * with the next render or trace; other estimators do not read it. */
int vpt_set_hetero_mis_fraction(vpt_context* ctx, double q);
int vpt_multi_set_hetero_mis_fraction(vpt_multi* m, double q);

/* MIS probe (csrc/vpt_grid_mis.h: vpt_grid_mis_one; one distance decision of estimator VPT_HETERO_MIS).  The inputs are
 * vpt_grid_eqa_probe's and the track fraction q.  psurf[i] = the grid's transmittance over [0, tmax[i]]; two draws,
 * always -- the equi-angular draw, then the coin c; c < q is the track strategy (strategy[i] = 1): a delta track from
 * the state after the coin, with steps[i] tentative steps; else (strategy[i] = 0, steps[i] = 0) the equi-angular
 * strategy with the surface coin (c - q) / (1 - q).  On the surface dist[i] = -1 and pdf[i] = pe[i] = T[i] = rho_t[i] = +0;
 * at the track's step cap dist[i] = NaN and the four are +0.  Else dist[i] = the sampled distance, pe[i] = the
 * equi-angular density there times 1 - psurf[i], rho_t[i] = the density at o + d dist[i], T[i] = the transmittance over
 * [0, dist[i]] (+0 where rho_t[i] == 0: the path ends there) and pdf[i] = q * (sigma_t * rho_t[i] * T[i]) + (1 - q) * pe[i],
 * the combined density the vertex is weighted by.  states_out[i] = the state after all draws.  Every output array may
 * be NULL in the host probe and none in the GPU probe.  The GPU probe reads the context's grid, majorant block,
 * interpolation and track fraction (VPT_E_INVALID without a grid); the host probe takes the density, the block size
 * (0: the global majorant), the mode and q (not finite or outside [0, 1] -> VPT_E_INVALID).  At q == 0 psurf, dist, pdf,
 * T, rho_t and states_out are vpt_grid_eqa_probe's bit for bit.  Host arrays, synchronous. */
int vpt_grid_mis_probe(vpt_context* ctx, double sigma_t, const vpt_ray* rays, const double* tmax, const double* light,
                       const uint64_t* states, int n, double* psurf, int32_t* strategy, double* dist, double* pdf, double* pe,
                       double* T, double* rho_t, uint32_t* steps, uint64_t* states_out);
int vpt_grid_mis_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, double sigma_t, double q,
                            const vpt_ray* rays, const double* tmax, const double* light, const uint64_t* states, int n,
                            double* psurf, int32_t* strategy, double* dist, double* pdf, double* pe, double* T, double* rho_t,
                            uint32_t* steps, uint64_t* states_out);

/* The medium colour of estimators VPT_HETERO_CHROMATIC and VPT_HETERO_SPECTRAL: per colour channel c the multipliers absorb[c] of the medium's
 * sigma_a and scatter[c] of its sigma_s, so that per unit density sa_c = sigma_a * absorb[c], ss_c = sigma_s * scatter[c]
 * and st_c = sa_c + ss_c.  Every value finite and >= 0, else VPT_E_INVALID and the previous values stay; the default is
 * (1, 1, 1) for both.  Belongs to the context, like the track fraction: it needs no grid and survives grid and scene
 * changes.  Takes effect with the next render or trace; other estimators do not read it.  A render or trace of either
 * estimator with some st_c == 0 is VPT_E_INVALID. */
int vpt_set_medium_colour(vpt_context* ctx, const double absorb[3], const double scatter[3]);
int vpt_multi_set_medium_colour(vpt_multi* m, const double absorb[3], const double scatter[3]);

/* Chromatic probe (csrc/vpt_grid_chroma.h: vpt_grid_chroma_one; one distance decision of estimator
 * VPT_HETERO_CHROMATIC).  For each of the n rays (unit directions) with surface distance tmax[i] and erand48 state
 * states[i]: hero[i] = the hero channel -- one draw, none and channel 0 where the three st_c are equal; a delta track
 * under st_hero from the state after that draw, with steps[i] tentative steps: t_coll[i] = the collision distance, -1
 * for "none", NaN at the step cap.  At a collision tau[i] = the optical depth over [0, t_coll[i]] and w = the weight
 * that stands in the albedo's place, w_c = ss_c e_c / ((sum_k st_k e_k) / 3) with e_k = exp(-(st_k tau - min_j st_j tau));
 * at "none" tau[i] = the optical depth over [0, tmax[i]] and w_c = e_c / ((sum_k e_k) / 3), the weight of the surface
 * branch; at the cap tau[i] and w are +0.  w holds 3 n doubles, channel c of ray i at w[c * n + i].  states_out[i] = the
 * state after all draws.  Every output array may be NULL in the host probe and none in the GPU probe.  The GPU probe
 * reads the context's grid, majorant block, interpolation and medium colour (VPT_E_INVALID without a grid) and takes
 * the medium's sigma_a and sigma_s; the host probe takes the density, the block size (0: the global majorant), the mode
 * and the six coefficients sa[3], ss[3] per unit density themselves (st_c = sa[c] + ss[c]).  A coefficient that is not
 * finite or negative, or some st_c == 0, is VPT_E_INVALID.  Host arrays, synchronous. */
int vpt_grid_chroma_probe(vpt_context* ctx, double sigma_a, double sigma_s, const vpt_ray* rays, const double* tmax,
                          const uint64_t* states, int n, int32_t* hero, double* t_coll, double* tau, double* w, uint32_t* steps,
                          uint64_t* states_out);
int vpt_grid_chroma_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, const double sa[3],
                               const double ss[3], const vpt_ray* rays, const double* tmax, const uint64_t* states, int n,
                               int32_t* hero, double* t_coll, double* tau, double* w, uint32_t* steps, uint64_t* states_out);

/* Spectral-tracking probe (csrc/vpt_grid_spectral.h: vpt_grid_spectral_one; the two walkers of estimator
 * VPT_HETERO_SPECTRAL), each from states[i].  The spectral delta track over [0, tmax[i]] of a path that carries the
 * throughput beta[3 i .. 3 i + 2] (beta may be NULL: ones): t_coll[i] = the collision distance, -1 for "none", NaN at the
 * step cap; w = the track's weight per channel -- at "none" the surface's weight W, at a collision W times the albedo
 * ss_c / st_c, +0 at the cap -- channel c of ray i at w[c * n + i]; steps[i] = its tentative steps, states_out[i] = the
 * state after it.  Chromatic ratio tracking over [0, tmax[i]]: T[c * n + i] = channel c's estimate of exp(-st_c tau) (NaN:
 * the step cap), ratio_steps[i] = its draws, ratio_states_out[i] = the state after it.  Every output array may be NULL in
 * the host probe and none in the GPU probe.  The GPU probe reads the context's grid, majorant block, interpolation and
 * medium colour (VPT_E_INVALID without a grid) and takes the medium's sigma_a and sigma_s; the host probe takes the
 * density, the block size (0: the global majorant), the mode and the six coefficients sa[3], ss[3] per unit density
 * themselves (st_c = sa[c] + ss[c]).  A coefficient that is not finite or negative, or some st_c == 0, is VPT_E_INVALID.
 * Host arrays, synchronous. */
int vpt_grid_spectral_probe(vpt_context* ctx, double sigma_a, double sigma_s, const vpt_ray* rays, const double* tmax,
                            const double* beta, const uint64_t* states, int n, double* t_coll, double* w, uint32_t* steps,
                            uint64_t* states_out, double* T, uint32_t* ratio_steps, uint64_t* ratio_states_out);
int vpt_grid_spectral_probe_host(const vpt_grid_desc* desc, const float* density, int block, int interp, const double sa[3],
                                 const double ss[3], const vpt_ray* rays, const double* tmax, const double* beta,
                                 const uint64_t* states, int n, double* t_coll, double* w, uint32_t* steps,
                                 uint64_t* states_out, double* T, uint32_t* ratio_steps, uint64_t* ratio_states_out);

/* PPM writer of main() (src/rt.cpp:812-820): clamp to [0,1] (src/rt.cpp:803), gamma 1/2.2,
 * int(v*255 + .5) (include/mathUtilities.h:43-45), "P3\n%d %d\n255\n" then "%d %d %d " per
 * pixel, byte-identical.  rgb: host framebuffer, w*h*3 of fb_format, file order. */
int vpt_write_ppm(const char* path, const void* rgb, int fb_format, int w, int h);
/* The same bytes into a caller buffer; returns the byte count (call with buf = NULL to size). */
int64_t vpt_encode_ppm(const void* rgb, int fb_format, int w, int h, char* buf, int64_t cap);

const char* vpt_last_error(void);
int vpt_abi_version(void);
/* Build provenance: 16 hex digits hashing the library's sources and compile flags
 * (scripts/build_id.py, baked in by csrc/Makefile). */
const char* vpt_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* VPT_H */
