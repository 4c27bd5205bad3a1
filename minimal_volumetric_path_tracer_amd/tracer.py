"""Host-side mirror of the reference's interface for the volumetric radiance loop.

Reference (gabo99cas/minimal_volumetric_path_tracer):
  * scene: ``std::vector<Sphere> spheres`` (include/Sphere.h:49, include/Sphere.cpp:7-107) with
    ``Sphere(r, p, c, radiance, material, eta, kappa, alpha)`` (include/Sphere.h:23);
  * per-sample estimators ``iterativeVPTracerFree(ray, sigma_a, sigma_s)``
    (include/vptShadeMethods.h:1263, the one ``main`` calls), ``MISVPTTracerRecursive(ray, sigma_a,
    sigma_s, depth)`` (:1345), ``explicitVPTracerRecursiveFree`` (:1153),
    ``implicitVPTracerRecursiveFree`` (:940) and ``explicitVPTracerRecursive`` (:1014), returning a Color;
  * ``main`` (src/rt.cpp:744-830): camera, pixel loop, average, clamp, ``image.ppm``.

Here the same names take batches and run through libvpt.so (HIP, gfx950).  Argument meaning is
the reference's; its undefined behaviour (uninitialised argv, >4 emitters, unchecked fopen)
becomes an exception.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, byref, c_int, c_uint64, c_void_p
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (EXPLICIT_EQUIANGULAR, EXPLICIT_FREE, FB_F32, FB_F64, FREE_FLIGHT, HETERO_EQUIANGULAR, HETERO_CHROMATIC, HETERO_FREE, HETERO_MIS, HETERO_RATIO, HETERO_RESIDUAL, HETERO_SPECTRAL, IMPLICIT_FREE, MIS_EQUIANGULAR,
                   RAY_DTYPE, RAY_MARCHING, RAY_MARCHING_EXPLICIT, RAY_MARCHING_GLOBAL, RAY_MARCHING_SA, SPHERE_DTYPE,
                   SURFACE_PT, check, lib)

ESTIMATORS = {"ff": FREE_FLIGHT, "free_flight": FREE_FLIGHT, "mis": MIS_EQUIANGULAR, "mis_equiangular": MIS_EQUIANGULAR,
              "explicit_free": EXPLICIT_FREE, "implicit_free": IMPLICIT_FREE, "explicit": EXPLICIT_EQUIANGULAR,
              "explicit_equiangular": EXPLICIT_EQUIANGULAR, "surface_pt": SURFACE_PT, "path_tracer": SURFACE_PT,
              "ray_marching": RAY_MARCHING, "ray_marching_sa": RAY_MARCHING_SA, "ray_marching_global": RAY_MARCHING_GLOBAL,
              "ray_marching_explicit": RAY_MARCHING_EXPLICIT, "hetero": HETERO_FREE, "hetero_free": HETERO_FREE,
              "hetero_ratio": HETERO_RATIO, "hetero_equiangular": HETERO_EQUIANGULAR, "hetero_eqa": HETERO_EQUIANGULAR,
              "hetero_mis": HETERO_MIS, "hetero_mis_equiangular": HETERO_MIS,
              "hetero_chromatic": HETERO_CHROMATIC, "hetero_rgb": HETERO_CHROMATIC,
              "hetero_residual": HETERO_RESIDUAL, "hetero_residual_ratio": HETERO_RESIDUAL,
              "hetero_spectral": HETERO_SPECTRAL, "hetero_spectral_tracking": HETERO_SPECTRAL}


def Sphere(r, p, c=(0, 0, 0), radiance=(0, 0, 0), material=0, eta=(0, 0, 0), kappa=(0, 0, 0), alpha=0.0) -> np.ndarray:
    """One reference Sphere record (include/Sphere.h:23 argument order) as a SPHERE_DTYPE scalar array."""
    s = np.zeros(1, dtype=SPHERE_DTYPE)
    s["r"], s["p"], s["c"], s["radiance"] = r, p, c, radiance
    s["material"], s["eta"], s["kappa"], s["alpha"] = material, eta, kappa, alpha
    return s


def scene(*spheres: np.ndarray) -> np.ndarray:
    return np.concatenate(spheres).astype(SPHERE_DTYPE)


def default_scene() -> np.ndarray:
    """The reference scene, include/Sphere.cpp:11-22 (10 spheres)."""
    n = lib().vpt_default_scene(None, 0)
    out = np.zeros(n, dtype=SPHERE_DTYPE)
    lib().vpt_default_scene(out.ctypes.data, n)
    return out


def Ray(o: Sequence[float], d: Sequence[float]) -> np.ndarray:
    r = np.zeros(1, dtype=RAY_DTYPE)
    r["o"], r["d"] = o, d
    return r


def stream_state(seed: int, pixel_idx: int, sample: int) -> int:
    """erand48 start state of one camera sample (csrc/vpt_rng.h)."""
    return int(lib().vpt_stream_state(seed, pixel_idx, sample))


def _grid_args(rho, lo, hi) -> tuple[_lib.vpt_grid_desc, np.ndarray]:
    """(vpt_grid_desc, float32 voxels) of a density array of shape [nz, ny, nx] (x fastest) in the box [lo, hi]."""
    r = np.ascontiguousarray(rho, dtype=np.float32)
    return _grid_desc(r, lo, hi), r


def _grid_desc(r, lo, hi) -> _lib.vpt_grid_desc:
    """the vpt_grid_desc of voxels r (an array or a tensor) of shape [nz, ny, nx] in the box [lo, hi]"""
    if r.ndim != 3:
        raise ValueError("rho must have shape [nz, ny, nx]")
    d = _lib.vpt_grid_desc()
    d.nz, d.ny, d.nx = r.shape
    d.lo[:] = [float(v) for v in lo]
    d.hi[:] = [float(v) for v in hi]
    return d


def _probe_args(rays, tmax, states):
    r = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float64), (len(r),)))
    s = np.ascontiguousarray(states, dtype=np.uint64)
    if len(r) != len(s):
        raise ValueError("rays and states must have the same length")
    return r, t, s, np.zeros(len(r)), np.zeros(len(r)), np.zeros(len(r), dtype=np.uint64)


INTERPOLATIONS = {"nearest": _lib.GRID_NEAREST, "trilinear": _lib.GRID_TRILINEAR}


def _interp_mode(name) -> int:
    """the vpt_grid_interp of "nearest" / "trilinear"; any other name is VPT_E_INVALID"""
    if name not in INTERPOLATIONS:
        raise _lib.VPTError(_lib.VPT_E_INVALID, f"interpolation {name!r} (one of {', '.join(INTERPOLATIONS)})")
    return INTERPOLATIONS[name]


def grid_probe_host(rho, lo, hi, sigma_t: float, rays, tmax, states, majorant_block: int = 0, return_steps: bool = False,
                    interpolation: str = "nearest"):
    """csrc/vpt_grid.h on the host (vpt_grid_probe_host, no GPU): per ray (unit direction) the optical depth of
    the grid over t in [0, tmax], the delta-tracking result from `states` (-1: none, NaN: step cap) and the
    erand48 states after the track.  majorant_block > 0 tracks with local majorants on super-voxels of that
    many voxels per axis (vpt_grid_probe_host_lm); return_steps appends the tentative steps of each track;
    interpolation "trilinear" reads the field trilinearly (vpt_grid_probe_host_ex)."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, s, tau, tc, so = _probe_args(rays, tmax, states)
    if mode:
        steps = np.zeros(len(ry), dtype=np.uint32)
        check(lib().vpt_grid_probe_host_ex(byref(d), r.ctypes.data, int(majorant_block), mode, float(sigma_t), ry.ctypes.data,
                                           t.ctypes.data, s.ctypes.data, len(ry), tau.ctypes.data, tc.ctypes.data,
                                           so.ctypes.data, steps.ctypes.data))
        return (tau, tc, so, steps) if return_steps else (tau, tc, so)
    if not majorant_block and not return_steps:
        check(lib().vpt_grid_probe_host(byref(d), r.ctypes.data, float(sigma_t), ry.ctypes.data, t.ctypes.data,
                                        s.ctypes.data, len(ry), tau.ctypes.data, tc.ctypes.data, so.ctypes.data))
        return tau, tc, so
    steps = np.zeros(len(ry), dtype=np.uint32)
    check(lib().vpt_grid_probe_host_lm(byref(d), r.ctypes.data, int(majorant_block), float(sigma_t), ry.ctypes.data,
                                       t.ctypes.data, s.ctypes.data, len(ry), tau.ctypes.data, tc.ctypes.data,
                                       so.ctypes.data, steps.ctypes.data))
    return (tau, tc, so, steps) if return_steps else (tau, tc, so)


def grid_ratio_probe_host(rho, lo, hi, sigma_t: float, rays, tmax, states, majorant_block: int = 0,
                          interpolation: str = "nearest"):
    """csrc/vpt_grid.h's ratio tracking on the host (vpt_grid_ratio_probe_host, no GPU): per ray (unit direction)
    the estimate That of exp(-sigma_t tau) over t in [0, tmax] from `states` (NaN: step cap), the erand48 states
    after it and its draws.  majorant_block > 0 walks with local majorants on super-voxels of that many voxels
    per axis; interpolation "trilinear" reads the field trilinearly (vpt_grid_ratio_probe_host_ex)."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, s, that, _, so = _probe_args(rays, tmax, states)
    steps = np.zeros(len(ry), dtype=np.uint32)
    if mode:
        check(lib().vpt_grid_ratio_probe_host_ex(byref(d), r.ctypes.data, int(majorant_block), mode, float(sigma_t),
                                                 ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry), that.ctypes.data,
                                                 so.ctypes.data, steps.ctypes.data))
        return that, so, steps
    check(lib().vpt_grid_ratio_probe_host(byref(d), r.ctypes.data, int(majorant_block), float(sigma_t), ry.ctypes.data,
                                          t.ctypes.data, s.ctypes.data, len(ry), that.ctypes.data, so.ctypes.data,
                                          steps.ctypes.data))
    return that, so, steps


def grid_residual_probe_host(rho, lo, hi, sigma_t: float, rays, tmax, states, majorant_block: int = 0,
                             interpolation: str = "nearest"):
    """csrc/vpt_grid.h's residual ratio tracking on the host (vpt_grid_residual_probe_host, no GPU): per ray (unit
    direction) the estimate That of exp(-sigma_t tau) over t in [0, tmax] from `states` (NaN: step cap), the control
    optical depth tauc taken analytically, the erand48 states after the walk and its draws.  majorant_block >= 1 is
    required (the control is the minimum of each super-voxel); interpolation "trilinear" reads the field trilinearly."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, s, that, tauc, so = _probe_args(rays, tmax, states)
    steps = np.zeros(len(ry), dtype=np.uint32)
    check(lib().vpt_grid_residual_probe_host(byref(d), r.ctypes.data, int(majorant_block), mode, float(sigma_t),
                                             ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry), that.ctypes.data,
                                             tauc.ctypes.data, so.ctypes.data, steps.ctypes.data))
    return that, tauc, so, steps


def _eqa_probe_args(rays, tmax, light, states):
    r, t, s, _, _, so = _probe_args(rays, tmax, states)
    lp = np.ascontiguousarray(np.broadcast_to(np.asarray(light, dtype=np.float64), (len(r), 3)))
    return r, t, lp, s, [np.zeros(len(r)) for _ in range(5)], so


def grid_eqa_probe_host(rho, lo, hi, sigma_t: float, rays, tmax, light, states, interpolation: str = "nearest"):
    """csrc/vpt_grid_eqa.h on the host (vpt_grid_eqa_probe_host, no GPU): one equi-angular distance decision of
    estimator "hetero_equiangular" per ray (unit direction) with surface distance tmax, toward the light position(s)
    `light` (one, or one per ray), from `states`.  Returns (psurf, dist, pdf, T, rho_t, states): the surface
    probability, the sampled distance (-1 where the coin chose the surface), its pdf times 1 - psurf, the
    transmittance to the sampled point, the density there, and the erand48 states after the two draws."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, lp, s, res, so = _eqa_probe_args(rays, tmax, light, states)
    check(lib().vpt_grid_eqa_probe_host(byref(d), r.ctypes.data, mode, float(sigma_t), ry.ctypes.data, t.ctypes.data,
                                        lp.ctypes.data, s.ctypes.data, len(ry), *[a.ctypes.data for a in res],
                                        so.ctypes.data))
    return (*res, so)


def _mis_probe_results(n):
    """the output arrays of a MIS probe in the C argument order, and the tuple the Python probes return"""
    f = [np.zeros(n) for _ in range(6)]  # psurf, dist, pdf, pe, T, rho_t
    strategy, steps, so = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    c_order = [f[0], strategy, f[1], f[2], f[3], f[4], f[5], steps, so]
    return c_order, (f[0], strategy, f[1], f[2], f[3], f[4], f[5], steps, so)


def grid_mis_probe_host(rho, lo, hi, sigma_t: float, rays, tmax, light, states, q: float = 0.5, majorant_block: int = 0,
                        interpolation: str = "nearest"):
    """csrc/vpt_grid_mis.h on the host (vpt_grid_mis_probe_host, no GPU): one distance decision of estimator
    "hetero_mis" per ray -- grid_eqa_probe_host's inputs and the track fraction q in [0, 1]: with the coin below q the
    distance is a delta track's (majorant_block as in grid_probe_host), else the equi-angular one.  Returns (psurf,
    strategy, dist, pdf, pe, T, rho_t, steps, states): the surface probability, 1 where the track was taken, the
    sampled distance (-1 on the surface, NaN at the track's step cap), the combined pdf
    q sigma_t rho_t T + (1 - q) pe, the equi-angular pdf times 1 - psurf at the distance, the transmittance to the
    sampled point, the density there, the track's tentative steps and the erand48 states after all draws.  q = 0
    gives grid_eqa_probe_host's psurf, dist, pdf, T, rho_t and states bit for bit."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, lp, s, _, _ = _eqa_probe_args(rays, tmax, light, states)
    c_order, out = _mis_probe_results(len(ry))
    check(lib().vpt_grid_mis_probe_host(byref(d), r.ctypes.data, int(majorant_block), mode, float(sigma_t), float(q),
                                        ry.ctypes.data, t.ctypes.data, lp.ctypes.data, s.ctypes.data, len(ry),
                                        *[a.ctypes.data for a in c_order]))
    return out


def _colour_args(absorption, scattering) -> tuple[np.ndarray, np.ndarray]:
    """the two float64 triples of a medium colour; anything that is not three numbers is VPT_E_INVALID"""
    out = []
    for name, v in (("absorption", absorption), ("scattering", scattering)):
        a = np.ascontiguousarray(v, dtype=np.float64)
        if a.shape != (3,):
            raise _lib.VPTError(_lib.VPT_E_INVALID, f"{name}: three numbers (r, g, b), got shape {a.shape}")
        out.append(a)
    return out[0], out[1]


def _chroma_probe_results(n):
    """the output arrays of a chromatic probe in the C argument order; w is (3, n), a channel per row"""
    hero, tc, tau, w = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n), np.zeros((3, n))
    steps, so = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    return hero, tc, tau, w, steps, so


def grid_chroma_probe_host(rho, lo, hi, sigma_a: float, sigma_s: float, rays, tmax, states, absorption=(1.0, 1.0, 1.0),
                           scattering=(1.0, 1.0, 1.0), majorant_block: int = 0, interpolation: str = "nearest"):
    """csrc/vpt_grid_chroma.h on the host (vpt_grid_chroma_probe_host, no GPU): one distance decision of estimator
    "hetero_chromatic" per ray (unit direction) with surface distance tmax, from `states`, in a medium with
    sa_c = sigma_a * absorption[c] and ss_c = sigma_s * scattering[c] per unit density.  Returns (hero, t_coll, tau, w,
    steps, states): the hero channel (one draw; 0 and no draw where the three st_c are equal), the collision distance
    of the track under st_hero (-1: none, NaN: step cap), the optical depth up to the collision (to tmax at "none"),
    the per-channel weights as a (3, n) array -- w_c, which stands in the albedo's place, at a collision and ws_c at
    "none" --, the track's tentative steps and the erand48 states after all draws."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, s, _, _, _ = _probe_args(rays, tmax, states)
    ca, cs = _colour_args(absorption, scattering)
    sa, ss = float(sigma_a) * ca, float(sigma_s) * cs
    out = _chroma_probe_results(len(ry))
    check(lib().vpt_grid_chroma_probe_host(byref(d), r.ctypes.data, int(majorant_block), mode, sa.ctypes.data, ss.ctypes.data,
                                           ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry),
                                           *[a.ctypes.data for a in out]))
    return out


def _spectral_probe_args(n, beta):
    """(beta as (n, 3) float64 or None, the output arrays of a spectral probe in the C argument order); w and T are (3, n),
    a channel per row"""
    b = None
    if beta is not None:
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (n, 3)))
    out = (np.zeros(n), np.zeros((3, n)), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros((3, n)),
           np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64))
    return b, out


def grid_spectral_probe_host(rho, lo, hi, sigma_a: float, sigma_s: float, rays, tmax, states, absorption=(1.0, 1.0, 1.0),
                             scattering=(1.0, 1.0, 1.0), majorant_block: int = 0, interpolation: str = "nearest", beta=None):
    """csrc/vpt_grid_spectral.h on the host (vpt_grid_spectral_probe_host, no GPU): the two walkers of estimator
    "hetero_spectral" per ray (unit direction), each from `states`, in a medium with sa_c = sigma_a * absorption[c] and
    ss_c = sigma_s * scattering[c] per unit density.  beta: the throughput the path carries, three numbers or (n, 3)
    (default ones).  Returns (t_coll, w, steps, states, T, ratio_steps, ratio_states): the spectral delta track over
    [0, tmax] -- the collision distance (-1: none, NaN: step cap), the per-channel weight as a (3, n) array (W at "none",
    W times the albedo ss_c / st_c at a collision), its tentative steps and end states -- and chromatic ratio tracking over
    [0, tmax]: the three estimates of exp(-st_c tau) as a (3, n) array, its draws and end states."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    ry, t, s, _, _, _ = _probe_args(rays, tmax, states)
    ca, cs = _colour_args(absorption, scattering)
    sa, ss = float(sigma_a) * ca, float(sigma_s) * cs
    b, out = _spectral_probe_args(len(ry), beta)
    check(lib().vpt_grid_spectral_probe_host(byref(d), r.ctypes.data, int(majorant_block), mode, sa.ctypes.data, ss.ctypes.data,
                                             ry.ctypes.data, t.ctypes.data, None if b is None else b.ctypes.data,
                                             s.ctypes.data, len(ry), *[a.ctypes.data for a in out]))
    return out


def _emission_colour(rgb) -> np.ndarray:
    c = np.ascontiguousarray(rgb, dtype=np.float64)
    if c.shape != (3,):
        raise _lib.VPTError(_lib.VPT_E_INVALID, f"emission colour of shape {c.shape}: three numbers (r, g, b)")
    return c


def _emission_args(eps, rgb, shape) -> tuple[np.ndarray, np.ndarray]:
    """(float32 voxels, float64 colour) of an emission grid for a density grid of `shape` (None: not known here, the
    library says what is missing); another shape or a colour that is not three numbers is VPT_E_INVALID"""
    e = np.ascontiguousarray(eps, dtype=np.float32)
    if shape is not None and e.shape != tuple(shape):
        raise _lib.VPTError(_lib.VPT_E_INVALID, f"emission grid of shape {e.shape}: the density grid's is {tuple(shape)}")
    return e, _emission_colour(rgb)


def _on_gpu(x) -> bool:
    """a torch tensor in GPU memory, told by its attributes: torch is not imported here"""
    return bool(getattr(x, "is_cuda", False)) and hasattr(x, "data_ptr")


def _device_voxels(x, device: int):
    """(float32 contiguous tensor, its producer's stream) of a GPU tensor of voxels for the tracer on `device`; made
    float32 and contiguous on the device where it is not (a torch op on the current stream, no host round trip).  A
    tensor on another device is VPT_E_INVALID."""
    import torch  # the tensor is torch's, so it is there

    if x.device.index != device:
        raise _lib.VPTError(_lib.VPT_E_INVALID, f"tensor on {x.device}: the tracer's device is cuda:{device}")
    t = x.detach().to(dtype=torch.float32).contiguous()
    return t, torch.cuda.current_stream(x.device).cuda_stream


def _emission_shape_check(eps, shape) -> None:
    """_emission_args' refusal of another shape, for a GPU tensor"""
    if shape is not None and tuple(eps.shape) != tuple(shape):
        raise _lib.VPTError(_lib.VPT_E_INVALID,
                            f"emission grid of shape {tuple(eps.shape)}: the density grid's is {tuple(shape)}")


def _refuse_gpu_tensor(*grids) -> None:
    """MultiTracer's grids come from host arrays: a set from device memory would need one peer copy per context"""
    if any(_on_gpu(g) for g in grids):
        raise _lib.VPTError(_lib.VPT_E_UNSUPPORTED, "MultiTracer does not take a grid from a GPU tensor (device memory): "
                            "pass a host array, or use a Tracer per device")


def _majorant_host(fn, rho, block: int, interpolation: str):
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    if int(block) < 1:
        raise _lib.VPTError(_lib.VPT_E_INVALID, f"block {block} (>= 1)")
    nb = tuple((n - 1) // int(block) + 1 for n in r.shape)
    out = np.zeros((2,) + nb, dtype=np.float32)
    rho_max = ctypes.c_double()
    check(fn(byref(d), r.ctypes.data, int(block), mode, out.ctypes.data, byref(rho_max)))
    return out[0], out[1], rho_max.value


def grid_majorant_gather_host(rho, block: int, interpolation: str = "nearest"):
    """csrc/vpt_grid_build.h on the host (vpt_grid_majorant_gather_host, no GPU): the block maxima and minima of rho
    ([nz, ny, nx]) for super-voxels of `block` voxels per axis, stated per output as the device builder runs them.
    Returns (maxima[nbz, nby, nbx], minima[nbz, nby, nbx], rho_max), float32 and a float."""
    return _majorant_host(lib().vpt_grid_majorant_gather_host, rho, block, interpolation)


def grid_majorant_scatter_host(rho, block: int, interpolation: str = "nearest"):
    """grid_majorant_gather_host's quantities from the build that set_density_grid runs on a host array
    (vpt_grid_majorant_scatter_host: csrc/vpt_grid.h's vpt_grid_majorant_control_build and rho_max scan)."""
    return _majorant_host(lib().vpt_grid_majorant_scatter_host, rho, block, interpolation)


def grid_emission_probe_host(rho, eps, lo, hi, sigma_t: float, rays, tmax, states, majorant_block: int = 0,
                             interpolation: str = "nearest"):
    """csrc/vpt_grid.h's emitting delta track on the host (vpt_grid_emission_probe_host, no GPU): per ray (unit
    direction) grid_probe_host's collision distance, end state and tentative steps -- bit for bit -- and esum, the sum
    of rho eps / majorant over the track's tentative collisions (expectation: sigma_t times the integral of
    T rho eps along the tracked segment).  eps: the emission grid, rho's shape.  Returns (t_coll, esum, states, steps)."""
    mode = _interp_mode(interpolation)
    d, r = _grid_args(rho, lo, hi)
    e, _ = _emission_args(eps, (1, 1, 1), r.shape)
    ry, t, s, tc, es, so = _probe_args(rays, tmax, states)
    steps = np.zeros(len(ry), dtype=np.uint32)
    check(lib().vpt_grid_emission_probe_host(byref(d), r.ctypes.data, e.ctypes.data, int(majorant_block), mode, float(sigma_t),
                                             ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry), tc.ctypes.data,
                                             es.ctypes.data, so.ctypes.data, steps.ctypes.data))
    return tc, es, so, steps


def _set_grid_with_block(owner, block, upload, interpolation=None) -> None:
    """set_density_grid(..., majorant_block=block, interpolation=...) of Tracer and MultiTracer: the grid first -- a
    rejected grid leaves the grid and the settings as they were -- then the block size and the interpolation, where
    they change."""
    if block is not None and int(block) < 0:
        owner.set_majorant_block(block)  # raises VPT_E_INVALID before anything is uploaded
    if interpolation is not None:
        _interp_mode(interpolation)  # the same for an unknown name
    upload()
    if block is not None and int(block) != owner._majorant_block:
        owner.set_majorant_block(block)
    if interpolation is not None and interpolation != owner._grid_interpolation:
        owner.set_grid_interpolation(interpolation)


@dataclass
class RenderConfig:
    width: int = 1024
    height: int = 768
    spp: int = 16
    estimator: str = "ff"
    sigma_a: float = 0.001
    sigma_s: float = 0.009
    hg_g: float = 0.0
    max_depth: int = 0
    seed: int = 0x5EED0001
    fp64: bool = False
    band_rows: int = 0          # 0 = whole image
    band_stride: int = 1
    band_offset: int = 0
    chunk_spp: int = 0          # 0 = auto (min(spp, 32), the last 64 samples tapered); 1 or >= spp = the reference's sequential sum
    march_step: float = 0.1     # ray marching: step (rayMarching3 / rayMarching2, src/rt.cpp:791) or segments
                                # (rayMarchingGlobal / rayMarching)
    march_light: int = 7        # rayMarching3 / rayMarching2: light sphere index (src/rt.cpp:791)

    def params(self) -> _lib.vpt_params:
        p = _lib.vpt_params()
        lib().vpt_default_params(byref(p))
        p.width, p.height, p.spp = self.width, self.height, self.spp
        p.fb_format = FB_F64 if self.fp64 else FB_F32
        p.medium.sigma_a, p.medium.sigma_s = self.sigma_a, self.sigma_s
        p.medium.hg_g, p.medium.max_depth = self.hg_g, self.max_depth
        p.medium.estimator = ESTIMATORS[self.estimator] if isinstance(self.estimator, str) else int(self.estimator)
        p.medium.march_step, p.medium.march_light = self.march_step, self.march_light
        p.seed = self.seed
        p.band_rows = self.band_rows if self.band_rows > 0 else self.height
        p.band_stride, p.band_offset = self.band_stride, self.band_offset
        p.chunk_spp = self.chunk_spp
        return p

    def shard_rows(self) -> int:
        return int(lib().vpt_shard_rows(byref(self.params())))

    def medium(self) -> _lib.vpt_medium:
        return self.params().medium


class Tracer:
    """One GPU context with one scene (replaces the reference's global ``spheres``)."""

    def __init__(self, device: int = 0, spheres: Optional[np.ndarray] = None):
        h = c_void_p()
        check(lib().vpt_context_create(device, byref(h)))
        self._ctx = h
        self.device = device
        self._majorant_block = 0  # the context's setting (vpt_set_grid_majorant_block)
        self._grid_interpolation = "nearest"  # the context's setting (vpt_set_grid_interpolation)
        self._grid_shape = None  # [nz, ny, nx] of the current density grid: what an emission grid has to have
        self.set_scene(default_scene() if spheres is None else spheres)

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            lib().vpt_context_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, spheres: np.ndarray) -> None:
        s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
        check(lib().vpt_set_scene(self._ctx, s.ctypes.data, len(s)))
        self.spheres = s

    # ---- heterogeneous medium (estimator "hetero") ----
    def set_density_grid(self, rho, lo, hi, majorant_block: Optional[int] = None,
                         interpolation: Optional[str] = None, emission=None, emission_rgb=(1, 1, 1)) -> None:
        """The density grid of estimator "hetero": rho of shape [nz, ny, nx] (float32, finite, >= 0) in the world
        box [lo, hi], zero outside; sigma_a / sigma_s are then per unit density.  Kept across set_scene.
        majorant_block: set_majorant_block for this and later grids (None leaves the tracer's setting alone); a
        grid that is rejected leaves the setting as it was.  interpolation: set_grid_interpolation in the same way.
        emission: set_emission_grid(emission, emission_rgb) for this grid; a new density grid always drops the
        previous grid's emission.
        rho and emission may also be torch tensors on the tracer's GPU (a CPU tensor is an array like any other): the
        voxels are then copied device to device, and checked, scanned and built into majorants by kernels
        (vpt_set_density_grid_device), with the same result bit for bit.  The tensor is made float32 and contiguous on
        the device where it is not, the call waits for torch's current stream, and the tensor may be freed or
        overwritten afterwards; a tensor on another device is VPT_E_INVALID."""
        if _on_gpu(rho):
            d = _grid_desc(rho, lo, hi)
            r, stream = _device_voxels(rho, self.device)
            shape = tuple(r.shape)
        else:
            d, r = _grid_args(rho, lo, hi)
            shape = r.shape
        if emission is not None:  # rejected before anything is uploaded
            if _on_gpu(emission):
                _emission_shape_check(emission, shape)
                _emission_colour(emission_rgb)
            else:
                _emission_args(emission, emission_rgb, shape)
        def upload():  # the shape goes with the grid the context holds, whatever the settings after it do
            if _on_gpu(rho):
                check(lib().vpt_set_density_grid_device(self._ctx, byref(d), r.data_ptr(), stream))
            else:
                check(lib().vpt_set_density_grid(self._ctx, byref(d), r.ctypes.data))
            self._grid_shape = shape

        _set_grid_with_block(self, majorant_block, upload, interpolation)
        if emission is not None:
            self.set_emission_grid(emission, emission_rgb)

    def set_emission_grid(self, eps, rgb=(1, 1, 1)) -> None:
        """Volumetric emission for the "hetero" estimators: eps of the density grid's shape (float32, finite, >= 0),
        looked up as the density is, and a colour rgb (finite, >= 0).  The medium emits sigma_a rho(x) eps(x) rgb per
        unit length (Kirchhoff's form: no absorption or no density, no emission), scored on every tentative collision
        of the delta track without a random draw, so paths and draw counts stay what they are.  Needs a density grid
        and goes with it: a new or cleared density grid drops it; the majorant block and the interpolation do not.
        eps may be a torch tensor on the tracer's GPU, as set_density_grid's rho may (vpt_set_emission_grid_device)."""
        if _on_gpu(eps):
            _emission_shape_check(eps, self._grid_shape)
            c = _emission_colour(rgb)
            e, stream = _device_voxels(eps, self.device)
            check(lib().vpt_set_emission_grid_device(self._ctx, e.data_ptr(), c.ctypes.data, stream))
            return
        e, c = _emission_args(eps, rgb, self._grid_shape)
        check(lib().vpt_set_emission_grid(self._ctx, e.ctypes.data, c.ctypes.data))

    def clear_emission_grid(self) -> None:
        check(lib().vpt_set_emission_grid(self._ctx, None, None))

    def set_majorant_block(self, block: int) -> None:
        """Local majorants for delta tracking: super-voxels of `block` voxels per axis, each with its own
        majorant (0, the default: the global majorant only).  Belongs to the tracer: applied to the current grid
        and to every later one.  Fewer null collisions on sparse fields; the same estimator, other draws."""
        check(lib().vpt_set_grid_majorant_block(self._ctx, int(block)))
        self._majorant_block = int(block)

    def set_hetero_mis_fraction(self, q: float) -> None:
        """The track fraction of estimator "hetero_mis": the probability q in [0, 1] (default 0.5) that a distance is
        sampled by delta tracking and not equi-angularly; 0 is estimator "hetero_equiangular" bit for bit.  Belongs to
        the tracer: it survives grid and scene changes.  A value that is refused leaves the setting as it was."""
        check(lib().vpt_set_hetero_mis_fraction(self._ctx, float(q)))

    def set_medium_colour(self, absorption=(1.0, 1.0, 1.0), scattering=(1.0, 1.0, 1.0)) -> None:
        """The medium colour of estimators "hetero_chromatic" and "hetero_spectral": per colour channel the multipliers
        (r, g, b) of the medium's sigma_a and of its sigma_s, each finite and >= 0 (default 1: a grey medium, estimators
        "hetero" and "hetero_ratio" bit for bit).  Belongs to the tracer: it survives grid and scene changes, and no
        other estimator reads it.  A value that is refused leaves the setting as it was; a channel whose absorption and
        scattering are both zero is refused by the render."""
        ca, cs = _colour_args(absorption, scattering)
        check(lib().vpt_set_medium_colour(self._ctx, ca.ctypes.data, cs.ctypes.data))

    def set_grid_interpolation(self, interpolation: str) -> None:
        """How the density is read between the voxel centres: "nearest" (the default: constant per voxel) or
        "trilinear" (a smooth field, clamped at the border of the box; include/vpt.h vpt_set_grid_interpolation).
        Belongs to the tracer: applied to the current grid and to every later one."""
        check(lib().vpt_set_grid_interpolation(self._ctx, _interp_mode(interpolation)))
        self._grid_interpolation = interpolation

    def clear_density_grid(self) -> None:
        check(lib().vpt_set_density_grid(self._ctx, None, None))
        self._grid_shape = None

    def grid_majorants(self):
        """The majorant grid as the kernels read it (vpt_get_grid_majorants), however the density grid was set:
        (maxima[nbz, nby, nbx], minima[nbz, nby, nbx], rho_max), float32 arrays and a float; (None, None, rho_max) with
        majorant block 0.  Needs a density grid."""
        nb = (ctypes.c_int32 * 3)()
        rho_max = ctypes.c_double()
        B = self._majorant_block
        if not B or self._grid_shape is None:
            check(lib().vpt_get_grid_majorants(self._ctx, None, None, 0, nb, byref(rho_max)))
            return None, None, rho_max.value
        shape = tuple((n - 1) // B + 1 for n in self._grid_shape)
        out = np.zeros((2,) + shape, dtype=np.float32)
        check(lib().vpt_get_grid_majorants(self._ctx, out[0].ctypes.data, out[1].ctypes.data, out[0].size, nb,
                                           byref(rho_max)))
        assert (nb[2], nb[1], nb[0]) == shape, (tuple(nb), shape)
        return out[0], out[1], rho_max.value

    def grid_emission_probe(self, sigma_t: float, rays, tmax, states):
        """grid_emission_probe_host's quantities for the tracer's density and emission grids, majorant block and
        interpolation, computed on the GPU (vpt_grid_emission_probe): (t_coll, esum, states, steps)."""
        ry, t, s, tc, es, so = _probe_args(rays, tmax, states)
        steps = np.zeros(len(ry), dtype=np.uint32)
        check(lib().vpt_grid_emission_probe(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry),
                                            tc.ctypes.data, es.ctypes.data, so.ctypes.data, steps.ctypes.data))
        return tc, es, so, steps

    def grid_probe(self, sigma_t: float, rays, tmax, states, return_steps: bool = False):
        """grid_probe_host's quantities for the tracer's grid and its majorant block, computed on the GPU
        (vpt_grid_probe_lm); return_steps appends the tentative steps of each track."""
        ry, t, s, tau, tc, so = _probe_args(rays, tmax, states)
        steps = np.zeros(len(ry), dtype=np.uint32)
        check(lib().vpt_grid_probe_lm(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry),
                                      tau.ctypes.data, tc.ctypes.data, so.ctypes.data, steps.ctypes.data))
        return (tau, tc, so, steps) if return_steps else (tau, tc, so)

    def grid_ratio_probe(self, sigma_t: float, rays, tmax, states):
        """grid_ratio_probe_host's quantities for the tracer's grid and its majorant block, computed on the GPU
        (vpt_grid_ratio_probe)."""
        ry, t, s, that, _, so = _probe_args(rays, tmax, states)
        steps = np.zeros(len(ry), dtype=np.uint32)
        check(lib().vpt_grid_ratio_probe(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry),
                                         that.ctypes.data, so.ctypes.data, steps.ctypes.data))
        return that, so, steps

    def grid_residual_probe(self, sigma_t: float, rays, tmax, states):
        """grid_residual_probe_host's quantities for the tracer's grid, majorant block and interpolation, computed on
        the GPU (vpt_grid_residual_probe): (That, tauc, states, steps)."""
        ry, t, s, that, tauc, so = _probe_args(rays, tmax, states)
        steps = np.zeros(len(ry), dtype=np.uint32)
        check(lib().vpt_grid_residual_probe(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, s.ctypes.data, len(ry),
                                            that.ctypes.data, tauc.ctypes.data, so.ctypes.data, steps.ctypes.data))
        return that, tauc, so, steps

    def grid_eqa_probe(self, sigma_t: float, rays, tmax, light, states):
        """grid_eqa_probe_host's quantities for the tracer's grid and interpolation, computed on the GPU
        (vpt_grid_eqa_probe)."""
        ry, t, lp, s, res, so = _eqa_probe_args(rays, tmax, light, states)
        check(lib().vpt_grid_eqa_probe(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, lp.ctypes.data,
                                       s.ctypes.data, len(ry), *[a.ctypes.data for a in res], so.ctypes.data))
        return (*res, so)

    def grid_mis_probe(self, sigma_t: float, rays, tmax, light, states):
        """grid_mis_probe_host's quantities for the tracer's grid, majorant block, interpolation and track fraction,
        computed on the GPU (vpt_grid_mis_probe)."""
        ry, t, lp, s, _, _ = _eqa_probe_args(rays, tmax, light, states)
        c_order, out = _mis_probe_results(len(ry))
        check(lib().vpt_grid_mis_probe(self._ctx, float(sigma_t), ry.ctypes.data, t.ctypes.data, lp.ctypes.data,
                                       s.ctypes.data, len(ry), *[a.ctypes.data for a in c_order]))
        return out

    def grid_chroma_probe(self, sigma_a: float, sigma_s: float, rays, tmax, states):
        """grid_chroma_probe_host's quantities for the tracer's grid, majorant block, interpolation and medium colour,
        computed on the GPU (vpt_grid_chroma_probe)."""
        ry, t, s, _, _, _ = _probe_args(rays, tmax, states)
        out = _chroma_probe_results(len(ry))
        check(lib().vpt_grid_chroma_probe(self._ctx, float(sigma_a), float(sigma_s), ry.ctypes.data, t.ctypes.data,
                                          s.ctypes.data, len(ry), *[a.ctypes.data for a in out]))
        return out

    def grid_spectral_probe(self, sigma_a: float, sigma_s: float, rays, tmax, states, beta=None):
        """grid_spectral_probe_host's quantities for the tracer's grid, majorant block, interpolation and medium colour,
        computed on the GPU (vpt_grid_spectral_probe)."""
        ry, t, s, _, _, _ = _probe_args(rays, tmax, states)
        b, out = _spectral_probe_args(len(ry), beta)
        check(lib().vpt_grid_spectral_probe(self._ctx, float(sigma_a), float(sigma_s), ry.ctypes.data, t.ctypes.data,
                                            None if b is None else b.ctypes.data, s.ctypes.data, len(ry),
                                            *[a.ctypes.data for a in out]))
        return out

    # ---- main()'s pixel loop (src/rt.cpp:767-805) ----
    def render(self, cfg: Optional[RenderConfig] = None, **kw) -> np.ndarray:
        """Renders on the GPU; returns (shard_rows, width, 3) in file order (row 0 = top), the
        per-pixel average before the clamp of src/rt.cpp:803."""
        cfg = cfg or RenderConfig(**kw)
        p = cfg.params()
        rows = int(lib().vpt_shard_rows(byref(p)))
        out = np.zeros((max(rows, 1), cfg.width, 3), dtype=np.float64 if cfg.fp64 else np.float32)
        check(lib().vpt_render(self._ctx, byref(p), out.ctypes.data))  # validates even an empty shard
        return out[:rows]

    def render_device(self, cfg: RenderConfig, out_ptr: int, stream: int = 0) -> None:
        """Enqueues a render into a device buffer (e.g. torch tensor .data_ptr()) on `stream`."""
        p = cfg.params()
        check(lib().vpt_render_device(self._ctx, byref(p), c_void_p(out_ptr), c_void_p(stream)))

    def accumulator(self, cfg: RenderConfig, chunk: Optional[int] = None) -> "Accumulator":
        """A progressive accumulator for cfg's image or shard (vpt_accum_*): cfg.spp is the cap, a multiple of
        the chunk (`chunk`, else cfg.chunk_spp, else min(32, spp)).  The scene must stay as it is while the
        accumulator holds samples."""
        return Accumulator(self, cfg, chunk)

    def grid_accumulator(self, cfg: RenderConfig, chunk: Optional[int] = None) -> "Accumulator":
        """A progressive accumulator for the density-grid estimators ("hetero" to "hetero_spectral", 10-16), which
        `accumulator` refuses (vpt_accum_create_grid): the same class with the second of its two contracts.  cfg.spp is
        the cap, a multiple of the chunk (`chunk`, else cfg.chunk_spp, else min(32, spp)); tile subsets work for every
        one of these estimators.  Every pass validates as a render does: once the grid is cleared, or a setting makes
        the estimator invalid, ``add`` and ``refine`` raise the render's error and change nothing.  The scene, the grid
        and its settings (majorant block, interpolation, emission, medium colour, track fraction) must stay as they are
        while the accumulator holds samples."""
        return Accumulator(self, cfg, chunk, grid=True)

    def count_work(self, cfg: RenderConfig) -> tuple[int, int]:
        """(ray-sphere tests, estimator iterations) of the reference algorithm for this render."""
        t, i = c_uint64(), c_uint64()
        check(lib().vpt_count_work(self._ctx, byref(cfg.params()), byref(t), byref(i)))
        return int(t.value), int(i.value)

    # ---- the per-sample estimators, batched ----
    def trace(self, estimator, rays: np.ndarray, states: np.ndarray, sigma_a=0.001, sigma_s=0.009, hg_g=0.0,
              max_depth=0, march_step=0.1, march_light=7) -> tuple[np.ndarray, np.ndarray]:
        m = _lib.vpt_medium(sigma_a, sigma_s, hg_g, max_depth,
                            ESTIMATORS[estimator] if isinstance(estimator, str) else int(estimator), march_step,
                            march_light)
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        s = np.ascontiguousarray(states, dtype=np.uint64)
        if len(r) != len(s):
            raise ValueError("rays and states must have the same length")
        out = np.zeros((len(r), 3), dtype=np.float64)
        st = np.zeros(len(r), dtype=np.uint64)
        check(lib().vpt_trace_batch(self._ctx, byref(m), r.ctypes.data, s.ctypes.data, len(r), out.ctypes.data,
                                    st.ctypes.data))
        return out, st

    def iterativeVPTracerFree(self, rays, states, sigma_a=0.001, sigma_s=0.009, **kw):
        """Batched include/vptShadeMethods.h:1263."""
        return self.trace("ff", rays, states, sigma_a, sigma_s, **kw)

    def MISVPTTracerRecursive(self, rays, states, sigma_a=0.001, sigma_s=0.009, **kw):
        """Batched include/vptShadeMethods.h:1345 (depth 0)."""
        return self.trace("mis", rays, states, sigma_a, sigma_s, **kw)

    def explicitVPTracerRecursiveFree(self, rays, states, sigma_a=0.001, sigma_s=0.009, **kw):
        """Batched include/vptShadeMethods.h:1153 (depth 0)."""
        return self.trace("explicit_free", rays, states, sigma_a, sigma_s, **kw)

    def implicitVPTracerRecursiveFree(self, rays, states, sigma_a=0.001, sigma_s=0.009, **kw):
        """Batched include/vptShadeMethods.h:940."""
        return self.trace("implicit_free", rays, states, sigma_a, sigma_s, **kw)

    def explicitVPTracerRecursive(self, rays, states, sigma_a=0.001, sigma_s=0.009, **kw):
        """Batched include/vptShadeMethods.h:1014 (depth 0)."""
        return self.trace("explicit", rays, states, sigma_a, sigma_s, **kw)

    def iterativePathTracer(self, rays, states):
        """Batched include/shadeMethods.h:104 (surface only: no medium arguments)."""
        return self.trace("surface_pt", rays, states)

    def rayMarching3(self, rays, states, sigma_a, sigma_s, step, idsource):
        """Batched include/rayMarchingMethods.h:330 (src/rt.cpp:791 passes 0.001, 0.0125, 0.1, 7)."""
        return self.trace("ray_marching", rays, states, sigma_a, sigma_s, march_step=step, march_light=idsource)

    def rayMarching2(self, rays, states, sigma_a, sigma_s, step, idsource):
        """Batched include/rayMarchingMethods.h:262."""
        return self.trace("ray_marching_sa", rays, states, sigma_a, sigma_s, march_step=step, march_light=idsource)

    def rayMarchingGlobal(self, rays, states, sigma_a, sigma_s, segmentos):
        """Batched include/rayMarchingMethods.h:106 (samples the hard-coded sphere 5)."""
        return self.trace("ray_marching_global", rays, states, sigma_a, sigma_s, march_step=segmentos)

    def rayMarching(self, rays, states, sigma_t, sigma_s, steps, x_new=None, idsource=None):
        """Batched include/rayMarchingMethods.h:34 with its reference parameters: returns
        (Color, x_new, idsource, end states); x_new / idsource are kept on a miss (inputs default
        to 0 / -1)."""
        r = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        s = np.ascontiguousarray(states, dtype=np.uint64)
        if len(r) != len(s):
            raise ValueError("rays and states must have the same length")
        xn = np.zeros((len(r), 3))
        if x_new is not None:
            xn[:] = x_new
        ids = np.full(len(r), -1, dtype=np.int32)
        if idsource is not None:
            ids[:] = idsource
        out = np.zeros((len(r), 3))
        st = np.zeros(len(r), dtype=np.uint64)
        check(lib().vpt_ray_marching_batch(self._ctx, float(sigma_t), float(sigma_s), float(steps), r.ctypes.data,
                                           s.ctypes.data, len(r), out.ctypes.data, xn.ctypes.data, ids.ctypes.data,
                                           st.ctypes.data))
        return out, xn, ids, st

    def punctualVolumetric(self, idsource: int, x: np.ndarray, phase: float, sigma_t: float, sigma_s: float) -> np.ndarray:
        """include/rayMarchingMethods.h:12 at every point of x (n x 3) -> (n x 3) Colors."""
        xs = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        out = np.zeros_like(xs)
        check(lib().vpt_punctual_volumetric(self._ctx, int(idsource), xs.ctypes.data, len(xs), float(phase),
                                            float(sigma_t), float(sigma_s), out.ctypes.data))
        return out

    def math_probe(self, fn: int, x: np.ndarray, y: Optional[np.ndarray] = None) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float64)
        out = np.zeros_like(x)
        check(lib().vpt_math_probe(self._ctx, fn, x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x)))
        return out

    def hg_phase(self, g: float, din, states: np.ndarray, wl: np.ndarray):
        """HG phase extension on the GPU (vpt_phase_probe): (directions sampled around din, end states,
        phase values toward the rows of wl)."""
        d = np.ascontiguousarray(din, dtype=np.float64)
        s = np.ascontiguousarray(states, dtype=np.uint64)
        w = np.ascontiguousarray(wl, dtype=np.float64).reshape(-1, 3)
        dirs = np.zeros((len(s), 3))
        so = np.zeros(len(s), dtype=np.uint64)
        vals = np.zeros(len(w))
        check(lib().vpt_phase_probe(self._ctx, float(g), d.ctypes.data, s.ctypes.data, len(s), dirs.ctypes.data,
                                    so.ctypes.data, w.ctypes.data, len(w), vals.ctypes.data))
        return dirs, so, vals


class Accumulator:
    """A render that can be continued (vpt_accum_*, include/vpt.h).  Samples arrive in chunk levels of
    `chunk` samples, for all 8x8 tiles or for chosen ones.  Tiles are numbered row-major over the shard,
    ``tiles_x`` per row.  Two contracts, by the constructor:

    ``Tracer.accumulator`` (estimators 0-5, the chunked sum): a pixel that holds m levels equals, bit for bit, the
    pixel of ``Tracer.render(spp=m * chunk, chunk_spp=chunk)``; its sum is the sum of the levels' chunk sums.

    ``Tracer.grid_accumulator`` (estimators 10-16, the in-order sum): a pixel that holds m levels equals, bit for
    bit, the pixel of ``Tracer.render(spp=m * chunk)`` -- its sum is ``acc = L + acc`` over its first m * chunk
    samples in order, so `chunk` does not change the image; it is the granularity of a level and of the error
    statistic (s1, s2 are folded from the levels' chunk sums as in the first contract)."""

    def __init__(self, tracer: Tracer, cfg: RenderConfig, chunk: Optional[int] = None, grid: bool = False):
        p = cfg.params()
        if chunk is not None:
            p.chunk_spp = int(chunk)
        h = c_void_p()
        create = lib().vpt_accum_create_grid if grid else lib().vpt_accum_create
        check(create(tracer._ctx, byref(p), byref(h)))
        self._a = h
        self._tracer = tracer  # the context must outlive the accumulator
        tx, ty, c, ml = c_int(), c_int(), c_int(), c_int()
        check(lib().vpt_accum_tiles(self._a, byref(tx), byref(ty), byref(c), byref(ml)))
        self.tiles_x, self.tiles_y, self.chunk, self.max_levels = tx.value, ty.value, c.value, ml.value
        self.width = cfg.width
        self.rows = int(lib().vpt_shard_rows(byref(p)))

    @property
    def tiles(self) -> int:
        return self.tiles_x * self.tiles_y

    def close(self) -> None:
        if getattr(self, "_a", None):
            lib().vpt_accum_destroy(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, levels: int = 1, tiles: Optional[Sequence[int]] = None) -> None:
        """`levels` more chunk levels for all tiles or the listed ones (any order, no duplicates)."""
        if tiles is None:
            check(lib().vpt_accum_add(self._a, int(levels), None, 0))
        else:
            t = np.ascontiguousarray(tiles, dtype=np.int32)
            check(lib().vpt_accum_add(self._a, int(levels), t.ctypes.data, len(t)))

    def refine(self, target: float, lum_floor: float = 0.01, min_levels: int = 4, levels_per_pass: int = 1) -> dict:
        """Adds levels to the tiles whose error is above `target` until none is left or capped."""
        r = _lib.vpt_refine(float(target), float(lum_floor), int(min_levels), int(levels_per_pass))
        rep = _lib.vpt_refine_report()
        check(lib().vpt_accum_refine(self._a, byref(r), byref(rep)))
        return {"passes": rep.passes, "tiles_converged": rep.tiles_converged, "tiles_capped": rep.tiles_capped,
                "samples": int(rep.samples), "max_err": rep.max_err}

    def image(self, fp64: bool = False) -> np.ndarray:
        """(rows, width, 3) in file order: the average of the samples each pixel holds (0 where none)."""
        out = np.zeros((self.rows, self.width, 3), dtype=np.float64 if fp64 else np.float32)
        check(lib().vpt_accum_resolve(self._a, FB_F64 if fp64 else FB_F32, out.ctypes.data))
        return out

    def resolve_device(self, ptr: int, stream: int = 0, fp64: bool = False) -> None:
        """Enqueues the resolve into a device buffer on `stream`; synchronise it before reading."""
        check(lib().vpt_accum_resolve_device(self._a, FB_F64 if fp64 else FB_F32, c_void_p(ptr), c_void_p(stream)))

    def state(self) -> dict:
        """The arrays of vpt_accum_read: sum (rows, w, 3), s1 and s2 (rows, w), tile_levels, tile_err (tiles)."""
        s = np.zeros((self.rows, self.width, 3))
        s12 = np.zeros((self.rows, self.width, 2))
        lv = np.zeros(self.tiles, dtype=np.int32)
        er = np.zeros(self.tiles)
        check(lib().vpt_accum_read(self._a, s.ctypes.data, s12.ctypes.data, lv.ctypes.data, er.ctypes.data))
        return {"sum": s, "s1": np.ascontiguousarray(s12[..., 0]), "s2": np.ascontiguousarray(s12[..., 1]),
                "tile_levels": lv, "tile_err": er}

    def _to_pixels(self, per_tile: np.ndarray) -> np.ndarray:
        g = per_tile.reshape(self.tiles_y, self.tiles_x)
        return np.repeat(np.repeat(g, 8, axis=0), 8, axis=1)[:self.rows, :self.width]

    def spp_map(self) -> np.ndarray:
        """(rows, width) samples each pixel holds."""
        return self._to_pixels(self.state()["tile_levels"].astype(np.int64) * self.chunk)

    def error_map(self) -> np.ndarray:
        """(rows, width) the tiles' errors, broadcast to their pixels."""
        return self._to_pixels(self.state()["tile_err"])


class MultiTracer:
    """Devices 0 .. n_gpus-1 of THIS process rendering one image together (vpt_multi_*, include/vpt.h):
    interleaved row bands per device, strips gathered to device 0 over RCCL.  Bit-identical to
    Tracer.render for any n_gpus."""

    def __init__(self, n_gpus: int, spheres: Optional[np.ndarray] = None, shared_device: bool = False):
        """shared_device (tests): n_gpus logical ranks on device 0, their strips copied on the device
        instead of sent over RCCL (vpt_debug_multi_create_shared) -- the n > 1 path on a one-GPU box"""
        h = c_void_p()
        if shared_device:
            f = lib().vpt_debug_multi_create_shared
            f.restype, f.argtypes = c_int, [c_int, POINTER(c_void_p)]
            check(f(n_gpus, byref(h)))
        else:
            check(lib().vpt_multi_create(n_gpus, byref(h)))
        self._m = h
        self.n_gpus = n_gpus
        self._majorant_block = 0
        self._grid_interpolation = "nearest"
        self._grid_shape = None
        s = np.ascontiguousarray(default_scene() if spheres is None else spheres, dtype=SPHERE_DTYPE)
        check(lib().vpt_multi_set_scene(self._m, s.ctypes.data, len(s)))
        self.spheres = s

    def set_density_grid(self, rho, lo, hi, majorant_block: Optional[int] = None,
                         interpolation: Optional[str] = None, emission=None, emission_rgb=(1, 1, 1)) -> None:
        """Tracer.set_density_grid on every rank's context (arrays only: a GPU tensor is VPT_E_UNSUPPORTED)."""
        _refuse_gpu_tensor(rho, emission)
        d, r = _grid_args(rho, lo, hi)
        if emission is not None:
            _emission_args(emission, emission_rgb, r.shape)
        def upload():
            self._grid_shape = None  # a failure part of the way leaves contexts with and without the new grid
            check(lib().vpt_multi_set_density_grid(self._m, byref(d), r.ctypes.data))
            self._grid_shape = r.shape

        _set_grid_with_block(self, majorant_block, upload, interpolation)
        if emission is not None:
            self.set_emission_grid(emission, emission_rgb)

    def set_emission_grid(self, eps, rgb=(1, 1, 1)) -> None:
        """Tracer.set_emission_grid on every rank's context (arrays only, as set_density_grid)."""
        _refuse_gpu_tensor(eps)
        e, c = _emission_args(eps, rgb, self._grid_shape)
        check(lib().vpt_multi_set_emission_grid(self._m, e.ctypes.data, c.ctypes.data))

    def clear_emission_grid(self) -> None:
        check(lib().vpt_multi_set_emission_grid(self._m, None, None))

    def set_hetero_mis_fraction(self, q: float) -> None:
        """Tracer.set_hetero_mis_fraction on every rank's context."""
        check(lib().vpt_multi_set_hetero_mis_fraction(self._m, float(q)))

    def set_medium_colour(self, absorption=(1.0, 1.0, 1.0), scattering=(1.0, 1.0, 1.0)) -> None:
        """Tracer.set_medium_colour on every rank's context."""
        ca, cs = _colour_args(absorption, scattering)
        check(lib().vpt_multi_set_medium_colour(self._m, ca.ctypes.data, cs.ctypes.data))

    def set_majorant_block(self, block: int) -> None:
        """Tracer.set_majorant_block on every rank's context."""
        check(lib().vpt_multi_set_grid_majorant_block(self._m, int(block)))
        self._majorant_block = int(block)

    def set_grid_interpolation(self, interpolation: str) -> None:
        """Tracer.set_grid_interpolation on every rank's context."""
        check(lib().vpt_multi_set_grid_interpolation(self._m, _interp_mode(interpolation)))
        self._grid_interpolation = interpolation

    def clear_density_grid(self) -> None:
        check(lib().vpt_multi_set_density_grid(self._m, None, None))
        self._grid_shape = None

    def render(self, cfg: Optional[RenderConfig] = None, **kw) -> np.ndarray:
        """(height, width, 3), file order; cfg.band_rows (when it cuts the image) is the band size."""
        cfg = cfg or RenderConfig(**kw)
        p = cfg.params()
        out = np.zeros((cfg.height, cfg.width, 3), dtype=np.float64 if cfg.fp64 else np.float32)
        check(lib().vpt_multi_render(self._m, byref(p), out.ctypes.data))
        return out

    def close(self) -> None:
        if getattr(self, "_m", None):
            lib().vpt_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_multi(n_gpus: int, cfg: Optional[RenderConfig] = None, spheres: Optional[np.ndarray] = None,
                 **kw) -> np.ndarray:
    """One-shot vpt_render_multi: the image of `cfg` on devices 0 .. n_gpus-1."""
    cfg = cfg or RenderConfig(**kw)
    s = np.ascontiguousarray(default_scene() if spheres is None else spheres, dtype=SPHERE_DTYPE)
    p = cfg.params()
    out = np.zeros((cfg.height, cfg.width, 3), dtype=np.float64 if cfg.fp64 else np.float32)
    check(lib().vpt_render_multi(s.ctypes.data, len(s), byref(p), n_gpus, out.ctypes.data))
    return out


# ---- output (src/rt.cpp:812-820) ----
def _fb(rgb: np.ndarray) -> tuple[np.ndarray, int, int, int]:
    a = np.ascontiguousarray(rgb)
    if a.dtype == np.float32:
        fmt = FB_F32
    elif a.dtype == np.float64:
        fmt = FB_F64
    else:
        a, fmt = np.ascontiguousarray(a, dtype=np.float64), FB_F64
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("framebuffer must be (height, width, 3)")
    return a, fmt, a.shape[1], a.shape[0]


def encode_ppm(rgb: np.ndarray) -> bytes:
    a, fmt, w, h = _fb(rgb)
    n = lib().vpt_encode_ppm(a.ctypes.data, fmt, w, h, None, 0)
    if n < 0:
        check(int(n))
    buf = ctypes.create_string_buffer(int(n))
    m = lib().vpt_encode_ppm(a.ctypes.data, fmt, w, h, buf, n)
    if m != n:
        check(int(m) if m < 0 else _lib.VPT_E_INVALID)
    return buf.raw


def write_ppm(path: str, rgb: np.ndarray) -> None:
    a, fmt, w, h = _fb(rgb)
    check(lib().vpt_write_ppm(path.encode(), a.ctypes.data, fmt, w, h))
