"""TEST INFRASTRUCTURE ONLY -- ctypes access to the parity oracle (oracle/README in DESIGN.md).

Loaders for
  * liboracle.so      C restatement, libm transcendentals  (pinned to the reference itself),
  * liboracle_vm.so   the same restatement with the build's portable FP64 math (= the kernel's arithmetic),
  * _ref/libvpt_ref.so  the reference's own functions compiled in place (only where /root/reference was
                        available at build time; the built .so travels with the repo).
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_double, c_int, c_int32, c_uint64, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SPHERE_BYTES = 144


class Medium(ctypes.Structure):
    _fields_ = [("sigma_a", c_double), ("sigma_s", c_double), ("hg_g", c_double), ("max_depth", c_int32),
                ("estimator", c_int32), ("march_step", c_double), ("march_light", c_int32), ("reserved_", c_int32)]


class Counters(ctypes.Structure):
    _fields_ = [("tests", c_uint64), ("iterations", c_uint64), ("surface", c_uint64), ("medium", c_uint64)]


_P = c_void_p
_U = c_uint64
_D = c_double
_I = c_int

_PRIMS = {
    # name: (restype, argtypes) -- identical for orc_* and ref_*
    "sphere_intersect": (_D, [_I, _P]),
    "intersect": (_I, [_P, _P, _P]),
    "visibility": (_I, [_P, _P]),
    "transmitance": (_D, [_P, _P, _D]),
    "coordinate_system": (None, [_P, _P, _P]),
    "solid_angle_dir": (_U, [_P, _D, _U, _P]),
    "cosine_hemispheric": (_U, [_P, _U, _P]),
    "isotropic_phase": (_U, [_U, _P]),
    "vector_facet": (_U, [_D, _U, _P]),
    "fresnel": (None, [_D, _P, _P, _P]),
    "fr_microfacet": (None, [_P, _P, _P, _P, _P, _D, _P, _P]),
    "microfacet_prob": (_D, [_P, _P, _D, _P]),
    "bdsf": (_U, [_P, _P, _I, _U, _P, _P, _P]),
    "plight": (None, [_I, _P, _P, _P, _P, _P, _D, _P]),
    "misv2": (_U, [_I, _P, _P, _P, _D, _D, _U, _P]),
    "free_single_scattering": (_U, [_P, _I, _D, _D, _U, _P]),
    "single_scattering": (_U, [_P, _I, _D, _D, _D, _D, _U, _P]),
    "equiangular_params2": (_U, [_I, _D, _P, _P, _U]),
    "equiangular_prob": (_D, [_D, _D, _D, _D]),
    "camera_ray": (_U, [_I, _I, _I, _I, _U, _P]),
    "to_display": (_I, [_D]),
    "punctual_volumetric": (None, [_I, _P, _D, _D, _D, _P]),
    "ray_marching_explicit": (_U, [_P, _D, _D, _D, _U, _P, _P, _P]),
}


def _bind(L: ctypes.CDLL, prefix: str) -> ctypes.CDLL:
    for name, (res, args) in _PRIMS.items():
        fn = getattr(L, f"{prefix}_{name}")
        fn.restype, fn.argtypes = res, args
    return L


def default_chunk(spp: int) -> int:
    """samples per chunk the GPU uses when vpt_params.chunk_spp == 0 (vpt_auto_chunk, csrc/vpt_chunks.h)"""
    return min(spp, max(32, -(-spp // 128)))


class Oracle:
    """liboracle.so (portable=False) or liboracle_vm.so (portable=True)."""

    def __init__(self, portable: bool = False):
        path = os.path.join(HERE, "liboracle_vm.so" if portable else "liboracle.so")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not built (make -C oracle oracle)")
        L = ctypes.CDLL(path)
        _bind(L, "orc")
        L.orc_set_scene.restype, L.orc_set_scene.argtypes = _I, [_P, _I]
        L.orc_trace.restype = _U
        L.orc_trace.argtypes = [_P, _U, POINTER(Medium), _P, POINTER(Counters)]
        L.orc_render.restype = None
        L.orc_render.argtypes = [_I, _I, _I, POINTER(Medium), _U, _I, _I, _P, _I, POINTER(Counters)]
        L.orc_render_chunked.restype = None
        L.orc_render_chunked.argtypes = [_I, _I, _I, _I, POINTER(Medium), _U, _I, _I, _P, _I, POINTER(Counters)]
        L.orc_render_layout.restype = None
        L.orc_render_layout.argtypes = [_I, _I, _I, _I, _I, POINTER(Medium), _U, _I, _I, _P, _I, POINTER(Counters)]
        L.orc_write_ppm.restype, L.orc_write_ppm.argtypes = _I, [ctypes.c_char_p, _P, _I, _I]
        L.orc_stream_state_c.restype, L.orc_stream_state_c.argtypes = _U, [_U, _U, _U]
        L.orc_is_portable_math.restype = _I
        L.orc_math_n.restype, L.orc_math_n.argtypes = None, [_I, _P, _P, _P, _I]
        L.orc_hg_phase_sample.restype, L.orc_hg_phase_sample.argtypes = _U, [_D, _P, _U, _P]
        L.orc_hg_phase_value.restype, L.orc_hg_phase_value.argtypes = _D, [_D, _P, _P]
        # the heterogeneous medium (oracle/vpt_oracle_grid.h): estimators 10 - 16
        L.orc_set_density_grid.restype, L.orc_set_density_grid.argtypes = _I, [_P, _I, _I, _I, _P, _P, _I, _I]
        L.orc_clear_density_grid.restype, L.orc_clear_density_grid.argtypes = None, []
        L.orc_set_emission_grid.restype, L.orc_set_emission_grid.argtypes = _I, [_P, _P]
        L.orc_clear_emission_grid.restype, L.orc_clear_emission_grid.argtypes = None, []
        L.orc_hetero_set_fault.restype, L.orc_hetero_set_fault.argtypes = None, [_I]
        L.orc_grid_probe.restype, L.orc_grid_probe.argtypes = _I, [_D, _P, _P, _P, _I, _P, _P, _P, _P]
        L.orc_grid_ratio_probe.restype, L.orc_grid_ratio_probe.argtypes = _I, [_D, _P, _P, _P, _I, _P, _P, _P]
        L.orc_grid_emission_probe.restype, L.orc_grid_emission_probe.argtypes = _I, [_D, _P, _P, _P, _I, _P, _P, _P, _P]
        # estimators 12, 13 and 14: their settings, what the library would answer, their decisions
        L.orc_set_hetero_mis_fraction.restype, L.orc_set_hetero_mis_fraction.argtypes = _I, [_D]
        L.orc_set_medium_colour.restype, L.orc_set_medium_colour.argtypes = _I, [_P, _P]
        L.orc_estimator_status.restype, L.orc_estimator_status.argtypes = _I, [POINTER(Medium)]
        L.orc_ext_counters.restype, L.orc_ext_counters.argtypes = None, [_P, _I]
        L.orc_ext_counters_15_16.restype, L.orc_ext_counters_15_16.argtypes = None, [_P, _I]
        L.orc_grid_eqa_probe.restype, L.orc_grid_eqa_probe.argtypes = _I, [_D, _P, _P, _P, _P, _I] + [_P] * 6
        L.orc_grid_mis_probe.restype, L.orc_grid_mis_probe.argtypes = _I, [_D, _D, _P, _P, _P, _P, _I] + [_P] * 9
        L.orc_grid_chroma_probe.restype, L.orc_grid_chroma_probe.argtypes = _I, [_P, _P, _P, _P, _P, _I] + [_P] * 6
        # estimators 15 and 16: the residual walk, the two spectral walkers
        L.orc_grid_residual_probe.restype, L.orc_grid_residual_probe.argtypes = _I, [_D, _P, _P, _P, _I] + [_P] * 4
        L.orc_grid_spectral_probe.restype, L.orc_grid_spectral_probe.argtypes = _I, [_P, _P, _P, _P, _P, _P, _I] + [_P] * 7
        self.L = L
        self.portable = bool(L.orc_is_portable_math())
        self.prefix = "orc"

    def set_scene(self, spheres: np.ndarray) -> None:
        b = np.ascontiguousarray(spheres).view(np.uint8)
        n = len(b) // SPHERE_BYTES
        if self.L.orc_set_scene(b.ctypes.data, n) != 0:
            raise ValueError("oracle: bad scene")

    def hg_phase(self, g: float, din, states: np.ndarray, wl: np.ndarray):
        """HG extension (phase_sample / phase_value): directions sampled around din from each erand48
        state, the end states, and the phase values toward the rows of wl."""
        d = np.ascontiguousarray(din, dtype=np.float64)
        w = np.ascontiguousarray(wl, dtype=np.float64).reshape(-1, 3)
        n = len(states)
        out = np.zeros((n, 3))
        st = np.zeros(n, dtype=np.uint64)
        pv = np.zeros(len(w))
        for i in range(n):
            st[i] = self.L.orc_hg_phase_sample(g, d.ctypes.data, int(states[i]), out[i].ctypes.data)
        for i in range(len(w)):
            pv[i] = self.L.orc_hg_phase_value(g, d.ctypes.data, w[i].ctypes.data)
        return out, st, pv

    # ---- the heterogeneous medium.  The grid, the emission grid, the fault, the track fraction and the medium colour
    # are state of the library, which the session's fixtures share: whoever sets one resets it in a `finally`
    # (clear_density_grid, set_hetero_fault(0), set_hetero_mis_fraction(0.5), set_medium_colour()).
    INTERPOLATIONS = {"nearest": 0, "trilinear": 1}

    def set_density_grid(self, rho, lo, hi, majorant_block: int = 0, interpolation: str = "nearest", emission=None,
                         emission_rgb=(1, 1, 1)) -> None:
        """rho: [nz, ny, nx] (x fastest) in the box [lo, hi]; the arguments of Tracer.set_density_grid, but the block
        and the mode do not persist: every call states them.  A new grid drops the emission grid."""
        r = np.ascontiguousarray(rho, dtype=np.float32)
        if r.ndim != 3:
            raise ValueError("rho must have shape [nz, ny, nx]")
        a, b = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        nz, ny, nx = r.shape
        if self.L.orc_set_density_grid(r.ctypes.data, nx, ny, nz, a.ctypes.data, b.ctypes.data, int(majorant_block),
                                       self.INTERPOLATIONS[interpolation]) != 0:
            raise ValueError("oracle: bad density grid")
        self._grid_shape = r.shape
        if emission is not None:
            self.set_emission_grid(emission, emission_rgb)

    def set_emission_grid(self, eps, rgb=(1, 1, 1)) -> None:
        e = np.ascontiguousarray(eps, dtype=np.float32)
        c = np.ascontiguousarray(rgb, dtype=np.float64)
        if e.shape != getattr(self, "_grid_shape", None) or c.shape != (3,):
            raise ValueError("oracle: the emission grid has the density grid's shape and three colour values")
        if self.L.orc_set_emission_grid(e.ctypes.data, c.ctypes.data) != 0:
            raise ValueError("oracle: bad emission grid, or no density grid")

    def clear_emission_grid(self) -> None:
        self.L.orc_clear_emission_grid()

    def clear_density_grid(self) -> None:
        self.L.orc_clear_density_grid()
        self._grid_shape = None

    def set_hetero_fault(self, kind: int) -> None:
        """test only: the mistake the heterogeneous tracers commit on purpose (0: none; oracle/vpt_oracle.c)"""
        self.L.orc_hetero_set_fault(int(kind))

    def set_hetero_mis_fraction(self, q: float) -> None:
        """Tracer.set_hetero_mis_fraction: estimator 13's track fraction in [0, 1] (default 0.5); state of the library"""
        if self.L.orc_set_hetero_mis_fraction(float(q)) != 0:
            raise ValueError("oracle: the track fraction is a number in [0, 1]")

    def set_medium_colour(self, absorption=(1.0, 1.0, 1.0), scattering=(1.0, 1.0, 1.0)) -> None:
        """Tracer.set_medium_colour: estimator 14's multipliers of sigma_a and sigma_s per channel (default 1); state
        of the library"""
        ca, cs = (np.ascontiguousarray(v, dtype=np.float64) for v in (absorption, scattering))
        if ca.shape != (3,) or cs.shape != (3,) or self.L.orc_set_medium_colour(ca.ctypes.data, cs.ctypes.data) != 0:
            raise ValueError("oracle: a medium colour is two triples of finite numbers >= 0")

    def ext_counters(self, reset: bool = True) -> dict:
        """test only: what the trace calls since the last reset did in estimators 12 - 16 -- medium vertices by the
        strategy that sampled them, estimator 14's decisions by hero channel, its collisions whose three weights differ;
        estimator 15's residual walks that ended as "none" with tauc > 0 and a product of weights other than 1, and those
        that passed a block with a control and no residual (mn > 0, mr == 0); estimator 16's decisions whose three W differ
        (at a collision, on a surface), its ratio walks that went on past a rho >= mu point, its track's real collisions
        taken without a draw, and its collisions that entered with three different beta"""
        c, c2 = np.zeros(6, dtype=np.uint64), np.zeros(7, dtype=np.uint64)  # ORC_EXT_COUNTERS, ORC_EXT_COUNTERS_15_16
        self.L.orc_ext_counters(c.ctypes.data, int(reset))
        self.L.orc_ext_counters_15_16(c2.ctypes.data, int(reset))
        c = [int(v) for v in c] + [int(v) for v in c2]
        return {"equiangular": c[0], "track": c[1], "hero": tuple(c[2:5]), "w_differ": c[5], "residual_both": c[6],
                "residual_flat_block": c[7], "W_differ_collision": c[8], "W_differ_surface": c[9], "ratio_went_on": c[10],
                "no_draw_collision": c[11], "beta_differ_collision": c[12]}

    def _check_estimator(self, m: Medium) -> None:
        """what the library refuses, the oracle refuses: VPT_E_INVALID (-1), VPT_E_UNSUPPORTED (-4)"""
        rc = self.L.orc_estimator_status(byref(m))
        if rc == -4 or (rc != 0 and m.estimator >= 12):
            raise ValueError(f"oracle: estimator {m.estimator} is refused in this state (library code {rc})")

    @staticmethod
    def _probe_args(rays, tmax, states):
        r = np.ascontiguousarray(rays)
        if r.dtype.itemsize != 48 and r.dtype != np.float64:
            raise ValueError("rays: records of (o, d), 6 doubles each")
        n = r.size if r.dtype.itemsize == 48 else r.size // 6
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,)))
        s = np.ascontiguousarray(states, dtype=np.uint64)
        if len(s) != n:
            raise ValueError("rays and states must have the same length")
        return r, t, s, n

    def grid_probe(self, rho, lo, hi, sigma_t, rays, tmax, states, majorant_block=0, return_steps=False,
                   interpolation="nearest"):
        """grid_probe_host's arguments and results: (tau, t_coll, states[, steps]).  Sets the grid and clears it."""
        r, t, s, n = self._probe_args(rays, tmax, states)
        tau, tc, so, steps = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_probe(float(sigma_t), r.ctypes.data, t.ctypes.data, s.ctypes.data, n, tau.ctypes.data,
                                       tc.ctypes.data, so.ctypes.data, steps.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return (tau, tc, so, steps) if return_steps else (tau, tc, so)

    def grid_ratio_probe(self, rho, lo, hi, sigma_t, rays, tmax, states, majorant_block=0, interpolation="nearest"):
        """grid_ratio_probe_host's arguments and results: (That, states, steps)"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        that, so, steps = np.zeros(n), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_ratio_probe(float(sigma_t), r.ctypes.data, t.ctypes.data, s.ctypes.data, n,
                                             that.ctypes.data, so.ctypes.data, steps.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return that, so, steps

    def grid_emission_probe(self, rho, eps, lo, hi, sigma_t, rays, tmax, states, majorant_block=0,
                            interpolation="nearest"):
        """grid_emission_probe_host's arguments and results: (t_coll, esum, states, steps)"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        tc, es, so, steps = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation, emission=eps)
        try:
            rc = self.L.orc_grid_emission_probe(float(sigma_t), r.ctypes.data, t.ctypes.data, s.ctypes.data, n,
                                                tc.ctypes.data, es.ctypes.data, so.ctypes.data, steps.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return tc, es, so, steps

    def grid_eqa_probe(self, rho, lo, hi, sigma_t, rays, tmax, light, states, interpolation="nearest"):
        """grid_eqa_probe_host's arguments and results: (psurf, dist, pdf, T, rho_t, states)"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(light, dtype=np.float64), (n, 3)))
        res, so = [np.zeros(n) for _ in range(5)], np.zeros(n, dtype=np.uint64)
        self.set_density_grid(rho, lo, hi, 0, interpolation)
        try:
            rc = self.L.orc_grid_eqa_probe(float(sigma_t), r.ctypes.data, t.ctypes.data, lp.ctypes.data, s.ctypes.data, n,
                                           *[a.ctypes.data for a in res], so.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return (*res, so)

    def grid_mis_probe(self, rho, lo, hi, sigma_t, rays, tmax, light, states, q=0.5, majorant_block=0,
                       interpolation="nearest"):
        """grid_mis_probe_host's arguments and results: (psurf, strategy, dist, pdf, pe, T, rho_t, steps, states)"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        lp = np.ascontiguousarray(np.broadcast_to(np.asarray(light, dtype=np.float64), (n, 3)))
        f = [np.zeros(n) for _ in range(6)]  # psurf, dist, pdf, pe, T, rho_t
        strategy, steps, so = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_mis_probe(float(sigma_t), float(q), r.ctypes.data, t.ctypes.data, lp.ctypes.data,
                                           s.ctypes.data, n, f[0].ctypes.data, strategy.ctypes.data,
                                           *[a.ctypes.data for a in f[1:]], steps.ctypes.data, so.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return f[0], strategy, f[1], f[2], f[3], f[4], f[5], steps, so

    def grid_chroma_probe(self, rho, lo, hi, sigma_a, sigma_s, rays, tmax, states, absorption=(1.0, 1.0, 1.0),
                          scattering=(1.0, 1.0, 1.0), majorant_block=0, interpolation="nearest"):
        """grid_chroma_probe_host's arguments and results: (hero, t_coll, tau, w, steps, states), w of shape (3, n)"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        sa = float(sigma_a) * np.ascontiguousarray(absorption, dtype=np.float64)
        ss = float(sigma_s) * np.ascontiguousarray(scattering, dtype=np.float64)
        hero, tc, tau, w = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n), np.zeros((3, n))
        steps, so = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_chroma_probe(sa.ctypes.data, ss.ctypes.data, r.ctypes.data, t.ctypes.data, s.ctypes.data, n,
                                              hero.ctypes.data, tc.ctypes.data, tau.ctypes.data, w.ctypes.data,
                                              steps.ctypes.data, so.ctypes.data)
        finally:
            self.clear_density_grid()
        assert rc == 0
        return hero, tc, tau, w, steps, so

    def grid_residual_probe(self, rho, lo, hi, sigma_t, rays, tmax, states, majorant_block=0, interpolation="nearest"):
        """grid_residual_probe_host's arguments and results: (That, tauc, states, steps); majorant_block >= 1"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        that, tauc, so, steps = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_residual_probe(float(sigma_t), r.ctypes.data, t.ctypes.data, s.ctypes.data, n,
                                                that.ctypes.data, tauc.ctypes.data, so.ctypes.data, steps.ctypes.data)
        finally:
            self.clear_density_grid()
        if rc != 0:
            raise ValueError("oracle: the residual walk needs a majorant block >= 1")
        return that, tauc, so, steps

    def grid_spectral_probe(self, rho, lo, hi, sigma_a, sigma_s, rays, tmax, states, absorption=(1.0, 1.0, 1.0),
                            scattering=(1.0, 1.0, 1.0), majorant_block=0, interpolation="nearest", beta=None):
        """grid_spectral_probe_host's arguments and results: (t_coll, w, steps, states, T, ratio_steps, ratio_states), w
        and T of shape (3, n); beta: three numbers or (n, 3), default ones"""
        r, t, s, n = self._probe_args(rays, tmax, states)
        sa = float(sigma_a) * np.ascontiguousarray(absorption, dtype=np.float64)
        ss = float(sigma_s) * np.ascontiguousarray(scattering, dtype=np.float64)
        b = None if beta is None else np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (n, 3)))
        out = (np.zeros(n), np.zeros((3, n)), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros((3, n)),
               np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64))
        self.set_density_grid(rho, lo, hi, majorant_block, interpolation)
        try:
            rc = self.L.orc_grid_spectral_probe(sa.ctypes.data, ss.ctypes.data, r.ctypes.data, t.ctypes.data,
                                                None if b is None else b.ctypes.data, s.ctypes.data, n,
                                                *[a.ctypes.data for a in out])
        finally:
            self.clear_density_grid()
        if rc != 0:
            raise ValueError("oracle: a channel without extinction")
        return out

    def trace(self, estimator: int, rays: np.ndarray, states: np.ndarray, sigma_a=0.001, sigma_s=0.009, hg_g=0.0,
              max_depth=0, counters: bool = False, march_step=0.1, march_light=7):
        """per-sample radiance and end state of include/vpt.h's estimator number (0-16; 10 and 11 need a density
        grid: without one the radiance is NaN and the state is the start state; 12-16 raise ValueError where the
        library refuses them: without a grid, with an emission grid, 14 and 16 with a channel without extinction, 15
        without a majorant block)"""
        m = Medium(sigma_a, sigma_s, hg_g, max_depth, estimator, march_step, march_light)
        self._check_estimator(m)
        if getattr(rays, "dtype", None) is not None and rays.dtype.names:  # records of (o, d), as Tracer.trace takes them
            rays = np.ascontiguousarray(rays).view(np.float64)
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros((len(r), 3))
        st = np.zeros(len(r), dtype=np.uint64)
        tot = [0, 0, 0, 0]
        c = Counters()
        for i in range(len(r)):
            st[i] = self.L.orc_trace(r[i].ctypes.data, int(states[i]), byref(m), out[i].ctypes.data,
                                     byref(c) if counters else None)
            if counters:
                tot = [tot[0] + c.tests, tot[1] + c.iterations, tot[2] + c.surface, tot[3] + c.medium]
        return (out, st, tot) if counters else (out, st)

    def render(self, w, h, spp, estimator=0, sigma_a=0.001, sigma_s=0.009, hg_g=0.0, max_depth=0, seed=0x5EED0001,
               y0=0, y1=None, threads=0, counters=False, chunk=None, march_step=0.1, march_light=7):
        """main()'s pixel loop over camera rows [y0, y1); returns (h, w, 3) float64 in file order.
        chunk: samples per partial sum in uniform chunks (spp = the reference's order); None = the
        GPU's default (vpt_params.chunk_spp == 0): for estimators 0-5 chunks of min(spp, 32), the last 64
        samples tapered (csrc/vpt_chunks.h); for estimators 6-16, whose kernels ignore chunk_spp (include/vpt.h),
        the reference's order."""
        m = Medium(sigma_a, sigma_s, hg_g, max_depth, estimator, march_step, march_light)
        self._check_estimator(m)
        out = np.zeros((h, w, 3))
        c = Counters()
        taper = 0
        if (chunk is None or chunk == 0) and estimator >= 6:
            chunk = spp
        elif chunk is None or chunk == 0:
            chunk, taper = default_chunk(spp), 1
        self.L.orc_render_layout(w, h, spp, chunk, taper, byref(m), seed, y0, h if y1 is None else y1,
                                 out.ctypes.data, threads, byref(c))
        return (out, c) if counters else out

    def math(self, fn: int, x: np.ndarray, y=None) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(np.zeros_like(x) if y is None else y, dtype=np.float64)
        out = np.zeros_like(x)
        self.L.orc_math_n(fn, x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x))
        return out

    def stream_state(self, seed, idx, sample) -> int:
        return int(self.L.orc_stream_state_c(seed, idx, sample))

    def camera_ray(self, w, h, x, y, state):
        r = np.zeros(6)
        s = self.L.orc_camera_ray(w, h, x, y, state, r.ctypes.data)
        return r, int(s)

    def write_ppm(self, path: str, lin: np.ndarray) -> None:
        a = np.ascontiguousarray(lin, dtype=np.float64)
        if self.L.orc_write_ppm(path.encode(), a.ctypes.data, a.shape[1], a.shape[0]) != 0:
            raise OSError(path)

    def prim(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")


class Reference:
    """oracle/_ref/libvpt_ref.so: the reference's own functions (ref_harness.cpp)."""

    PATH = os.path.join(HERE, "_ref", "libvpt_ref.so")

    def __init__(self):
        if not os.path.exists(self.PATH):
            raise FileNotFoundError(self.PATH)
        L = ctypes.CDLL(self.PATH)
        _bind(L, "ref")
        L.ref_default_scene.restype, L.ref_default_scene.argtypes = _I, [_P, _I]
        L.ref_set_scene.restype, L.ref_set_scene.argtypes = None, [_P, _I]
        L.ref_trace.restype, L.ref_trace.argtypes = _U, [_I, _P, _U, _D, _D, _P]
        L.ref_render.restype = None
        L.ref_render.argtypes = [_I, _I, _I, _I, _D, _D, _U, _I, _I, _P, _P]
        L.ref_sizeof_sphere.restype = _I
        L.ref_set_march.restype, L.ref_set_march.argtypes = None, [_D, _I]
        self.L = L
        self.prefix = "ref"

    @staticmethod
    def available() -> bool:
        return os.path.exists(Reference.PATH)

    def default_scene(self) -> np.ndarray:
        n = self.L.ref_default_scene(None, 0)
        b = np.zeros(n * SPHERE_BYTES, dtype=np.uint8)
        self.L.ref_default_scene(b.ctypes.data, n)
        return b

    def set_scene(self, spheres: np.ndarray) -> None:
        b = np.ascontiguousarray(spheres).view(np.uint8)
        self.L.ref_set_scene(b.ctypes.data, len(b) // SPHERE_BYTES)

    def trace(self, estimator, rays, states, sigma_a=0.001, sigma_s=0.009, march_step=0.1, march_light=7):
        self.L.ref_set_march(march_step, march_light)
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        out = np.zeros((len(r), 3))
        st = np.zeros(len(r), dtype=np.uint64)
        for i in range(len(r)):
            st[i] = self.L.ref_trace(estimator, r[i].ctypes.data, int(states[i]), sigma_a, sigma_s, out[i].ctypes.data)
        return out, st

    def render(self, w, h, spp, estimator=0, sigma_a=0.001, sigma_s=0.009, seed=0x5EED0001, y0=0, y1=None,
               per_sample=False, march_step=0.1, march_light=7):
        self.L.ref_set_march(march_step, march_light)
        out = np.zeros((h, w, 3))
        ps = np.zeros((h * w * spp, 3)) if per_sample else None
        self.L.ref_render(w, h, spp, estimator, sigma_a, sigma_s, seed, y0, h if y1 is None else y1, out.ctypes.data,
                          ps.ctypes.data if per_sample else None)
        return (out, ps) if per_sample else out

    def prim(self, name):
        return getattr(self.L, f"{self.prefix}_{name}")
