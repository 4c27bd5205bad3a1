"""Residual ratio tracking on the CPU (vpt_grid_residual_probe_host: csrc/vpt_grid.h's vpt_grid_residual_lm_m and the
two control builders compiled for the host): the walker against a plain-Python restatement bit for bit, the reduction
to estimator 11's walker where the control grid is zero, the exact, one-draw estimate where every super-voxel is
uniform, the reduction of one super-voxel, unbiasedness and the variance against ratio tracking, and the argument
errors.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import residual_model as rs
from minimal_volumetric_path_tracer_amd import (VPTError, _lib, grid_probe_host, grid_ratio_probe_host,
                                                grid_residual_probe_host, lib)

LO, HI = mm.SPARSE_LO, mm.SPARSE_HI


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _tc(sigma_t, tauc):
    """exp(sigma_t * tauc * -1.0) with libm's exp, the walker's own (numpy's may differ by an ulp)"""
    return np.array([math.exp(sigma_t * v * -1.0) for v in tauc])


def _same(got, want, what):
    for name, g, w in zip(("That", "tauc", "states", "steps"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        diff = _bits(g) != _bits(w) if g.dtype == np.float64 else g != w
        assert not diff.any(), f"{what}: {int(diff.sum())} {name} differ"


def test_walker_equals_the_python_model():
    """256 rays through the sparse field with and without a density floor, B = 1, 2 and 8, two sigma_t, nearest, and
    trilinear at B = 2: That, tauc, end state and draws bit for bit; the set exercises every exit"""
    rays, tmax = mm.box_rays(LO, HI, n=256)
    st = gm.states(11, len(rays))
    seen = dict(zero=0, product=0, analytic=0, nodraw=0)
    cases = [(b, "nearest") for b in (1, 2, 8)] + [(2, "trilinear")]
    for rho in (mm.sparse_field() + np.float32(0.5), mm.sparse_field()):
        for b, interp in cases:
            for sigma_t in (0.7, 0.05):
                got = grid_residual_probe_host(rho, LO, HI, sigma_t, rays, tmax, st, majorant_block=b, interpolation=interp)
                want = rs.residual_rays(rho, LO, HI, sigma_t, rays, tmax, st, b, interp)
                _same(got, want, f"block {b}, {interp}, sigma_t {sigma_t}")
                that, tauc, so, steps = got
                tc = _tc(sigma_t, tauc)
                assert ((that >= 0) & (that <= tc)).all()
                seen["zero"] += int((_bits(that) == 0).sum())
                seen["product"] += int(((that > 0) & (that < tc) & (steps > 2)).sum())
                seen["analytic"] += int(((_bits(that) == _bits(tc)) & (steps == 1) & (tauc > 0)).sum())
                seen["nodraw"] += int(((that == 1) & (steps == 0) & (so == st)).sum())
    print(seen)
    assert seen["zero"] >= 1 and seen["product"] > 50 and seen["analytic"] > 50
    # rays that miss the box: 1.0, no draw, tauc == +0
    miss = np.zeros(3, dtype=gm.RAY_DTYPE)
    miss["o"] = [(10, 10, 10), (-5, 3, 0), (2, 3, 20)]
    miss["d"] = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for rho in (mm.sparse_field(), np.zeros(mm.SPARSE_SHAPE, np.float32)):
        got = grid_residual_probe_host(rho, LO, HI, 0.7, miss, 1e30, st[:3], majorant_block=2)
        _same(got, rs.residual_rays(rho, LO, HI, 0.7, miss, 1e30, st[:3], 2), "no-draw")
        that, tauc, so, steps = got
        assert (_bits(that) == _bits(np.ones(3))).all() and (_bits(tauc) == 0).all() and (so == st[:3]).all() and (steps == 0).all()
        seen["nodraw"] += 3
    assert seen["nodraw"] >= 6


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_zero_control_is_ratio_tracking(interp):
    """identity (i): every block of B = 2 holds a zero voxel (under the dilation too), so the control grid is zero and
    the walker is vpt_grid_ratio_lm_m bit for bit -- value, end state, draws -- on 4096 rays; tauc == 0"""
    f = mm.sparse_field()
    f[::2, ::2, ::2] = 0
    assert (rs.control(f, 2, interp) == 0).all() and (rs.majorants(f, 2, interp) > 0).any()
    rays, tmax = mm.box_rays(LO, HI)
    st = gm.states(11, len(rays))
    for sigma_t in (0.7, 0.05):
        that, tauc, so, steps = grid_residual_probe_host(f, LO, HI, sigma_t, rays, tmax, st, majorant_block=2, interpolation=interp)
        want, wso, wsteps = grid_ratio_probe_host(f, LO, HI, sigma_t, rays, tmax, st, majorant_block=2, interpolation=interp)
        assert (_bits(that) == _bits(want)).all(), f"{(_bits(that) != _bits(want)).sum()} estimates differ"
        assert (so == wso).all() and (steps == wsteps).all()
        assert (tauc == 0).all()
        assert ((that > 0) & (that < 1)).sum() > 100  # products of weights, not only the exits 0 and 1


def test_uniform_blocks_are_exact():
    """identity (ii): a block-constant field at B = 2 (every super-voxel uniform): one draw per ray with a slab interval
    and That = exp(-sigma_t tau) within 1e-12 relative (the order of the sum alone differs: sigma_t tau (pieces + 2)
    2^-53 is below 1e-13 here); the same on a uniform grid at B = 1, 2 and >= max(n).  Estimator 11's walker differs on
    the same rays: under the global majorant it takes several draws and returns products on more than 1000 of them, and
    at B = 2, where each majorant is its block's own density, it is the collision test -- one draw, an estimate in {0, 1}
    with zeros on more than 1000 rays and ones on more than 100 -- where this walker is exact"""
    coarse = np.random.default_rng(3).permutation(12).reshape(3, 2, 2).astype(np.float32) * np.float32(0.25) + np.float32(0.3)
    assert len(np.unique(coarse)) == 12 and coarse.min() > 0
    f = mm.resample2(coarse)
    rays, tmax = mm.box_rays(LO, HI)
    st = gm.states(11, len(rays))
    sigma_t = mm.SIGMA_T
    tau = grid_probe_host(f, LO, HI, sigma_t, rays, tmax, st)[0]
    that, tauc, so, steps = grid_residual_probe_host(f, LO, HI, sigma_t, rays, tmax, st, majorant_block=2)
    assert (steps == 1).all()  # every ray of the set has a slab interval
    T = np.exp(-sigma_t * tau)
    rel = np.abs(that - T) / T
    print(f"block-constant field: max relative difference {rel.max():.2e}, max |tauc - tau| / tau {np.abs(tauc - tau).max():.2e}")
    assert (rel <= 1e-12).all()
    assert (_bits(that) == _bits(_tc(sigma_t, tauc))).all()
    r11, _, s11 = grid_ratio_probe_host(f, LO, HI, sigma_t, rays, tmax, st)
    assert ((s11 > 1) & (r11 > 0) & (r11 < 1)).sum() > 1000
    r11, _, s11 = grid_ratio_probe_host(f, LO, HI, sigma_t, rays, tmax, st, majorant_block=2)
    assert (s11 == 1).all() and (r11 == 0).sum() > 1000 and (r11 == 1).sum() > 100 and ((r11 == 0) | (r11 == 1)).all()
    u = np.full(mm.SPARSE_SHAPE, 1.7, np.float32)
    tau = grid_probe_host(u, LO, HI, sigma_t, rays, tmax, st)[0]
    T = np.exp(-sigma_t * tau)
    for b in (1, 2, max(u.shape)):
        for interp in ("nearest", "trilinear"):
            that, _, _, steps = grid_residual_probe_host(u, LO, HI, sigma_t, rays, tmax, st, majorant_block=b, interpolation=interp)
            assert (steps == 1).all() and (np.abs(that - T) <= 1e-12 * T).all(), (b, interp)


def test_one_super_voxel():
    """B = max(n) and max(n) + 3 are the same single block: bit for bit"""
    rays, tmax = mm.box_rays(LO, HI)
    st = gm.states(11, len(rays))
    for rho in (mm.sparse_field() + np.float32(0.5), mm.sparse_field()):
        for interp in ("nearest", "trilinear"):
            a = grid_residual_probe_host(rho, LO, HI, 0.7, rays, tmax, st, majorant_block=max(rho.shape), interpolation=interp)
            b = grid_residual_probe_host(rho, LO, HI, 0.7, rays, tmax, st, majorant_block=max(rho.shape) + 3, interpolation=interp)
            _same(a, b, interp)
            assert ((a[0] > 0) & (a[0] < 1)).sum() > 1000


def test_unbiased():
    """tests/test_grid_ratio.py's oblique ray through rho = (1, 3) at sigma_t = 0.5, 65 536 states, B = 2: one block with
    mn = 1, mu = 3.  The estimate lies in [0, Tc], Tc = exp(-sigma_t tauc) <= 1, with mean T, so its variance is at most
    T (1 - T) and the mean of N estimates is within 4.5 sqrt(T (1 - T) / N) of T, as for ratio tracking.  The sample
    variance is below ratio tracking's on the same states.  At B = 1 every estimate is exact."""
    n, sigma_t = gm.KS_N, 0.5
    rays = mm.same_ray((-0.3, 0.2, 0.1), (2.5, 0.6, 0.75), n)
    st = gm.states(gm.KS_SEED, n)
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays[:1], 1e30, st[:1])[0][0]
    T = np.exp(-sigma_t * tau)
    assert 2.0 < tau < 6.0  # the ray crosses both voxels
    assert rs.control(gm.KS_RHO, 2).tolist() == [[[1.0]]] and rs.majorants(gm.KS_RHO, 2).tolist() == [[[3.0]]]
    that, tauc, _, steps = grid_residual_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays, 1e30, st, majorant_block=2)
    assert ((that >= 0) & (that <= _tc(sigma_t, tauc))).all()
    bound = 4.5 * np.sqrt(T * (1 - T) / n)
    r11, _, s11 = grid_ratio_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays, 1e30, st, majorant_block=2)
    print(f"mean(That) = {that.mean():.6f}, T = {T:.6f}, |diff| = {abs(that.mean() - T):.2e}, bound {bound:.2e}; variance "
          f"{that.var():.5f} (ratio tracking {r11.var():.5f}); draws per ray {steps.mean():.2f} (ratio tracking {s11.mean():.2f})")
    assert abs(that.mean() - T) <= bound
    assert that.var() < r11.var()
    assert ((that > 0) & (that < 1)).sum() > 1000
    exact, _, _, s1 = grid_residual_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays, 1e30, st, majorant_block=1)
    assert (np.abs(exact - T) <= 1e-12 * T).all() and (s1 == 1).all()


def _status(nx, ny, nz, lo, hi, density, block, interp=0):
    d = _lib.vpt_grid_desc()
    d.nx, d.ny, d.nz = nx, ny, nz
    d.lo[:] = lo
    d.hi[:] = hi
    rays, tmax = gm.ks_rays(1)
    st = gm.states(1, 1)
    out, tc = np.zeros(1), np.zeros(1)
    so = np.zeros(1, np.uint64)
    steps = np.zeros(1, np.uint32)
    dens = None if density is None else np.ascontiguousarray(density, dtype=np.float32)
    return lib().vpt_grid_residual_probe_host(ctypes.byref(d), None if dens is None else dens.ctypes.data, block, interp, 1.0,
                                              rays.ctypes.data, tmax.ctypes.data, st.ctypes.data, 1, out.ctypes.data,
                                              tc.ctypes.data, so.ctypes.data, steps.ctypes.data)


def test_argument_errors():
    ones = np.ones(8, np.float32)
    box = ([0.0] * 3, [1.0] * 3)
    assert _status(2, 2, 2, *box, ones, 1) == _lib.VPT_OK
    assert _status(2, 2, 2, *box, ones, 2, 1) == _lib.VPT_OK
    for block in (0, -1):
        assert _status(2, 2, 2, *box, ones, block) == _lib.VPT_E_INVALID
        assert lib().vpt_last_error()
    assert _status(2, 2, 2, *box, ones, 2, 2) == _lib.VPT_E_INVALID  # a bad mode
    bad = ones.copy()
    bad[3] = np.nan
    for args in ((0, 2, 2, [0.0] * 3, [1.0] * 3, ones), (2, 2, 2, [0.0] * 3, [1.0, 0.0, 1.0], ones),
                 (2, 2, 2, *box, bad), (2, 2, 2, *box, None)):
        assert _status(*args, 2) == _lib.VPT_E_INVALID
    rays, tmax = gm.ks_rays(1)
    for kw in (dict(majorant_block=0), dict(), dict(majorant_block=-1), dict(majorant_block=2, interpolation="cubic")):
        with pytest.raises(VPTError) as ei:
            grid_residual_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, gm.states(1, 1), **kw)
        assert ei.value.code == _lib.VPT_E_INVALID
