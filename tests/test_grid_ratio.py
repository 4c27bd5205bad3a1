"""Ratio tracking on the CPU (vpt_grid_ratio_probe_host: csrc/vpt_grid.h's vpt_grid_ratio and vpt_grid_ratio_lm
compiled for the host): the global-majorant walker against a plain-Python restatement bit for bit, the reduction
of one super-voxel to the global walker, the {0, 1} estimate at block size 1 against the delta track from the same
states, unbiasedness against the deterministic optical depth, and the argument errors.  No GPU."""
import ctypes

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import ratio_model as rm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_probe_host, grid_ratio_probe_host, lib

SIGMA_T = mm.SIGMA_T


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_global_walker_equals_the_python_model():
    """256 rays through the sparse field: value, draws and end state bit for bit"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI, n=256)
    st = gm.states(11, len(rays))
    that, so, steps = grid_ratio_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st)
    want, wso, wsteps = rm.ratio_global_rays(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st)
    assert (_bits(that) == _bits(want)).all(), f"{(_bits(that) != _bits(want)).sum()} estimates differ"
    assert (so == wso).all() and (steps == wsteps).all()
    # the set exercises every exit: an exact zero, a product of several weights, the empty product
    assert (that == 0).sum() >= 1 and ((that > 0) & (that < 1)).sum() > 50 and (that == 1).sum() > 10
    assert steps.max() > 3 and (steps >= 1).all()
    # the first tentative point is the delta track's: in a thin medium, where the track ends as "none" on its first
    # step (one draw), the estimate is the empty product after the same single draw
    thin = 0.05
    _, tc, tso, tsteps = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, thin, rays, tmax, st, return_steps=True)
    that, so, steps = grid_ratio_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, thin, rays, tmax, st)
    first = (tsteps == 1) & (tc == -1)
    assert first.sum() > 5 and (that[first] == 1).all() and (tso[first] == so[first]).all() and (steps[first] == 1).all()


@pytest.mark.parametrize("block", [0, 1, 2, 8])
def test_no_medium_no_draw(block):
    """a zero-density grid and rays that miss the box: That == 1.0, the start state, no step"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI, n=64)
    st = gm.states(5, len(rays))
    that, so, steps = grid_ratio_probe_host(np.zeros_like(rho), mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st,
                                            majorant_block=block)
    assert (_bits(that) == _bits(np.ones(len(rays)))).all() and (so == st).all() and (steps == 0).all()
    miss = np.zeros(3, dtype=gm.RAY_DTYPE)
    miss["o"] = [(10, 10, 10), (-5, 3, 0), (2, 3, 20)]
    miss["d"] = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    that, so, steps = grid_ratio_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, miss, 1e30, st[:3], majorant_block=block)
    assert (_bits(that) == _bits(np.ones(3))).all() and (so == st[:3]).all() and (steps == 0).all()


def _reduction_sets():
    """the tau and KS ray sets of tests/test_grid_host.py"""
    rho = gm.tau_grid()
    rays, tmax = gm.tau_rays()
    for sigma_t in (0.7, 0.05):
        yield rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, gm.states(3, len(rays))
    rays, tmax = gm.ks_rays()
    yield gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, gm.states(gm.KS_SEED, gm.KS_N)


def test_one_super_voxel_is_the_global_walker():
    """property (i): block >= max(n) equals block 0 bit for bit -- value, draws and end state"""
    partial = 0
    for rho, lo, hi, sigma_t, rays, tmax, st in _reduction_sets():
        that0, so0, steps0 = grid_ratio_probe_host(rho, lo, hi, sigma_t, rays, tmax, st)
        assert (steps0[so0 != st] >= 1).all() and (steps0[so0 == st] == 0).all()
        partial += int(((that0 > 0) & (that0 < 1)).sum())
        for b in (max(rho.shape), max(rho.shape) + 3):
            that, so, steps = grid_ratio_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, majorant_block=b)
            assert (_bits(that) == _bits(that0)).all(), f"block {b}: {(_bits(that) != _bits(that0)).sum()} estimates differ"
            assert (so == so0).all(), f"block {b}: {(so != so0).sum()} end states differ"
            assert (steps == steps0).all(), f"block {b}: {(steps != steps0).sum()} step counts differ"
    assert partial > 1000


def test_block_1_is_the_delta_track():
    """property (ii): at block 1 the majorant is the voxel's own density: one draw, That is 1 where the delta track
    (block 1) from the same state ends as "none" and +0 where it collides, and the end states are equal"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    that, so, steps = grid_ratio_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st, majorant_block=1)
    _, tc, tso, _ = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st, majorant_block=1,
                                    return_steps=True)
    none = tc < 0
    assert not np.isnan(tc).any() and none.sum() > 200 and (~none).sum() > 1000
    assert (_bits(that[none]) == _bits(np.ones(int(none.sum())))).all()
    assert (_bits(that[~none]) == 0).all()  # +0.0
    assert (so == tso).all()
    assert (steps == 1).all()  # every ray of the set has a slab interval


@pytest.mark.parametrize("block", [0, 2, 1])
def test_unbiased(block):
    """one oblique ray through rho = (1, 3), 65 536 states: That lies in [0, 1] with mean T = exp(-sigma_t tau), so its
    variance is at most T (1 - T) and the mean of N estimates is within 4.5 sqrt(T (1 - T) / N) of T (4.5 standard
    deviations: 7e-6 two-sided).  Block 1 (estimates in {0, 1}, the variance bound attained) is checked as well."""
    n, sigma_t = gm.KS_N, 0.5
    rays = mm.same_ray((-0.3, 0.2, 0.1), (2.5, 0.6, 0.75), n)
    st = gm.states(gm.KS_SEED, n)
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays[:1], 1e30, st[:1])[0][0]
    T = np.exp(-sigma_t * tau)
    assert 2.0 < tau < 6.0  # the ray crosses both voxels
    that, _, steps = grid_ratio_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays, 1e30, st, majorant_block=block)
    assert ((that >= 0) & (that <= 1)).all()
    bound = 4.5 * np.sqrt(T * (1 - T) / n)
    print(f"block {block}: mean(That) = {that.mean():.6f}, T = {T:.6f}, |diff| = {abs(that.mean() - T):.2e}, bound {bound:.2e}, "
          f"draws per ray {steps.mean():.2f}")
    assert abs(that.mean() - T) <= bound
    if block != 1:
        assert ((that > 0) & (that < 1)).sum() > 1000  # weights, not only a collision test


def _status(nx, ny, nz, lo, hi, density, block):
    d = _lib.vpt_grid_desc()
    d.nx, d.ny, d.nz = nx, ny, nz
    d.lo[:] = lo
    d.hi[:] = hi
    rays, tmax = gm.ks_rays(1)
    st = gm.states(1, 1)
    out = np.zeros(1)
    so = np.zeros(1, np.uint64)
    steps = np.zeros(1, np.uint32)
    dens = None if density is None else np.ascontiguousarray(density, dtype=np.float32)
    return lib().vpt_grid_ratio_probe_host(ctypes.byref(d), None if dens is None else dens.ctypes.data, block, 1.0,
                                           rays.ctypes.data, tmax.ctypes.data, st.ctypes.data, 1, out.ctypes.data,
                                           so.ctypes.data, steps.ctypes.data)


def test_argument_errors():
    ones = np.ones(8, np.float32)
    assert _status(2, 2, 2, [0.0] * 3, [1.0] * 3, ones, 0) == _lib.VPT_OK
    assert _status(2, 2, 2, [0.0] * 3, [1.0] * 3, ones, 2) == _lib.VPT_OK
    assert _status(2, 2, 2, [0.0] * 3, [1.0] * 3, ones, -1) == _lib.VPT_E_INVALID
    assert lib().vpt_last_error()
    bad = ones.copy()
    bad[3] = np.nan
    for args in ((0, 2, 2, [0.0] * 3, [1.0] * 3, ones), (2, 2, 2, [0.0] * 3, [1.0, 0.0, 1.0], ones),
                 (2, 2, 2, [0.0] * 3, [1.0] * 3, bad), (2, 2, 2, [0.0] * 3, [1.0] * 3, None)):
        assert _status(*args, 0) == _lib.VPT_E_INVALID
        assert _status(*args, 2) == _lib.VPT_E_INVALID
    rays, tmax = gm.ks_rays(1)
    with pytest.raises(VPTError) as ei:
        grid_ratio_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, gm.states(1, 1), majorant_block=-1)
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_ratio_probe_host(np.full((1, 1, 1), -1.0), (0, 0, 0), (1, 1, 1), 1.0, rays, 1.0, gm.states(1, 1))
    assert ei.value.code == _lib.VPT_E_INVALID
