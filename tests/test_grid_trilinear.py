"""Trilinear density interpolation on the CPU (vpt_grid_probe_host_ex, vpt_grid_ratio_probe_host_ex: csrc/vpt_grid.h
compiled for the host): the optical depth against an independent numpy model (tests/trilinear_model.py) and closed
forms, the reduction to the nearest lookup on uniform fields, an affine field at two resolutions, the distribution of
the track, the dilated local majorants, unbiasedness of ratio tracking, and the argument errors.  No GPU."""
import ctypes

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import trilinear_model as tm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_probe_host, grid_ratio_probe_host, lib

SIGMA_T = 0.7
TL = dict(interpolation="trilinear")
CRIT = 1.95 / np.sqrt(gm.KS_N)  # test_delta_tracking_distribution's: alpha = 0.001, 0.00762


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


_CACHE = {}


def _tau_set():
    """the tau grid and rays of tests/test_grid_host.py with the trilinear optical depth of the code under test and
    of the model, computed once"""
    if "tau" not in _CACHE:
        rho = gm.tau_grid()
        rays, tmax = gm.tau_rays()
        st = gm.states(3, len(rays))
        tau = grid_probe_host(rho, gm.TAU_LO, gm.TAU_HI, SIGMA_T, rays, tmax, st, **TL)[0]
        want = np.array([tm.tau_model(rho, gm.TAU_LO, gm.TAU_HI, rays["o"][i], rays["d"][i], tmax[i]) for i in range(len(rays))])
        for a in (tau, want, tmax):
            a.setflags(write=False)
        _CACHE["tau"] = (rho, rays, tmax, st, tau, want)
    return _CACHE["tau"]


def test_optical_depth_matches_the_numpy_model():
    rho, rays, tmax, st, tau, want = _tau_set()
    bound = 1e-10 * float(rho.max()) * tmax  # tests/test_grid_host.py's own
    err = np.abs(tau - want)
    print(f"max |tau - model| = {err.max():.3e}, largest error / bound = {np.max(err[tmax > 0] / bound[tmax > 0]):.3e}")
    assert (err <= bound).all(), f"{(err > bound).sum()} segments off, worst {err.max():.3e}"
    assert (want == 0).sum() > 50 and (want > 0).sum() > 1000
    # the ray set tells the two fields apart
    nearest = np.array([gm.tau_model(rho, gm.TAU_LO, gm.TAU_HI, rays["o"][i], rays["d"][i], tmax[i]) for i in range(len(rays))])
    assert (np.abs(tau - nearest) > bound).sum() > 1000


def test_closed_forms():
    """rho = (1, 2, 3, 4) on [0, 4] x [0, 1]^2: along x the field is 1 up to 0.5, then linear through (1.5, 2), (2.5, 3)"""
    rho = np.array([[[1.0, 2.0, 3.0, 4.0]]], dtype=np.float32)
    lo, hi = (0.0, 0.0, 0.0), (4.0, 1.0, 1.0)
    rays = np.zeros(4, dtype=gm.RAY_DTYPE)
    rays["o"] = [(0.5, 0.5, 0.5), (2.0, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 2.0, 0.5)]
    rays["d"] = [(1, 0, 0), (-1, 0, 0), (1, 0, 0), (1, 0, 0)]
    tmax = np.array([1.5, 1.5, 0.0, 1.5])
    st = gm.states(2, 4)
    tau, tc, so = grid_probe_host(rho, lo, hi, SIGMA_T, rays, tmax, st, **TL)
    ulp = np.spacing(2.625)
    print(f"tau = {tau[0]!r}, {tau[1]!r} (2.625); off by {abs(tau[0] - 2.625) / ulp:.1f}, {abs(tau[1] - 2.625) / ulp:.1f} ulp")
    assert abs(tau[0] - 2.625) <= 4 * ulp and abs(tau[1] - 2.625) <= 4 * ulp
    assert grid_probe_host(rho, lo, hi, SIGMA_T, rays[:1], tmax[:1], st[:1])[0][0] == 2.5  # nearest
    assert tau[2] == 0 and not np.signbit(tau[2])
    assert tau[3] == 0 and not np.signbit(tau[3]) and tc[3] == -1 and so[3] == st[3]  # a miss: no draw
    that, rso, steps = grid_ratio_probe_host(rho, lo, hi, SIGMA_T, rays[3:], tmax[3:], st[3:], **TL)
    assert that[0] == 1.0 and rso[0] == st[3] and steps[0] == 0


@pytest.mark.parametrize("shape", [gm.TAU_SHAPE, (1, 1, 1)])
def test_uniform_field_is_the_nearest_lookup(shape):
    """a + f * (b - a) is a exactly when a == b: rho == 0.7f gives nearest's tracks and estimates bit for bit"""
    rho = np.full(shape, 0.7, dtype=np.float32)
    rays, tmax = gm.tau_rays()
    st = gm.states(3, len(rays))
    args = (rho, gm.TAU_LO, gm.TAU_HI, SIGMA_T, rays, tmax, st)
    collided = 0
    for block in (0, 2, 8):
        near = grid_probe_host(*args, majorant_block=block, return_steps=True)
        tri = grid_probe_host(*args, majorant_block=block, return_steps=True, **TL)
        assert (_bits(tri[1]) == _bits(near[1])).all() and (tri[2] == near[2]).all() and (tri[3] == near[3]).all(), f"block {block}"
        collided += int((near[1] >= 0).sum())
        bound = 1e-10 * 0.7 * tmax
        assert (np.abs(tri[0] - near[0]) <= bound).all()
        near = grid_ratio_probe_host(*args, majorant_block=block)
        tri = grid_ratio_probe_host(*args, majorant_block=block, **TL)
        assert (_bits(tri[0]) == _bits(near[0])).all() and (tri[1] == near[1]).all() and (tri[2] == near[2]).all(), f"block {block}"
    assert collided > 1000


def test_affine_field_at_two_resolutions():
    """rho = 1 + 0.3 x' + 0.5 y' + 0.7 z' (box-normalised) sampled at the voxel centres of a 3 x 4 x 5 and a 6 x 5 x 7
    grid: trilinear interpolation reproduces an affine function, so on segments inside the hull of the coarser grid's
    centres both optical depths are the analytic integral, length x rho(midpoint).  A swapped axis or stride moves tau
    by tenths.  The voxels are float32: what is stored is the affine function plus a rounding residual of relative
    size 2^-25, about two hundred times the bound (measured: 181 and 196 times).  Both the lookup and the integral are linear in the voxel values, so the
    stored field's optical depth is the analytic integral plus the optical depth of the residual field, which the numpy
    model supplies (a term of 1e-7 tau, known to 1e-12 of itself); the bound is test 1's, unchanged."""
    lo, hi = np.array(gm.TAU_LO), np.array(gm.TAU_HI)
    ext = hi - lo
    coef = np.array([0.3, 0.5, 0.7])

    def affine(p):
        return 1.0 + ((p - lo) / ext) @ coef

    rng = np.random.default_rng(44)
    n = 500
    hull_lo, hull_hi = lo + 0.5 * ext / np.array([3, 4, 5]), hi - 0.5 * ext / np.array([3, 4, 5])
    a = hull_lo + rng.uniform(0, 1, (n, 3)) * (hull_hi - hull_lo)
    b = hull_lo + rng.uniform(0, 1, (n, 3)) * (hull_hi - hull_lo)
    seg = b - a
    tmax = np.sqrt((seg * seg).sum(axis=1))
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"], rays["d"] = a, seg / tmax[:, None]
    analytic = tmax * affine(0.5 * (a + b))
    st = gm.states(7, n)
    for nx, ny, nz in ((3, 4, 5), (6, 5, 7)):
        z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
        exact = 1.0 + 0.3 * x + 0.5 * y + 0.7 * z
        rho = exact.astype(np.float32)
        residual = rho.astype(np.float64) - exact
        tau = grid_probe_host(rho, lo, hi, SIGMA_T, rays, tmax, st, **TL)[0]
        want = analytic + np.array([tm.tau_model(residual, lo, hi, a[i], rays["d"][i], tmax[i]) for i in range(n)])
        bound = 1e-10 * float(rho.max()) * tmax
        err = np.abs(tau - want)
        print(f"{nx} x {ny} x {nz}: largest error / bound = {np.max(err / bound):.3e}; against the analytic integral alone "
              f"{np.max(np.abs(tau - analytic) / bound):.3e}")
        assert (err <= bound).all(), f"{nx} x {ny} x {nz}: {(err > bound).sum()} segments off, worst {err.max():.3e}"


def _slab(lo, hi, o, d):
    with np.errstate(divide="ignore"):
        t = np.stack([(np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d])
    return max(float(t.min(axis=0).max()), 0.0), float(t.max(axis=0).min())


def test_track_distribution():
    """65 536 tracks through rho = (1, 3), trilinear: the Kolmogorov distance to 1 - exp(-sigma_t tau_model(t)) lies
    below test_delta_tracking_distribution's critical value for blocks 0 and 1, and above it against the piecewise
    constant field's CDF (the two differ by 0.081 at x = 1); an oblique ray through the tau grid with block 2 passes too"""
    rays, tmax = gm.ks_rays()
    st = gm.states(gm.KS_SEED, gm.KS_N)
    o, d = np.array([0.0, 0.5, 0.5]), np.array([1.0, 0.0, 0.0])

    def trilinear(t):
        return 1 - np.exp(-gm.KS_SIGMA_T * tm.tau_along(gm.KS_RHO, gm.KS_LO, gm.KS_HI, o, d, t))

    def nearest(t):
        return 1 - np.exp(-gm.KS_SIGMA_T * (np.minimum(t, 1.0) * 1.0 + np.maximum(t - 1.0, 0.0) * 3.0))

    for block in (0, 1):
        tc = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, st, majorant_block=block, **TL)[1]
        assert not np.isnan(tc).any() and ((tc == -1) | ((tc > 0) & (tc < 2))).all()
        d_tl, d_near = gm.ks_statistic(tc, 2.0, trilinear), gm.ks_statistic(tc, 2.0, nearest)
        print(f"block {block}: D_N = {d_tl:.5f} (critical {CRIT:.5f}); against the piecewise constant CDF: {d_near:.5f}")
        assert d_tl < CRIT
        assert d_near > CRIT
    # oblique, through the tau grid, local majorants on 2-voxel blocks
    rho = gm.tau_grid()
    o, b = np.array([-2.0, 1.7, -4.5]), np.array([5.5, 4.2, 7.5])
    d = (b - o) / np.linalg.norm(b - o)
    t0, t1 = _slab(gm.TAU_LO, gm.TAU_HI, o, d)
    assert 0 < t0 < t1
    sigma_t = 0.15
    tc = grid_probe_host(rho, gm.TAU_LO, gm.TAU_HI, sigma_t, mm.same_ray(o, d, gm.KS_N), 1e30, st, majorant_block=2, **TL)[1]
    assert not np.isnan(tc).any() and ((tc == -1) | ((tc > t0) & (tc < t1))).all()

    def oblique(t):
        return 1 - np.exp(-sigma_t * tm.tau_along(rho, gm.TAU_LO, gm.TAU_HI, o, d, t))

    d_tl = gm.ks_statistic(tc, t1, oblique)
    print(f"oblique, block 2: D_N = {d_tl:.5f} (critical {CRIT:.5f}), {np.mean(tc < 0):.3f} of the tracks leave")
    assert d_tl < CRIT
    assert 0.02 < np.mean(tc < 0) < 0.98


def test_dilated_majorants():
    """rho = (0, 0, 8, 0), block 2: the first super-voxel's own maximum is 0, yet the trilinear field is positive on
    x in (1.5, 2) -- its majorant has to come from the neighbour voxel"""
    rho = np.array([[[0.0, 0.0, 8.0, 0.0]]], dtype=np.float32)
    lo, hi = (0.0, 0.0, 0.0), (4.0, 1.0, 1.0)
    sigma_t = 0.25
    o, d = np.array([0.0, 0.5, 0.5]), np.array([1.0, 0.0, 0.0])
    rays = mm.same_ray(o, d, gm.KS_N)
    st = gm.states(gm.KS_SEED, gm.KS_N)
    tau, tc, _ = grid_probe_host(rho, lo, hi, sigma_t, rays, 1e30, st, majorant_block=2, **TL)
    assert abs(tau[0] - 8.0) <= 1e-10 * 8.0 * 4.0  # a triangle of base 2 and height 8
    assert not np.isnan(tc).any()
    assert ((tc > 1.5) & (tc < 2.0)).sum() > 0.1 * gm.KS_N  # 1 - exp(-0.25) = 0.22 of them

    def cdf(t):
        return 1 - np.exp(-sigma_t * tm.tau_along(rho, lo, hi, o, d, t))

    d_tl = gm.ks_statistic(tc, 4.0, cdf)
    print(f"D_N = {d_tl:.5f} (critical {CRIT:.5f}); {((tc > 1.5) & (tc < 2.0)).sum()} collisions in (1.5, 2)")
    assert d_tl < CRIT
    that, _, _ = grid_ratio_probe_host(rho, lo, hi, sigma_t, rays, 1e30, st, majorant_block=2, **TL)
    T = np.exp(-sigma_t * tau[0])
    bound = 4.5 * np.sqrt(T * (1 - T) / gm.KS_N)  # test_grid_ratio.py::test_unbiased's
    print(f"mean(That) = {that.mean():.6f}, T = {T:.6f}, |diff| = {abs(that.mean() - T):.2e}, bound {bound:.2e}")
    assert ((that >= 0) & (that <= 1)).all() and abs(that.mean() - T) <= bound


def test_one_super_voxel_is_the_global_walk():
    """block >= max(n) equals block 0 bit for bit under trilinear: results, end states, steps, both walkers"""
    rho = gm.tau_grid()
    rays, tmax = gm.tau_rays()
    st = gm.states(3, len(rays))
    for sigma_t in (0.7, 0.05):
        args = (rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, st)
        t0 = grid_probe_host(*args, return_steps=True, **TL)
        r0 = grid_ratio_probe_host(*args, **TL)
        assert (t0[1] >= 0).sum() > 100 and ((r0[0] > 0) & (r0[0] < 1)).sum() > 100
        for b in (max(rho.shape), max(rho.shape) + 3):
            t = grid_probe_host(*args, majorant_block=b, return_steps=True, **TL)
            r = grid_ratio_probe_host(*args, majorant_block=b, **TL)
            for name, g, w in zip(("tau", "t_coll", "states", "steps"), t, t0):
                same = _bits(g) == _bits(w) if g.dtype.kind == "f" else g == w
                assert same.all(), f"track {name}, block {b}, sigma_t {sigma_t}"
            assert (_bits(r[0]) == _bits(r0[0])).all() and (r[1] == r0[1]).all() and (r[2] == r0[2]).all(), f"ratio, block {b}"


@pytest.mark.parametrize("block", [0, 2])
def test_ratio_tracking_is_unbiased(block):
    """test_grid_ratio.py::test_unbiased's oblique ray and bound, T from the trilinear optical depth"""
    n, sigma_t = gm.KS_N, 0.5
    rays = mm.same_ray((-0.3, 0.2, 0.1), (2.5, 0.6, 0.75), n)
    st = gm.states(gm.KS_SEED, n)
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays[:1], 1e30, st[:1], **TL)[0][0]
    model = tm.tau_model(gm.KS_RHO, gm.KS_LO, gm.KS_HI, rays["o"][0], rays["d"][0], 10.0)
    assert abs(tau - model) <= 1e-10 * 3.0 * 10.0 and 2.0 < tau < 6.0
    T = np.exp(-sigma_t * tau)
    that, _, steps = grid_ratio_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, sigma_t, rays, 1e30, st, majorant_block=block, **TL)
    assert ((that >= 0) & (that <= 1)).all()
    bound = 4.5 * np.sqrt(T * (1 - T) / n)
    print(f"block {block}: mean(That) = {that.mean():.6f}, T = {T:.6f}, |diff| = {abs(that.mean() - T):.2e}, bound {bound:.2e}, "
          f"draws per ray {steps.mean():.2f}")
    assert abs(that.mean() - T) <= bound
    assert ((that > 0) & (that < 1)).sum() > 1000


def _ex_status(fn, interp, block=0, n=1):
    d = _lib.vpt_grid_desc()
    d.nx, d.ny, d.nz = 2, 1, 1
    d.lo[:] = gm.KS_LO
    d.hi[:] = gm.KS_HI
    rays, tmax = gm.ks_rays(n)
    st = gm.states(1, n)
    out = [np.zeros(n), np.zeros(n), np.zeros(n, np.uint64), np.zeros(n, np.uint32)]
    dens = np.ascontiguousarray(gm.KS_RHO, dtype=np.float32)
    if fn == "track":
        rc = lib().vpt_grid_probe_host_ex(ctypes.byref(d), dens.ctypes.data, block, interp, 1.0, rays.ctypes.data,
                                          tmax.ctypes.data, st.ctypes.data, n, out[0].ctypes.data, out[1].ctypes.data,
                                          out[2].ctypes.data, out[3].ctypes.data)
    else:
        rc = lib().vpt_grid_ratio_probe_host_ex(ctypes.byref(d), dens.ctypes.data, block, interp, 1.0, rays.ctypes.data,
                                                tmax.ctypes.data, st.ctypes.data, n, out[0].ctypes.data, out[2].ctypes.data,
                                                out[3].ctypes.data)
    return rc, out


def test_errors_and_the_old_probes():
    for fn in ("track", "ratio"):
        for mode in (-1, 2):
            assert _ex_status(fn, mode)[0] == _lib.VPT_E_INVALID
            assert lib().vpt_last_error()
        assert _ex_status(fn, 0)[0] == _lib.VPT_OK and _ex_status(fn, 1)[0] == _lib.VPT_OK
        assert _ex_status(fn, 1, block=-1)[0] == _lib.VPT_E_INVALID
    rays, tmax = gm.ks_rays(256)
    st = gm.states(1, 256)
    for wrapper in (grid_probe_host, grid_ratio_probe_host):
        for name in ("cubic", "Trilinear", None, 1):
            with pytest.raises(VPTError) as ei:
                wrapper(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, st, interpolation=name)
            assert ei.value.code == _lib.VPT_E_INVALID
    # the probes that were there return what the _ex probes return with mode 0, bit for bit
    for block in (0, 1):
        rc, ex = _ex_status("track", 0, block=block, n=256)
        assert rc == _lib.VPT_OK
        old = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, st, majorant_block=block, return_steps=True)
        assert (_bits(old[0]) == _bits(ex[0])).all() and (_bits(old[1]) == _bits(ex[1])).all()
        assert (old[2] == ex[2]).all() and (old[3] == ex[3]).all()
        rc, ex = _ex_status("ratio", 0, block=block, n=256)
        assert rc == _lib.VPT_OK
        old = grid_ratio_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, st, majorant_block=block)
        assert (_bits(old[0]) == _bits(ex[0])).all() and (old[1] == ex[2]).all() and (old[2] == ex[3]).all()
    plain = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, st)  # vpt_grid_probe_host itself
    rc, ex = _ex_status("track", 0, n=256)
    assert (_bits(plain[0]) == _bits(ex[0])).all() and (_bits(plain[1]) == _bits(ex[1])).all() and (plain[2] == ex[2]).all()
