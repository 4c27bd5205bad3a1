"""Equi-angular distance sampling in the density grid on the CPU (vpt_grid_eqa_probe_host: csrc/vpt_grid_eqa.h compiled
for the host): the probe against a plain-Python restatement bit for bit, the invariants of rays without medium and of
segments inside the box, unbiasedness against the deterministic optical depth, and the distribution of the sampled
distance.  No GPU."""
import math

import numpy as np
import pytest

import eqa_model as em
import grid_model as gm
import majorant_model as mm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_eqa_probe_host, grid_probe_host
from ratio_model import _slab

LIGHT_IN = (1.5, 3.1, 1.5)      # inside grid_model's box, in the half the sparse field leaves empty
LIGHT_OUT = (7.5, 6.0, -6.0)    # outside it
NAMES = ("psurf", "dist", "pdf", "T", "rho_t")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fields():
    """grid_model's tau grid (every voxel > 0: a sampled point always has medium) and, in the same box, the sparse
    field of the majorant tests (half the voxels empty) with the lower half of its x layers emptied, so that the trilinear
    field too is exactly zero in a region: the rho_t == 0 exit"""
    sparse = mm.sparse_field()
    sparse[:, :, :4] = 0.0
    return {"tau": gm.tau_grid(), "sparse": sparse}


@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
@pytest.mark.parametrize("sigma_t", [0.7, 0.05])
@pytest.mark.parametrize("field", ["tau", "sparse"])
@pytest.mark.parametrize("light", [LIGHT_IN, LIGHT_OUT], ids=["light_in", "light_out"])
def test_host_probe_equals_the_python_model(light, field, sigma_t, interpolation):
    """grid_model's rays (origins inside and outside the box, rays that miss it, axis-parallel and zero-length ones):
    every output and the end state bit for bit"""
    rho = _fields()[field]
    rays, tmax = gm.tau_rays(n=2000 if sigma_t > 0.1 else 8000)  # the thin medium scatters a sixth of its rays
    st = gm.states(3, len(rays))
    D = np.array([em.geometry(rays["o"][i], rays["d"][i], light)[0] for i in range(len(rays))])
    keep = D != 0  # a light on the ray's line keeps the reference's 0 / 0
    rays, tmax, st = rays[keep], tmax[keep], st[keep]
    assert len(rays) >= 256
    got = grid_eqa_probe_host(rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, light, st, interpolation=interpolation)
    want, (a, _) = em.eqa_rays(rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, light, st, interpolation)
    for name, g, w in zip(NAMES, got, want):
        assert (_bits(g) == _bits(w)).all(), f"{name}: {(_bits(g) != _bits(w)).sum()} of {len(g)} differ"
    assert (got[5] == want[5]).all()
    psurf, dist, _, T, rho_t, _ = got
    surface, medium, empty = dist == -1, (dist != -1) & (rho_t > 0), (dist != -1) & (rho_t == 0)
    print(f"{field} {interpolation} sigma_t {sigma_t}: surface {surface.sum()}, medium {medium.sum()}, empty {empty.sum()}, "
          f"a > 0 among medium {(a[~surface] > 0).sum()}")
    assert surface.sum() >= 50 and medium.sum() >= 50
    if field == "sparse":
        assert empty.sum() >= 50 and (T[empty] == 0).all()
    else:
        assert empty.sum() == 0  # no voxel of the tau grid is empty
    assert (a[~surface] > 0).sum() >= 20 and (a[~surface] == 0).sum() >= 20  # origins outside and inside the box
    assert ((T[medium] > 0) & (T[medium] <= 1)).all() and ((psurf >= 0) & (psurf <= 1)).all()


@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
def test_no_medium_is_the_surface_after_two_draws(interpolation):
    """rays that miss the box, and an all-zero grid: psurf == 1.0, dist == -1, and the state two draws on"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI, n=64)
    st = gm.states(5, len(rays))
    two = np.array([gm.erand48_step(gm.erand48_step(s)[0])[0] for s in st], dtype=np.uint64)
    got = grid_eqa_probe_host(np.zeros_like(rho), mm.SPARSE_LO, mm.SPARSE_HI, 0.7, rays, tmax, LIGHT_IN, st,
                              interpolation=interpolation)
    assert (_bits(got[0]) == _bits(np.ones(len(rays)))).all() and (got[1] == -1).all() and (got[5] == two).all()
    assert all((_bits(got[k]) == 0).all() for k in (2, 3, 4))
    miss = np.zeros(3, dtype=gm.RAY_DTYPE)
    miss["o"] = [(10, 10, 10), (-5, 3, 0), (2, 3, 20)]
    miss["d"] = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    got = grid_eqa_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, 0.7, miss, 1e30, LIGHT_OUT, st[:3], interpolation=interpolation)
    assert (_bits(got[0]) == _bits(np.ones(3))).all() and (got[1] == -1).all() and (got[5] == two[:3]).all()


def test_segment_inside_the_box_is_the_reference_interval():
    """with both ends of the segment inside the box the interval is [+0.0, tmax] bit for bit, so the distance and
    the pdf are equiAngularParams2's and equiAngularProb's on tMax, operation for operation"""
    rho = gm.tau_grid()
    rays, tmax = gm.tau_rays()
    lo, hi = np.array(gm.TAU_LO), np.array(gm.TAU_HI)
    end = rays["o"] + rays["d"] * tmax[:, None]
    inside = (np.all((rays["o"] > lo) & (rays["o"] < hi), axis=1) & np.all((end > lo + 1e-9) & (end < hi - 1e-9), axis=1)
              & (tmax > 0))
    rays, tmax = rays[inside], tmax[inside]
    assert len(rays) >= 256
    st = gm.states(3, len(rays))
    ab = np.array([em.interval(list(gm.TAU_LO), list(gm.TAU_HI), list(rays["o"][i]), list(rays["d"][i]), float(tmax[i]))
                   for i in range(len(rays))])
    assert (_bits(ab[:, 0]) == 0).all()  # +0.0, not -0.0
    assert (_bits(ab[:, 1]) == _bits(tmax)).all()
    psurf, dist, pdf, _, _, _ = grid_eqa_probe_host(rho, gm.TAU_LO, gm.TAU_HI, 0.7, rays, tmax, LIGHT_IN, st)
    checked = 0
    for i in np.nonzero(dist != -1)[0]:
        o, d = rays["o"][i], rays["d"][i]
        D, proj = em.geometry(o, d, LIGHT_IN)
        x = gm.erand48_step(st[i])[1]
        ta, tb = math.atan2(0.0 - proj, D), math.atan2(float(tmax[i]) - proj, D)
        s = D * math.tan((1 - x) * ta + x * tb)
        assert dist[i] == s + proj and pdf[i] == D / math.fabs(tb - ta) / (s * s + D * D) * (1 - psurf[i])
        checked += 1
    assert checked >= 100


# one oblique ray through rho = (1, 3) (tests/test_grid_ratio.py's) and a light off it
UB_O, UB_D, UB_LIGHT, UB_SIGMA_T = (-0.3, 0.2, 0.1), (2.5, 0.6, 0.75), (1.2, 1.5, 0.5), 0.5


def _oblique():
    n = gm.KS_N
    rays = mm.same_ray(UB_O, UB_D, n)
    st = gm.states(gm.KS_SEED, n)
    o, d = [float(v) for v in rays["o"][0]], [float(v) for v in rays["d"][0]]
    a, b = _slab([float(v) for v in gm.KS_LO], [float(v) for v in gm.KS_HI], o, d)  # tmax = 1e30: b is the exit
    D, proj = em.geometry(o, d, UB_LIGHT)
    assert a > 0 and D > 0.5
    return rays, st, a, b, D, proj


def test_unbiased():
    """w = sigma_t rho_t T / pdf on the medium branch and 0 on the surface branch has the mean 1 - psurf exactly: the
    integral of sigma_t rho T over [a, b] is 1 - Tr(a, b), and nothing lies in front of a.  0 <= w <= w_max =
    sigma_t rho_max |tb - ta| (s_max^2 + D^2) / (D (1 - psurf)), so Var w <= (1 - psurf) w_max - (1 - psurf)^2 and
    the mean of N samples is within 4.5 standard deviations of that (7e-6 two-sided).  The right side is computed from
    the deterministic walker's tau and the geometry alone.  Measured: |mean - (1 - psurf)| = 1.07e-3, 0.022 of the bound
    4.76e-2 (w_max 9.2, the largest w 3.1)."""
    rays, st, a, b, D, proj = _oblique()
    n = len(rays)
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays[:1], 1e30, st[:1])[0][0]
    assert 2.0 < tau < 6.0  # the ray crosses both voxels
    want = 1 - math.exp(-UB_SIGMA_T * tau)
    ta, tb = math.atan2(a - proj, D), math.atan2(b - proj, D)
    s_max = max(abs(a - proj), abs(b - proj))
    w_max = UB_SIGMA_T * float(gm.KS_RHO.max()) * abs(tb - ta) * (s_max * s_max + D * D) / (D * want)
    bound = 4.5 * math.sqrt((want * w_max - want * want) / n)
    psurf, dist, pdf, T, rho_t, _ = grid_eqa_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays, 1e30, UB_LIGHT, st)
    med = dist != -1
    w = np.zeros(n)
    w[med] = UB_SIGMA_T * rho_t[med] * T[med] / pdf[med]
    print(f"mean(w) = {w.mean():.6f}, 1 - psurf = {want:.6f}, |diff| = {abs(w.mean() - want):.2e}, bound {bound:.2e}, "
          f"fraction {abs(w.mean() - want) / bound:.3f}, w_max {w_max:.3f}, max(w) {w.max():.3f}, medium {med.sum()}")
    assert abs(psurf[0] - (1 - want)) < 1e-15 and (_bits(psurf) == _bits(psurf[:1])).all()
    assert (w >= 0).all() and (w <= w_max * (1 + 1e-12)).all()
    assert (dist[med] >= a * (1 - 1e-12)).all() and (dist[med] <= b * (1 + 1e-12)).all()
    assert abs(w.mean() - want) <= bound
    assert 1000 < med.sum() < n - 1000  # both branches are taken


def test_distance_distribution():
    """the medium-branch distances on the same ray are equi-angular in [a, b]: Kolmogorov-Smirnov against
    (atan2(dist - proj, D) - ta) / (tb - ta) at grid_model's significance, alpha = 0.001 (1.95 / sqrt(N)); the
    uniform law on [a, b] is rejected"""
    rays, st, a, b, D, proj = _oblique()
    dist = grid_eqa_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays, 1e30, UB_LIGHT, st)[1]
    t = np.sort(dist[dist != -1])
    n = len(t)
    ta, tb = math.atan2(a - proj, D), math.atan2(b - proj, D)
    hi_, lo_ = np.arange(1, n + 1) / n, np.arange(0, n) / n

    def ks(F):
        return float(np.max(np.maximum(np.abs(hi_ - F), np.abs(F - lo_))))

    d_eqa = ks((np.arctan2(t - proj, D) - ta) / (tb - ta))
    d_uni = ks((t - a) / (b - a))
    crit = 1.95 / math.sqrt(n)
    print(f"N = {n}, D_N = {d_eqa:.5f} (critical {crit:.5f}); against the uniform law: {d_uni:.5f}")
    assert n > 10000 and d_eqa < crit and d_uni > crit


def test_argument_errors():
    rays, tmax = gm.ks_rays(1)
    st = gm.states(1, 1)
    with pytest.raises(VPTError) as ei:
        grid_eqa_probe_host(np.full((1, 1, 1), -1.0), (0, 0, 0), (1, 1, 1), 1.0, rays, 1.0, UB_LIGHT, st)
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_eqa_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, UB_LIGHT, st, interpolation="cubic")
    assert ei.value.code == _lib.VPT_E_INVALID
