"""The one-sample combination of delta tracking and equi-angular sampling on the CPU (vpt_grid_mis_probe_host:
csrc/vpt_grid_mis.h compiled for the host): the probe against a plain-Python restatement bit for bit, q = 0 against the
equi-angular probe bit for bit, the invariants of the combined pdf, unbiasedness from the inputs alone, and the
distribution of the sampled distance against the mixture.  No GPU."""
import functools
import math

import numpy as np
import pytest

import eqa_model as em
import grid_model as gm
import majorant_model as mm
import mis_model as mi
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_eqa_probe_host, grid_mis_probe_host, grid_probe_host
from test_grid_eqa import LIGHT_IN, LIGHT_OUT, UB_LIGHT, UB_SIGMA_T, _bits, _fields, _oblique

LIGHTS = {"light_in": LIGHT_IN, "light_out": LIGHT_OUT}
CASES = [(light, field, sigma_t, interpolation) for light in LIGHTS for field in ("tau", "sparse") for sigma_t in (0.7, 0.05)
         for interpolation in ("nearest", "trilinear")]
CASE_IDS = ["-".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(light, sigma_t):
    """test_grid_eqa.py's ray sets: grid_model's rays without those whose line holds the light (D == 0 keeps the
    reference's 0 / 0); the thin medium scatters a sixth of its rays and gets four times as many"""
    rays, tmax = gm.tau_rays(n=2000 if sigma_t > 0.1 else 8000)
    st = gm.states(3, len(rays))
    D = np.array([em.geometry(rays["o"][i], rays["d"][i], LIGHTS[light])[0] for i in range(len(rays))])
    keep = D != 0
    assert keep.sum() >= 256
    return rays[keep], tmax[keep], st[keep]


def _probe(case, q, block):
    light, field, sigma_t, interpolation = case
    rays, tmax, st = _inputs(light, sigma_t)
    return grid_mis_probe_host(_fields()[field], gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, LIGHTS[light], st, q=q,
                               majorant_block=block, interpolation=interpolation)


def _model(case, q, block):
    light, field, sigma_t, interpolation = case
    rays, tmax, st = _inputs(light, sigma_t)
    return mi.mis_rays(_fields()[field], gm.TAU_LO, gm.TAU_HI, sigma_t, q, rays, tmax, LIGHTS[light], st, interpolation, block)


def _outcomes(res):
    """the four outcomes of a decision as masks: track -> surface, track -> medium with rho_t > 0, equi-angular ->
    surface, equi-angular -> medium with rho_t > 0"""
    _, strategy, dist, _, _, _, rho_t, _, _ = res
    surf, med = dist == -1, (dist >= 0) & (rho_t > 0)
    return (strategy == 1) & surf, (strategy == 1) & med, (strategy == 0) & surf, (strategy == 0) & med


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("q", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_probe_equals_the_python_model(case, q, block):
    """every output and the end state bit for bit.  The condition on the inputs is asserted from the model alone: at
    q = 0.5 each case has at least 50 rays of each of the four outcomes"""
    want = _model(case, q, block)
    if q == 0.5:
        counts = [int(m.sum()) for m in _outcomes(want)]
        print(f"{case} block {block}: track/surface {counts[0]}, track/medium {counts[1]}, eqa/surface {counts[2]}, "
              f"eqa/medium {counts[3]}")
        assert min(counts) >= 50, counts
    got = _probe(case, q, block)
    for name, g, w in zip(mi.NAMES, got, want):
        if g.dtype == np.float64:
            assert (_bits(g) == _bits(w)).all(), f"{name}: {(_bits(g) != _bits(w)).sum()} of {len(g)} differ"
        else:
            assert (g == w).all(), f"{name}: {(g != w).sum()} of {len(g)} differ"
    assert (got[8] == want[8]).all()
    assert not np.isnan(got[2]).any()  # no track reaches the step cap
    if q == 1.0:
        assert (got[1] == 1).all()
    trk = got[1] == 1
    assert (got[7][~trk] == 0).all() and (got[7][trk & (got[2] >= 0)] >= 1).all()


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fraction_zero_is_the_equiangular_probe(case, block):
    """q = 0: psurf, dist, pdf, T, rho_t and the end state are grid_eqa_probe_host's bit for bit, on every case"""
    light, field, sigma_t, interpolation = case
    rays, tmax, st = _inputs(light, sigma_t)
    want = grid_eqa_probe_host(_fields()[field], gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, LIGHTS[light], st,
                               interpolation=interpolation)
    psurf, strategy, dist, pdf, pe, T, rho_t, steps, so = _probe(case, 0.0, block)
    for name, g, w in zip(("psurf", "dist", "pdf", "T", "rho_t"), (psurf, dist, pdf, T, rho_t), want):
        assert (_bits(g) == _bits(w)).all(), f"{name}: {(_bits(g) != _bits(w)).sum()} of {len(g)} differ"
    assert (so == want[5]).all()
    assert (strategy == 0).all() and (steps == 0).all() and (_bits(pe) == _bits(pdf)).all()
    assert (dist != -1).sum() >= 50


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("q", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_invariants(case, q, block):
    """on every medium outcome: the combined pdf is its formula on the outputs, bitwise, and the vertex weight
    sigma_t rho_t T / pdf is at most 1 / q (the quotient pff / (q pff + x), x >= 0, is at most 1 / q but for one
    rounding of the product, one of the sum and one of the division: 2^-50 holds three half-ulps); the share of
    track-strategy rays is binomial in q"""
    sigma_t = case[2]
    psurf, strategy, dist, pdf, pe, T, rho_t, _, _ = _probe(case, q, block)
    med = (dist >= 0) & (rho_t > 0)
    assert med.sum() >= 100
    pff = sigma_t * rho_t[med] * T[med]
    assert (_bits(pdf[med]) == _bits(q * pff + (1 - q) * pe[med])).all()
    w = pff / pdf[med]
    print(f"{case} q {q} block {block}: max weight {w.max():.6f} of {1 / q:.6f}, track share {strategy.mean():.4f}")
    assert (w >= 0).all() and (w <= (1 / q) * (1 + 2.0 ** -50)).all()
    assert ((pe[med] >= 0) & (T[med] > 0) & (T[med] <= 1)).all()
    n = len(strategy)
    assert abs(strategy.mean() - q) <= 4.5 * math.sqrt(q * (1 - q) / n)
    assert abs((dist == -1).mean() - psurf.mean()) <= 4.5 * math.sqrt(0.25 / n)  # the surface has probability psurf


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("q", [0.25, 0.5, 1.0])
def test_unbiased(q, block):
    """test_grid_eqa.py's oblique ray through rho = (1, 3), 65 536 states: w = sigma_t rho_t T / pdf on the medium
    outcomes and 0 otherwise has the mean 1 - psurf exactly -- the integral of sigma_t rho T over [a, b] is
    1 - Tr(a, b) -- whatever q is.  The right side comes from the deterministic walker's tau alone; the mean of N
    samples lies within 4.5 sample standard errors of it (7e-6 two-sided), and that standard error is at most 5 % of
    1 - psurf, so a wrong weight is seen"""
    rays, st, a, b, D, proj = _oblique()
    n = len(rays)
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays[:1], 1e30, st[:1])[0][0]
    want = 1 - math.exp(-UB_SIGMA_T * tau)
    psurf, strategy, dist, pdf, pe, T, rho_t, _, _ = grid_mis_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays, 1e30,
                                                                          UB_LIGHT, st, q=q, majorant_block=block)
    med = dist >= 0
    assert (rho_t[med] > 0).all() and not np.isnan(dist).any()
    w = np.zeros(n)
    w[med] = UB_SIGMA_T * rho_t[med] * T[med] / pdf[med]
    se = float(w.std(ddof=1)) / math.sqrt(n)
    print(f"q {q} block {block}: mean(w) = {w.mean():.6f}, 1 - psurf = {want:.6f}, |diff| = {abs(w.mean() - want):.2e}, "
          f"standard error {se:.2e} ({se / want:.4f} of 1 - psurf), max(w) {w.max():.3f}, medium {med.sum()}, "
          f"track {strategy.sum()}")
    assert abs(psurf[0] - (1 - want)) < 1e-15 and (_bits(psurf) == _bits(psurf[:1])).all()
    assert (dist[med] >= a * (1 - 1e-12)).all() and (dist[med] <= b * (1 + 1e-12)).all()
    assert se <= 0.05 * want
    assert abs(w.mean() - want) <= 4.5 * se
    assert 1000 < med.sum() < n - 1000


def test_distance_distribution():
    """the medium-branch distances on the same ray at q = 0.5 follow the mixture
    [q (1 - exp(-sigma_t tau(s))) + (1 - q) (1 - psurf) F_eq(s)] / (1 - psurf), tau(s) from grid_probe_host:
    Kolmogorov-Smirnov at alpha = 0.001 (1.95 / sqrt(N)); the pure equi-angular law and the pure track law are both
    rejected by the same statistic"""
    q = 0.5
    rays, st, a, b, D, proj = _oblique()
    psurf, _, dist, _, _, _, _, _, _ = grid_mis_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays, 1e30, UB_LIGHT, st,
                                                           q=q)
    t = np.sort(dist[dist >= 0])
    n = len(t)
    ps = float(psurf[0])
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SIGMA_T, rays[:n], t, st[:n])[0]
    ta, tb = math.atan2(a - proj, D), math.atan2(b - proj, D)
    F_trk = (1 - np.exp(-UB_SIGMA_T * tau)) / (1 - ps)
    F_eqa = (np.arctan2(t - proj, D) - ta) / (tb - ta)
    F_mix = q * F_trk + (1 - q) * F_eqa
    hi_, lo_ = np.arange(1, n + 1) / n, np.arange(0, n) / n

    def ks(F):
        return float(np.max(np.maximum(np.abs(hi_ - F), np.abs(F - lo_))))

    crit = 1.95 / math.sqrt(n)
    print(f"N = {n}, D_N = {ks(F_mix):.5f} (critical {crit:.5f}); against the equi-angular law {ks(F_eqa):.5f}, "
          f"against the track's {ks(F_trk):.5f}")
    assert n > 10000 and ks(F_mix) < crit and ks(F_eqa) > crit and ks(F_trk) > crit


def test_argument_errors():
    rays, tmax = gm.ks_rays(4)
    st = gm.states(1, 4)
    args = (gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, UB_LIGHT, st)
    for q in (-0.1, 1.0 + 2.0 ** -52, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(VPTError) as ei:
            grid_mis_probe_host(*args, q=q)
        assert ei.value.code == _lib.VPT_E_INVALID, q
    for q in (0.0, 1.0, -0.0):
        grid_mis_probe_host(*args, q=q)
    with pytest.raises(VPTError) as ei:
        grid_mis_probe_host(*args, majorant_block=-1)
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_mis_probe_host(*args, interpolation="cubic")
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_mis_probe_host(np.full((1, 1, 1), -1.0), (0, 0, 0), (1, 1, 1), 1.0, rays, tmax, UB_LIGHT, st)
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(ValueError):
        grid_mis_probe_host(gm.KS_RHO[0], gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, UB_LIGHT, st)  # rho is not [nz, ny, nx]
    with pytest.raises(ValueError):
        grid_mis_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, UB_LIGHT, st[:3])  # states of another length
    with pytest.raises(ValueError):
        grid_mis_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, np.zeros((3, 3)), st)  # three lights, four rays
    with pytest.raises(ValueError):
        grid_mis_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax[:3], UB_LIGHT, st)  # tmax of another length
