"""Volumetric emission on the CPU (vpt_grid_emission_probe_host: the emitting tracks of csrc/vpt_grid.h compiled for the
host): the walk is grid_probe_host's bit for bit, the score under analytic inversion (B = 1) is the collision voxel's
eps, the mean of esum against sigma_t int T rho eps dt from an independent numpy model (tests/emission_model.py), and
the argument errors.  No GPU."""
import numpy as np
import pytest

import emission_model as em
import grid_model as gm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_emission_probe_host, grid_probe_host

SIGMA_T = 0.7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
@pytest.mark.parametrize("block", [0, 2, 1, 8])
def test_the_walk_is_the_track_bit_for_bit(block, interpolation):
    """emission takes no draw and changes no branch: t_coll, end states and steps are the plain probe's"""
    rho, eps = em.fields()
    rays, tmax = em.rays()
    st = gm.states(7, len(rays))
    tc, es, so, steps = grid_emission_probe_host(rho, eps, em.LO, em.HI, SIGMA_T, rays, tmax, st, majorant_block=block,
                                                 interpolation=interpolation)
    _, tc0, so0, steps0 = grid_probe_host(rho, em.LO, em.HI, SIGMA_T, rays, tmax, st, majorant_block=block, return_steps=True,
                                          interpolation=interpolation)
    assert (_bits(tc) == _bits(tc0)).all(), f"{(_bits(tc) != _bits(tc0)).sum()} collision distances differ"
    assert (so == so0).all() and (steps == steps0).all()
    # the set exercises both ends of a track, origins inside and outside, and the score
    assert (tc >= 0).sum() > 100 and (tc == -1).sum() > 30
    assert ((tc >= 0) & (np.arange(len(tc)) % 2 == 1)).sum() > 30 and (es > 0).sum() > 100
    assert (es >= 0).all() and not np.signbit(es).any()
    assert (es[steps == 0] == 0).all()
    # eps == 0 scores +0 on the same walk
    tz, ez, sz, _ = grid_emission_probe_host(rho, np.zeros_like(eps), em.LO, em.HI, SIGMA_T, rays, tmax, st,
                                             majorant_block=block, interpolation=interpolation)
    assert (_bits(tz) == _bits(tc0)).all() and (sz == so0).all() and (_bits(ez) == 0).all()


def test_analytic_inversion_scores_the_collision_voxel():
    """B = 1, nearest: the majorant is the voxel's own density, the only tentative collision is the real one, and
    (rho eps) / rho is eps bit for bit (the product of two widened float32 values is exact)"""
    rho, eps = em.fields()
    rays, tmax = em.rays()
    st = gm.states(7, len(rays))
    tc, es, _, steps = grid_emission_probe_host(rho, eps, em.LO, em.HI, SIGMA_T, rays, tmax, st, majorant_block=1)
    hit = tc >= 0
    assert (steps <= 1).all() and hit.sum() > 100
    p = rays["o"][hit] + rays["d"][hit] * tc[hit][:, None]
    want = em.voxel_value(eps, em.LO, em.HI, p)
    assert (_bits(es[hit]) == _bits(want)).all(), f"{(es[hit] != want).sum()} scores are not the voxel's eps"
    assert (want > 0).sum() > 50 and (want == 0).sum() > 5
    assert (_bits(es[~hit]) == 0).all()  # no collision: +0


_EX = {}


def _expectation_inputs():
    if not _EX:
        rays = np.zeros(em.EX_N, dtype=gm.RAY_DTYPE)
        rays["o"], rays["d"] = em.EX_O, em.EX_D
        _EX["in"] = (rays, np.full(em.EX_N, 20.0), gm.states(em.EX_SEED, em.EX_N))
    return _EX["in"]


@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
@pytest.mark.parametrize("block", [0, 2])
def test_expectation_of_the_collision_estimator(block, interpolation):
    """65 536 tracks along one oblique ray (it starts outside the box, crosses both densities and leaves the box on
    about one track in ten): |mean(esum) - sigma_t int T rho eps dt| <= 4 std(esum) / sqrt(N), the deviation from the sample itself.  The seed
    (emission_model.EX_SEED) and the ray were fixed on the CPU with this bar holding for all four cases; at four
    standard errors a correct estimator misses it about once in 16 000 seeds."""
    rho, eps = em.expectation_fields()
    rays, tmax, st = _expectation_inputs()
    tc, es, _, steps = grid_emission_probe_host(rho, eps, em.EX_LO, em.EX_HI, em.EX_SIGMA_T, rays, tmax, st,
                                                majorant_block=block, interpolation=interpolation)
    want = em.reference(rho, eps, em.EX_LO, em.EX_HI, em.EX_O, em.EX_D, 20.0, em.EX_SIGMA_T, interpolation)
    mean, se = es.mean(), es.std(ddof=1) / np.sqrt(len(es))
    print(f"block {block}, {interpolation}: mean {mean:.6f}, reference {want:.6f}, off by {(mean - want) / se:+.2f} standard errors "
          f"({se:.2e}); {steps.mean():.2f} tentative steps per track, {np.mean(tc >= 0):.3f} collide")
    assert want > 0.1 and se > 0
    assert abs(mean - want) <= 4 * se
    # the bar tells the estimator from a neighbour: the same sum without the factor sigma_t does not pass
    assert abs(mean / em.EX_SIGMA_T - want) > 4 * se


def test_the_reference_integrals_agree_on_a_uniform_field():
    """the two quadratures of the model against each other and a closed form: rho = 2, eps = 0.5 on the whole box"""
    rho, eps = np.full((2, 2, 8), 2.0, np.float32), np.full((2, 2, 8), 0.5, np.float32)
    o, d = np.array([0.5, 0.5, 0.5]), np.array([1.0, 0.0, 0.0])
    want = 0.5 * (1 - np.exp(-0.9 * 2.0 * 3.5))
    for interpolation in ("nearest", "trilinear"):
        assert abs(em.reference(rho, eps, em.EX_LO, em.EX_HI, o, d, 20.0, 0.9, interpolation) - want) < 1e-12


def test_argument_errors():
    rho, eps = em.fields()
    rays, tmax = em.rays(8)
    st = gm.states(7, 8)

    def probe(r=rho, e=eps, **kw):
        return grid_emission_probe_host(r, e, em.LO, em.HI, SIGMA_T, rays, tmax, st, **kw)

    for value in (np.nan, -1e-3, np.inf):
        bad = eps.copy()
        bad[1, 2, 3] = value
        with pytest.raises(VPTError) as ei:
            probe(e=bad)
        assert ei.value.code == _lib.VPT_E_INVALID and "emission" in str(ei.value)
    for shape in ((4, 5, 5), (5, 4, 6), (4 * 5 * 6,)):  # another shape, even with as many voxels
        with pytest.raises(VPTError) as ei:
            probe(e=np.zeros(shape, np.float32))
        assert ei.value.code == _lib.VPT_E_INVALID
    bad = rho.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(VPTError) as ei:
        probe(r=bad)
    assert ei.value.code == _lib.VPT_E_INVALID
    for kw in (dict(majorant_block=-1), dict(interpolation="cubic")):
        with pytest.raises(VPTError) as ei:
            probe(**kw)
        assert ei.value.code == _lib.VPT_E_INVALID
    probe()  # and the arguments as they stand are accepted
