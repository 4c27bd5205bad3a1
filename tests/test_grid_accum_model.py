"""The CPU model of the grid accumulator (tests/grid_accum_model.py) against the oracle and against accum_model, and the
refine targets of tests/test_gpu_grid_accum.py, chosen here on the oracle's samples alone.

The model's per-sample radiances come from Oracle.trace on the oracle's own camera samples; its image after all levels
must be Oracle.render's, the in-order sum, bit for bit, whatever the chunk; its statistic must be accum_model.stat's on
the same chunk sums."""
import numpy as np
import pytest

import accum_model as am
import grid_accum_model as gam
import hetero_cloud as hc
import test_gpu_hetero as T
from conftest import bitwise_equal
from scenes import default_scene

C, CAP, SEED = 4, 24, 11
ESTS = {"hetero": 10, "hetero_ratio": 11}

# The adaptive test's target, chosen on the oracle's samples alone (40x24, hetero_cloud's MAIN cloud with SA, SS, seed 11,
# chunk 4, cap 6 levels, min_levels 2, one level per pass), and the level counts the model reaches with it: under both
# estimators 2 tiles reach the cap and 13 stop below it.
REFINE_TARGET = 0.75
REFINE_LEVELS = {
    "hetero": [4, 5, 3, 4, 4, 6, 4, 4, 4, 6, 5, 4, 4, 4, 4],
    "hetero_ratio": [4, 5, 3, 4, 4, 5, 6, 4, 4, 5, 4, 4, 4, 5, 6],
}
# add(2), then refine(FLOOR_TARGET, lum_floor=1.0, min_levels=2, levels_per_pass=3) under estimator 10: one pass of 3 levels
# for all 15 tiles, a second for 4 of them, clipped to 1 level at the cap
FLOOR_TARGET = 0.625
FLOOR_LEVELS = [5, 5, 5, 5, 5, 5, 6, 6, 5, 5, 6, 5, 5, 5, 6]
FLOOR_SETS = [15, 4]


@pytest.fixture()
def cloud_orc(orc_vm):
    """the session's oracle with the default scene and the MAIN cloud; left without a grid"""
    orc_vm.set_hetero_fault(0)
    orc_vm.set_scene(default_scene())
    hc.set_cloud(orc_vm, *hc.MAIN)
    yield orc_vm
    orc_vm.clear_density_grid()


_L = {}


def oracle_radiances(orc, w, h, spp, est, file_rows=None):
    """L[rows, w, spp, 3] of the MAIN cloud from Oracle.trace, computed once per shape and shared (read-only)"""
    key = (w, h, spp, est, None if file_rows is None else tuple(file_rows))
    if key not in _L:
        rays, st = T._camera_samples(orc, w, h, spp, SEED)
        _L[key] = gam.radiances(lambda r, s: orc.trace(ESTS[est], r, s, hc.SA, hc.SS), rays, st, file_rows)
    return _L[key]


@pytest.mark.parametrize("est", list(ESTS))
def test_image_is_the_oracles_render(cloud_orc, est):
    """after all levels the model's image is Oracle.render's in-order sum, bit for bit, at every chunk"""
    w, h, spp = 12, 10, 8
    L = oracle_radiances(cloud_orc, w, h, spp, est)
    want = cloud_orc.render(w, h, spp, ESTS[est], hc.SA, hc.SS, seed=SEED)
    assert np.count_nonzero(want.any(axis=-1)) * 2 >= w * h
    for chunk in (4, 1, 2, 8):
        m = gam.GridAccumModel(L, chunk)
        m.add(spp // chunk)
        assert bitwise_equal(m.image(), want).all(), f"chunk {chunk}: {(~bitwise_equal(m.image(), want)).sum()} values differ"
    # level by level and in tile subsets: the same sum, and after one level of 4 the render of 4 spp
    m = gam.GridAccumModel(L, 4)
    m.add(1, tiles=[3, 0])
    m.add(1)
    m.add(1, tiles=[1, 2])
    assert list(m.levels) == [2, 2, 2, 2] and bitwise_equal(m.image(), want).all()
    m = gam.GridAccumModel(L, 4)
    m.add(1)
    assert bitwise_equal(m.image(), cloud_orc.render(w, h, 4, ESTS[est], hc.SA, hc.SS, seed=SEED)).all()
    # the chunked sum of accum_model on the same chunk sums is another image: the two contracts are told apart
    chunked = am.AccumModel(gam.chunk_sums(L, 2), 2)
    chunked.add(4)
    assert (~bitwise_equal(chunked.image(), want)).sum() > 10


@pytest.mark.parametrize("est", list(ESTS))
def test_statistic_is_accum_models(cloud_orc, est):
    """s1, s2 and the errors equal accum_model.stat on the same chunk sums, after every number of levels"""
    w, h = 20, 12
    L = oracle_radiances(cloud_orc, w, h, CAP, est)
    cs = gam.chunk_sums(L, C)
    m = gam.GridAccumModel(L, C)
    for lv in range(1, CAP // C + 1):
        m.add(1)
        _, s12, err = am.stat(cs[:lv].reshape(lv, -1, 3), C)
        assert bitwise_equal(m.s1.reshape(-1), s12[:, 0]).all() and bitwise_equal(m.s2.reshape(-1), s12[:, 1]).all()
        err = err.reshape(h, w)
        for t in range(m.ntiles):
            r, c = m._slice(t)
            assert bitwise_equal(m.tile_err[t], np.max(err[r, c]))
    assert (m.s2 > 0).any() and np.isfinite(m.tile_err).all()
    # the sum is the in-order sum, not the sum of the chunk sums
    insum = np.zeros((h, w, 3))
    for s in range(CAP):
        insum = L[:, :, s] + insum
    assert bitwise_equal(m.sum, insum).all()
    assert (~bitwise_equal(m.sum, am.stat(cs.reshape(CAP // C, -1, 3), C)[0].reshape(h, w, 3))).any()


@pytest.mark.parametrize("est", list(ESTS))
def test_refine_target(cloud_orc, est):
    """the target of the GPU's adaptive test: at least 2 tiles stop below the cap and at least 2 reach it"""
    L = oracle_radiances(cloud_orc, 40, 24, CAP, est)
    m = gam.GridAccumModel(L, C)
    sets = m.refine(REFINE_TARGET, min_levels=2, levels_per_pass=1)
    assert list(m.levels) == REFINE_LEVELS[est]
    assert (m.levels < CAP // C).sum() >= 2 and (m.levels == CAP // C).sum() >= 2
    assert len(sets) == 6 and sets[0] == list(range(15))


def test_floor_target(cloud_orc):
    L = oracle_radiances(cloud_orc, 40, 24, CAP, "hetero")
    m = gam.GridAccumModel(L, C)
    m.add(2)
    sets = m.refine(FLOOR_TARGET, lum_floor=1.0, min_levels=2, levels_per_pass=3)
    assert list(m.levels) == FLOOR_LEVELS and [len(s) for s in sets] == FLOOR_SETS
    # another floor gives other errors: the floor takes part
    other = gam.GridAccumModel(L, C)
    other.add(2)
    other.refine(9.0, lum_floor=1.0, min_levels=2)
    plain = gam.GridAccumModel(L, C)
    plain.add(2)
    assert (other.tile_err != plain.tile_err).any()
