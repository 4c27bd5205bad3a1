"""The grid accumulator on the GPU (vpt_accum_create_grid, Tracer.grid_accumulator; estimators 10 to 16): every value of
the state against the CPU model (tests/grid_accum_model.py) and every pixel against the one-shot render of its sample
count, bit for bit.

The model's per-sample radiances come from Tracer.trace on the oracle's camera samples (the per-sample kernels are pinned
to the oracle sample for sample by the *_oracle test modules); estimators 10 and 11 are tied to Oracle.trace here once
more, at 20x12.  Shapes are the accumulator's awkward ones: 20x12 has padded tiles on the right and bottom edges (3x2
tiles), 40x24 has 15 tiles; chunk 4, cap 24 spp (6 levels).  The grids and media are tests/hetero_cloud.py's."""
import numpy as np
import pytest

import accum_model as am
import grid_accum_model as gam
import hetero_cloud as hc
import test_gpu_hetero as T
import test_grid_accum_model as M
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import RenderConfig, Tracer, VPTError, _lib
from scenes import default_scene

pytestmark = pytest.mark.gpu

C, CAP, SEED = M.C, M.CAP, M.SEED
# estimator: (sigma_a, sigma_s), the grid's setter, its main configuration, the configurations of test_every_instantiation
SETUPS = {
    "hetero": ((hc.SA, hc.SS), hc.set_cloud, hc.MAIN, hc.CONFIGS),
    "hetero_ratio": ((hc.SA, hc.SS), hc.set_cloud, hc.MAIN, hc.CONFIGS),
    "hetero_equiangular": ((hc.EXT_SA, hc.EXT_SS), hc.set_ext_cloud, hc.EXT_MAIN, [(0, "nearest"), (0, "trilinear")]),
    "hetero_mis": ((hc.EXT_SA, hc.EXT_SS), hc.set_ext_cloud, hc.EXT_MAIN, hc.EXT_CONFIGS),
    "hetero_chromatic": ((hc.EXT_SA, hc.EXT_SS), hc.set_ext_cloud, hc.EXT_MAIN, hc.EXT_CONFIGS),
    "hetero_residual": ((hc.RES_SA, hc.RES_SS), hc.set_floor_cloud, hc.RES_MAIN, hc.RES_CONFIGS),
    "hetero_spectral": ((hc.EXT_SA, hc.EXT_SS), hc.set_ext_cloud, hc.SPECTRAL_MAIN, hc.EXT_CONFIGS),
}
INSTANTIATIONS = [(est, cfg) for est, s in SETUPS.items() for cfg in s[3]]


@pytest.fixture(scope="module")
def gt():
    """a tracer of this module's own: its grids and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    _reset(t)
    t.close()


def _reset(t):
    t.set_scene(default_scene())
    hc.reset_ext(t)
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")


def _setup(t, est, config=None):
    _reset(t)
    _, setter, main, _ = SETUPS[est]
    setter(t, *(main if config is None else config))


def _cfg(est, w, h, spp=CAP, fp64=True, **bands):
    sa, ss = SETUPS[est][0]
    return RenderConfig(width=w, height=h, spp=spp, estimator=est, sigma_a=sa, sigma_s=ss, seed=SEED, fp64=fp64, **bands)


_RENDERS = {}
_MODELS = {}


def _render(t, est, w, h, spp, fp64=True, config=None, **bands):
    """one-shot renders under the setup in force, computed once and shared (read-only)"""
    key = (est, config, w, h, spp, fp64, tuple(sorted(bands.items())))
    if key not in _RENDERS:
        img = t.render(_cfg(est, w, h, spp, fp64, **bands))
        img.setflags(write=False)
        _RENDERS[key] = img
    return _RENDERS[key]


def _radiances(t, orc_vm, est, w, h, spp=CAP, config=None, bands=(0, 1, 0)):
    """L[rows, w, spp, 3] from Tracer.trace under the setup in force, once per configuration"""
    key = (est, config, w, h, spp, bands)
    if key not in _MODELS:
        rays, st = T._camera_samples(orc_vm, w, h, spp, SEED)
        sa, ss = SETUPS[est][0]
        _MODELS[key] = gam.radiances(lambda r, s: t.trace(est, r, s, sa, ss), rays, st, am.shard_file_rows(h, *bands))
    return _MODELS[key]


def _model(t, orc_vm, est, w, h, **kw):
    return gam.GridAccumModel(_radiances(t, orc_vm, est, w, h, **kw), C)


def _assert_state(acc, model):
    st = acc.state()
    assert (st["tile_levels"] == model.levels).all()
    for name, want in (("sum", model.sum), ("s1", model.s1), ("s2", model.s2), ("tile_err", model.tile_err)):
        eq = bitwise_equal(st[name], want)
        assert eq.all(), f"{name}: {(~eq).sum()} values differ from the model"
    assert (acc.spp_map() == model.spp_map()).all()
    assert bitwise_equal(acc.error_map(), model.to_pixels(model.tile_err)).all()


def _assert_pixels_equal_one_shot(t, acc, est, w, h, **bands):
    """every pixel equals the pixel of render(spp = its count), float32 and float64"""
    spp = acc.spp_map()
    for fp64 in (True, False):
        img = acc.image(fp64=fp64)
        for n in np.unique(spp):
            want = _render(t, est, w, h, int(n), fp64, **bands) if n else np.zeros_like(img)
            sel = spp == n
            assert bitwise_equal(img[sel], want[sel]).all(), f"pixels with {n} samples differ from render(spp={n})"


@pytest.mark.parametrize("est", list(SETUPS))
def test_progressive_equals_one_shot(gt, orc_vm, est):
    w, h = 20, 12
    try:
        _setup(gt, est)
        model = _model(gt, orc_vm, est, w, h)
        if est in M.ESTS:  # the model's samples are the oracle's
            try:
                orc_vm.set_hetero_fault(0)
                orc_vm.set_scene(default_scene())
                hc.set_cloud(orc_vm, *hc.MAIN)
                assert bitwise_equal(model.L, M.oracle_radiances(orc_vm, w, h, CAP, est)).all()
            finally:
                orc_vm.clear_density_grid()
        acc = gt.grid_accumulator(_cfg(est, w, h), chunk=C)
        try:
            assert (acc.tiles_x, acc.tiles_y, acc.chunk, acc.max_levels) == (3, 2, C, CAP // C)
            st = acc.state()  # empty: zeros and +inf
            assert not st["sum"].any() and not st["s1"].any() and not st["s2"].any() and not st["tile_levels"].any()
            assert not acc.image(fp64=True).any() and np.isposinf(st["tile_err"]).all()
            for levels in (1, 2, 3):
                acc.add(levels)
                model.add(levels)
                _assert_state(acc, model)
                if levels == 1:
                    assert bitwise_equal(acc.image(fp64=True), _render(gt, est, w, h, C)).all()
                    assert bitwise_equal(acc.image(), _render(gt, est, w, h, C, fp64=False)).all()
            assert (acc.spp_map() == CAP).all()
            assert bitwise_equal(acc.image(fp64=True), _render(gt, est, w, h, CAP)).all()
            assert bitwise_equal(acc.image(), _render(gt, est, w, h, CAP, fp64=False)).all()
            assert bitwise_equal(acc.image(fp64=True), model.image()).all()
            with pytest.raises(VPTError) as ei:  # the cap is reached
                acc.add(1)
            assert ei.value.code == _lib.VPT_E_INVALID
            _assert_state(acc, model)
            # the inputs: a lit image with noise in it
            assert 2 * np.count_nonzero(model.sum.any(axis=-1)) >= w * h and (model.s2 > 0).any()
        finally:
            acc.close()
    finally:
        _reset(gt)


@pytest.mark.parametrize("est,config", INSTANTIATIONS, ids=[f"{e}-{'-'.join(map(str, c))}" for e, c in INSTANTIATIONS])
def test_every_instantiation(gt, est, config):
    """every kernel of every unit: the lookups, the majorant grid or none, the emission grid"""
    w, h = 20, 12
    try:
        _setup(gt, est, config)
        acc = gt.grid_accumulator(_cfg(est, w, h), chunk=C)
        try:
            acc.add(2)
            want = _render(gt, est, w, h, 2 * C, config=config)
            assert bitwise_equal(acc.image(fp64=True), want).all()
            assert (acc.state()["tile_levels"] == 2).all() and np.isfinite(acc.state()["tile_err"]).all()
            assert 2 * np.count_nonzero(want.any(axis=-1)) >= w * h
        finally:
            acc.close()
    finally:
        _reset(gt)


@pytest.mark.parametrize("est", ["hetero", "hetero_mis"])
def test_tile_subsets(gt, orc_vm, est):
    w, h = 40, 24
    try:
        _setup(gt, est)
        model = _model(gt, orc_vm, est, w, h)
        acc = gt.grid_accumulator(_cfg(est, w, h), chunk=C)
        try:
            assert acc.tiles == 15
            acc.add(1)
            acc.add(2, tiles=[13, 2, 7])  # unsorted on purpose
            model.add(1)
            model.add(2, tiles=[13, 2, 7])
            want = np.full(15, C)
            want[[2, 7, 13]] = 3 * C
            assert (acc.spp_map() == model.to_pixels(want)).all()
            _assert_state(acc, model)
            _assert_pixels_equal_one_shot(gt, acc, est, w, h)
            # refused calls render nothing: a duplicate, an index out of range, a tile that would pass the cap
            before = acc.state()
            for levels, tiles in ((1, [3, 5, 3]), (1, [0, 15]), (1, [-1]), (4, [0, 13]), (6, None), (0, [1])):
                with pytest.raises(VPTError) as ei:
                    acc.add(levels, tiles=tiles)
                assert ei.value.code == _lib.VPT_E_INVALID, (levels, tiles)
            after = acc.state()
            for k in before:
                assert bitwise_equal(before[k], after[k]).all(), k
            # tiles that stand at different level counts in one call: one launch serves both
            acc.add(1)
            model.add(1)
            acc.add(2, tiles=[14, 13, 0])
            model.add(2, tiles=[14, 13, 0])
            assert len(np.unique(model.levels)) == 3
            _assert_state(acc, model)
            _assert_pixels_equal_one_shot(gt, acc, est, w, h)
        finally:
            acc.close()
    finally:
        _reset(gt)


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_adaptive_refine(gt, orc_vm, est):
    w, h, cap_levels = 40, 24, 6
    try:
        _setup(gt, est)
        model = _model(gt, orc_vm, est, w, h)
        sets = model.refine(M.REFINE_TARGET, min_levels=2, levels_per_pass=1)
        # the model alone first, so the test cannot pass vacuously: some tiles stop early, some reach the cap
        assert list(model.levels) == M.REFINE_LEVELS[est]
        assert (model.levels < cap_levels).sum() >= 2 and (model.levels == cap_levels).sum() >= 2
        acc = gt.grid_accumulator(_cfg(est, w, h), chunk=C)
        try:
            assert acc.max_levels == cap_levels
            rep = acc.refine(M.REFINE_TARGET, min_levels=2, levels_per_pass=1)
            _assert_state(acc, model)
            assert bitwise_equal(acc.image(fp64=True), model.image()).all()
            _assert_pixels_equal_one_shot(gt, acc, est, w, h)
            assert rep["passes"] == len(sets)
            assert rep["samples"] == int(model.spp_map().sum())
            capped = int((model.tile_err > M.REFINE_TARGET).sum())
            assert (rep["tiles_capped"], rep["tiles_converged"]) == (capped, 15 - capped)
            assert rep["max_err"] == model.tile_err.max()
            # nothing is active any more: a second call renders nothing
            again = acc.refine(M.REFINE_TARGET, min_levels=2, levels_per_pass=1)
            assert again["passes"] == 0 and again["samples"] == 0
            _assert_state(acc, model)
        finally:
            acc.close()
    finally:
        _reset(gt)


def test_levels_per_pass_and_floor(gt, orc_vm):
    """several levels per pass (clipped at the cap) after a plain add, and another luminance floor"""
    w, h, est = 40, 24, "hetero"
    try:
        _setup(gt, est)
        model = _model(gt, orc_vm, est, w, h)
        acc = gt.grid_accumulator(_cfg(est, w, h), chunk=C)
        try:
            acc.add(2)
            model.add(2)
            rep = acc.refine(M.FLOOR_TARGET, lum_floor=1.0, min_levels=2, levels_per_pass=3)
            sets = model.refine(M.FLOOR_TARGET, lum_floor=1.0, min_levels=2, levels_per_pass=3)
            # on the model: one pass of 3 levels for every tile, a second for some, clipped to 1 level at the cap
            assert list(model.levels) == M.FLOOR_LEVELS and [len(s) for s in sets] == M.FLOOR_SETS
            assert rep["passes"] == 2
            _assert_state(acc, model)
            _assert_pixels_equal_one_shot(gt, acc, est, w, h)
        finally:
            acc.close()
    finally:
        _reset(gt)


def test_banded_shard(gt, orc_vm):
    w, h, est = 20, 12, "hetero_ratio"
    bands = dict(band_rows=4, band_stride=2, band_offset=1)
    try:
        _setup(gt, est)
        model = _model(gt, orc_vm, est, w, h, bands=(4, 2, 1))
        acc = gt.grid_accumulator(_cfg(est, w, h, **bands), chunk=C)
        try:
            assert acc.rows == 4 and (acc.tiles_x, acc.tiles_y) == (3, 1)
            for levels in (1, 2, 3):
                acc.add(levels)
                model.add(levels)
                _assert_state(acc, model)
                if levels == 1:
                    assert bitwise_equal(acc.image(fp64=True), _render(gt, est, w, h, C, **bands)).all()
            assert bitwise_equal(acc.image(fp64=True), _render(gt, est, w, h, CAP, **bands)).all()
            assert bitwise_equal(acc.image(), _render(gt, est, w, h, CAP, fp64=False, **bands)).all()
            # the shard is the file rows 4 .. 7 of the whole image's render
            assert bitwise_equal(acc.image(fp64=True), _render(gt, est, w, h, CAP)[4:8]).all()
        finally:
            acc.close()
    finally:
        _reset(gt)


def _code(call):
    with pytest.raises(VPTError) as ei:
        call()
    return ei.value.code


def test_refusals(gt):
    w, h = 20, 12
    try:
        _reset(gt)
        # without a grid: the render's status
        assert _code(lambda: gt.grid_accumulator(_cfg("hetero", w, h), chunk=C)) == _code(lambda: gt.render(_cfg("hetero", w, h)))
        _setup(gt, "hetero")
        # estimators 0-5 are vpt_accum_create's
        assert _code(lambda: gt.grid_accumulator(RenderConfig(width=w, height=h, spp=CAP, estimator="ff"), chunk=C)) == _lib.VPT_E_INVALID
        # the cap is no multiple of the chunk
        assert _code(lambda: gt.grid_accumulator(_cfg("hetero", w, h, spp=22), chunk=C)) == _lib.VPT_E_INVALID
        assert _code(lambda: gt.grid_accumulator(_cfg("hetero", w, h, spp=40))) == _lib.VPT_E_INVALID  # auto chunk 32
        # vpt_accum_create still refuses the grid estimators
        assert _code(lambda: gt.accumulator(_cfg("hetero", w, h), chunk=C)) == _lib.VPT_E_UNSUPPORTED
        # an emission grid under estimator 12 (MAIN has one)
        assert _code(lambda: gt.grid_accumulator(_cfg("hetero_equiangular", w, h), chunk=C)) == _lib.VPT_E_UNSUPPORTED
        # estimator 15 without a majorant block
        _setup(gt, "hetero_residual", (0, "nearest"))
        assert _code(lambda: gt.grid_accumulator(_cfg("hetero_residual", w, h), chunk=C)) == _lib.VPT_E_INVALID
        # every pass validates again: without the grid an add fails as the render does and changes nothing
        _setup(gt, "hetero")
        acc = gt.grid_accumulator(_cfg("hetero", w, h), chunk=C)
        try:
            assert (acc.chunk, acc.max_levels) == (C, CAP // C)
            acc.add(2, tiles=[1, 4])
            before = acc.state()
            gt.clear_density_grid()
            want = _code(lambda: gt.render(_cfg("hetero", w, h)))
            assert _code(lambda: acc.add(1)) == want
            assert _code(lambda: acc.refine(0.5, min_levels=2)) == want
            after = acc.state()
            for k in before:
                assert bitwise_equal(before[k], after[k]).all(), k
            assert list(after["tile_levels"]) == [0, 2, 0, 0, 2, 0]
        finally:
            acc.close()
    finally:
        _reset(gt)
