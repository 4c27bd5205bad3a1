"""Progressive accumulator on the GPU (vpt_accum_*, Tracer.accumulator): every value against the one-shot
render and the CPU model (tests/accum_model.py), bit for bit.  Shapes are small and awkward on purpose: 20x12 and
40x24 have padded tiles on the right edge, 20x12 on the bottom edge too; chunk 4, cap 24 spp."""
import os
import subprocess

import numpy as np
import pytest

import accum_model as am
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import RenderConfig, VPTError, _lib, default_scene, encode_ppm
from scenes import SCENES

pytestmark = pytest.mark.gpu

C, CAP, SEED = 4, 24, 11
ESTS = {"ff": (0, {}), "mis": (1, {"hg_g": 0.5}), "surface_pt": (5, {})}

# the adaptive test's target, chosen on the CPU model alone (40x24, default scene, seed 11, chunk 4, cap 6 levels,
# min_levels 2, one level per pass), and the level counts the model reaches with it
REFINE_TARGET = 0.96875
REFINE_LEVELS = {
    "ff": [4, 6, 6, 6, 3, 6, 6, 5, 5, 6, 4, 6, 5, 4, 3],
    "mis": [3, 5, 3, 5, 3, 3, 6, 5, 3, 3, 3, 6, 4, 4, 5],
}

_RENDERS = {}


def _cfg(w, h, est, spp=CAP, fp64=True, **bands):
    return RenderConfig(width=w, height=h, spp=spp, estimator=est, seed=SEED, fp64=fp64, chunk_spp=C, **ESTS[est][1], **bands)


def _render(tracer, w, h, est, spp, fp64=True, **bands):
    """one-shot renders, computed once and shared (read-only)"""
    key = (w, h, est, spp, fp64, tuple(sorted(bands.items())))
    if key not in _RENDERS:
        img = tracer.render(_cfg(w, h, est, spp, fp64, **bands))
        img.setflags(write=False)
        _RENDERS[key] = img
    return _RENDERS[key]


def _model(orc_vm, w, h, est, levels=CAP // C, bands=(0, 1, 0)):
    e, kw = ESTS[est]
    cs = am.cached_chunk_sums(orc_vm, "default", SCENES["default"](), w, h, C, levels, e, SEED, bands=bands, **kw)
    return am.AccumModel(cs, C)


def _assert_state(acc, model):
    st = acc.state()
    assert (st["tile_levels"] == model.levels).all()
    for name, want in (("sum", model.sum), ("s1", model.s1), ("s2", model.s2), ("tile_err", model.tile_err)):
        eq = bitwise_equal(st[name], want)
        assert eq.all(), f"{name}: {(~eq).sum()} values differ from the model"
    assert (acc.spp_map() == model.spp_map()).all()
    assert bitwise_equal(acc.error_map(), model.to_pixels(model.tile_err)).all()


def _assert_pixels_equal_one_shot(tracer, acc, w, h, est, **bands):
    """every pixel equals the pixel of render(spp = its count), float32 and float64"""
    spp = acc.spp_map()
    for fp64 in (True, False):
        img = acc.image(fp64=fp64)
        for n in np.unique(spp):
            want = _render(tracer, w, h, est, int(n), fp64, **bands) if n else np.zeros_like(img)
            sel = spp == n
            assert bitwise_equal(img[sel], want[sel]).all(), f"pixels with {n} samples differ from render(spp={n})"


@pytest.mark.parametrize("est", list(ESTS))
def test_progressive_equals_one_shot(gpu_tracer, orc_vm, est):
    w, h = 20, 12
    gpu_tracer.set_scene(SCENES["default"]())
    model = _model(orc_vm, w, h, est)
    acc = gpu_tracer.accumulator(_cfg(w, h, est))
    try:
        assert (acc.tiles_x, acc.tiles_y, acc.chunk, acc.max_levels) == (3, 2, C, CAP // C)
        assert not acc.image(fp64=True).any() and np.isposinf(acc.state()["tile_err"]).all()  # empty: zeros
        for levels in (1, 2, 3):
            acc.add(levels)
            model.add(levels)
            _assert_state(acc, model)
            if levels == 1:
                assert bitwise_equal(acc.image(fp64=True), _render(gpu_tracer, w, h, est, C)).all()
                assert bitwise_equal(acc.image(), _render(gpu_tracer, w, h, est, C, fp64=False)).all()
        assert (acc.spp_map() == CAP).all()
        assert bitwise_equal(acc.image(fp64=True), _render(gpu_tracer, w, h, est, CAP)).all()
        assert bitwise_equal(acc.image(), _render(gpu_tracer, w, h, est, CAP, fp64=False)).all()
        assert bitwise_equal(acc.image(fp64=True), model.image()).all()
        with pytest.raises(VPTError) as ei:  # the cap is reached
            acc.add(1)
        assert ei.value.code == _lib.VPT_E_INVALID
    finally:
        acc.close()


def test_banded_shard(gpu_tracer, orc_vm):
    w, h, est = 20, 12, "ff"
    bands = dict(band_rows=4, band_stride=2, band_offset=1)
    gpu_tracer.set_scene(SCENES["default"]())
    model = _model(orc_vm, w, h, est, bands=(4, 2, 1))
    acc = gpu_tracer.accumulator(_cfg(w, h, est, **bands))
    try:
        assert acc.rows == 4 and (acc.tiles_x, acc.tiles_y) == (3, 1)
        for levels in (1, 2, 3):
            acc.add(levels)
            model.add(levels)
            _assert_state(acc, model)
            if levels == 1:
                assert bitwise_equal(acc.image(fp64=True), _render(gpu_tracer, w, h, est, C, **bands)).all()
        assert bitwise_equal(acc.image(fp64=True), _render(gpu_tracer, w, h, est, CAP, **bands)).all()
        assert bitwise_equal(acc.image(), _render(gpu_tracer, w, h, est, CAP, fp64=False, **bands)).all()
    finally:
        acc.close()


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_tile_subsets(gpu_tracer, orc_vm, est):
    w, h = 40, 24
    gpu_tracer.set_scene(SCENES["default"]())
    model = _model(orc_vm, w, h, est)
    acc = gpu_tracer.accumulator(_cfg(w, h, est))
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
        _assert_pixels_equal_one_shot(gpu_tracer, acc, w, h, est)
        # refused calls render nothing: a duplicate, an index out of range, a tile that would pass the cap
        before = acc.state()
        for levels, tiles in ((1, [3, 5, 3]), (1, [0, 15]), (1, [-1]), (4, [0, 13]), (6, None), (0, [1])):
            with pytest.raises(VPTError) as ei:
                acc.add(levels, tiles=tiles)
            assert ei.value.code == _lib.VPT_E_INVALID, (levels, tiles)
        after = acc.state()
        for k in before:
            assert bitwise_equal(before[k], after[k]).all(), k
        # tiles that stand at different level counts in one call (two groups of one pass)
        acc.add(1)
        model.add(1)
        acc.add(2, tiles=[14, 13, 0])
        model.add(2, tiles=[14, 13, 0])
        _assert_state(acc, model)
        _assert_pixels_equal_one_shot(gpu_tracer, acc, w, h, est)
    finally:
        acc.close()


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_adaptive_refine(gpu_tracer, orc_vm, est):
    w, h, cap_levels = 40, 24, 6
    gpu_tracer.set_scene(SCENES["default"]())
    model = _model(orc_vm, w, h, est, levels=cap_levels)
    sets = model.refine(REFINE_TARGET, min_levels=2, levels_per_pass=1)
    # the model alone first, so the test cannot pass vacuously: some tiles stop early, some reach the cap
    assert list(model.levels) == REFINE_LEVELS[est]
    assert (model.levels < cap_levels).sum() >= 2 and (model.levels == cap_levels).sum() >= 2
    acc = gpu_tracer.accumulator(_cfg(w, h, est))
    try:
        assert acc.max_levels == cap_levels
        rep = acc.refine(REFINE_TARGET, min_levels=2, levels_per_pass=1)
        _assert_state(acc, model)
        assert bitwise_equal(acc.image(fp64=True), model.image()).all()
        _assert_pixels_equal_one_shot(gpu_tracer, acc, w, h, est)
        assert rep["passes"] == len(sets)
        assert rep["samples"] == int(model.spp_map().sum())
        capped = int((model.tile_err > REFINE_TARGET).sum())
        assert (rep["tiles_capped"], rep["tiles_converged"]) == (capped, 15 - capped)
        assert rep["max_err"] == model.tile_err.max()
        # nothing is active any more: a second call renders nothing
        again = acc.refine(REFINE_TARGET, min_levels=2, levels_per_pass=1)
        assert again["passes"] == 0 and again["samples"] == 0
        _assert_state(acc, model)
    finally:
        acc.close()


def test_refine_levels_per_pass_and_floor(gpu_tracer, orc_vm):
    """several levels per pass (clipped at the cap) after a plain add, and another luminance floor"""
    w, h, est = 40, 24, "ff"
    gpu_tracer.set_scene(SCENES["default"]())
    model = _model(orc_vm, w, h, est)
    acc = gpu_tracer.accumulator(_cfg(w, h, est))
    try:
        acc.add(2)
        model.add(2)
        rep = acc.refine(0.5, lum_floor=1.0, min_levels=2, levels_per_pass=3)
        sets = model.refine(0.5, lum_floor=1.0, min_levels=2, levels_per_pass=3)
        # on the model: tiles left at 2 levels, tiles at 5 (one pass of 3), tiles at 6 (a second pass, clipped to 1)
        assert list(model.levels) == [2, 2, 2, 6, 2, 5, 6, 6, 6, 2, 2, 6, 2, 2, 2] and [len(s) for s in sets] == [6, 5]
        assert rep["passes"] == 2
        _assert_state(acc, model)
        _assert_pixels_equal_one_shot(gpu_tracer, acc, w, h, est)
    finally:
        acc.close()


def test_tile_subsets_need_estimator_0_or_1(gpu_tracer):
    """the tile-list kernel exists for ff and mis; the others accumulate whole tile sets only"""
    gpu_tracer.set_scene(SCENES["default"]())
    acc = gpu_tracer.accumulator(_cfg(40, 24, "surface_pt"))
    try:
        acc.add(1)
        before = acc.state()
        with pytest.raises(VPTError) as ei:
            acc.add(1, tiles=[3, 4])
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        after = acc.state()
        for k in before:
            assert bitwise_equal(before[k], after[k]).all(), k
        acc.add(1, tiles=list(range(15)))  # every tile is the whole set again
        assert bitwise_equal(acc.image(fp64=True), _render(gpu_tracer, 40, 24, "surface_pt", 2 * C)).all()
    finally:
        acc.close()


def test_unsupported_and_invalid(gpu_tracer):
    gpu_tracer.set_scene(SCENES["default"]())
    with pytest.raises(VPTError) as ei:
        gpu_tracer.accumulator(RenderConfig(width=20, height=12, spp=24, estimator="ray_marching", chunk_spp=4))
    assert ei.value.code == _lib.VPT_E_UNSUPPORTED
    with pytest.raises(VPTError) as ei:
        gpu_tracer.accumulator(RenderConfig(width=20, height=12, spp=22, chunk_spp=4))
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        gpu_tracer.accumulator(RenderConfig(width=20, height=12, spp=40))  # auto chunk 32: 40 is no multiple
    assert ei.value.code == _lib.VPT_E_INVALID
    acc = gpu_tracer.accumulator(RenderConfig(width=20, height=12, spp=64))
    try:
        assert (acc.chunk, acc.max_levels) == (32, 2)
        for kw in (dict(target=-1.0), dict(target=float("nan")), dict(target=0.1, lum_floor=-1.0),
                   dict(target=0.1, min_levels=1), dict(target=0.1, levels_per_pass=0)):
            with pytest.raises(VPTError) as ei:
                acc.refine(**kw)
            assert ei.value.code == _lib.VPT_E_INVALID, kw
        assert not acc.state()["tile_levels"].any()
    finally:
        acc.close()


def test_cli_target_error(gpu_tracer, tmp_path):
    w, h = 40, 24
    out = str(tmp_path / "a.ppm")
    r = subprocess.run([_lib.CLI_PATH, "24", "--width", str(w), "--height", str(h), "--target-error", str(REFINE_TARGET),
                        "--min-spp", "8", "--chunk", "4", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    gpu_tracer.set_scene(default_scene())
    acc = gpu_tracer.accumulator(RenderConfig(width=w, height=h, spp=24), chunk=4)
    try:
        rep = acc.refine(REFINE_TARGET, min_levels=2, levels_per_pass=1)
        assert len(np.unique(acc.spp_map())) > 1  # an adaptive image, not a uniform one
        with open(out, "rb") as f:
            assert f.read() == encode_ppm(acc.image())
        line = [s for s in r.stderr.splitlines() if s.startswith("adaptive:")]
        assert len(line) == 1 and f"{rep['passes']} passes" in line[0] and f"{rep['tiles_capped']} capped" in line[0]
    finally:
        acc.close()
    # without the flag: the plain render's bytes, as before
    out2 = str(tmp_path / "b.ppm")
    r = subprocess.run([_lib.CLI_PATH, "4", "--width", str(w), "--height", str(h), "--out", out2], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    with open(out2, "rb") as f:
        assert f.read() == encode_ppm(gpu_tracer.render(RenderConfig(width=w, height=h, spp=4)))
    assert os.path.getsize(out2) > 0
