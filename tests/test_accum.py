"""Progressive accumulator, CPU side: the numpy model against the oracle's chunked render, and the two host
entry points of libvpt.so (vpt_accum_stat_host, vpt_accum_select_host: csrc/vpt_accum.h on host arrays)
against the model, bit for bit.  No GPU."""
import ctypes
from ctypes import byref

import numpy as np
import pytest

import accum_model as am
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import _lib
from scenes import SCENES

W, H, C, SEED = 20, 12, 4, 11
ESTS = {"ff": (0, {}), "mis": (1, {"hg_g": 0.5}), "surface_pt": (5, {})}


def _csum(orc_vm, est, levels=6):
    e, kw = ESTS[est]
    return am.cached_chunk_sums(orc_vm, "default", SCENES["default"](), W, H, C, levels, e, SEED, **kw)


@pytest.mark.parametrize("est", list(ESTS))
def test_model_equals_oracle_chunked_render(orc_vm, est):
    """the model's uniform image at k levels is the oracle's render of k C samples in chunks of C"""
    e, kw = ESTS[est]
    cs = _csum(orc_vm, est)
    orc_vm.set_scene(SCENES["default"]())
    m = am.AccumModel(cs, C)
    have = 0
    for k in (1, 3, 6):
        m.add(k - have)
        have = k
        ref = orc_vm.render(W, H, k * C, e, seed=SEED, chunk=C, **kw)
        assert bitwise_equal(m.image(), ref).all(), f"{est}: {k} levels"
        assert (m.spp_map() == k * C).all()


def _stat_host(csum, chunk, lum_floor=0.01):
    csum = np.ascontiguousarray(csum, dtype=np.float64)
    m, npix = csum.shape[0], csum.shape[1]
    s, s12, err = np.zeros((npix, 3)), np.zeros((npix, 2)), np.zeros(npix)
    rc = _lib.lib().vpt_accum_stat_host(csum.ctypes.data, m, npix, chunk, lum_floor, s.ctypes.data, s12.ctypes.data,
                                        err.ctypes.data)
    assert rc == 0, _lib.lib().vpt_last_error()
    return s, s12, err


@pytest.mark.parametrize("est", list(ESTS))
@pytest.mark.parametrize("m", [1, 2, 6])
def test_stat_host_equals_model_on_renders(orc_vm, est, m):
    cs = _csum(orc_vm, est)[:m].reshape(m, -1, 3)
    got, want = _stat_host(cs, C), am.stat(cs, C)
    for g, w_, name in zip(got, want, ("sum", "s12", "err")):
        assert bitwise_equal(g, w_).all(), name
    if m >= 2:
        assert np.isfinite(got[2]).all() and (got[2] > 0).any()


def test_stat_host_crafted_columns():
    # pixel 0: varying; 1: constant (var clamps to 0); 2: black (the floor); 3: one NaN chunk; 4: dim, below the floor
    cs = np.zeros((3, 5, 3))
    cs[:, 0] = [[1.0, 2.0, 3.0], [0.5, 0.25, 4.0], [3.0, 1.0, 0.125]]
    cs[:, 1] = [0.3, 0.7, 0.1]
    cs[1, 3] = [np.nan, 1.0, 1.0]
    cs[:, 4] = [[1e-3, 2e-3, 0.0], [3e-3, 0.0, 1e-3], [0.0, 1e-3, 2e-3]]
    s, s12, err = _stat_host(cs, C)
    ws, ws12, werr = am.stat(cs, C)
    assert bitwise_equal(s, ws).all() and bitwise_equal(s12, ws12).all() and bitwise_equal(err, werr).all()
    assert err[0] > 0 and err[1] == 0.0 and err[2] == 0.0 and err[4] > 0
    assert np.isnan(s12[3]).all() and err[3] == 0.0  # a NaN sum clamps var to 0 and fails the floor test
    # the dim pixel's error is relative to the floor C * lum_floor, not to its own mean
    _, _, e_lo = _stat_host(cs, C, 0.0)
    assert e_lo[4] > err[4] and np.isnan(e_lo[2])  # black pixel without a floor: 0 / 0
    # m = 1: no variance yet
    _, _, e1 = _stat_host(cs[:1], C)
    assert np.isposinf(e1).all()
    # m = 0: the empty state
    s0, s120, e0 = _stat_host(cs[:0], C)
    assert not s0.any() and not s120.any() and np.isposinf(e0).all()


def _select_host(levels, err, target, min_levels, max_levels, lum_floor=0.01, lpp=1):
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    er = np.ascontiguousarray(err, dtype=np.float64)
    out = np.full(len(lv), -1, dtype=np.int32)
    r = _lib.vpt_refine(target, lum_floor, min_levels, lpp)
    n = _lib.lib().vpt_accum_select_host(lv.ctypes.data, er.ctypes.data, len(lv), byref(r), max_levels, out.ctypes.data)
    return n, out


def test_select_host_policy():
    target, min_levels, max_levels = 0.125, 3, 6
    #          below min   at cap       == target    NaN       above      below      cap, converged  fresh
    levels = [2,           6,           4,           4,        5,         3,         6,              0]
    err = [0.0,            1.0,         0.125,       np.nan,   0.126,     0.124,     0.01,           np.inf]
    n, out = _select_host(levels, err, target, min_levels, max_levels)
    want = am.active(levels, err, target, min_levels, max_levels)
    assert want == [0, 4, 7]
    assert n == len(want) and list(out[:n]) == want and (out[n:] == -1).all()
    # a NaN below min_levels is still active; at min_levels it is not
    n, out = _select_host([2, 3], [np.nan, np.nan], target, min_levels, max_levels)
    assert n == 1 and out[0] == 0
    # random arrays against the model
    rng = np.random.default_rng(5)
    lv = rng.integers(0, 8, 200)
    er = rng.choice([0.0, 0.05, 0.125, 0.2, np.inf, np.nan], 200)
    n, out = _select_host(lv, er, target, 2, 7)
    assert list(out[:n]) == am.active(lv, er, target, 2, 7)
    assert _select_host([], [], target, 2, 7)[0] == 0


def test_host_entry_points_validate():
    L = _lib.lib()
    a = np.zeros((2, 3, 3))
    out = np.zeros(9)
    bad = _lib.VPT_E_INVALID
    assert L.vpt_accum_stat_host(None, 2, 3, 4, 0.01, out.ctypes.data, None, None) == bad
    assert L.vpt_accum_stat_host(a.ctypes.data, -1, 3, 4, 0.01, out.ctypes.data, None, None) == bad
    assert L.vpt_accum_stat_host(a.ctypes.data, 2, -3, 4, 0.01, out.ctypes.data, None, None) == bad
    assert L.vpt_accum_stat_host(a.ctypes.data, 2, 3, 0, 0.01, out.ctypes.data, None, None) == bad
    for lf in (-0.5, np.nan, np.inf):
        assert L.vpt_accum_stat_host(a.ctypes.data, 2, 3, 4, lf, out.ctypes.data, None, None) == bad
    assert b"lum_floor" in L.vpt_last_error()
    assert L.vpt_accum_stat_host(a.ctypes.data, 2, 3, 4, 0.01, None, None, None) == 0  # every output is optional
    lv, er, act = np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2, dtype=np.int32)
    ok = _lib.vpt_refine(0.1, 0.01, 2, 1)
    args = (lv.ctypes.data, er.ctypes.data, 2)
    assert L.vpt_accum_select_host(*args, byref(ok), 4, act.ctypes.data) == 2
    assert L.vpt_accum_select_host(None, er.ctypes.data, 2, byref(ok), 4, act.ctypes.data) == bad
    assert L.vpt_accum_select_host(lv.ctypes.data, None, 2, byref(ok), 4, act.ctypes.data) == bad
    assert L.vpt_accum_select_host(*args, None, 4, act.ctypes.data) == bad
    assert L.vpt_accum_select_host(*args, byref(ok), 4, None) == bad
    assert L.vpt_accum_select_host(lv.ctypes.data, er.ctypes.data, -1, byref(ok), 4, act.ctypes.data) == bad
    for r in (_lib.vpt_refine(-0.1, 0.01, 2, 1), _lib.vpt_refine(np.nan, 0.01, 2, 1), _lib.vpt_refine(np.inf, 0.01, 2, 1),
              _lib.vpt_refine(0.1, -1.0, 2, 1), _lib.vpt_refine(0.1, np.nan, 2, 1), _lib.vpt_refine(0.1, 0.01, 1, 1),
              _lib.vpt_refine(0.1, 0.01, 2, 0)):
        assert L.vpt_accum_select_host(*args, byref(r), 4, act.ctypes.data) == bad


def test_accum_struct_layouts():
    assert ctypes.sizeof(_lib.vpt_refine) == 24
    assert ctypes.sizeof(_lib.vpt_refine_report) == 32
    assert _lib.vpt_refine_report.samples.offset == 16 and _lib.vpt_refine_report.max_err.offset == 24
    assert _lib.lib().vpt_abi_version() == 3
