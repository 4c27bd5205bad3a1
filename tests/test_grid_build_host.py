"""Grids from device memory, the part that needs no GPU: the block build stated per output (csrc/vpt_grid_build.h,
vpt_grid_majorant_gather_host) against the scatter build that vpt_set_density_grid runs (csrc/vpt_grid.h,
vpt_grid_majorant_scatter_host) bit for bit, the argument checks of the _device entry points, which come before any GPU
call, and the way a CPU tensor takes through Tracer.set_density_grid."""
import ctypes

import numpy as np
import pytest

import minimal_volumetric_path_tracer_amd as vpt
from minimal_volumetric_path_tracer_amd import _lib, tracer

BLOCKS = (1, 2, 3, 4, 7, 16)
INTERPS = ("nearest", "trilinear")
VALUES = np.array([0.0, -0.0, 0.5, 1.25, 2.0, 0.5, -0.0], dtype=np.float32)  # both zeros, repeated values


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_gather_is_scatter(field, block, interp):
    gmax, gmin, grho = vpt.grid_majorant_gather_host(field, block, interp)
    smax, smin, srho = vpt.grid_majorant_scatter_host(field, block, interp)
    what = f"{field.shape[::-1]}, B {block}, {interp}"
    assert _same(gmax, smax), f"maxima: {what}"
    assert _same(gmin, smin), f"minima: {what}"
    assert np.float64(grho).view(np.uint64) == np.float64(srho).view(np.uint64), f"rho_max: {what}"
    return gmax, gmin, grho


@pytest.mark.parametrize("nx", [1, 2, 3, 5, 9])
def test_gather_equals_scatter(nx):
    rng = np.random.default_rng(100 + nx)
    zero_minima = 0
    for ny in (1, 3, 4):
        for nz in (1, 2, 5):
            fields = [rng.choice(VALUES, size=(nz, ny, nx)),
                      rng.choice(VALUES[:2], size=(nz, ny, nx)),  # zeros of both signs only
                      rng.uniform(0.0, 3.0, (nz, ny, nx)).astype(np.float32)]
            for f in fields:
                for block in BLOCKS:
                    for interp in INTERPS:
                        _, gmin, _ = _assert_gather_is_scatter(f, block, interp)
                        zero_minima += int((gmin == 0).sum())
    assert zero_minima > 100  # the sign of a zero minimum was at stake


def test_the_earlier_of_two_zeros_stays():
    """the two-voxel blocks [+0.0, -0.0] and [-0.0, +0.0], along every axis: the minimum is the first voxel's zero, the
    maximum the +0.0 the scan starts from"""
    for first in (0.0, -0.0):
        pair = np.array([first, -first], dtype=np.float32)
        for axis in range(3):
            shape = [1, 1, 1]
            shape[axis] = 2
            f = pair.reshape(shape)
            for block in (2, 16):
                for interp in INTERPS:
                    gmax, gmin, rho_max = _assert_gather_is_scatter(f, block, interp)
                    assert gmin.shape == (1, 1, 1)
                    assert np.signbit(gmin[0, 0, 0]) == np.signbit(pair[0]) and gmin[0, 0, 0] == 0
                    assert not np.signbit(gmax[0, 0, 0]) and gmax[0, 0, 0] == 0
                    assert rho_max == 0 and not np.signbit(rho_max)


def test_rho_max_of_negative_zeros_is_positive_zero():
    f = np.full((2, 3, 5), -0.0, dtype=np.float32)
    for block in BLOCKS:
        for interp in INTERPS:
            gmax, gmin, rho_max = _assert_gather_is_scatter(f, block, interp)
            assert rho_max == 0 and not np.signbit(rho_max)
            assert not np.signbit(gmax).any() and np.signbit(gmin).all()


def test_probe_arguments():
    f = np.ones((2, 2, 2), np.float32)
    for fn in (vpt.grid_majorant_gather_host, vpt.grid_majorant_scatter_host):
        with pytest.raises(vpt.VPTError) as ei:
            fn(f, 0)
        assert ei.value.code == _lib.VPT_E_INVALID
        with pytest.raises(vpt.VPTError) as ei:
            fn(f, 2, "cubic")
        assert ei.value.code == _lib.VPT_E_INVALID
    L = vpt.lib()
    d = _lib.vpt_grid_desc()
    out, rho_max = np.zeros(2, np.float32), ctypes.c_double()
    assert L.vpt_grid_majorant_gather_host(ctypes.byref(d), f.ctypes.data, 0, 0, out.ctypes.data, ctypes.byref(rho_max)) \
        == _lib.VPT_E_INVALID  # block 0
    assert L.vpt_grid_majorant_gather_host(ctypes.byref(d), f.ctypes.data, 2, 0, out.ctypes.data, ctypes.byref(rho_max)) \
        == _lib.VPT_E_INVALID  # a grid of 0 x 0 x 0
    assert "each dimension >= 1" in L.vpt_last_error().decode()
    assert L.vpt_grid_majorant_gather_host(None, None, 2, 0, None, None) == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == "vpt_grid_majorant_gather_host: NULL grid"


# what each _device entry point says of NULL arguments, the context first: before any GPU call
DEVICE_NULLS = {
    "vpt_set_density_grid_device": "vpt_set_density_grid_device: NULL context",
    "vpt_set_emission_grid_device": "vpt_set_emission_grid_device: NULL context",
    "vpt_get_grid_majorants": "vpt_get_grid_majorants: NULL context",
}


@pytest.mark.parametrize("name", sorted(DEVICE_NULLS))
def test_device_entry_points_refuse_a_null_context(name):
    L = vpt.lib()
    fn = getattr(L, name)
    rc = fn(*[t() for t in fn.argtypes])  # every argument zero or NULL
    assert rc == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == DEVICE_NULLS[name]


def test_device_entry_points_refuse_null_arguments():
    """a context that is not NULL is not looked into before the other arguments are found missing"""
    L = vpt.lib()
    ctx = ctypes.c_void_p(0x1000)  # never dereferenced: the checks below come first
    d = _lib.vpt_grid_desc()
    rgb = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    assert L.vpt_set_density_grid_device(ctx, None, None, None) == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == "vpt_set_density_grid_device: NULL grid"
    assert L.vpt_set_density_grid_device(ctx, ctypes.byref(d), None, None) == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == "vpt_set_density_grid_device: NULL grid"
    assert L.vpt_set_emission_grid_device(ctx, None, rgb, None) == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == "vpt_set_emission_grid_device: NULL grid"
    assert L.vpt_get_grid_majorants(ctx, None, None, 0, None, None) == _lib.VPT_E_INVALID
    assert L.vpt_last_error().decode() == "vpt_get_grid_majorants: bad arguments"


class _Recorder:
    """stands in for libvpt.so: records the entry points Tracer calls and answers VPT_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return _lib.VPT_OK

        return fn


def test_cpu_tensor_takes_the_host_path(monkeypatch):
    import torch

    rec = _Recorder()
    monkeypatch.setattr(tracer, "lib", lambda: rec)
    t = tracer.Tracer.__new__(tracer.Tracer)  # no context: every call goes to the recorder
    t._ctx, t.device, t._majorant_block, t._grid_interpolation, t._grid_shape = ctypes.c_void_p(1), 0, 0, "nearest", None
    try:
        rho = torch.ones((4, 5, 6), dtype=torch.float64)
        assert not tracer._on_gpu(rho) and not tracer._on_gpu(np.ones(3)) and not tracer._on_gpu([[1.0]])
        t.set_density_grid(rho, (0, 0, 0), (1, 1, 1), emission=torch.ones((4, 5, 6)))
        assert rec.calls == ["vpt_set_density_grid", "vpt_set_emission_grid"]
        assert t._grid_shape == (4, 5, 6)
    finally:
        t._ctx = None  # nothing to destroy


def test_tracer_module_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT

    code = f"import sys; sys.path.insert(0, {ROOT!r}); import minimal_volumetric_path_tracer_amd; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
