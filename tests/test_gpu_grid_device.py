"""Grids from device memory on the GPU (Tracer.set_density_grid / set_emission_grid with a torch tensor on the tracer's GPU;
vpt_set_density_grid_device, vpt_set_emission_grid_device, csrc/vpt_grid_build.hip): the device builder against the host's
scatter build bit for bit, the check kernel's verdicts and messages against the host's, renders, the grid accumulator and
the emission probe on a device-set grid against the same from a numpy-set grid, and the semantics of the copy.
Shapes are small: at most 65 x 33 x 17 voxels, 16 x 12 x 8 spp images on the 6 x 5 x 4 cloud."""
import numpy as np
import pytest
import torch

import emission_model as em
import grid_model as gm
import test_gpu_hetero as T
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import (MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_emission_probe_host,
                                                grid_majorant_scatter_host)
from scenes import default_scene

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
W, H, SPP, SEED = 16, 12, 8, 5
RGB = (0.9, 0.5, 0.25)
LO, HI = T.ROOM_LO, T.ROOM_HI
SHAPES = [(1, 1, 1), (7, 5, 3), (70, 9, 5), (65, 33, 17)]  # (nx, ny, nz)
BLOCKS = (1, 2, 3, 8, 100)
INTERPS = ("nearest", "trilinear")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dt():
    """a tracer of this module's own: its grids and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cfg(est="hetero", fp64=True, spp=SPP):
    return RenderConfig(width=W, height=H, spp=spp, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_majorants(t, want, what):
    gmax, gmin, rho_max = t.grid_majorants()
    assert gmax.shape == want[0].shape, what
    assert np.array_equal(_bits(gmax), _bits(want[0])), f"maxima: {what}"
    assert np.array_equal(_bits(gmin), _bits(want[1])), f"minima: {what}"
    assert np.float64(rho_max).view(np.uint64) == np.float64(want[2]).view(np.uint64), f"rho_max: {what}"


def _fields(shape):
    """a random field with a quarter of its voxels zero, and one of zeros of both signs and repeated values"""
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * 1000 + ny * 10 + nz)
    a = (rng.uniform(0.1, 3.0, (nz, ny, nx)) * (rng.uniform(0, 1, (nz, ny, nx)) > 0.25)).astype(np.float32)
    b = rng.choice(np.array([0.0, -0.0, 0.5, 1.25, 2.0, -0.0], dtype=np.float32), size=(nz, ny, nx))
    return a, b


@pytest.mark.parametrize("shape", SHAPES)
def test_builder_bit_for_bit(dt, shape):
    for f in _fields(shape):
        d = _gpu(f)
        dt.set_density_grid(d, LO, HI)
        for block in BLOCKS:
            for interp in INTERPS:
                want = grid_majorant_scatter_host(f, block, interp)
                what = f"{shape}, B {block}, {interp}"
                # the rebuilds of a device-set grid: no voxel crosses to the host
                dt.set_majorant_block(block)
                dt.set_grid_interpolation(interp)
                _assert_majorants(dt, want, "rebuilt: " + what)
                # a set with the block and the mode in force
                dt.set_density_grid(d, LO, HI)
                _assert_majorants(dt, want, "set: " + what)
                # and the same field from numpy
                dt.set_density_grid(f, LO, HI)
                _assert_majorants(dt, want, "numpy: " + what)
                dt.set_density_grid(d, LO, HI, majorant_block=block, interpolation=interp)
    dt.set_majorant_block(0)
    assert dt.grid_majorants()[:2] == (None, None)
    dt.set_grid_interpolation("nearest")


def _message(call):
    with pytest.raises(VPTError) as ei:
        call()
    assert ei.value.code == _lib.VPT_E_INVALID
    return str(ei.value)


def test_validation(dt):
    nx, ny, nz = 65, 33, 17
    nv = nx * ny * nz
    rho, eps = (np.random.default_rng(3).uniform(0.0, 2.0, (2, nz, ny, nx))).astype(np.float32)
    small_rho, small_eps = em.fields()
    dt.set_majorant_block(2)
    dt.set_density_grid(_gpu(small_rho), LO, HI, emission=_gpu(small_eps * np.float32(40.0)), emission_rgb=RGB)
    before = dt.render(_cfg())
    for value in (np.nan, -1.0, np.inf):
        for at in (0, nv // 2 + 7, nv - 1):
            bad = rho.copy()
            bad.reshape(-1)[at] = value
            got = _message(lambda: dt.set_density_grid(_gpu(bad), LO, HI))
            want = _message(lambda: dt.set_density_grid(bad, LO, HI))
            assert got == want.replace("vpt_set_density_grid:", "vpt_set_density_grid_device:") and "_device" in got
            assert bitwise_equal(dt.render(_cfg()), before).all()  # the previous grid and its emission are intact
    for lo, hi, shape in ((LO, LO, (2, 2, 2)), ((0, 0, np.nan), HI, (2, 2, 2))):
        got = _message(lambda: dt.set_density_grid(torch.ones(shape, device=DEV), lo, hi))
        want = _message(lambda: dt.set_density_grid(np.ones(shape, np.float32), lo, hi))
        assert got == want.replace("vpt_set_density_grid:", "vpt_set_density_grid_device:")
        assert bitwise_equal(dt.render(_cfg()), before).all()
    # -0.0 is a valid density, and the maximum in the last voxel is found
    ok = rho.copy()
    ok.reshape(-1)[5] = -0.0
    ok.reshape(-1)[nv - 1] = 7.5
    dt.set_density_grid(_gpu(ok), LO, HI)
    assert dt.grid_majorants()[2] == 7.5
    # emission: the lowest bad voxel and its value
    for value in (np.nan, -1.0, np.inf):
        bad = eps.copy()
        bad.reshape(-1)[[nv // 3, nv - 2]] = value, -3.0
        got = _message(lambda: dt.set_emission_grid(_gpu(bad), RGB))
        want = _message(lambda: dt.set_emission_grid(bad, RGB))
        assert got == want.replace("vpt_set_emission_grid:", "vpt_set_emission_grid_device:")
        assert f"at voxel {nv // 3} " in got
    got = _message(lambda: dt.set_emission_grid(_gpu(eps), (1.0, -2.0, 1.0)))
    assert got == _message(lambda: dt.set_emission_grid(eps, (1.0, -2.0, 1.0))).replace("grid:", "grid_device:")
    dt.set_emission_grid(_gpu(eps), RGB)
    dt.set_majorant_block(0)


# estimator: (blocks, emission, medium colour)
E2E = {
    "hetero": ((0, 2), True, False), "hetero_ratio": ((0, 2), True, False), "hetero_equiangular": ((0, 2), False, False),
    "hetero_mis": ((0, 2), False, False), "hetero_chromatic": ((0, 2), False, True), "hetero_residual": ((2,), False, False),
    "hetero_spectral": ((0, 2), False, True),
}
E2E_CASES = [(est, block, interp) for est, (blocks, _, _) in E2E.items() for block in blocks for interp in INTERPS]


def _set_cloud(t, est, block, interp, on_gpu):
    rho, eps = em.fields()
    eps = eps * np.float32(40.0)
    _, emission, colour = E2E[est]
    wrap = _gpu if on_gpu else (lambda a: a)
    if colour:
        t.set_medium_colour((1.0, 0.6, 0.3), (0.8, 1.0, 0.5))
    else:
        t.set_medium_colour()
    t.set_density_grid(wrap(rho), LO, HI, majorant_block=block, interpolation=interp,
                       emission=wrap(eps) if emission else None, emission_rgb=RGB)


@pytest.mark.parametrize("est,block,interp", E2E_CASES)
def test_renders_equal_the_numpy_set_grid(dt, est, block, interp):
    try:
        _set_cloud(dt, est, block, interp, True)
        got = dt.render(_cfg(est))
        _set_cloud(dt, est, block, interp, False)
        want = dt.render(_cfg(est))
        assert bitwise_equal(got, want).all(), f"{(~bitwise_equal(got, want)).sum()} values differ"
        assert np.count_nonzero(want) > W * H  # a lit image
    finally:
        dt.set_medium_colour()
        dt.set_majorant_block(0)
        dt.set_grid_interpolation("nearest")


def test_grid_accumulator_and_emission_probe(dt):
    try:
        _set_cloud(dt, "hetero_ratio", 2, "trilinear", True)
        acc = dt.grid_accumulator(_cfg("hetero_ratio", spp=8), chunk=4)
        try:
            acc.add(1)
            acc.add(1)
            assert bitwise_equal(acc.image(fp64=True), dt.render(_cfg("hetero_ratio", spp=8))).all()
        finally:
            acc.close()
        rho, eps = em.fields()
        rays, tmax = em.rays()
        st = gm.states(7, len(rays))
        for block, interp in ((0, "nearest"), (2, "trilinear")):
            dt.set_density_grid(_gpu(rho), em.LO, em.HI, majorant_block=block, interpolation=interp, emission=_gpu(eps))
            got = dt.grid_emission_probe(0.7, rays, tmax, st)
            want = grid_emission_probe_host(rho, eps, em.LO, em.HI, 0.7, rays, tmax, st, majorant_block=block,
                                            interpolation=interp)
            for name, g, w in zip(("t_coll", "esum", "states", "steps"), got, want):
                assert bitwise_equal(g, w).all(), f"{name} (block {block}, {interp})"
            assert (want[1] > 0).sum() > 100
    finally:
        dt.set_majorant_block(0)
        dt.set_grid_interpolation("nearest")


class _ElsewhereTensor:
    """what Tracer looks at of a tensor, for one that lies on another GPU"""
    is_cuda, ndim, shape = True, 3, (4, 5, 6)
    device = torch.device("cuda", 1)

    def data_ptr(self):
        raise AssertionError("a tensor on another device is refused before its memory is asked for")


def test_semantics(dt):
    rho, eps = em.fields()
    eps = eps * np.float32(40.0)
    try:
        dt.set_density_grid(rho, LO, HI, majorant_block=2, interpolation="trilinear", emission=eps, emission_rgb=RGB)
        want = dt.render(_cfg())
        # a copy, not a borrow: the source is overwritten and freed after the call
        d, e = _gpu(rho), _gpu(eps)
        dt.set_density_grid(d, LO, HI, emission=e, emission_rgb=RGB)
        d.fill_(9.0)
        e.zero_()
        torch.cuda.synchronize()
        del d, e
        torch.cuda.empty_cache()
        assert bitwise_equal(dt.render(_cfg()), want).all()
        # float64 and non-contiguous tensors are made float32 and contiguous on the device
        dt.set_density_grid(_gpu(rho.astype(np.float64)), LO, HI, emission=_gpu(eps.astype(np.float64)), emission_rgb=RGB)
        assert bitwise_equal(dt.render(_cfg()), want).all()
        swapped = _gpu(np.ascontiguousarray(rho.transpose(2, 0, 1))).permute(1, 2, 0)
        assert not swapped.is_contiguous() and tuple(swapped.shape) == rho.shape
        dt.set_density_grid(swapped, LO, HI, emission=_gpu(eps), emission_rgb=RGB)
        assert bitwise_equal(dt.render(_cfg()), want).all()
        # a 2-D tensor, an emission tensor of another shape, a tensor on another device: refused, nothing changes
        with pytest.raises(ValueError):
            dt.set_density_grid(_gpu(rho[0]), LO, HI)
        for call in (lambda: dt.set_emission_grid(_gpu(eps[:, :, :5]), RGB),
                     lambda: dt.set_density_grid(_gpu(rho), LO, HI, emission=_gpu(eps[1:])),
                     lambda: dt.set_density_grid(_ElsewhereTensor(), LO, HI),
                     lambda: dt.set_emission_grid(_ElsewhereTensor(), RGB)):
            _message(call)
            assert bitwise_equal(dt.render(_cfg()), want).all()
        # cleared, then set from the host: as ever
        dt.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            dt.render(_cfg())
        assert ei.value.code == _lib.VPT_E_INVALID
        with pytest.raises(VPTError) as ei:
            dt.set_emission_grid(_gpu(eps), RGB)
        assert ei.value.code == _lib.VPT_E_INVALID and "density grid" in str(ei.value)
        dt.set_density_grid(rho, LO, HI, emission=eps, emission_rgb=RGB)
        assert bitwise_equal(dt.render(_cfg()), want).all()
        _assert_majorants(dt, grid_majorant_scatter_host(rho, 2, "trilinear"), "host-set after a clear")
    finally:
        dt.set_majorant_block(0)
        dt.set_grid_interpolation("nearest")


def test_multi_tracer_refuses_a_gpu_tensor():
    rho, eps = em.fields()
    m = MultiTracer(2, default_scene(), shared_device=True)
    try:
        for call in (lambda: m.set_density_grid(_gpu(rho), LO, HI), lambda: m.set_density_grid(rho, LO, HI, emission=_gpu(eps))):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED and "GPU tensor" in str(ei.value)
        m.set_density_grid(rho, LO, HI)
        with pytest.raises(VPTError) as ei:
            m.set_emission_grid(_gpu(eps), RGB)
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
    finally:
        m.close()
