"""Estimator 15 (VPT_HETERO_RESIDUAL: estimator 11 with every transmittance factor a residual ratio-tracking estimate
over the block minima) on the GPU: the residual probe against its host build bit for bit (control grid staged in LDS
and read from global memory), hetero_residual_kernel against render_kernel_simple_residual and the per-sample call, the
reduction to estimator 11 where the control grid is zero and to estimator 10 in vacuum, the expectation against
estimator 10's, the multi-tracer and the errors.  Shapes are those of tests/test_gpu_ratio.py: 4096 samples per batch,
24 x 20 x 8 spp images; the expectation test alone takes 2^20 samples per estimator."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_residual_probe_host
from scenes import big_light_scene, default_scene
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = T.W, T.H, T.SPP, T.SEED
CASES = ((1, "nearest"), (2, "nearest"), (1, "trilinear"), (2, "trilinear"))  # (majorant block, interpolation)
BIG_SHAPE = (20, 18, 16)  # 5760 super-voxels at block 1: more than the 5461 of which the LDS budget holds three arrays


@pytest.fixture(scope="module")
def rt():
    """a tracer of this module's own: its grid, block size and interpolation never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _cfg(est="hetero_residual", fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


def _zero_corner_field():
    """every block of B = 2 holds a zero voxel, under the trilinear dilation too: the control grid is zero"""
    f = mm.sparse_field()
    f[::2, ::2, ::2] = 0
    return f


def test_probe_equals_host_build(rt):
    """4096 rays through the sparse field on a density floor at block 1, 2 and 8 (nearest) and 2 (trilinear), two
    sigma_t: That, tauc, end state and draws bit for bit.  Those grids fit the LDS budget with their majorants and
    minima; the 16 x 18 x 20 field at block 1 does not (3 x 5760 floats), so its minima are read from global memory"""
    rho = mm.sparse_field() + np.float32(0.5)
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    big = mm.sparse_field(BIG_SHAPE) + np.float32(0.5)
    assert big.size > 5461 and 3 * big.size > 16384 >= 2 * big.size
    try:
        for field, b, interp in [(rho, 1, "nearest"), (rho, 2, "nearest"), (rho, 8, "nearest"), (rho, 2, "trilinear"),
                                 (big, 1, "nearest"), (big, 1, "trilinear")]:
            rt.set_density_grid(field, mm.SPARSE_LO, mm.SPARSE_HI, majorant_block=b, interpolation=interp)
            for sigma_t in (0.7, 0.05):
                got = rt.grid_residual_probe(sigma_t, rays, tmax, st)
                want = grid_residual_probe_host(field, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays, tmax, st, majorant_block=b,
                                                interpolation=interp)
                for name, g, w in zip(("That", "tauc", "states", "steps"), got, want):
                    assert bitwise_equal(g, w).all(), \
                        f"{name} ({field.shape}, block {b}, {interp}, sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
                assert ((want[0] >= 0) & (want[0] <= 1)).all() and (want[1] > 0).any() and (want[3] >= 1).all()
    finally:
        rt.set_grid_interpolation("nearest")
        rt.set_majorant_block(0)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_residual as R
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
out = {{}}
for k, (b, interp) in enumerate(R.CASES):
    t.set_density_grid(R.T._field(), R.ROOM_LO, R.ROOM_HI, majorant_block=b, interpolation=interp)
    out["img%d" % k] = t.render(R._cfg())
    out["work%d" % k] = np.array(t.count_work(R._cfg()), dtype=np.uint64)
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(rt, orc_vm, tmp_path):
    """hetero_residual_kernel against render_kernel_simple_residual (a fresh process with VPT_SIMPLE_KERNEL=1) and against
    the in-order per-pixel sum of the per-sample call, bitwise, fp64 and fp32, at block 1 and 2, nearest and trilinear;
    count_work (render_kernel_simple's counting mode in either process) is equal; the image is neither estimator 11's
    nor estimator 10's"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_residual_kernel"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    try:
        for k, (b, interp) in enumerate(CASES):
            what = f"block {b}, {interp}"
            rt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b, interpolation=interp)
            img = rt.render(_cfg())
            assert bitwise_equal(img, simple[f"img{k}"]).all(), f"{what}: {(~bitwise_equal(img, simple[f'img{k}'])).sum()} differ"
            L, _ = rt.trace("hetero_residual", rays.reshape(-1), st.reshape(-1), SA, SS)
            L = L.reshape(H, W, SPP, 3)
            acc = np.zeros((H, W, 3))
            for s in range(SPP):
                acc = L[:, :, s] + acc
            want = acc * (1 / float(SPP))
            assert bitwise_equal(img, want).all(), f"{what}: {(~bitwise_equal(img, want)).sum()} values differ from the sample sum"
            assert bitwise_equal(rt.render(_cfg(fp64=False)), want.astype(np.float32)).all()
            assert np.count_nonzero(img) > W * H
            work = rt.count_work(_cfg())
            assert work == tuple(int(v) for v in simple[f"work{k}"]) and work[0] > 0 and work[1] > 0
            assert not bitwise_equal(img, rt.render(_cfg("hetero_ratio"))).all()
            assert not bitwise_equal(img, rt.render(_cfg("hetero"))).all()
    finally:
        rt.set_grid_interpolation("nearest")
        rt.set_majorant_block(0)


@pytest.mark.parametrize("interp", ["nearest", "trilinear"])
def test_zero_control_is_estimator_11(rt, orc_vm, interp):
    """identity (i) in the renderer: on the field whose blocks of 2 all hold a zero voxel the control grid is zero and
    estimator 15 is estimator 11 bit for bit -- the 4096 samples (values and end states) and the render"""
    rays, st = T._batch(orc_vm)
    try:
        rt.set_density_grid(_zero_corner_field(), ROOM_LO, ROOM_HI, majorant_block=2, interpolation=interp)
        L11, s11 = rt.trace("hetero_ratio", rays, st, SA, SS)
        L15, s15 = rt.trace("hetero_residual", rays, st, SA, SS)
        assert (s11 == s15).all() and bitwise_equal(L11, L15).all()
        assert np.count_nonzero(L11.any(axis=1)) > 1000
        img = rt.render(_cfg())
        assert bitwise_equal(img, rt.render(_cfg("hetero_ratio"))).all() and np.count_nonzero(img) > W * H
    finally:
        rt.set_grid_interpolation("nearest")
        rt.set_majorant_block(0)


def test_vacuum_anchor(rt, orc_vm):
    """rho == 0 everywhere at block 2: no factor draws and every factor is exactly 1, so estimator 15 is estimator 10
    bit for bit -- the 4096 samples (values and end states) and the render"""
    rays, st = T._batch(orc_vm)
    rt.set_density_grid(np.zeros((2, 3, 2), np.float32), ROOM_LO, ROOM_HI, majorant_block=2)
    L10, s10 = rt.trace("hetero", rays, st, SA, SS)
    L15, s15 = rt.trace("hetero_residual", rays, st, SA, SS)
    assert (s10 == s15).all() and bitwise_equal(L10, L15).all()
    assert np.count_nonzero(L10.any(axis=1)) > 1000
    assert bitwise_equal(rt.render(_cfg()), rt.render(_cfg("hetero"))).all()
    rt.set_majorant_block(0)


def test_same_expectation_as_estimator_10():
    """tests/test_gpu_ratio.py's test_same_expectation_as_estimator_10 with estimator 15 at block 2 in estimator 11's
    place: N = 2^20 camera samples of a 32 x 32 image per estimator, independent jitters and streams, the 2 x 3 x 2
    field in the room box at sigma_t = 0.002 per unit density, so that no segment inside the box has a transmittance
    below T_min >= 0.4.  Every residual estimate is at most exp(-sigma_t tauc) <= 1 where estimator 10 has a factor
    >= T_min, so L15 <= L10 / T_min path by path and the derivation carries over unchanged:
        |m15 - m10| <= 4.5 sqrt((M2_10 - m10^2) / N + M2_10 / (T_min^2 N))
    from estimator 10's samples and the inputs alone.  The condition on the inputs (bound <= 5 % of m10) is asserted."""
    n_side, spp = 32, 1024
    sa, ss = 0.0002, 0.0018
    f = T._field()
    lo, hi = np.array(ROOM_LO), np.array(ROOM_HI)
    t_min = np.exp(-(sa + ss) * float(f.max()) * np.linalg.norm(hi - lo))
    assert t_min >= 0.4
    lum = np.array([0.2126, 0.7152, 0.0722])
    r10, s10 = _camera_batch(n_side, spp, 101)
    r15, s15 = _camera_batch(n_side, spp, 202)
    N = len(r10)
    assert N == 1 << 20
    t = Tracer(0, big_light_scene())
    try:
        t.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=2)
        l10 = t.trace("hetero", r10, s10, sa, ss)[0] @ lum
        l15 = t.trace("hetero_residual", r15, s15, sa, ss)[0] @ lum
    finally:
        t.close()
    assert np.isfinite(l10).all() and np.isfinite(l15).all()
    m10, m2_10, m15 = l10.mean(), (l10 * l10).mean(), l15.mean()
    bound = 4.5 * np.sqrt((m2_10 - m10 * m10) / N + m2_10 / (t_min * t_min * N))
    print(f"T_min = {t_min:.4f}, m10 = {m10:.6f}, m15 = {m15:.6f}, |m15 - m10| = {abs(m15 - m10):.3e}, bound = {bound:.3e} "
          f"({100 * bound / m10:.2f} % of m10), ratio {abs(m15 - m10) / bound:.3f}")
    assert m10 > 0 and bound <= 0.05 * m10  # the condition on the inputs
    assert abs(m15 - m10) <= bound


def test_multi_tracer_equals_single(rt):
    try:
        for b, interp in ((2, "nearest"), (1, "trilinear")):
            rt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b, interpolation=interp)
            img = rt.render(_cfg())
            m = MultiTracer(2, default_scene(), shared_device=True)
            try:
                with pytest.raises(VPTError) as ei:
                    m.render(_cfg())
                assert ei.value.code == _lib.VPT_E_INVALID  # no grid yet
                m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b, interpolation=interp)
                assert bitwise_equal(m.render(_cfg(band_rows=4)), img).all()
            finally:
                m.close()
    finally:
        rt.set_grid_interpolation("nearest")
        rt.set_majorant_block(0)


def test_errors():
    t = Tracer(0, default_scene())
    try:
        res = RenderConfig(width=8, height=8, spp=4, estimator="hetero_residual_ratio", seed=SEED, fp64=True)
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        calls = (lambda: t.render(res), lambda: t.trace("hetero_residual", rays, gm.states(1, 1)), lambda: t.count_work(res),
                 lambda: t.grid_residual_probe(1.0, rays, 1.0, gm.states(1, 1)))
        for call in calls:  # no grid
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        t.set_density_grid(T._field(), ROOM_LO, ROOM_HI)
        before = [t.render(RenderConfig(width=8, height=8, spp=4, estimator=e, seed=SEED, fp64=True))
                  for e in ("hetero", "hetero_ratio")]
        for call in calls:  # a grid, but block 0
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID and "vpt_set_grid_majorant_block" in str(ei.value)
        t.set_majorant_block(2)
        assert t.render(res).any()
        t.set_emission_grid(np.ones_like(T._field()))
        for call in calls[:3]:
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.clear_emission_grid()
        assert t.render(res).any()
        with pytest.raises(VPTError) as ei:
            t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator="hetero_residual"))
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.set_majorant_block(0)
        after = [t.render(RenderConfig(width=8, height=8, spp=4, estimator=e, seed=SEED, fp64=True))
                 for e in ("hetero", "hetero_ratio")]
        assert all(bitwise_equal(a, b).all() and a.any() for a, b in zip(before, after))
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(res)
        assert ei.value.code == _lib.VPT_E_INVALID
    finally:
        t.close()
