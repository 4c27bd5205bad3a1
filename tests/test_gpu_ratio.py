"""Estimator 11 (VPT_HETERO_RATIO: estimator 10 with every transmittance factor a ratio-tracking estimate) on the
GPU: the ratio probe against its host build bit for bit, hetero_ratio_kernel against render_kernel_simple_ratio and
the per-sample call, the vacuum anchor against estimator 10, resolution independence, the expectation against
estimator 10's, the multi-tracer and the errors.  Shapes are those of tests/test_gpu_hetero.py: 4096 samples per
batch, 24 x 20 x 8 spp images; the expectation test alone takes 2^20 samples per estimator."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_ratio_probe_host
from scenes import big_light_scene, default_scene

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = T.W, T.H, T.SPP, T.SEED
BLOCKS = (0, 2)


@pytest.fixture(scope="module")
def rt():
    """a tracer of this module's own: its grid and its block size never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _cfg(est="hetero_ratio", fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


def test_probe_equals_host_build(rt):
    """4096 rays through the sparse field at block 0, 1, 2 and 8: value, end state and draws bit for bit"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    for b in (0, 1, 2, 8):
        rt.set_density_grid(rho, mm.SPARSE_LO, mm.SPARSE_HI, majorant_block=b)
        for sigma_t in (0.7, 0.05):
            got = rt.grid_ratio_probe(sigma_t, rays, tmax, st)
            want = grid_ratio_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays, tmax, st, majorant_block=b)
            for name, g, w in zip(("That", "states", "steps"), got, want):
                assert bitwise_equal(g, w).all(), f"{name} (block {b}, sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
            assert ((want[0] >= 0) & (want[0] <= 1)).all() and (want[0] == 0).any() and (want[0] == 1).any()
    rt.set_majorant_block(0)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_ratio as R
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import big_light_scene, default_scene
t = Tracer(0, default_scene())
out = {{}}
for b in R.BLOCKS:
    t.set_density_grid(R.T._field(), R.ROOM_LO, R.ROOM_HI, majorant_block=b)
    out["img%d" % b] = t.render(R._cfg())
    out["work%d" % b] = np.array(t.count_work(R._cfg()), dtype=np.uint64)
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(rt, orc_vm, tmp_path):
    """hetero_ratio_kernel against render_kernel_simple_ratio (a fresh process with VPT_SIMPLE_KERNEL=1) and against the
    in-order per-pixel sum of the per-sample call, bitwise, at block 0 and 2; count_work (render_kernel_simple's
    counting mode in either process) is equal"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_ratio_kernel"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    imgs = {}
    for b in BLOCKS:
        rt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b)
        img = imgs[b] = rt.render(_cfg())
        assert bitwise_equal(img, simple[f"img{b}"]).all(), f"block {b}: {(~bitwise_equal(img, simple[f'img{b}'])).sum()} differ"
        L, _ = rt.trace("hetero_ratio", rays.reshape(-1), st.reshape(-1), SA, SS)
        L = L.reshape(H, W, SPP, 3)
        acc = np.zeros((H, W, 3))
        for s in range(SPP):
            acc = L[:, :, s] + acc
        want = acc * (1 / float(SPP))
        assert bitwise_equal(img, want).all(), f"block {b}: {(~bitwise_equal(img, want)).sum()} values differ from the sample sum"
        assert bitwise_equal(rt.render(_cfg(fp64=False)), want.astype(np.float32)).all()
        assert np.count_nonzero(img) > W * H
        work = rt.count_work(_cfg())
        assert work == tuple(int(v) for v in simple[f"work{b}"]) and work[0] > 0 and work[1] > 0
        # the estimator is not estimator 10 on this field
        assert not bitwise_equal(img, rt.render(_cfg("hetero"))).all()
    assert not bitwise_equal(imgs[0], imgs[2]).all()  # the block is felt
    rt.set_majorant_block(0)


@pytest.mark.parametrize("block", BLOCKS)
def test_vacuum_anchor(rt, orc_vm, block):
    """rho == 0 everywhere: no factor draws and every factor is exactly 1, so estimator 11 is estimator 10 bit for
    bit -- the 4096 samples (values and end states) and the render"""
    rays, st = T._batch(orc_vm)
    rt.set_density_grid(np.zeros((2, 3, 2), np.float32), ROOM_LO, ROOM_HI, majorant_block=block)
    L10, s10 = rt.trace("hetero", rays, st, SA, SS)
    L11, s11 = rt.trace("hetero_ratio", rays, st, SA, SS)
    assert (s10 == s11).all() and bitwise_equal(L10, L11).all()
    assert np.count_nonzero(L10.any(axis=1)) > 1000
    assert bitwise_equal(rt.render(_cfg()), rt.render(_cfg("hetero"))).all()
    rt.set_majorant_block(0)


def test_resolution_independence(rt, orc_vm):
    """block 0: the 2 x 3 x 2 field and its 4 x 6 x 4 resampling have the same majorant and the same density at every
    point, so the tentative points, the weights and the draws are the same: equal end states on all 4096 samples
    and radiances within the bound of tests/test_gpu_hetero.py's resampling test"""
    rays, st = T._batch(orc_vm)
    f = T._field()
    rt.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=0)
    La, sa = rt.trace("hetero_ratio", rays, st, SA, SS)
    rt.set_density_grid(mm.resample2(f), ROOM_LO, ROOM_HI)
    Lb, sb = rt.trace("hetero_ratio", rays, st, SA, SS)
    assert (sa == sb).all(), f"{(sa != sb).sum()} end states differ"
    ok = T._radiance_bound(La, Lb)
    print(f"max |La - Lb| = {np.abs(La - Lb).max():.3e}, max L = {La.max():.3e}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
    assert np.count_nonzero(La.any(axis=1)) > 1000  # (an estimate is an exact zero more often than exp(-tau) is small)
    # the field is felt: the uniform field of the same maximum gives other draws
    rt.set_density_grid(np.full((2, 3, 2), f.max(), np.float32), ROOM_LO, ROOM_HI)
    assert (rt.trace("hetero_ratio", rays, st, SA, SS)[1] != sa).any()


def _camera_batch(n_pix_side, spp, seed):
    """spp camera samples per pixel of an n x n image of the default camera (src/rt.cpp:755-759, 787), jitter and
    start states from numpy: (rays, states)"""
    rng = np.random.default_rng(seed)
    w = h = n_pix_side
    n = w * h * spp
    x = np.repeat(np.arange(w * h) % w, spp).astype(float)
    y = np.repeat(np.arange(w * h) // w, spp).astype(float)
    jx, jy = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    cd = np.array([0.0, -0.042612, -1.0])
    cd = cd / np.linalg.norm(cd)
    cx = np.array([w * 0.5095 / h, 0.0, 0.0])
    cy = np.cross(cx, cd)
    cy = cy / np.linalg.norm(cy) * 0.5095
    d = cx[None, :] * (((x + jx - 0.5) / w) - 0.5)[:, None] + cy[None, :] * (((y + jy - 0.5) / h) - 0.5)[:, None] + cd[None, :]
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"] = (0.0, 11.2, 214.0)
    rays["d"] = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return rays, rng.integers(0, 1 << 48, n, dtype=np.uint64)


def test_same_expectation_as_estimator_10():
    """N = 2^20 camera samples of a 32 x 32 image per estimator, independent jitters and streams, the 2 x 3 x 2 field
    in the room box at block 0 and at sigma_t = 0.002 per unit density, so that no segment inside the box has a
    transmittance below T_min = exp(-sigma_t rho_max |hi - lo|) >= 0.4.  Along any path every ratio estimate is at
    most 1 where estimator 10 has a factor >= T_min, so L11 <= L10 / T_min path by path and, the path law being the
    same, Var(L11) <= E[L11^2] <= M2_10 / T_min^2.  Hence
        |m11 - m10| <= 4.5 sqrt((M2_10 - m10^2) / N + M2_10 / (T_min^2 N))
    from estimator 10's samples and the inputs alone (4.5 standard deviations of the difference of the two means).
    A factor site that was missed, or taken over another segment, shifts the mean by the order of 1 - T.
    The scene is scenes.big_light_scene: the default scene (a point light and two spherical lights, so every factor
    site is reached) under an emissive ceiling, which keeps the per-sample luminance light-tailed enough for the
    condition on the inputs (bound <= 5 % of m10) at this N; on the default scene alone the point light's 1 / d^2
    puts the bound at 15.5 % of m10.  Measured: m10 = 1.14000, m11 = 1.14445, |m11 - m10| = 0.120 of the bound,
    the bound 3.25 % of m10."""
    n_side, spp = 32, 1024
    sa, ss = 0.0002, 0.0018
    f = T._field()
    lo, hi = np.array(ROOM_LO), np.array(ROOM_HI)
    t_min = np.exp(-(sa + ss) * float(f.max()) * np.linalg.norm(hi - lo))
    assert t_min >= 0.4
    lum = np.array([0.2126, 0.7152, 0.0722])
    r10, s10 = _camera_batch(n_side, spp, 101)
    r11, s11 = _camera_batch(n_side, spp, 202)
    N = len(r10)
    assert N == 1 << 20
    t = Tracer(0, big_light_scene())
    try:
        t.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=0)
        l10 = t.trace("hetero", r10, s10, sa, ss)[0] @ lum
        l11 = t.trace("hetero_ratio", r11, s11, sa, ss)[0] @ lum
    finally:
        t.close()
    assert np.isfinite(l10).all() and np.isfinite(l11).all()
    m10, m2_10, m11 = l10.mean(), (l10 * l10).mean(), l11.mean()
    bound = 4.5 * np.sqrt((m2_10 - m10 * m10) / N + m2_10 / (t_min * t_min * N))
    print(f"T_min = {t_min:.4f}, m10 = {m10:.6f}, m11 = {m11:.6f}, |m11 - m10| = {abs(m11 - m10):.3e}, bound = {bound:.3e} "
          f"({100 * bound / m10:.2f} % of m10), ratio {abs(m11 - m10) / bound:.3f}")
    assert m10 > 0 and bound <= 0.05 * m10  # the condition on the inputs
    assert abs(m11 - m10) <= bound


def test_multi_tracer_equals_single(rt):
    for b in BLOCKS:
        rt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b)
        img = rt.render(_cfg())
        m = MultiTracer(2, default_scene(), shared_device=True)
        try:
            with pytest.raises(VPTError) as ei:
                m.render(_cfg())
            assert ei.value.code == _lib.VPT_E_INVALID  # no grid yet
            m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=b)
            assert bitwise_equal(m.render(_cfg(band_rows=4)), img).all()
        finally:
            m.close()
    rt.set_majorant_block(0)


def test_errors():
    t = Tracer(0, default_scene())
    try:
        het = RenderConfig(width=8, height=8, spp=4, estimator="hetero_ratio", seed=SEED, fp64=True)
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        for call in (lambda: t.render(het), lambda: t.trace("hetero_ratio", rays, gm.states(1, 1)), lambda: t.count_work(het),
                     lambda: t.grid_ratio_probe(1.0, rays, 1.0, gm.states(1, 1))):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        t.set_density_grid(T._field(), ROOM_LO, ROOM_HI)
        assert t.render(het).any()
        with pytest.raises(VPTError) as ei:
            t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator="hetero_ratio"))
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(het)
        assert ei.value.code == _lib.VPT_E_INVALID
    finally:
        t.close()
