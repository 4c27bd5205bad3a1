"""Estimator 13 (VPT_HETERO_MIS: the one-sample combination of a delta track and the equi-angular distance under the
balance heuristic) on the GPU: the MIS probe against its host build bit for bit, the track fraction 0 against estimator
12 bit for bit, hetero_mis_kernel against render_kernel_simple_mis and the per-sample call, the expectation against
estimator 10's and the per-sample noise against estimator 12's, the multi-tracer and the errors.  Shapes are those of
tests/test_gpu_hetero_eqa.py: 4096 samples per batch, 24 x 20 x 8 spp images; the expectation test alone takes 2^20
samples per estimator."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_mis_probe_host
from scenes import big_light_scene, default_scene
from test_gpu_hetero_eqa import LIGHTS, SCENES
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = T.W, T.H, T.SPP, T.SEED
EST, EQA = "hetero_mis", "hetero_equiangular"
INTERPS = ("nearest", "trilinear")
BLOCKS = (0, 2)
PROBE_NAMES = ("psurf", "strategy", "dist", "pdf", "pe", "T", "rho_t", "steps", "states")


@pytest.fixture(scope="module")
def mt():
    """a tracer of this module's own: its grid, block, interpolation and fraction never reach the other modules'"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _reset(t):
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")
    t.set_hetero_mis_fraction(0.5)


def _cfg(est=EST, fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("interpolation", INTERPS)
def test_probe_equals_host_build(mt, interpolation, block):
    """4096 rays through the sparse field and grid_model's tau grid, a light inside and one outside the box, the
    fractions 0, 0.5 and 1: every output and the end state bit for bit"""
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    assert len(rays) == 4096
    try:
        for rho in (mm.sparse_field(), gm.tau_grid()):
            mt.set_density_grid(rho, mm.SPARSE_LO, mm.SPARSE_HI, majorant_block=block, interpolation=interpolation)
            for sigma_t, light in zip((0.7, 0.05), LIGHTS):
                for q in (0.0, 0.5, 1.0):
                    mt.set_hetero_mis_fraction(q)
                    got = mt.grid_mis_probe(sigma_t, rays, tmax, light, st)
                    want = grid_mis_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays, tmax, light, st, q=q,
                                               majorant_block=block, interpolation=interpolation)
                    for name, g, w in zip(PROBE_NAMES, got, want):
                        assert bitwise_equal(g, w).all(), f"{name} (sigma_t {sigma_t}, q {q}): {(~bitwise_equal(g, w)).sum()} differ"
                    strategy, dist, rho_t = want[1], want[2], want[6]
                    assert (dist == -1).sum() > 100 and ((dist >= 0) & (rho_t > 0)).sum() > 100
                    if q == 0.5:
                        assert 1800 < strategy.sum() < 2300 and ((strategy == 1) & (dist >= 0)).sum() > 50
    finally:
        _reset(mt)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("hg_g,max_depth", [(0.0, 0), (0.6, 3)])
def test_fraction_zero_is_estimator_12_per_sample(orc_vm, hg_g, max_depth, scene):
    """q = 0: radiances and end states of all 4096 samples are estimator 12's bit for bit, nearest and trilinear, with
    and without a majorant block (which estimator 12 ignores and a fraction of 0 never reaches)"""
    rays, st = T._batch(orc_vm)
    t = Tracer(0, SCENES[scene]())
    try:
        t.set_hetero_mis_fraction(0.0)
        for ip in INTERPS:
            for block in BLOCKS:
                t.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                L13, s13 = t.trace(EST, rays, st, SA, SS, hg_g=hg_g, max_depth=max_depth)
                L12, s12 = t.trace(EQA, rays, st, SA, SS, hg_g=hg_g, max_depth=max_depth)
                assert (s13 == s12).all(), f"{ip} block {block}: {(s13 != s12).sum()} end states differ"
                assert bitwise_equal(L13, L12).all(), f"{ip} block {block}: {(~bitwise_equal(L13, L12)).sum()} values differ"
                assert np.count_nonzero(L12.any(axis=1)) > 500
        t.set_hetero_mis_fraction(0.5)
        assert (t.trace(EST, rays, st, SA, SS, hg_g=hg_g, max_depth=max_depth)[1] != s12).any()  # the fraction is felt
    finally:
        t.close()


def test_fraction_zero_is_estimator_12_rendered(mt):
    """q = 0: the 24 x 20 x 8 render is estimator 12's bitwise, fp64 and fp32, and count_work is equal"""
    try:
        mt.set_hetero_mis_fraction(0.0)
        for ip in INTERPS:
            mt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, interpolation=ip)
            for fp64 in (True, False):
                img = mt.render(_cfg(fp64=fp64))
                assert bitwise_equal(img, mt.render(_cfg(EQA, fp64=fp64))).all()
                assert np.count_nonzero(img) > W * H
            assert mt.count_work(_cfg()) == mt.count_work(_cfg(EQA))
    finally:
        _reset(mt)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero_mis as M
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
t.set_hetero_mis_fraction(0.5)
out = {{}}
for ip in M.INTERPS:
    for block in M.BLOCKS:
        t.set_density_grid(M.T._field(), M.ROOM_LO, M.ROOM_HI, majorant_block=block, interpolation=ip)
        out[f"f64{{ip}}{{block}}"] = t.render(M._cfg())
        out[f"f32{{ip}}{{block}}"] = t.render(M._cfg(fp64=False))
        out[f"work{{ip}}{{block}}"] = np.array(t.count_work(M._cfg()), dtype=np.uint64)
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(mt, orc_vm, tmp_path):
    """q = 0.5: hetero_mis_kernel against render_kernel_simple_mis (a fresh process with VPT_SIMPLE_KERNEL=1) and
    against the in-order per-pixel sum of the per-sample call, bitwise, fp64 and fp32, nearest and trilinear, blocks 0
    and 2; count_work is equal; the image is neither estimator 10's nor 12's; the fraction and the block are felt;
    interleaved band shards reassemble"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_mis_kernel"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    imgs = {}
    try:
        mt.set_hetero_mis_fraction(0.5)
        for ip in INTERPS:
            for block in BLOCKS:
                mt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                key = f"{ip}{block}"
                img = imgs[key] = mt.render(_cfg())
                img32 = mt.render(_cfg(fp64=False))
                assert bitwise_equal(img, simple["f64" + key]).all(), f"{key}: {(~bitwise_equal(img, simple['f64' + key])).sum()} differ"
                assert bitwise_equal(img32, simple["f32" + key]).all()
                L, _ = mt.trace(EST, rays.reshape(-1), st.reshape(-1), SA, SS)
                L = L.reshape(H, W, SPP, 3)
                acc = np.zeros((H, W, 3))
                for s in range(SPP):
                    acc = L[:, :, s] + acc
                want = acc * (1 / float(SPP))
                assert bitwise_equal(img, want).all(), f"{key}: {(~bitwise_equal(img, want)).sum()} values differ from the sample sum"
                assert bitwise_equal(img32, want.astype(np.float32)).all()
                assert np.isfinite(img).all() and np.count_nonzero(img) > W * H
                work = mt.count_work(_cfg())
                assert work == tuple(int(v) for v in simple["work" + key]) and work[0] > 0 and work[1] > 0
                assert not bitwise_equal(img, mt.render(_cfg("hetero"))).all()  # not estimator 10
                assert not bitwise_equal(img, mt.render(_cfg(EQA))).all()       # nor estimator 12
        assert not bitwise_equal(imgs["nearest0"], imgs["trilinear0"]).all()  # the interpolation is felt
        assert not bitwise_equal(imgs["nearest0"], imgs["nearest2"]).all()    # the block is felt
        assert not bitwise_equal(imgs["trilinear0"], imgs["trilinear2"]).all()
        mt.set_hetero_mis_fraction(0.25)                                      # the fraction is felt
        assert not bitwise_equal(mt.render(_cfg()), imgs["trilinear2"]).all()
        mt.set_hetero_mis_fraction(0.5)
        # shards: bands of 4 rows, two interleaved shards, reassembled
        whole = np.zeros_like(imgs["trilinear2"])
        for off in (0, 1):
            shard = mt.render(_cfg(band_rows=4, band_stride=2, band_offset=off))
            rows = [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]
            whole[rows] = shard
        assert bitwise_equal(whole, imgs["trilinear2"]).all()
    finally:
        _reset(mt)


def test_multi_tracer_equals_single(mt):
    """two ranks on one device: the default fraction, and one set through the multi-tracer"""
    try:
        for ip, block, q in (("nearest", 0, None), ("trilinear", 2, 0.25)):
            mt.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
            mt.set_hetero_mis_fraction(0.5 if q is None else q)
            img = mt.render(_cfg())
            m = MultiTracer(2, default_scene(), shared_device=True)
            try:
                with pytest.raises(VPTError) as ei:
                    m.render(_cfg())
                assert ei.value.code == _lib.VPT_E_INVALID  # no grid yet
                if q is not None:
                    m.set_hetero_mis_fraction(q)
                    with pytest.raises(VPTError) as ei:
                        m.set_hetero_mis_fraction(1.5)
                    assert ei.value.code == _lib.VPT_E_INVALID
                m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                assert bitwise_equal(m.render(_cfg(band_rows=4)), img).all()
            finally:
                m.close()
    finally:
        _reset(mt)


def test_same_expectation_as_estimator_10():
    """The shape and the conditions of test_gpu_hetero_eqa.test_same_expectation_as_estimator_10: N = 2^20 camera samples
    of a 32 x 32 image per estimator, independent jitters and streams, the 2 x 3 x 2 field in the room box,
    scenes.big_light_scene, the thin medium (0.0002, 0.0018), q = 0.5.  Both estimators are unbiased for the same
    radiance, so
        |m13 - m10| <= 4.5 sqrt((M2_10 - m10^2) / N + (M2_13 - m13^2) / N)
    (4.5 standard deviations: 7e-6 two-sided).  Asserted beside it, so that the test cannot pass vacuously: the bound is
    at most 5 % of m10, and estimator 13 on the uniform field of _field().max() -- another medium -- lies outside the
    bound around m10.
    At the dense medium (0.003, 0.027) every figure is printed, and one thing is asserted: on the same rays and streams
    estimator 13's per-sample rms / mean is below estimator 12's, with no margin -- its vertex weights are bounded by
    2 sigma_s / sigma_t where estimator 12's are not.
    Measured at the thin medium: m10 = 1.140005, m13 = 1.139375, |m13 - m10| = 6.30e-4 = 0.028 of the bound 2.219e-2
    (1.95 % of m10); rms / mean 3.11 (10), 3.59 (12), 3.15 (13); the uniform field: m = 1.182987, 1.94 bounds away.
    At the dense medium: m10 = 1.447830, m13 = 1.439127, m12 = 1.462027, |m13 - m10| = 8.70e-3 = 0.190 of the bound
    4.570e-2 (3.16 % of m10: estimator 12's was 16.5 %); rms / mean 3.81 (10), 36.93 (12), 6.13 (13); the largest
    sample 39 221 (12) against 3 819 (13)."""
    n_side, spp = 32, 1024
    f = T._field()
    lum = np.array([0.2126, 0.7152, 0.0722])
    r10, s10 = _camera_batch(n_side, spp, 101)
    r13, s13 = _camera_batch(n_side, spp, 303)
    N = len(r10)
    assert N == 1 << 20
    res = {}
    t = Tracer(0, big_light_scene())
    try:
        t.set_hetero_mis_fraction(0.5)
        for name, (sa, ss) in (("dense", (SA, SS)), ("thin", (0.0002, 0.0018))):
            t.set_density_grid(f, ROOM_LO, ROOM_HI)
            l10 = t.trace("hetero", r10, s10, sa, ss)[0] @ lum
            l13 = t.trace(EST, r13, s13, sa, ss)[0] @ lum
            l12 = t.trace(EQA, r13, s13, sa, ss)[0] @ lum  # estimator 12 on estimator 13's rays and streams
            t.set_density_grid(np.full(f.shape, f.max(), np.float32), ROOM_LO, ROOM_HI)
            lu = t.trace(EST, r13, s13, sa, ss)[0] @ lum
            assert all(np.isfinite(v).all() for v in (l10, l12, l13, lu))
            m10, m2_10, m13, m2_13, mu = l10.mean(), (l10 * l10).mean(), l13.mean(), (l13 * l13).mean(), lu.mean()
            m12, m2_12 = l12.mean(), (l12 * l12).mean()
            bound = 4.5 * np.sqrt((m2_10 - m10 * m10) / N + (m2_13 - m13 * m13) / N)
            rms = {10: np.sqrt(m2_10 - m10 * m10) / m10, 12: np.sqrt(m2_12 - m12 * m12) / m12,
                   13: np.sqrt(m2_13 - m13 * m13) / m13}
            print(f"{name}: m10 = {m10:.6f}, m13 = {m13:.6f}, m12 = {m12:.6f}, |m13 - m10| = {abs(m13 - m10):.3e}, "
                  f"bound = {bound:.3e} ({100 * bound / m10:.2f} % of m10), fraction {abs(m13 - m10) / bound:.3f}; rms/mean "
                  f"10: {rms[10]:.2f}, 12: {rms[12]:.2f}, 13: {rms[13]:.2f}; max sample 12: {l12.max():.1f}, 13: {l13.max():.1f}; "
                  f"uniform field: m = {mu:.6f}, {abs(mu - m10) / bound:.2f} bounds away")
            res[name] = (m10, m13, mu, bound, rms)
    finally:
        t.close()
    m10, m13, mu, bound, _ = res["thin"]
    assert m10 > 0 and bound <= 0.05 * m10  # the condition on the inputs
    assert abs(mu - m10) > bound            # another medium is told apart
    assert abs(m13 - m10) <= bound
    rms = res["dense"][4]
    assert rms[13] < rms[12]


def test_errors_and_settings():
    t = Tracer(0, default_scene())
    try:
        cfg8 = dict(width=8, height=8, spp=4, seed=SEED, fp64=True)
        het = RenderConfig(estimator=EST, **cfg8)
        for name in ("hetero_mis", "hetero_mis_equiangular"):
            assert RenderConfig(estimator=name, **cfg8).params().medium.estimator == _lib.HETERO_MIS == 13
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        one = gm.states(1, 1)
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one), lambda: t.count_work(het),
                     lambda: t.grid_mis_probe(1.0, rays, 1.0, (0, 0, 0), one)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID  # no grid
        t.set_hetero_mis_fraction(0.25)  # needs no grid
        f = T._field()
        t.set_density_grid(f, ROOM_LO, ROOM_HI)
        img = t.render(het)
        assert img.any()
        # a fraction that is refused leaves the old one
        for q in (-0.25, 1.25, float("nan"), float("inf")):
            with pytest.raises(VPTError) as ei:
                t.set_hetero_mis_fraction(q)
            assert ei.value.code == _lib.VPT_E_INVALID
            assert bitwise_equal(t.render(het), img).all()
        # the fraction survives a scene and a new grid
        t.set_scene(default_scene())
        t.set_density_grid(f.copy(), ROOM_LO, ROOM_HI)
        assert bitwise_equal(t.render(het), img).all()
        t.set_hetero_mis_fraction(0.5)
        assert not bitwise_equal(t.render(het), img).all()
        t.set_hetero_mis_fraction(0.25)
        # an emission grid: estimator 13 refuses it and estimators 10 and 11 go on scoring it -- "13 alone" among what
        # this change touches.  Estimator 12 refuses it too, as it did before (test_gpu_hetero_eqa.test_errors_and_clear)
        t.set_emission_grid(np.full(f.shape, 0.5, np.float32), (1.0, 0.5, 0.25))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one), lambda: t.count_work(het)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        for est in ("hetero", "hetero_ratio"):
            assert np.isfinite(t.render(RenderConfig(estimator=est, **cfg8))).all()
        t.clear_emission_grid()
        assert bitwise_equal(t.render(het), img).all()
        with pytest.raises(VPTError) as ei:
            t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator=EST))
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(het)
        assert ei.value.code == _lib.VPT_E_INVALID
    finally:
        t.close()
