"""Estimator 16 (VPT_HETERO_SPECTRAL: estimator 11 in the chromatic medium of estimator 14, by spectral tracking) on the
GPU: the probe of the two walkers against its host build bit for bit, the grey medium against estimator 11 bit for bit,
hetero_spectral_kernel against render_kernel_simple_spectral and the per-sample call, every channel's expectation against
estimator 10 under that channel's coefficients, the multi-tracer, the errors and the setting.  Shapes: 4096 rays or
samples per batch, 20 x 12 x 8 spp images; the expectation test alone takes 2^20 samples per trace."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chroma_model as cm
import grid_model as gm
import spectral_model as sm
import test_gpu_hetero as T
import test_grid_spectral as S
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib
from scenes import big_light_scene, default_scene
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = 20, 12, 8, T.SEED
EST, E11, E10 = "hetero_spectral", "hetero_ratio", "hetero"
INTERPS = ("nearest", "trilinear")
BLOCKS = (0, 2)
CA, CS = cm.CA, cm.CS
GREY = ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
# a coloured albedo on a grey extinction: dyadic multipliers on sigma_a == sigma_s, so the three st_c are one number
ALB_S, ALB_CA, ALB_CS = 0.015625, (1.5, 1.0, 0.5), (0.5, 1.0, 1.5)


@pytest.fixture(scope="module")
def ct():
    """a tracer of this module's own: its grid, block, interpolation and colour never reach the other modules'"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _reset(t):
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")
    t.set_medium_colour(*GREY)


def _cfg(est=EST, fp64=True, sa=SA, ss=SS, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=sa, sigma_s=ss, seed=SEED, fp64=fp64, **kw)


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_probe_equals_host_build(ct, case):
    """the 4096 rays and the media of test_grid_spectral, a 2 x 3 x 2 grid (LDS holds it): every output of both walkers
    and their end states bit for bit, with beta = 1 and with a throughput per ray"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = S._medium(name)
    rays, tmax, st = S._inputs(name)
    assert len(rays) == 4096
    betas = np.random.default_rng(6).uniform(-1.0, 2.0, (len(rays), 3))
    betas[::3, 2] = 0.0
    try:
        ct.set_density_grid(rho, cm.LO, cm.HI, majorant_block=block, interpolation=ip)
        ct.set_medium_colour(ca, cs)
        for beta in (None, betas):
            want = S.probe(case, beta)
            got = ct.grid_spectral_probe(sigma_a, sigma_s, rays, tmax, st, beta=beta)
            for nm, g, w in zip(sm.NAMES, got, want):
                assert bitwise_equal(g, w).all(), f"{nm}: {(~bitwise_equal(g, w)).sum()} differ"
    finally:
        _reset(ct)


@pytest.mark.parametrize("hg_g,max_depth", [(0.0, 0), (0.6, 3)])
def test_grey_is_estimator_11(ct, orc_vm, hg_g, max_depth):
    """the default multipliers: the 20 x 12 x 8 render in fp64 and fp32, radiances and end states of 4096 samples and
    count_work are estimator 11's bit for bit, nearest and trilinear, blocks 0 and 2.  A coloured albedo on a grey
    extinction: end states and count_work are estimator 11's, and the three channels differ"""
    rays, st = T._batch(orc_vm)
    kw = dict(hg_g=hg_g, max_depth=max_depth)
    try:
        for ip in INTERPS:
            for block in BLOCKS:
                ct.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                ct.set_medium_colour(*GREY)
                for fp64 in (True, False):
                    img = ct.render(_cfg(fp64=fp64, **kw))
                    assert bitwise_equal(img, ct.render(_cfg(E11, fp64=fp64, **kw))).all(), f"{ip} block {block} fp64 {fp64}"
                    assert np.count_nonzero(img) > W * H
                L16, s16 = ct.trace(EST, rays, st, SA, SS, **kw)
                L11, s11 = ct.trace(E11, rays, st, SA, SS, **kw)
                assert (s16 == s11).all(), f"{ip} block {block}: {(s16 != s11).sum()} end states differ"
                assert bitwise_equal(L16, L11).all(), f"{ip} block {block}: {(~bitwise_equal(L16, L11)).sum()} values differ"
                assert np.count_nonzero(L11.any(axis=1)) > 500
                assert ct.count_work(_cfg(**kw)) == ct.count_work(_cfg(E11, **kw))
                ct.set_medium_colour(ALB_CA, ALB_CS)
                La, sa_ = ct.trace(EST, rays, st, ALB_S, ALB_S, **kw)
                _, sb = ct.trace(E11, rays, st, ALB_S, ALB_S, **kw)
                assert (sa_ == sb).all()
                assert ct.count_work(_cfg(sa=ALB_S, ss=ALB_S, **kw)) == ct.count_work(_cfg(E11, sa=ALB_S, ss=ALB_S, **kw))
                lit = La.all(axis=1)
                assert lit.sum() > 500 and (La[lit, 0] != La[lit, 1]).any() and (La[lit, 1] != La[lit, 2]).any()
    finally:
        _reset(ct)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero_spectral as M
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
t.set_medium_colour(M.CA, M.CS)
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


def _band_rows(off):
    return [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]


def test_kernels_agree(ct, orc_vm, tmp_path):
    """the coloured medium, 20 x 12 (edge tiles that are no multiples of 8): hetero_spectral_kernel against
    render_kernel_simple_spectral (a fresh process with VPT_SIMPLE_KERNEL=1) and against the in-order per-pixel sum of the
    per-sample call, bitwise, fp64 and fp32, nearest and trilinear, blocks 0 and 2; count_work is equal; the banded
    shards (band_rows 4, band_stride 2) are the whole image's rows; the image is neither estimator 11's nor 14's"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_spectral_kernel"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    imgs = {}
    try:
        ct.set_medium_colour(CA, CS)
        for ip in INTERPS:
            for block in BLOCKS:
                ct.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                key = f"{ip}{block}"
                img = imgs[key] = ct.render(_cfg())
                img32 = ct.render(_cfg(fp64=False))
                assert bitwise_equal(img, simple["f64" + key]).all(), f"{key}: {(~bitwise_equal(img, simple['f64' + key])).sum()} differ"
                assert bitwise_equal(img32, simple["f32" + key]).all()
                L, _ = ct.trace(EST, rays.reshape(-1), st.reshape(-1), SA, SS)
                L = L.reshape(H, W, SPP, 3)
                acc = np.zeros((H, W, 3))
                for s in range(SPP):
                    acc = L[:, :, s] + acc
                want = acc * (1 / float(SPP))
                assert bitwise_equal(img, want).all(), f"{key}: {(~bitwise_equal(img, want)).sum()} values differ from the sample sum"
                assert bitwise_equal(img32, want.astype(np.float32)).all()
                assert np.isfinite(img).all() and np.count_nonzero(img) > W * H
                work = ct.count_work(_cfg())
                assert work == tuple(int(v) for v in simple["work" + key]) and work[0] > 0 and work[1] > 0
                assert not bitwise_equal(img, ct.render(_cfg(E11))).all()                 # not estimator 11
                assert not bitwise_equal(img, ct.render(_cfg("hetero_chromatic"))).all()  # nor estimator 14
                whole = np.zeros_like(img)
                for off in (0, 1):
                    shard = ct.render(_cfg(band_rows=4, band_stride=2, band_offset=off))
                    rows = _band_rows(off)
                    assert shard.shape[0] == len(rows)
                    whole[rows] = shard
                assert bitwise_equal(whole, img).all(), key
        assert not bitwise_equal(imgs["nearest0"], imgs["trilinear0"]).all()  # the interpolation is felt
        assert not bitwise_equal(imgs["nearest0"], imgs["nearest2"]).all()    # the block is felt
    finally:
        _reset(ct)


def test_multi_tracer_equals_the_single_tracer(ct):
    """two bands (on one device where only one is present): the coloured medium, trilinear, block 2"""
    try:
        ct.set_medium_colour(CA, CS)
        ct.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=2, interpolation="trilinear")
        img = ct.render(_cfg())
        m = MultiTracer(2, default_scene(), shared_device=True)
        try:
            m.set_medium_colour(CA, CS)
            m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=2, interpolation="trilinear")
            assert bitwise_equal(m.render(_cfg(band_rows=4)), img).all()
            m.set_medium_colour(*GREY)
            assert bitwise_equal(m.render(_cfg(band_rows=4)), ct.render(_cfg(E11))).all()
        finally:
            m.close()
    finally:
        _reset(ct)


SEP_SA, SEP_SS = 0.001, 0.009  # test_gpu_hetero_chroma's medium of the same test


def channel_means(sa, ss, n_side=32, spp=1024):
    """per channel c: (m10_c, m16_c, the bound, channel c of estimator 10 under the two other channels' coefficients), N"""
    f = T._field()
    r16, s16 = _camera_batch(n_side, spp, 404)
    N = len(r16)
    t = Tracer(0, big_light_scene())
    try:
        t.set_density_grid(f, ROOM_LO, ROOM_HI)
        t.set_medium_colour(CA, CS)
        L16 = t.trace(EST, r16, s16, sa, ss)[0]
        L10 = []
        for c in range(3):
            r10, s10 = _camera_batch(n_side, spp, 111 + c)
            L10.append(t.trace(E10, r10, s10, sa * CA[c], ss * CS[c])[0])
    finally:
        t.close()
    assert np.isfinite(L16).all() and all(np.isfinite(v).all() for v in L10)
    rows = []
    for c in range(3):
        a, b = L16[:, c], L10[c][:, c]
        m16, m10 = a.mean(), b.mean()
        v16, v10 = (a * a).mean() - m16 * m16, (b * b).mean() - m10 * m10
        bound = 4.5 * np.sqrt(v16 / N + v10 / N)
        others = [L10[k][:, c].mean() for k in range(3) if k != c]
        print(f"({sa}, {ss}) channel {c}: m10 = {m10:.6f}, m16 = {m16:.6f}, |m16 - m10| = {abs(m16 - m10):.3e}, bound = "
              f"{bound:.3e} ({100 * bound / m10:.2f} % of m10), fraction {abs(m16 - m10) / bound:.3f}; rms / mean: estimator 16 "
              f"{np.sqrt(v16) / m16:.2f}, estimator 10 {np.sqrt(v10) / m10:.2f}; under the other channels' coefficients: "
              f"{others[0]:.6f} ({abs(others[0] - m10) / bound:.2f} bounds away), {others[1]:.6f} "
              f"({abs(others[1] - m10) / bound:.2f})")
        rows.append((m10, m16, bound, others))
    return rows, N


def test_channels_separate():
    """The shape of test_gpu_hetero_chroma.test_channels_separate: N = 2^20 camera samples of a 32 x 32 image per trace,
    independent jitters and streams, the 2 x 3 x 2 field in the room box, scenes.big_light_scene, the medium
    (0.001, 0.009) under the coloured multipliers.  Channel c of estimator 16 and channel c of estimator 10 traced with
    (sigma_a ca[c], sigma_s cs[c]) are unbiased for the same radiance, so for each c
        |m16_c - m10_c| <= 4.5 sqrt(var10 / N + var16 / N)
    (4.5 standard deviations: 7e-6 two-sided).  Asserted beside it, so that the test cannot pass vacuously: the bound is
    at most 5 % of m10_c, and channel c of estimator 10 under either other channel's coefficients lies outside the bound
    around m10_c.
    Measured at N = 2^20: channel 0: m10 = 1.734084, m16 = 1.726006, |m16 - m10| = 8.08e-3 = 0.148 of the bound 5.455e-2
    (3.15 % of m10), the other channels' media 5.13 and 11.64 bounds away, rms / mean 6.27 (estimator 10: 3.52); channel 1:
    1.434231, 1.429921, 4.31e-3 = 0.166 of 2.602e-2 (1.81 %), 11.14 and 13.78 bounds, rms / mean 3.02 (2.82); channel 2:
    0.844528, 0.844089, 4.39e-4 = 0.029 of 1.524e-2 (1.80 %), 35.84 and 20.01 bounds, rms / mean 3.15 (2.63)."""
    rows, N = channel_means(SEP_SA, SEP_SS)
    assert N == 1 << 20
    for m10, m16, bound, others in rows:
        assert m10 > 0 and bound <= 0.05 * m10                 # the condition on the inputs
        assert all(abs(o - m10) > bound for o in others)       # another channel's medium is told apart
        assert abs(m16 - m10) <= bound


def test_errors_and_settings():
    t = Tracer(0, default_scene())
    try:
        cfg8 = dict(width=8, height=8, spp=4, seed=SEED, fp64=True, sigma_a=SA, sigma_s=SS)
        het = RenderConfig(estimator=EST, **cfg8)
        for name in ("hetero_spectral", "hetero_spectral_tracking"):
            assert RenderConfig(estimator=name, **cfg8).params().medium.estimator == _lib.HETERO_SPECTRAL == 16
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        one = gm.states(1, 1)
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one), lambda: t.count_work(het),
                     lambda: t.grid_spectral_probe(0.5, 0.5, rays, 1.0, one)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID  # no grid
        t.set_medium_colour(CA, CS)  # needs no grid
        f = T._field()
        t.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=2)
        others = {est: t.render(RenderConfig(estimator=est, **cfg8))
                  for est in ("hetero", "hetero_ratio", "hetero_eqa", "hetero_mis", "hetero_residual")}
        img = t.render(het)
        assert img.any()
        # the colour survives a scene and a new grid
        t.set_scene(default_scene())
        t.set_density_grid(f.copy(), ROOM_LO, ROOM_HI, majorant_block=2)
        assert bitwise_equal(t.render(het), img).all()
        # a channel without extinction: refused by the render, the trace, count_work and the probe, not by the setter
        t.set_medium_colour((1.0, 0.0, 1.0), (1.0, 0.0, 1.0))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one, SA, SS), lambda: t.count_work(het),
                     lambda: t.grid_spectral_probe(SA, SS, rays, 1.0, one)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        # estimators 10 to 13 and 15 render what they rendered before the colour was set
        t.set_medium_colour(*GREY)
        for est, before in others.items():
            assert bitwise_equal(t.render(RenderConfig(estimator=est, **cfg8)), before).all(), est
        assert not bitwise_equal(t.render(het), img).all()  # changing the colour changes the image
        assert bitwise_equal(t.render(het), others["hetero_ratio"]).all()
        t.set_medium_colour(CA, CS)
        for est, before in others.items():
            assert bitwise_equal(t.render(RenderConfig(estimator=est, **cfg8)), before).all(), est
        # an emission grid: estimator 16 refuses it and estimator 11 goes on scoring it
        t.set_emission_grid(np.full(f.shape, 0.5, np.float32), (1.0, 0.5, 0.25))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one, SA, SS), lambda: t.count_work(het)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        assert np.isfinite(t.render(RenderConfig(estimator="hetero_ratio", **cfg8))).all()
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
