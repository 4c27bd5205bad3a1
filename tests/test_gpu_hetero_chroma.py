"""Estimator 14 (VPT_HETERO_CHROMATIC: estimator 10 in a medium whose coefficients depend on the colour channel) on the
GPU: the chromatic probe against its host build bit for bit, the grey medium against estimator 10 bit for bit,
hetero_chroma_kernel against render_kernel_simple_chroma and the per-sample call, every channel's expectation against
estimator 10 under that channel's coefficients, the multi-tracer, the errors and the setting.  Shapes: 4096 rays or
samples per batch, 16 x 16 x 4 spp images (and 24 x 20 x 8 where the two render kernels are compared); the expectation
test alone takes 2^20 samples per trace."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chroma_model as cm
import grid_model as gm
import test_gpu_hetero as T
import test_grid_chroma as C
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib
from scenes import big_light_scene, default_scene
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = 16, 16, 4, T.SEED
ODD = (24, 20, 8)  # width and height no multiples of the one-lane-per-pixel kernel's 16 x 16 workgroup
EST, E10 = "hetero_chromatic", "hetero"
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


def _cfg(est=EST, fp64=True, sa=SA, ss=SS, shape=(W, H, SPP), **kw):
    w, h, spp = shape
    return RenderConfig(width=w, height=h, spp=spp, estimator=est, sigma_a=sa, sigma_s=ss, seed=SEED, fp64=fp64, **kw)


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_probe_equals_host_build(ct, case):
    """the rays and media of test_grid_chroma.test_host_probe_equals_the_python_model: every output and the end state
    bit for bit"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = C._medium(name)
    rays, tmax, st = C._inputs()
    want = C.probe(case)
    try:
        ct.set_density_grid(rho, cm.LO, cm.HI, majorant_block=block, interpolation=ip)
        ct.set_medium_colour(ca, cs)
        got = ct.grid_chroma_probe(sigma_a, sigma_s, rays, tmax, st)
        for nm, g, w in zip(cm.NAMES, got, want):
            assert bitwise_equal(g, w).all(), f"{nm}: {(~bitwise_equal(g, w)).sum()} differ"
    finally:
        _reset(ct)


@pytest.mark.parametrize("hg_g,max_depth", [(0.0, 0), (0.6, 3)])
def test_grey_is_estimator_10(ct, orc_vm, hg_g, max_depth):
    """the default multipliers: the 16 x 16 x 4 fp64 render, radiances and end states of 4096 samples and count_work
    are estimator 10's bit for bit, nearest and trilinear, blocks 0 and 2.  A coloured albedo on a grey extinction: end
    states and count_work are estimator 10's, and the three channels differ"""
    rays, st = T._batch(orc_vm)
    kw = dict(hg_g=hg_g, max_depth=max_depth)
    try:
        for ip in INTERPS:
            for block in BLOCKS:
                ct.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=block, interpolation=ip)
                ct.set_medium_colour(*GREY)
                img = ct.render(_cfg(**kw))
                assert bitwise_equal(img, ct.render(_cfg(E10, **kw))).all(), f"{ip} block {block}"
                assert np.count_nonzero(img) > W * H
                L14, s14 = ct.trace(EST, rays, st, SA, SS, **kw)
                L10, s10 = ct.trace(E10, rays, st, SA, SS, **kw)
                assert (s14 == s10).all(), f"{ip} block {block}: {(s14 != s10).sum()} end states differ"
                assert bitwise_equal(L14, L10).all(), f"{ip} block {block}: {(~bitwise_equal(L14, L10)).sum()} values differ"
                assert np.count_nonzero(L10.any(axis=1)) > 500
                assert ct.count_work(_cfg(**kw)) == ct.count_work(_cfg(E10, **kw))
                ct.set_medium_colour(ALB_CA, ALB_CS)
                La, sa_ = ct.trace(EST, rays, st, ALB_S, ALB_S, **kw)
                _, sb = ct.trace(E10, rays, st, ALB_S, ALB_S, **kw)
                assert (sa_ == sb).all()
                assert ct.count_work(_cfg(sa=ALB_S, ss=ALB_S, **kw)) == ct.count_work(_cfg(E10, sa=ALB_S, ss=ALB_S, **kw))
                lit = La.all(axis=1)
                assert lit.sum() > 500 and (La[lit, 0] != La[lit, 1]).any() and (La[lit, 1] != La[lit, 2]).any()
    finally:
        _reset(ct)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero_chroma as M
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
        out[f"odd64{{ip}}{{block}}"] = t.render(M._cfg(shape=M.ODD))
        out[f"odd32{{ip}}{{block}}"] = t.render(M._cfg(shape=M.ODD, fp64=False))
        out[f"oddwork{{ip}}{{block}}"] = np.array(t.count_work(M._cfg(shape=M.ODD)), dtype=np.uint64)
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(ct, orc_vm, tmp_path):
    """the coloured medium: hetero_chroma_kernel against render_kernel_simple_chroma (a fresh process with
    VPT_SIMPLE_KERNEL=1) and against the in-order per-pixel sum of the per-sample call, bitwise, fp64 and fp32, nearest
    and trilinear, blocks 0 and 2; count_work is equal; the two kernels and count_work agree at 24 x 20 x 8 too, where the
    one-lane-per-pixel kernel's workgroups overhang the image; the image is not estimator 10's; the multi-tracer's is the
    single tracer's"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_chroma_kernel"
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
                odd = ct.render(_cfg(shape=ODD))
                assert odd.shape == (ODD[1], ODD[0], 3) and np.count_nonzero(odd) > ODD[0] * ODD[1]
                assert bitwise_equal(odd, simple["odd64" + key]).all(), f"{key}: {(~bitwise_equal(odd, simple['odd64' + key])).sum()} differ"
                assert bitwise_equal(ct.render(_cfg(shape=ODD, fp64=False)), simple["odd32" + key]).all()
                assert ct.count_work(_cfg(shape=ODD)) == tuple(int(v) for v in simple["oddwork" + key])
                assert not bitwise_equal(img, ct.render(_cfg(E10))).all()  # not estimator 10
        assert not bitwise_equal(imgs["nearest0"], imgs["trilinear0"]).all()  # the interpolation is felt
        assert not bitwise_equal(imgs["nearest0"], imgs["nearest2"]).all()    # the block is felt
        m = MultiTracer(2, default_scene(), shared_device=True)
        try:
            m.set_medium_colour(CA, CS)
            with pytest.raises(VPTError) as ei:
                m.set_medium_colour((1.0, -1.0, 1.0), CS)
            assert ei.value.code == _lib.VPT_E_INVALID
            m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, majorant_block=2, interpolation="trilinear")
            assert bitwise_equal(m.render(_cfg(band_rows=4)), imgs["trilinear2"]).all()
        finally:
            m.close()
    finally:
        _reset(ct)


# the expectation test's medium: the library's default one.  Under bench.py's dense medium (0.003, 0.027) channel 0
# (st_0 = 0.0555 per unit density) is so noisy in both estimators that the bound is 10.1 % of its mean at N = 2^20, and
# under half of it still 5.9 %: the condition on the inputs would not hold
SEP_SA, SEP_SS = 0.001, 0.009


def channel_means(sa, ss, n_side=32, spp=1024):
    """per channel c: (m10_c, m14_c, the bound, channel c of estimator 10 under the two other channels' coefficients), N"""
    f = T._field()
    r14, s14 = _camera_batch(n_side, spp, 404)
    N = len(r14)
    t = Tracer(0, big_light_scene())
    try:
        t.set_density_grid(f, ROOM_LO, ROOM_HI)
        t.set_medium_colour(CA, CS)
        L14 = t.trace(EST, r14, s14, sa, ss)[0]
        L10 = []
        for c in range(3):
            r10, s10 = _camera_batch(n_side, spp, 111 + c)
            L10.append(t.trace(E10, r10, s10, sa * CA[c], ss * CS[c])[0])
    finally:
        t.close()
    assert np.isfinite(L14).all() and all(np.isfinite(v).all() for v in L10)
    rows = []
    for c in range(3):
        a, b = L14[:, c], L10[c][:, c]
        m14, m10 = a.mean(), b.mean()
        bound = 4.5 * np.sqrt(((a * a).mean() - m14 * m14) / N + ((b * b).mean() - m10 * m10) / N)
        others = [L10[k][:, c].mean() for k in range(3) if k != c]
        print(f"({sa}, {ss}) channel {c}: m10 = {m10:.6f}, m14 = {m14:.6f}, |m14 - m10| = {abs(m14 - m10):.3e}, bound = "
              f"{bound:.3e} ({100 * bound / m10:.2f} % of m10), fraction {abs(m14 - m10) / bound:.3f}; under the other "
              f"channels' coefficients: {others[0]:.6f} ({abs(others[0] - m10) / bound:.2f} bounds away), {others[1]:.6f} "
              f"({abs(others[1] - m10) / bound:.2f})")
        rows.append((m10, m14, bound, others))
    return rows, N


def test_channels_separate():
    """The shape and the conditions of test_gpu_hetero_mis.test_same_expectation_as_estimator_10: N = 2^20 camera samples
    of a 32 x 32 image per trace, independent jitters and streams, the 2 x 3 x 2 field in the room box,
    scenes.big_light_scene, the medium (0.001, 0.009) under the coloured multipliers.  Channel c of estimator 14 and
    channel c of estimator 10 traced with (sigma_a ca[c], sigma_s cs[c]) are unbiased for the same radiance, so for each c
        |m14_c - m10_c| <= 4.5 sqrt((M2_10 - m10_c^2) / N + (M2_14 - m14_c^2) / N)
    (4.5 standard deviations: 7e-6 two-sided).  Asserted beside it, so that the test cannot pass vacuously: the bound is
    at most 5 % of m10_c, and channel c of estimator 10 under either other channel's coefficients lies outside the bound
    around m10_c.
    Measured: channel 0: m10 = 1.734084, m14 = 1.726584, |m14 - m10| = 7.50e-3 = 0.132 of the bound 5.673e-2 (3.27 % of
    m10), the other channels' media 4.94 and 11.20 bounds away; channel 1: 1.434231, 1.434888, 6.57e-4 = 0.026 of 2.499e-2
    (1.74 %), 11.60 and 14.35 bounds; channel 2: 0.844528, 0.844447, 8.05e-5 = 0.006 of 1.456e-2 (1.72 %), 37.53 and 20.95
    bounds."""
    rows, N = channel_means(SEP_SA, SEP_SS)
    assert N == 1 << 20
    for m10, m14, bound, others in rows:
        assert m10 > 0 and bound <= 0.05 * m10                 # the condition on the inputs
        assert all(abs(o - m10) > bound for o in others)       # another channel's medium is told apart
        assert abs(m14 - m10) <= bound


def test_errors_and_settings():
    t = Tracer(0, default_scene())
    try:
        cfg8 = dict(width=8, height=8, spp=4, seed=SEED, fp64=True, sigma_a=SA, sigma_s=SS)
        het = RenderConfig(estimator=EST, **cfg8)
        for name in ("hetero_chromatic", "hetero_rgb"):
            assert RenderConfig(estimator=name, **cfg8).params().medium.estimator == _lib.HETERO_CHROMATIC == 14
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        one = gm.states(1, 1)
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one), lambda: t.count_work(het),
                     lambda: t.grid_chroma_probe(0.5, 0.5, rays, 1.0, one)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID  # no grid
        t.set_medium_colour(CA, CS)  # needs no grid
        f = T._field()
        t.set_density_grid(f, ROOM_LO, ROOM_HI)
        others = {est: t.render(RenderConfig(estimator=est, **cfg8)) for est in ("hetero", "hetero_ratio", "hetero_eqa", "hetero_mis")}
        img = t.render(het)
        assert img.any()
        # a multiplier that is refused leaves the old ones
        for bad in (-0.25, float("nan"), float("inf")):
            for ca, cs in (((1.0, bad, 1.0), CS), (CA, (bad, 1.0, 1.0))):
                with pytest.raises(VPTError) as ei:
                    t.set_medium_colour(ca, cs)
                assert ei.value.code == _lib.VPT_E_INVALID
                assert bitwise_equal(t.render(het), img).all()
        # the colour survives a scene and a new grid
        t.set_scene(default_scene())
        t.set_density_grid(f.copy(), ROOM_LO, ROOM_HI)
        assert bitwise_equal(t.render(het), img).all()
        # a channel without extinction: refused by the render, the trace, count_work and the probe, not by the setter
        t.set_medium_colour((1.0, 0.0, 1.0), (1.0, 0.0, 1.0))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one, SA, SS), lambda: t.count_work(het),
                     lambda: t.grid_chroma_probe(SA, SS, rays, 1.0, one)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        # estimators 10 to 13 do not read the colour
        for est, before in others.items():
            assert bitwise_equal(t.render(RenderConfig(estimator=est, **cfg8)), before).all(), est
        t.set_medium_colour(*GREY)
        assert not bitwise_equal(t.render(het), img).all()  # the colour is felt
        assert bitwise_equal(t.render(het), others["hetero"]).all()
        t.set_medium_colour(CA, CS)
        # an emission grid: estimator 14 refuses it and estimator 10 goes on scoring it
        t.set_emission_grid(np.full(f.shape, 0.5, np.float32), (1.0, 0.5, 0.25))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, one, SA, SS), lambda: t.count_work(het)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        assert np.isfinite(t.render(RenderConfig(estimator="hetero", **cfg8))).all()
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
