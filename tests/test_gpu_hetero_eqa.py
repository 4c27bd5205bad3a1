"""Estimator 12 (VPT_HETERO_EQUIANGULAR: estimator 1's control flow in the density grid) on the GPU: the equi-angular
probe against its host build bit for bit, the reduction to estimator 1 on uniform grids, voxel indexing on a resampled
field, hetero_eqa_kernel against render_kernel_simple_eqa and the per-sample call, the expectation against estimator
10's, the multi-tracer and the errors.  Shapes are those of tests/test_gpu_hetero.py: 4096 samples per batch,
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
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_eqa_probe_host
from scenes import big_light_scene, default_scene, point_lights_scene, sph
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
W, H, SPP, SEED = T.W, T.H, T.SPP, T.SEED
EST = "hetero_equiangular"
INTERPS = ("nearest", "trilinear")
LIGHTS = ((1.5, 3.1, 1.5), (7.5, 6.0, -6.0))  # inside and outside grid_model's box


@pytest.fixture(scope="module")
def et():
    """a tracer of this module's own: its grid and its interpolation never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _cfg(est=EST, fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


@pytest.mark.parametrize("interpolation", INTERPS)
def test_probe_equals_host_build(et, interpolation):
    """4096 rays through the sparse field and grid_model's tau grid, a light inside and one outside the box: every
    output and the end state bit for bit"""
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    assert len(rays) == 4096
    try:
        for rho in (mm.sparse_field(), gm.tau_grid()):
            et.set_density_grid(rho, mm.SPARSE_LO, mm.SPARSE_HI, interpolation=interpolation)
            for sigma_t, light in zip((0.7, 0.05), LIGHTS):
                got = et.grid_eqa_probe(sigma_t, rays, tmax, light, st)
                want = grid_eqa_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays, tmax, light, st,
                                           interpolation=interpolation)
                for name, g, w in zip(("psurf", "dist", "pdf", "T", "rho_t", "states"), got, want):
                    assert bitwise_equal(g, w).all(), f"{name} (sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
                assert (want[1] == -1).sum() > 100 and ((want[1] != -1) & (want[4] > 0)).sum() > 100
    finally:
        et.set_grid_interpolation("nearest")


def _closed_scene():
    """the default scene with a wall behind the camera: no ray escapes"""
    return np.concatenate([default_scene(), sph(1e5, (0, 0, 1e5 + 225), (.5, .5, .5))])


SCENES = {"default": default_scene, "point_lights": point_lights_scene, "closed": _closed_scene}


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("hg_g,max_depth", [(0.0, 0), (0.6, 3)])
@pytest.mark.parametrize("rho", [1.0, 2.0])
def test_uniform_grid_reduces_to_estimator_1(orc_vm, rho, hg_g, max_depth, scene):
    """uniform rho on [-4096, 4096]^3 (4^3 voxels): the interval is [+0.0, t] bit for bit, so estimator 12 walks
    estimator 1's paths at (rho sigma_a, rho sigma_s) with the same draws -- equal end states on all 4096 samples,
    radiances within the rounding of tau.  Beside test_gpu_hetero's factors there is 1 / (1 - psurf), which turns a
    one-ulp difference of psurf into 2^-53 / (sigma_t t) relative: below 1e-11 for every segment longer than 1e-3
    units at sigma_t = 0.03.  No sample is exempt."""
    rays, st = T._batch(orc_vm)
    t = Tracer(0, SCENES[scene]())
    try:
        t.set_density_grid(np.full((4, 4, 4), rho, np.float32), T.BIG_LO, T.BIG_HI)
        L12, s12 = t.trace(EST, rays, st, SA, SS, hg_g=hg_g, max_depth=max_depth)
        L1, s1 = t.trace("mis", rays, st, rho * SA, rho * SS, hg_g=hg_g, max_depth=max_depth)
        assert (s12 == s1).all(), f"{(s12 != s1).sum()} end states differ"
        ok = T._radiance_bound(L12, L1)
        print(f"rho {rho}: max |L12 - L1| = {np.abs(L12 - L1).max():.3e}, max L = {L1.max():.3e}, "
              f"nonzero {np.count_nonzero(L1.any(axis=1))}")
        assert ok.all(), f"{(~ok).sum()} channels beyond the bound, worst {np.abs(L12 - L1).max():.3e}"
        # the samples carry light.  (Under point lights alone estimator 1 itself lights fewer: a cone sample toward a
        # point light scores an exact zero, so only the shadow-ray branch of single scattering and pLight contribute)
        assert np.count_nonzero(L1.any(axis=1)) > (500 if scene == "point_lights" else 2000)
        if rho == 1.0:
            cfg = dict(width=16, height=16, spp=4, sigma_a=SA, sigma_s=SS, seed=SEED, hg_g=hg_g, max_depth=max_depth)
            assert t.count_work(RenderConfig(estimator=EST, **cfg)) == t.count_work(RenderConfig(estimator="mis", **cfg))
    finally:
        t.close()


def test_resampled_field_gives_the_same_samples(et, orc_vm):
    """the 2 x 3 x 2 field and its 4 x 6 x 4 piecewise-constant resampling: equal end states, radiances within the
    bound of the reduction test; the uniform field of the same maximum gives other end states; and under "trilinear"
    a uniform grid gives the nearest result's end states (a lerp of equal values is exact)"""
    rays, st = T._batch(orc_vm)
    f = T._field()
    et.set_density_grid(f, ROOM_LO, ROOM_HI, interpolation="nearest")
    La, sa = et.trace(EST, rays, st, SA, SS)
    et.set_density_grid(mm.resample2(f), ROOM_LO, ROOM_HI)
    Lb, sb = et.trace(EST, rays, st, SA, SS)
    assert (sa == sb).all(), f"{(sa != sb).sum()} end states differ"
    ok = T._radiance_bound(La, Lb)
    print(f"max |La - Lb| = {np.abs(La - Lb).max():.3e}, max L = {La.max():.3e}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
    assert np.count_nonzero(La.any(axis=1)) > 2000
    uniform = np.full((2, 3, 2), f.max(), np.float32)
    et.set_density_grid(uniform, ROOM_LO, ROOM_HI)
    Lu, su = et.trace(EST, rays, st, SA, SS)
    assert (su != sa).any()  # the field is felt
    try:
        et.set_density_grid(uniform, ROOM_LO, ROOM_HI, interpolation="trilinear")
        Lt, s_t = et.trace(EST, rays, st, SA, SS)
        assert (s_t == su).all() and T._radiance_bound(Lt, Lu).all()
        et.set_density_grid(f, ROOM_LO, ROOM_HI)
        assert (et.trace(EST, rays, st, SA, SS)[1] != sa).any()  # the trilinear field is another field
    finally:
        et.set_grid_interpolation("nearest")


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero_eqa as E
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
out = {{}}
for ip in E.INTERPS:
    t.set_density_grid(E.T._field(), E.ROOM_LO, E.ROOM_HI, interpolation=ip)
    out["f64" + ip] = t.render(E._cfg())
    out["f32" + ip] = t.render(E._cfg(fp64=False))
    out["work" + ip] = np.array(t.count_work(E._cfg()), dtype=np.uint64)
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(et, orc_vm, tmp_path):
    """hetero_eqa_kernel against render_kernel_simple_eqa (a fresh process with VPT_SIMPLE_KERNEL=1) and against the
    in-order per-pixel sum of the per-sample call, bitwise, fp64 and fp32, nearest and trilinear; count_work is equal"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_eqa_kernel"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    imgs = {}
    try:
        for ip in INTERPS:
            et.set_density_grid(T._field(), ROOM_LO, ROOM_HI, interpolation=ip)
            img = imgs[ip] = et.render(_cfg())
            img32 = et.render(_cfg(fp64=False))
            assert bitwise_equal(img, simple["f64" + ip]).all(), f"{ip}: {(~bitwise_equal(img, simple['f64' + ip])).sum()} differ"
            assert bitwise_equal(img32, simple["f32" + ip]).all()
            L, _ = et.trace(EST, rays.reshape(-1), st.reshape(-1), SA, SS)
            L = L.reshape(H, W, SPP, 3)
            acc = np.zeros((H, W, 3))
            for s in range(SPP):
                acc = L[:, :, s] + acc
            want = acc * (1 / float(SPP))
            assert bitwise_equal(img, want).all(), f"{ip}: {(~bitwise_equal(img, want)).sum()} values differ from the sample sum"
            assert bitwise_equal(img32, want.astype(np.float32)).all()
            assert np.count_nonzero(img) > W * H
            work = et.count_work(_cfg())
            assert work == tuple(int(v) for v in simple["work" + ip]) and work[0] > 0 and work[1] > 0
            assert not bitwise_equal(img, et.render(_cfg("hetero"))).all()  # the estimator is not estimator 10
            # the majorant block is accepted and ignored
            et.set_majorant_block(2)
            assert bitwise_equal(et.render(_cfg()), img).all()
            et.set_majorant_block(0)
        assert not bitwise_equal(imgs["nearest"], imgs["trilinear"]).all()  # the interpolation is felt
        # shards: bands of 4 rows, two interleaved shards, reassembled
        whole = np.zeros_like(imgs["trilinear"])
        for off in (0, 1):
            shard = et.render(_cfg(band_rows=4, band_stride=2, band_offset=off))
            rows = [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]
            whole[rows] = shard
        assert bitwise_equal(whole, imgs["trilinear"]).all()
    finally:
        et.set_majorant_block(0)
        et.set_grid_interpolation("nearest")


def test_multi_tracer_equals_single(et):
    try:
        for ip in INTERPS:
            et.set_density_grid(T._field(), ROOM_LO, ROOM_HI, interpolation=ip)
            img = et.render(_cfg())
            m = MultiTracer(2, default_scene(), shared_device=True)
            try:
                with pytest.raises(VPTError) as ei:
                    m.render(_cfg())
                assert ei.value.code == _lib.VPT_E_INVALID  # no grid yet
                m.set_density_grid(T._field(), ROOM_LO, ROOM_HI, interpolation=ip)
                assert bitwise_equal(m.render(_cfg(band_rows=4)), img).all()
            finally:
                m.close()
    finally:
        et.set_grid_interpolation("nearest")


def test_same_expectation_as_estimator_10():
    """The shape of test_gpu_ratio.test_same_expectation_as_estimator_10: N = 2^20 camera samples of a 32 x 32 image per
    estimator, independent jitters and streams, the 2 x 3 x 2 field in the room box, scenes.big_light_scene.  Both
    estimators are unbiased for the same radiance, so the difference of the two sample means has the variance
    Var10 / N + Var12 / N, and
        |m12 - m10| <= 4.5 sqrt((M2_10 - m10^2) / N + (M2_12 - m12^2) / N)
    (4.5 standard deviations: 7e-6 two-sided).  Two conditions keep the test from passing vacuously, both asserted: the
    bound is at most 5 % of m10, and estimator 12 on the uniform field of _field().max() -- another medium -- lies
    outside the bound around m10.
    The medium is test_gpu_ratio.py's thin one (0.0002, 0.0018), not the bench's dense one (0.003, 0.027): at the dense
    medium the first condition fails -- measured there m10 = 1.447830, m12 = 1.462027, the bound 16.5 % of m10 (and
    |m12 - m10| 0.060 of it), with a per-sample rms / mean of 3.8 for estimator 10 and 36.9 for estimator 12: in a
    thick medium estimator 1's throughput sigma_s T / pdf over long equi-angular segments is heavy-tailed under the
    emissive ceiling, whose centre is 1e5 units away.  The dense figures are printed for the record and not asserted.
    Measured at the thin medium: m10 = 1.140005, m12 = 1.139474, |m12 - m10| = 5.31e-4 = 0.022 of the bound 2.381e-2
    (2.09 % of m10); rms / mean 3.11 and 3.59; the uniform field: m = 1.178337, 1.61 bounds away."""
    n_side, spp = 32, 1024
    f = T._field()
    lum = np.array([0.2126, 0.7152, 0.0722])
    r10, s10 = _camera_batch(n_side, spp, 101)
    r12, s12 = _camera_batch(n_side, spp, 303)
    N = len(r10)
    assert N == 1 << 20
    res = {}
    t = Tracer(0, big_light_scene())
    try:
        for name, (sa, ss) in (("dense", (SA, SS)), ("thin", (0.0002, 0.0018))):
            t.set_density_grid(f, ROOM_LO, ROOM_HI)
            l10 = t.trace("hetero", r10, s10, sa, ss)[0] @ lum
            l12 = t.trace(EST, r12, s12, sa, ss)[0] @ lum
            t.set_density_grid(np.full(f.shape, f.max(), np.float32), ROOM_LO, ROOM_HI)
            lu = t.trace(EST, r12, s12, sa, ss)[0] @ lum
            assert np.isfinite(l10).all() and np.isfinite(l12).all() and np.isfinite(lu).all()
            m10, m2_10, m12, m2_12, mu = l10.mean(), (l10 * l10).mean(), l12.mean(), (l12 * l12).mean(), lu.mean()
            bound = 4.5 * np.sqrt((m2_10 - m10 * m10) / N + (m2_12 - m12 * m12) / N)
            print(f"{name}: m10 = {m10:.6f}, m12 = {m12:.6f}, |m12 - m10| = {abs(m12 - m10):.3e}, bound = {bound:.3e} "
                  f"({100 * bound / m10:.2f} % of m10), fraction {abs(m12 - m10) / bound:.3f}; rms/mean 10: "
                  f"{np.sqrt(m2_10 - m10 * m10) / m10:.2f}, 12: {np.sqrt(m2_12 - m12 * m12) / m12:.2f}; uniform field: "
                  f"m = {mu:.6f}, {abs(mu - m10) / bound:.2f} bounds away")
            res[name] = (m10, m12, mu, bound)
    finally:
        t.close()
    m10, m12, mu, bound = res["thin"]
    assert m10 > 0 and bound <= 0.05 * m10  # the condition on the inputs
    assert abs(mu - m10) > bound            # another medium is told apart
    assert abs(m12 - m10) <= bound


def test_errors_and_clear():
    t = Tracer(0, default_scene())
    try:
        ff = RenderConfig(width=8, height=8, spp=4, estimator="ff", seed=SEED, fp64=True)
        before = t.render(ff)
        het = RenderConfig(width=8, height=8, spp=4, estimator=EST, seed=SEED, fp64=True)
        assert RenderConfig(width=8, height=8, spp=4, estimator="hetero_eqa").params().medium.estimator == _lib.HETERO_EQUIANGULAR
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, gm.states(1, 1)), lambda: t.count_work(het),
                     lambda: t.grid_eqa_probe(1.0, rays, 1.0, (0, 0, 0), gm.states(1, 1))):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        f = T._field()
        t.set_density_grid(f, ROOM_LO, ROOM_HI)
        img = t.render(het)
        assert img.any()
        imgs = {est: t.render(RenderConfig(width=8, height=8, spp=4, estimator=est, seed=SEED, fp64=True))
                for est in ("hetero", "hetero_ratio")}
        # an emission grid: estimator 12 alone refuses it
        t.set_emission_grid(np.full(f.shape, 0.5, np.float32), (1.0, 0.5, 0.25))
        for call in (lambda: t.render(het), lambda: t.trace(EST, rays, gm.states(1, 1)), lambda: t.count_work(het)):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        for est in ("hetero", "hetero_ratio"):
            lit = t.render(RenderConfig(width=8, height=8, spp=4, estimator=est, seed=SEED, fp64=True))
            assert np.isfinite(lit).all() and lit.sum() > imgs[est].sum()
        t.clear_emission_grid()
        assert bitwise_equal(t.render(het), img).all()
        for est in ("hetero", "hetero_ratio"):
            again = t.render(RenderConfig(width=8, height=8, spp=4, estimator=est, seed=SEED, fp64=True))
            assert bitwise_equal(again, imgs[est]).all()
        with pytest.raises(VPTError) as ei:
            t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator=EST))
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(het)
        assert ei.value.code == _lib.VPT_E_INVALID
        assert bitwise_equal(t.render(ff), before).all()
    finally:
        t.close()
