"""Volumetric emission on the GPU (Tracer.set_emission_grid; the EM = true kernels of csrc/vpt_hetero_em.hip and
csrc/vpt_hetero_em_tl.hip): the emitting tracks against their host build bit for bit, the persistent-wave kernels against
the one-lane-per-pixel kernels and the per-sample call, the draws and the eps == 0 image against the render without an
emission grid, a pure absorber and a ray into a light against closed forms, and the semantics of the setting.
Shapes are small: 16 x 12 x 8 spp images on a 6 x 5 x 4 cloud, 4096 samples per batch, 65 536 for the one mean."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emission_model as em
import grid_model as gm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import (MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_emission_probe_host)
from scenes import default_scene, sph

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
W, H, SPP, SEED = 16, 12, 8, 5
RGB = (0.9, 0.5, 0.25)
CASES = [(est, block, interp) for est in ("hetero", "hetero_ratio") for block in (0, 2) for interp in ("nearest", "trilinear")]


@pytest.fixture(scope="module")
def et():
    """a tracer of this module's own: its grids and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")
    t.close()


def _cfg(est="hetero", fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


def _cloud():
    """the 6 x 5 x 4 cloud in the room: (rho, eps), some voxels of each zero; eps scaled so that the glow is of the
    order of the lit room"""
    rho, eps = em.fields()
    return rho, eps * np.float32(40.0)


def test_probe_equals_the_host_build(et):
    rho, eps = em.fields()
    rays, tmax = em.rays()
    st = gm.states(7, len(rays))
    scored = 0
    for block in (0, 2):
        for interp in ("nearest", "trilinear"):
            et.set_density_grid(rho, em.LO, em.HI, majorant_block=block, interpolation=interp, emission=eps)
            for sigma_t in (0.7, 0.05):
                got = et.grid_emission_probe(sigma_t, rays, tmax, st)
                want = grid_emission_probe_host(rho, eps, em.LO, em.HI, sigma_t, rays, tmax, st, majorant_block=block,
                                                interpolation=interp)
                for name, g, w in zip(("t_coll", "esum", "states", "steps"), got, want):
                    assert bitwise_equal(g, w).all(), f"{name} (block {block}, {interp}, sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
                scored += int((want[1] > 0).sum())
    assert scored > 800  # the tracks score


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_emission as R
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
rho, eps = R._cloud()
out = {{}}
for est, block, interp in R.CASES:
    t.set_density_grid(rho, R.T.ROOM_LO, R.T.ROOM_HI, majorant_block=block, interpolation=interp, emission=eps, emission_rgb=R.RGB)
    out[f"{{est}}_{{block}}_{{interp}}_f64"] = t.render(R._cfg(est, True))
    out[f"{{est}}_{{block}}_{{interp}}_f32"] = t.render(R._cfg(est, False))
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(et, orc_vm, tmp_path):
    """the persistent-wave kernel, the one-lane-per-pixel kernel (VPT_SIMPLE_KERNEL=1, read when a render starts: a
    child process) and the per-pixel in-order sum of the per-sample call, bit for bit"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run the persistent-wave kernels"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    rho, eps = _cloud()
    for est, block, interp in CASES:
        et.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation=interp)
        dark = et.render(_cfg(est, True))
        et.set_emission_grid(eps, RGB)
        img64, img32 = et.render(_cfg(est, True)), et.render(_cfg(est, False))
        key = f"{est}_{block}_{interp}"
        assert bitwise_equal(img64, simple[key + "_f64"]).all(), key
        assert bitwise_equal(img32, simple[key + "_f32"]).all(), key
        L, _ = et.trace(est, rays.reshape(-1), st.reshape(-1), SA, SS)
        L = L.reshape(H, W, SPP, 3)
        acc = np.zeros((H, W, 3))
        for s in range(SPP):
            acc = L[:, :, s] + acc
        want = acc * (1 / float(SPP))
        assert bitwise_equal(img64, want).all(), f"{key}: {(~bitwise_equal(img64, want)).sum()} values differ"
        assert bitwise_equal(img32, want.astype(np.float32)).all(), key
        # the cloud glows: no pixel is darker than without the emission grid, most are brighter
        assert (img64 >= dark).all() and (img64 > dark).sum() > W * H


def test_emission_takes_no_draw(et, orc_vm):
    rays, st = T._batch(orc_vm)
    rho, eps = _cloud()
    for est, block, interp in CASES:
        et.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation=interp)
        L0, s0 = et.trace(est, rays, st, SA, SS)
        img0 = et.render(_cfg(est))
        work0 = et.count_work(_cfg(est))
        et.set_emission_grid(eps, RGB)
        L1, s1 = et.trace(est, rays, st, SA, SS)
        assert (s1 == s0).all(), f"{est}, {block}, {interp}: {(s1 != s0).sum()} end states differ"
        assert (L1 >= L0).all() and (L1 > L0).sum() > 2000
        assert et.count_work(_cfg(est)) == work0
        # eps == 0: the emitting kernels add +0 everywhere
        et.set_emission_grid(np.zeros_like(eps), RGB)
        Lz, sz = et.trace(est, rays, st, SA, SS)
        assert (sz == s0).all() and bitwise_equal(Lz, L0).all(), f"{est}, {block}, {interp}: {(~bitwise_equal(Lz, L0)).sum()} radiances differ"
        assert bitwise_equal(et.render(_cfg(est)), img0).all()
        # and without the grid the image is the original again
        et.set_emission_grid(eps, RGB)
        assert not bitwise_equal(et.render(_cfg(est)), img0).all()
        et.clear_emission_grid()
        assert bitwise_equal(et.render(_cfg(est)), img0).all()


def _far_light():
    """one emitter, far from every ray of the two tests below (the estimators end a path at once without one)"""
    return sph(1.0, (0.0, 1000.0, 0.0), rad=(1.0, 1.0, 1.0))


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_pure_absorber(est):
    """sigma_s = 0, rho == 1, eps == 1 on [0, 2] x [0, 1]^2, a ray along x through the box that hits nothing: the
    radiance is rgb (1 - exp(-sigma_a d)), d = 2.  65 536 samples; the mean within 4 standard errors of the sample.
    (The repeat at depth > 0 behind a mirror is left out: the conductor's Fresnel factor and roughness leave no closed
    form for the reflected segment's weight; test_equilibrium_radiance_needs_every_depth pins the later depths.)"""
    n, sa, d = 65536, 0.5, 2.0
    t = Tracer(0, _far_light())
    try:
        t.set_density_grid(np.ones((1, 1, 2), np.float32), (0, 0, 0), (d, 1, 1), emission=np.ones((1, 1, 2), np.float32),
                           emission_rgb=RGB)
        rays = np.zeros(n, dtype=gm.RAY_DTYPE)
        rays["o"], rays["d"] = (-5.0, 0.5, 0.5), (1.0, 0.0, 0.0)
        L, _ = t.trace(est, rays, gm.states(77, n), sa, 0.0)
    finally:
        t.close()
    want = np.array(RGB) * (1 - np.exp(-sa * d))
    mean, se = L.mean(axis=0), L.std(axis=0, ddof=1) / np.sqrt(n)
    print(f"{est}: mean {mean}, closed form {want}, off by {(mean - want) / se} standard errors")
    assert np.isfinite(L).all() and (se > 0).all()
    assert (np.abs(mean - want) <= 4 * se).all()


def test_equilibrium_radiance_needs_every_depth():
    """rho == 1, eps == 1 on [-4096, 4096]^3, sigma_a = sigma_s = 0.5: a medium that fills all a path can reach, emitting
    and absorbing at the same rate, has the radiance eps rgb in every direction (Kirchhoff).  The estimate of it is
    the sum over the depths k of rgb (sigma_a / sigma_t) albedo^k, so depth 0 gives half of it and the rest has to come
    from the later segments with the path's beta.  The emission's share of a sample is L(with eps) - L(without): the
    paths are the same.  65 536 samples; the mean within 4 standard errors of rgb, and the depth-0 term alone far outside."""
    n = 65536
    t = Tracer(0, _far_light())
    try:
        one = np.ones((2, 2, 2), np.float32)
        t.set_density_grid(one, T.BIG_LO, T.BIG_HI)
        rays = np.zeros(n, dtype=gm.RAY_DTYPE)
        rays["o"], rays["d"] = (0.3, -0.2, 0.1), (0.6, 0.0, 0.8)
        st = gm.states(78, n)
        L0, s0 = t.trace("hetero", rays, st, 0.5, 0.5)
        t.set_emission_grid(one, RGB)
        L1, s1 = t.trace("hetero", rays, st, 0.5, 0.5)
    finally:
        t.close()
    assert (s1 == s0).all() and np.isfinite(L1).all()
    glow = L1 - L0
    mean, se = glow.mean(axis=0), glow.std(axis=0, ddof=1) / np.sqrt(n)
    want = np.array(RGB)
    print(f"mean {mean}, eps rgb {want}, off by {(mean - want) / se} standard errors")
    assert (np.abs(mean - want) <= 4 * se).all()
    assert (np.abs(mean - 0.5 * want) > 20 * se).all()


def test_a_camera_ray_into_a_light_keeps_its_emission():
    """one ray through a two-density cloud (null collisions score) into an emitter.  Where the track ends without a
    collision the sample is the light's radiance plus the segment's term, rebuilt here from the host probe: the track
    starts two draws into the sample's stream (the roulette, the light pick)."""
    n, sa, ss = 4096, 0.1, 0.05
    rad = (3.0, 2.0, 1.0)
    rho, eps = em.expectation_fields()
    scene = np.concatenate([sph(2.0, (12.0, 0.7, 1.2), rad=rad)])
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"], rays["d"] = (-5.0, 0.7, 1.2), (1.0, 0.0, 0.0)
    st = gm.states(91, n)
    t = Tracer(0, scene)
    try:
        t.set_density_grid(rho, em.EX_LO, em.EX_HI)
        L0, s0 = t.trace("hetero", rays, st, sa, ss)
        t.set_emission_grid(eps, RGB)
        L1, s1 = t.trace("hetero", rays, st, sa, ss)
    finally:
        t.close()
    assert (s1 == s0).all()
    on_light = (L0 == np.array(rad)).all(axis=1)  # depth 0, no collision: the emitter alone
    assert on_light.sum() > 500
    at_track = np.array([gm.erand48_step(gm.erand48_step(x)[0])[0] for x in st], dtype=np.uint64)
    tc, esum, _, _ = grid_emission_probe_host(rho, eps, em.EX_LO, em.EX_HI, sa + ss, rays, 15.0, at_track)
    assert (tc[on_light] == -1).all()
    term = (np.array(RGB) * 1.0)[None, :] * (((sa / (sa + ss)) * esum) * (1 / 0.6))[:, None]
    want = (0.0 + term) + np.array(rad)[None, :]
    assert bitwise_equal(L1[on_light], want[on_light]).all()
    assert (esum[on_light] > 0).sum() > 200
    assert (L1[on_light] >= L0[on_light]).all() and (L1[on_light] > L0[on_light]).any(axis=1).sum() > 200


def test_resampled_fields_give_the_same_samples(et, orc_vm):
    """a 2 x 3 x 2 field with its eps and both resampled to 4 x 6 x 4: equal end states, radiances within the bound
    tests/test_gpu_hetero.py uses for the density alone"""
    rays, st = T._batch(orc_vm)
    f = T._field()
    e = np.random.default_rng(22).uniform(0.0, 60.0, f.shape).astype(np.float32)

    def twice(a):
        return np.repeat(np.repeat(np.repeat(a, 2, axis=0), 2, axis=1), 2, axis=2)

    et.set_density_grid(f, T.ROOM_LO, T.ROOM_HI, majorant_block=0, interpolation="nearest", emission=e, emission_rgb=RGB)
    La, sa = et.trace("hetero", rays, st, SA, SS)
    et.set_density_grid(twice(f), T.ROOM_LO, T.ROOM_HI, emission=twice(e), emission_rgb=RGB)
    Lb, sb = et.trace("hetero", rays, st, SA, SS)
    assert (sa == sb).all(), f"{(sa != sb).sum()} end states differ"
    ok = T._radiance_bound(La, Lb)
    print(f"max |La - Lb| = {np.abs(La - Lb).max():.3e}, max L = {La.max():.3e}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
    et.clear_emission_grid()
    assert (et.trace("hetero", rays, st, SA, SS)[0] < Lb).sum() > 2000  # the emission is felt


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_local_majorants_have_the_same_expectation(et, orc_vm, est):
    """other draws, the same estimator: the mean over 4096 camera samples with B = 0 against B = 2, within 4 combined
    standard errors taken from the per-sample values (sum of the channels)"""
    rays, st = T._batch(orc_vm)
    rho, eps = _cloud()
    v = []
    for block in (0, 2):
        et.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation="nearest", emission=eps, emission_rgb=RGB)
        v.append(et.trace(est, rays, st, SA, SS)[0].sum(axis=1))
    assert (v[0] != v[1]).sum() > 1000
    mean = [x.mean() for x in v]
    se = np.sqrt(sum(x.var(ddof=1) / len(x) for x in v))
    print(f"{est}: means {mean[0]:.5f}, {mean[1]:.5f}, combined standard error {se:.5f}")
    assert abs(mean[0] - mean[1]) <= 4 * se


def test_multi_tracer_equals_single(et):
    rho, eps = _cloud()
    m = MultiTracer(2, default_scene(), shared_device=True)
    try:
        for est, block, interp in (("hetero", 2, "trilinear"), ("hetero_ratio", 0, "nearest")):
            et.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation=interp)
            dark = et.render(_cfg(est))
            et.set_emission_grid(eps, RGB)
            single = et.render(_cfg(est))
            m.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation=interp, emission=eps, emission_rgb=RGB)
            assert bitwise_equal(m.render(_cfg(est, True, band_rows=4)), single).all(), est
            m.clear_emission_grid()
            assert bitwise_equal(m.render(_cfg(est, True, band_rows=4)), dark).all(), est
            m.set_emission_grid(eps, RGB)
            assert bitwise_equal(m.render(_cfg(est, True, band_rows=4)), single).all(), est
    finally:
        m.close()


def test_setting_semantics_and_errors():
    rho, eps = _cloud()
    t = Tracer(0, default_scene())
    try:
        # no density grid
        with pytest.raises(VPTError) as ei:
            t.set_emission_grid(eps, RGB)
        assert ei.value.code == _lib.VPT_E_INVALID and "density grid" in str(ei.value)
        t.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI)
        dark = t.render(_cfg())
        with pytest.raises(VPTError) as ei:  # no emission grid to probe
            t.grid_emission_probe(0.7, *em.rays(4), gm.states(1, 4))
        assert ei.value.code == _lib.VPT_E_INVALID
        t.set_emission_grid(eps, RGB)
        lit = t.render(_cfg())
        assert (lit >= dark).all() and (lit > dark).sum() > W * H
        # rejected arguments leave the emission grid as it was
        bad_eps = []
        for value in (np.nan, -1.0, np.inf):
            bad = eps.copy()
            bad[2, 1, 4] = value
            bad_eps.append((bad, RGB))
        for rgb in ((1.0, np.nan, 1.0), (1.0, 1.0, -0.5), (np.inf, 1.0, 1.0), (1.0, 1.0), (1.0, 1.0, 1.0, 1.0)):
            bad_eps.append((eps, rgb))
        for shape in ((4, 5, 5), (5, 4, 6), (120,)):
            bad_eps.append((np.ones(shape, np.float32), RGB))
        for e, rgb in bad_eps:
            with pytest.raises(VPTError) as ei:
                t.set_emission_grid(e, rgb)
            assert ei.value.code == _lib.VPT_E_INVALID
            assert bitwise_equal(t.render(_cfg()), lit).all()
        with pytest.raises(VPTError) as ei:
            t.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, emission=np.ones((4, 5, 5), np.float32))
        assert ei.value.code == _lib.VPT_E_INVALID
        assert bitwise_equal(t.render(_cfg()), lit).all()
        # the colour scales the glow channel by channel
        t.set_emission_grid(eps, (0.0, 0.5, 0.0))
        green = t.render(_cfg())
        assert bitwise_equal(green[..., 0], dark[..., 0]).all() and bitwise_equal(green[..., 2], dark[..., 2]).all()
        assert (green[..., 1] > dark[..., 1]).sum() > W * H // 2
        t.set_emission_grid(eps, RGB)
        # the block size and the interpolation leave the emission grid in place
        t.set_majorant_block(2)
        t.set_grid_interpolation("trilinear")
        a = t.render(_cfg())
        t.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI, emission=eps, emission_rgb=RGB)
        assert bitwise_equal(t.render(_cfg()), a).all()
        t.set_majorant_block(0)
        t.set_grid_interpolation("nearest")
        assert bitwise_equal(t.render(_cfg()), lit).all()
        # a new density grid, or none, drops it: its dimensions belong to the grid it came with
        t.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI)
        assert bitwise_equal(t.render(_cfg()), dark).all()
        t.set_emission_grid(eps, RGB)
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.set_emission_grid(eps, RGB)
        assert ei.value.code == _lib.VPT_E_INVALID
        t.set_density_grid(rho, T.ROOM_LO, T.ROOM_HI)
        assert bitwise_equal(t.render(_cfg()), dark).all()
        # the accumulator still refuses both estimators
        t.set_emission_grid(eps, RGB)
        for est in ("hetero", "hetero_ratio"):
            with pytest.raises(VPTError) as ei:
                t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator=est))
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
    finally:
        t.close()
