"""Estimator 10 (heterogeneous medium: density grid, delta tracking) on the GPU: the grid walkers against their
host build bit for bit, the reduction to estimator 0 on uniform grids, voxel indexing on a resampled field,
the persistent-wave kernel against the one-lane-per-pixel kernel and the per-sample call, and the errors.
Shapes are small: 4096 samples per batch, 24 x 20 x 8 spp images (neither side a multiple of 8 or 16)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_probe_host
from scenes import default_scene, stream_state

pytestmark = pytest.mark.gpu

SA, SS = 0.003, 0.027          # bench.py's dense medium: the medium matters
BIG_LO, BIG_HI = (-4096.0,) * 3, (4096.0,) * 3
ROOM_LO, ROOM_HI = (-60.0, -50.0, -100.0), (60.0, 50.0, 230.0)  # contains the room and the camera
W, H, SPP, SEED = 24, 20, 8, 5


@pytest.fixture(scope="module")
def ht():
    """a tracer of this module's own: the grid it sets never reaches the other modules' tracer"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


_CACHE = {}


def _camera_samples(orc_vm, w, h, spp, seed):
    """(rays, states after the camera draws) of every sample of a w x h x spp image, [file row, x, sample]"""
    key = ("cam", w, h, spp, seed)
    if key not in _CACHE:
        rays = np.zeros((h, w, spp), dtype=gm.RAY_DTYPE)
        st = np.zeros((h, w, spp), dtype=np.uint64)
        for fr in range(h):
            for x in range(w):
                for s in range(spp):
                    r, st[fr, x, s] = orc_vm.camera_ray(w, h, x, h - 1 - fr, stream_state(seed, fr * w + x, s))
                    rays[fr, x, s]["o"], rays[fr, x, s]["d"] = r[:3], r[3:]
        rays.setflags(write=False)
        st.setflags(write=False)
        _CACHE[key] = (rays, st)
    return _CACHE[key]


def _batch(orc_vm):
    """4096 camera samples (64 x 64 x 1)"""
    rays, st = _camera_samples(orc_vm, 64, 64, 1, 3)
    return rays.reshape(-1), st.reshape(-1)


def _field():
    """the non-uniform field of tests 7 and 8: 2 x 3 x 2 voxels, rho in [0.2, 1]"""
    return np.random.default_rng(21).uniform(0.2, 1.0, (2, 3, 2)).astype(np.float32)


def _radiance_bound(a, b):
    """|a - b| <= 1e-10 max(|a|, |b|, the sample's largest channel): each transmittance's exponent is off by at
    most sigma_t tau (cells + 2) 2^-53 (about 2e-13 at these box sizes), at most three such factors per term, the
    terms sums of non-negative quantities -- 1e-10 leaves more than two orders"""
    scale = np.maximum(np.abs(a), np.abs(b)).max(axis=1, keepdims=True)
    return np.abs(a - b) <= 1e-10 * np.maximum(np.maximum(np.abs(a), np.abs(b)), scale)


def test_probe_equals_host_build(ht):
    rho = gm.tau_grid()
    rays, tmax = gm.tau_rays()
    st = gm.states(3, len(rays))
    ht.set_density_grid(rho, gm.TAU_LO, gm.TAU_HI)
    for sigma_t in (0.7, 0.05):
        got = ht.grid_probe(sigma_t, rays, tmax, st)
        want = grid_probe_host(rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, st)
        for name, g, w in zip(("tau", "t_coll", "states"), got, want):
            assert bitwise_equal(g, w).all(), f"{name} (sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
    assert (want[1] >= 0).sum() > 200 and (want[1] == -1).sum() > 200
    n = 4096
    rays, tmax = gm.ks_rays(n)
    st = gm.states(gm.KS_SEED, n)
    ht.set_density_grid(gm.KS_RHO, gm.KS_LO, gm.KS_HI)
    got = ht.grid_probe(gm.KS_SIGMA_T, rays, tmax, st)
    want = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, st)
    for g, w in zip(got, want):
        assert bitwise_equal(g, w).all()


@pytest.mark.parametrize("rho", [1.0, 2.0])
def test_uniform_grid_reduces_to_estimator_0(ht, orc_vm, rho):
    """uniform rho on [-4096, 4096]^3 (4^3 voxels): estimator 10 walks estimator 0's paths at (rho sigma_a,
    rho sigma_s) with the same draws -- equal end states, radiances within the rounding of tau.  At sigma_t = 0.03
    an escaping ray leaves the box uncollided with probability < e^-100, so estimator 0's always-collide-on-a-miss
    rule is met on every sample."""
    rays, st = _batch(orc_vm)
    ht.set_density_grid(np.full((4, 4, 4), rho, np.float32), BIG_LO, BIG_HI)
    L10, s10 = ht.trace("hetero", rays, st, SA, SS)
    L0, s0 = ht.trace("ff", rays, st, rho * SA, rho * SS)
    assert (s10 == s0).all(), f"{(s10 != s0).sum()} end states differ"
    ok = _radiance_bound(L10, L0)
    print(f"rho {rho}: max |L10 - L0| = {np.abs(L10 - L0).max():.3e}, max L = {L0.max():.3e}, nonzero {np.count_nonzero(L0.any(axis=1))}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound, worst {np.abs(L10 - L0).max():.3e}"
    assert np.count_nonzero(L0.any(axis=1)) > 2000  # the samples carry light
    if rho == 1.0:
        cfg = dict(width=16, height=16, spp=4, sigma_a=SA, sigma_s=SS, seed=SEED)
        assert ht.count_work(RenderConfig(estimator="hetero", **cfg)) == ht.count_work(RenderConfig(estimator="ff", **cfg))


def test_resampled_field_gives_the_same_samples(ht, orc_vm):
    """a 2 x 3 x 2 field and the same field resampled to 4 x 6 x 4 (each voxel repeated 2 x 2 x 2): equal end
    states, radiances within the bound of the reduction test"""
    rays, st = _batch(orc_vm)
    f = _field()
    ht.set_density_grid(f, ROOM_LO, ROOM_HI)
    La, sa = ht.trace("hetero", rays, st, SA, SS)
    ht.set_density_grid(np.repeat(np.repeat(np.repeat(f, 2, axis=0), 2, axis=1), 2, axis=2), ROOM_LO, ROOM_HI)
    Lb, sb = ht.trace("hetero", rays, st, SA, SS)
    assert (sa == sb).all(), f"{(sa != sb).sum()} end states differ"
    ok = _radiance_bound(La, Lb)
    print(f"max |La - Lb| = {np.abs(La - Lb).max():.3e}, max L = {La.max():.3e}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
    # the field is felt: the uniform field of the same maximum gives other paths
    ht.set_density_grid(np.full((2, 3, 2), f.max(), np.float32), ROOM_LO, ROOM_HI)
    assert (ht.trace("hetero", rays, st, SA, SS)[1] != sa).any()


def _cfg(fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator="hetero", sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero as T
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI)
np.savez({out!r}, f64=t.render(T._cfg(True)), f32=t.render(T._cfg(False)))
t.close()
"""


def _simple_kernel_images(tmp_path):
    """the render of render_kernel_simple_hetero: a fresh process with VPT_SIMPLE_KERNEL=1"""
    out = str(tmp_path / "simple.npz")
    env = dict(os.environ, VPT_SIMPLE_KERNEL="1")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=300)
    return np.load(out)


def test_kernels_agree(ht, orc_vm, tmp_path):
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_kernel"
    ht.set_density_grid(_field(), ROOM_LO, ROOM_HI)
    img64, img32 = ht.render(_cfg(True)), ht.render(_cfg(False))
    simple = _simple_kernel_images(tmp_path)
    assert bitwise_equal(img64, simple["f64"]).all() and bitwise_equal(img32, simple["f32"]).all()
    # the per-pixel sequential sum of the per-sample call on the same streams
    rays, st = _camera_samples(orc_vm, W, H, SPP, SEED)
    L, _ = ht.trace("hetero", rays.reshape(-1), st.reshape(-1), SA, SS)
    L = L.reshape(H, W, SPP, 3)
    acc = np.zeros((H, W, 3))
    for s in range(SPP):
        acc = L[:, :, s] + acc
    want = acc * (1 / float(SPP))
    assert bitwise_equal(img64, want).all(), f"{(~bitwise_equal(img64, want)).sum()} values differ from the sample sum"
    assert bitwise_equal(img32, want.astype(np.float32)).all()
    assert np.count_nonzero(img64) > W * H
    # shards: bands of 4 rows, two interleaved shards, reassembled
    whole = np.zeros_like(img64)
    for off in (0, 1):
        shard = ht.render(_cfg(True, band_rows=4, band_stride=2, band_offset=off))
        rows = [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]
        assert shard.shape[0] == len(rows)
        whole[rows] = shard
    assert bitwise_equal(whole, img64).all()


def test_multi_tracer_equals_single(ht):
    ht.set_density_grid(_field(), ROOM_LO, ROOM_HI)
    img = ht.render(_cfg(True))
    m = MultiTracer(2, default_scene(), shared_device=True)
    try:
        with pytest.raises(VPTError) as ei:
            m.render(_cfg(True))
        assert ei.value.code == _lib.VPT_E_INVALID  # no grid yet
        m.set_density_grid(_field(), ROOM_LO, ROOM_HI)
        assert bitwise_equal(m.render(_cfg(True, band_rows=4)), img).all()
    finally:
        m.close()


def test_errors_and_clear():
    t = Tracer(0, default_scene())
    try:
        ff = RenderConfig(width=8, height=8, spp=4, estimator="ff", seed=SEED, fp64=True)
        before = t.render(ff)
        het = RenderConfig(width=8, height=8, spp=4, estimator="hetero", seed=SEED, fp64=True)
        rays = np.zeros(1, dtype=gm.RAY_DTYPE)
        rays["d"] = (0, 0, -1)
        for call in (lambda: t.render(het), lambda: t.trace("hetero", rays, gm.states(1, 1)), lambda: t.count_work(het),
                     lambda: t.grid_probe(1.0, rays, 1.0, gm.states(1, 1))):
            with pytest.raises(VPTError) as ei:
                call()
            assert ei.value.code == _lib.VPT_E_INVALID
        with pytest.raises(VPTError) as ei:
            t.set_density_grid(np.full((2, 2, 2), np.nan), (0, 0, 0), (1, 1, 1))
        assert ei.value.code == _lib.VPT_E_INVALID
        t.set_density_grid(_field(), ROOM_LO, ROOM_HI)
        t.set_scene(default_scene())  # the grid persists across set_scene
        assert t.render(het).any()
        with pytest.raises(VPTError) as ei:
            t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator="hetero"))
        assert ei.value.code == _lib.VPT_E_UNSUPPORTED
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(het)
        assert ei.value.code == _lib.VPT_E_INVALID
        assert bitwise_equal(t.render(ff), before).all()
        for est in ("mis", "surface_pt", "ray_marching", "ray_marching_explicit"):
            assert np.isfinite(t.render(RenderConfig(width=8, height=8, spp=2, estimator=est, seed=SEED))).all()
    finally:
        t.close()
