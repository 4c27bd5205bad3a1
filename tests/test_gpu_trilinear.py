"""Trilinear density interpolation on the GPU (Tracer.set_grid_interpolation; the TL = true kernels of
csrc/vpt_hetero_tl.hip): the walkers against their host build bit for bit, the reduction to the nearest lookup on a
uniform grid, the persistent-wave kernels against the one-lane-per-pixel kernels and the per-sample call, and the
semantics of the setting.  Shapes are test_gpu_hetero.py's: 4096 samples per batch, 24 x 20 x 8 spp images."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import (MultiTracer, RenderConfig, Tracer, VPTError, _lib, grid_probe_host,
                                                grid_ratio_probe_host)
from scenes import default_scene

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
W, H, SPP, SEED = T.W, T.H, T.SPP, T.SEED
CASES = [(est, block) for est in ("hetero", "hetero_ratio") for block in (0, 2)]


@pytest.fixture(scope="module")
def tt():
    """a tracer of this module's own: its grid and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _cfg(est="hetero", fp64=True, **kw):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=SA, sigma_s=SS, seed=SEED, fp64=fp64, **kw)


def test_probes_equal_the_host_build(tt):
    sets = []
    rays, tmax = gm.tau_rays()
    for sigma_t in (0.7, 0.05):
        sets.append((gm.tau_grid(), gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, gm.states(3, len(rays))))
    rays, tmax = gm.ks_rays(4096)
    sets.append((gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, gm.states(gm.KS_SEED, 4096)))
    differ = 0
    for rho, lo, hi, sigma_t, rays, tmax, st in sets:
        for block in (0, 2, 8):
            tt.set_density_grid(rho, lo, hi, majorant_block=block, interpolation="trilinear")
            got = tt.grid_probe(sigma_t, rays, tmax, st, return_steps=True)
            want = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, majorant_block=block, return_steps=True,
                                   interpolation="trilinear")
            for name, g, w in zip(("tau", "t_coll", "states", "steps"), got, want):
                assert bitwise_equal(g, w).all(), f"{name} (sigma_t {sigma_t}, block {block}): {(~bitwise_equal(g, w)).sum()} differ"
            assert bitwise_equal(tt.grid_probe(sigma_t, rays, tmax, st)[1], want[1]).all()
            got = tt.grid_ratio_probe(sigma_t, rays, tmax, st)
            want_r = grid_ratio_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, majorant_block=block, interpolation="trilinear")
            for name, g, w in zip(("That", "states", "steps"), got, want_r):
                assert bitwise_equal(g, w).all(), f"ratio {name} (sigma_t {sigma_t}, block {block}): {(~bitwise_equal(g, w)).sum()} differ"
        near = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st)
        differ += int((near[0] != want[0]).sum())
    assert differ > 1000  # the device ran the trilinear walkers, not the nearest ones
    tt.set_majorant_block(0)
    tt.set_grid_interpolation("nearest")


def test_uniform_grid_reduces_to_nearest(tt, orc_vm):
    """rho == 1 on [-4096, 4096]^3, 4^3 voxels: every lookup is 1.0 either way, so the draws are the same; estimator 11
    has no deterministic factor and is equal bit for bit, estimator 10 differs in the rounding of tau only"""
    rays, st = T._batch(orc_vm)
    work = dict(width=16, height=16, spp=4, sigma_a=SA, sigma_s=SS, seed=SEED)
    tt.set_density_grid(np.ones((4, 4, 4), np.float32), T.BIG_LO, T.BIG_HI, majorant_block=0, interpolation="nearest")
    near = {est: tt.trace(est, rays, st, SA, SS) for est in ("hetero", "hetero_ratio")}
    near_work = {est: tt.count_work(RenderConfig(estimator=est, **work)) for est in ("hetero", "hetero_ratio")}
    tt.set_grid_interpolation("trilinear")
    try:
        L, s = tt.trace("hetero_ratio", rays, st, SA, SS)
        assert (s == near["hetero_ratio"][1]).all() and bitwise_equal(L, near["hetero_ratio"][0]).all()
        L, s = tt.trace("hetero", rays, st, SA, SS)
        assert (s == near["hetero"][1]).all(), f"{(s != near['hetero'][1]).sum()} end states differ"
        ok = T._radiance_bound(L, near["hetero"][0])
        print(f"max |L_tl - L_nearest| = {np.abs(L - near['hetero'][0]).max():.3e}, max L = {L.max():.3e}")
        assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
        assert np.count_nonzero(L.any(axis=1)) > 2000
        for est in ("hetero", "hetero_ratio"):
            assert tt.count_work(RenderConfig(estimator=est, **work)) == near_work[est]
    finally:
        tt.set_grid_interpolation("nearest")


def test_the_field_is_felt(tt, orc_vm):
    rays, st = T._batch(orc_vm)
    tt.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI, majorant_block=0, interpolation="nearest")
    near = {est: tt.trace(est, rays, st, SA, SS)[1] for est in ("hetero", "hetero_ratio")}
    tt.set_grid_interpolation("trilinear")
    try:
        for est in ("hetero", "hetero_ratio"):
            assert (tt.trace(est, rays, st, SA, SS)[1] != near[est]).any(), est
    finally:
        tt.set_grid_interpolation("nearest")


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_trilinear as R
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
out = {{}}
for est, block in R.CASES:
    t.set_density_grid(R.T._field(), R.T.ROOM_LO, R.T.ROOM_HI, majorant_block=block, interpolation="trilinear")
    out[f"{{est}}_{{block}}_f64"] = t.render(R._cfg(est, True))
    out[f"{{est}}_{{block}}_f32"] = t.render(R._cfg(est, False))
np.savez({out!r}, **out)
t.close()
"""


def test_kernels_agree(tt, orc_vm, tmp_path):
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run the persistent-wave kernels"
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    try:
        for est, block in CASES:
            tt.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI, majorant_block=block, interpolation="trilinear")
            img64, img32 = tt.render(_cfg(est, True)), tt.render(_cfg(est, False))
            assert bitwise_equal(img64, simple[f"{est}_{block}_f64"]).all(), (est, block)
            assert bitwise_equal(img32, simple[f"{est}_{block}_f32"]).all(), (est, block)
            # the per-pixel sequential sum of the per-sample call on the same streams
            L, _ = tt.trace(est, rays.reshape(-1), st.reshape(-1), SA, SS)
            L = L.reshape(H, W, SPP, 3)
            acc = np.zeros((H, W, 3))
            for s in range(SPP):
                acc = L[:, :, s] + acc
            want = acc * (1 / float(SPP))
            assert bitwise_equal(img64, want).all(), f"{est}, block {block}: {(~bitwise_equal(img64, want)).sum()} values differ"
            assert bitwise_equal(img32, want.astype(np.float32)).all()
            assert np.count_nonzero(img64) > W * H
            # shards: bands of 4 rows, two interleaved shards, reassembled
            whole = np.zeros_like(img64)
            for off in (0, 1):
                shard = tt.render(_cfg(est, True, band_rows=4, band_stride=2, band_offset=off))
                rows = [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]
                assert shard.shape[0] == len(rows)
                whole[rows] = shard
            assert bitwise_equal(whole, img64).all(), (est, block)
    finally:
        tt.set_majorant_block(0)
        tt.set_grid_interpolation("nearest")


def test_setting_semantics():
    t = Tracer(0, default_scene())
    try:
        cfgs = [_cfg("hetero"), _cfg("hetero_ratio")]
        t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI)
        near = [t.render(c) for c in cfgs]
        t.set_grid_interpolation("trilinear")
        tri = [t.render(c) for c in cfgs]
        assert all((a != b).any() for a, b in zip(near, tri))
        t.set_grid_interpolation("nearest")
        assert all(bitwise_equal(t.render(c), a).all() for c, a in zip(cfgs, near))
        # the mode belongs to the tracer: it survives a new grid and a clear
        t.set_grid_interpolation("trilinear")
        t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI)
        assert all(bitwise_equal(t.render(c), a).all() for c, a in zip(cfgs, tri))
        t.clear_density_grid()
        with pytest.raises(VPTError) as ei:
            t.render(cfgs[0])
        assert ei.value.code == _lib.VPT_E_INVALID
        t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI)
        assert all(bitwise_equal(t.render(c), a).all() for c, a in zip(cfgs, tri))
        # an invalid mode changes nothing
        for bad in (-1, 2):
            assert _lib.lib().vpt_set_grid_interpolation(t._ctx, bad) == _lib.VPT_E_INVALID
            assert _lib.lib().vpt_last_error()
        for name in ("cubic", None):
            with pytest.raises(VPTError) as ei:
                t.set_grid_interpolation(name)
            assert ei.value.code == _lib.VPT_E_INVALID
        with pytest.raises(VPTError) as ei:
            t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI, interpolation="cubic")
        assert ei.value.code == _lib.VPT_E_INVALID
        assert all(bitwise_equal(t.render(c), a).all() for c, a in zip(cfgs, tri))
        # the majorant grid follows the mode: a block set under nearest is rebuilt dilated
        t.set_grid_interpolation("nearest")
        t.set_majorant_block(2)
        t.set_grid_interpolation("trilinear")
        a = t.render(cfgs[0])
        t.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI, majorant_block=2, interpolation="trilinear")
        assert bitwise_equal(t.render(cfgs[0]), a).all()
        t.set_majorant_block(0)
        # several ranks
        m = MultiTracer(2, default_scene(), shared_device=True)
        try:
            m.set_grid_interpolation("trilinear")
            m.set_density_grid(T._field(), T.ROOM_LO, T.ROOM_HI)
            for c, a in zip(cfgs, tri):
                assert bitwise_equal(m.render(_cfg(c.estimator, True, band_rows=4)), a).all()
            with pytest.raises(VPTError) as ei:
                m.set_grid_interpolation("cubic")
            assert ei.value.code == _lib.VPT_E_INVALID
        finally:
            m.close()
        # the accumulator still refuses both estimators
        for est in ("hetero", "hetero_ratio"):
            with pytest.raises(VPTError) as ei:
                t.accumulator(RenderConfig(width=8, height=8, spp=4, estimator=est))
            assert ei.value.code == _lib.VPT_E_UNSUPPORTED
    finally:
        t.close()
