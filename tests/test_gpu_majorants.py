"""Local majorants for the delta tracking of estimator 10 on the GPU (vpt_set_grid_majorant_block): the probe
against its host build bit for bit, the reduction to the global majorant with one super-voxel (per-sample call
and render), a resampled field with the block doubled, hetero_kernel<LM> against render_kernel_simple_hetero, the
per-sample call, shards and the multi-tracer, the step counts, and the estimator's mean.  Shapes are those of
tests/test_gpu_hetero.py: 4096 samples per batch, 24 x 20 x 8 spp images."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
import test_gpu_hetero as T
from conftest import ROOT, bitwise_equal
from minimal_volumetric_path_tracer_amd import MultiTracer, Tracer, VPTError, _lib, grid_probe_host, lib
from scenes import default_scene

pytestmark = pytest.mark.gpu

SA, SS = T.SA, T.SS
ROOM_LO, ROOM_HI = T.ROOM_LO, T.ROOM_HI
KERNEL_BLOCK = 2


def sparse_room_field():
    """6 x 5 x 4 voxels, about half of them empty, for the room box"""
    return mm.sparse_field((4, 5, 6), seed=34)


@pytest.fixture(scope="module")
def mt():
    """a tracer of this module's own: its grid and its block size never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.close()


def _probe_inputs(which):
    """(rho, lo, hi, rays, tmax, states, the sigma_t values): the two sets of tests/test_grid_host.py's test 1 --
    the tau grid and rays, and the 65 536 KS tracks through rho = (1, 3) (block 1: two super-voxels, block 2: one)
    -- and the sparse field of the inversion test"""
    if which == "tau":
        rays, tmax = gm.tau_rays()
        return gm.tau_grid(), gm.TAU_LO, gm.TAU_HI, rays, tmax, gm.states(3, len(rays)), (0.7, 0.05)
    if which == "ks":
        rays, tmax = gm.ks_rays()
        return gm.KS_RHO, gm.KS_LO, gm.KS_HI, rays, tmax, gm.states(gm.KS_SEED, gm.KS_N), (gm.KS_SIGMA_T,)
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    return mm.sparse_field(), mm.SPARSE_LO, mm.SPARSE_HI, rays, tmax, gm.states(11, len(rays)), (0.7, 0.05)


@pytest.mark.parametrize("which", ["tau", "ks", "sparse"])
def test_probe_equals_host_build(mt, which):
    rho, lo, hi, rays, tmax, st, sigmas = _probe_inputs(which)
    for b in (0, 1, 2, max(rho.shape)):
        mt.set_density_grid(rho, lo, hi, majorant_block=b)
        for sigma_t in sigmas:
            got = mt.grid_probe(sigma_t, rays, tmax, st, return_steps=True)
            want = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, majorant_block=b, return_steps=True)
            for name, g, w in zip(("tau", "t_coll", "states", "steps"), got, want):
                assert bitwise_equal(g, w).all(), f"{name} (block {b}, sigma_t {sigma_t}): {(~bitwise_equal(g, w)).sum()} differ"
        if which != "ks":
            assert (want[1] >= 0).sum() > 200 and (want[1] == -1).sum() > 200
    # the probe without the suffix keeps the global majorant whatever the context's block size
    mt.set_majorant_block(1)
    tau, tc, so = (np.zeros(len(rays)), np.zeros(len(rays)), np.zeros(len(rays), np.uint64))
    _lib.check(lib().vpt_grid_probe(mt._ctx, sigmas[0], rays.ctypes.data, np.ascontiguousarray(tmax).ctypes.data, st.ctypes.data,
                                    len(rays), tau.ctypes.data, tc.ctypes.data, so.ctypes.data))
    for g, w in zip((tau, tc, so), grid_probe_host(rho, lo, hi, sigmas[0], rays, tmax, st)):
        assert bitwise_equal(g, w).all()
    mt.set_majorant_block(0)


def test_one_super_voxel_reduces_to_the_global_majorant(mt, orc_vm):
    """block >= max(n): the per-sample call (radiance and end states) and the render are those of block 0, bitwise"""
    rays, st = T._batch(orc_vm)
    f = T._field()
    mt.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=0)
    L0, s0 = mt.trace("hetero", rays, st, SA, SS)
    img0 = mt.render(T._cfg(True))
    assert np.count_nonzero(L0.any(axis=1)) > 2000
    for b in (max(f.shape), max(f.shape) + 2):
        mt.set_majorant_block(b)
        L, s = mt.trace("hetero", rays, st, SA, SS)
        assert (s == s0).all() and bitwise_equal(L, L0).all()
        assert bitwise_equal(mt.render(T._cfg(True)), img0).all()
    mt.set_majorant_block(0)


def test_resampled_field_with_the_block_doubled(mt, orc_vm):
    """the 2 x 3 x 2 field at block 1 and its 2 x 2 x 2 resampling at block 2: the same super-voxels (the planes
    coincide exactly: the cells differ by a factor of two), so equal end states and radiances within the bound
    of tests/test_gpu_hetero.py's resampling test"""
    rays, st = T._batch(orc_vm)
    f = T._field()
    mt.set_density_grid(f, ROOM_LO, ROOM_HI, majorant_block=1)
    La, sa = mt.trace("hetero", rays, st, SA, SS)
    mt.set_density_grid(mm.resample2(f), ROOM_LO, ROOM_HI, majorant_block=2)
    Lb, sb = mt.trace("hetero", rays, st, SA, SS)
    assert (sa == sb).all(), f"{(sa != sb).sum()} end states differ"
    ok = T._radiance_bound(La, Lb)
    print(f"max |La - Lb| = {np.abs(La - Lb).max():.3e}, max L = {La.max():.3e}")
    assert ok.all(), f"{(~ok).sum()} channels beyond the bound"
    # the block is felt: the global majorant walks other paths on this field
    mt.set_majorant_block(0)
    assert (mt.trace("hetero", rays, st, SA, SS)[1] != sb).any()


_CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_hetero as T
import test_gpu_majorants as M
from minimal_volumetric_path_tracer_amd import Tracer
from scenes import default_scene
t = Tracer(0, default_scene())
t.set_density_grid(M.sparse_room_field(), M.ROOM_LO, M.ROOM_HI, majorant_block=M.KERNEL_BLOCK)
np.savez({out!r}, f64=t.render(T._cfg(True)), f32=t.render(T._cfg(False)))
t.close()
"""


def test_kernels_agree_with_local_majorants(mt, orc_vm, tmp_path):
    """block 2 on the sparse 6 x 5 x 4 field: hetero_kernel<LM> against render_kernel_simple_hetero (a fresh process
    with VPT_SIMPLE_KERNEL=1), the in-order per-pixel sum of the per-sample call, the two-shard reassembly and the
    multi-tracer, bitwise (the pattern of tests/test_gpu_hetero.py's test_kernels_agree)"""
    assert not os.environ.get("VPT_SIMPLE_KERNEL"), "this process must run hetero_kernel"
    W, H, SPP = T.W, T.H, T.SPP
    mt.set_density_grid(sparse_room_field(), ROOM_LO, ROOM_HI, majorant_block=KERNEL_BLOCK)
    img64, img32 = mt.render(T._cfg(True)), mt.render(T._cfg(False))
    out = str(tmp_path / "simple.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VPT_SIMPLE_KERNEL="1"), timeout=300)
    simple = np.load(out)
    assert bitwise_equal(img64, simple["f64"]).all() and bitwise_equal(img32, simple["f32"]).all()
    rays, st = T._camera_samples(orc_vm, W, H, SPP, T.SEED)
    L, _ = mt.trace("hetero", rays.reshape(-1), st.reshape(-1), SA, SS)
    L = L.reshape(H, W, SPP, 3)
    acc = np.zeros((H, W, 3))
    for s in range(SPP):
        acc = L[:, :, s] + acc
    want = acc * (1 / float(SPP))
    assert bitwise_equal(img64, want).all(), f"{(~bitwise_equal(img64, want)).sum()} values differ from the sample sum"
    assert bitwise_equal(img32, want.astype(np.float32)).all()
    assert np.count_nonzero(img64) > W * H
    for fp64, img in ((True, img64), (False, img32)):
        whole = np.zeros_like(img)
        for off in (0, 1):
            shard = mt.render(T._cfg(fp64, band_rows=4, band_stride=2, band_offset=off))
            rows = [fr for b in range(off, (H + 3) // 4, 2) for fr in range(b * 4, min(H, (b + 1) * 4))]
            assert shard.shape[0] == len(rows)
            whole[rows] = shard
        assert bitwise_equal(whole, img).all()
    m = MultiTracer(2, default_scene(), shared_device=True)
    try:
        m.set_majorant_block(KERNEL_BLOCK)  # before the grid: applied when it arrives
        m.set_density_grid(sparse_room_field(), ROOM_LO, ROOM_HI)
        assert bitwise_equal(m.render(T._cfg(True, band_rows=4)), img64).all()
        assert bitwise_equal(m.render(T._cfg(False, band_rows=4)), img32).all()
        m.set_majorant_block(0)
        mt.set_majorant_block(0)
        img0 = mt.render(T._cfg(True))
        assert not bitwise_equal(img0, img64).all()  # the block is felt
        assert bitwise_equal(m.render(T._cfg(True, band_rows=4)), img0).all()
    finally:
        m.close()


def _steps_per_track(tracer, rays, st):
    """(radiances, tentative steps per delta-tracking call) of the per-sample call (vpt_debug_hetero_steps)"""
    f = lib().vpt_debug_hetero_steps
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_lib.vpt_medium)] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + \
        [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 2
    rays, st = np.ascontiguousarray(rays), np.ascontiguousarray(st)
    out = np.zeros((len(rays), 3))
    tracks, steps = ctypes.c_uint64(), ctypes.c_uint64()
    m = T._cfg(True).medium()
    _lib.check(f(tracer._ctx, ctypes.byref(m), rays.ctypes.data, st.ctypes.data, len(rays), out.ctypes.data,
                 ctypes.byref(tracks), ctypes.byref(steps)))
    assert tracks.value > len(rays)
    return out, steps.value / tracks.value


def test_fewer_steps_and_the_same_mean(mt, orc_vm):
    """the 4096 camera samples on the sparse field at block 0 and block 2: strictly fewer tentative steps per track
    (the paths differ, so the track counts do: the ratios are compared), and mean luminances within 5 combined
    standard errors (the same estimator in distribution; the inputs are fixed, so z is deterministic)"""
    rays, st = T._batch(orc_vm)
    res = {}
    for b in (0, KERNEL_BLOCK):
        mt.set_density_grid(sparse_room_field(), ROOM_LO, ROOM_HI, majorant_block=b)
        L, per_track = _steps_per_track(mt, rays, st)
        Lt, _ = mt.trace("hetero", rays, st, SA, SS)
        assert bitwise_equal(L, Lt).all()  # counting does not change the samples
        lum = L @ np.array([0.2126, 0.7152, 0.0722])
        res[b] = (per_track, lum.mean(), lum.std(ddof=1) / np.sqrt(len(lum)))
    mt.set_majorant_block(0)
    (p0, m0, e0), (p2, m2, e2) = res[0], res[KERNEL_BLOCK]
    z = abs(m0 - m2) / np.sqrt(e0 * e0 + e2 * e2)
    print(f"steps per track: block 0 {p0:.3f}, block {KERNEL_BLOCK} {p2:.3f}; mean luminance {m0:.6f} +- {e0:.6f} / "
          f"{m2:.6f} +- {e2:.6f}, z = {z:.3f}")
    assert p2 < p0
    assert m0 > 0 and m2 > 0
    assert z <= 5.0


def test_setting_belongs_to_the_context():
    t = Tracer(0, default_scene())
    try:
        with pytest.raises(VPTError) as ei:
            t.set_majorant_block(-1)
        assert ei.value.code == _lib.VPT_E_INVALID
        rho, lo, hi, rays, tmax, st, _ = _probe_inputs("sparse")
        rays, tmax, st = rays[:256], tmax[:256], st[:256]
        want = grid_probe_host(rho, lo, hi, 0.7, rays, tmax, st, majorant_block=2, return_steps=True)
        t.set_majorant_block(2)       # no grid yet
        t.set_density_grid(rho, lo, hi)
        assert all(bitwise_equal(g, w).all() for g, w in zip(t.grid_probe(0.7, rays, tmax, st, return_steps=True), want))
        t.clear_density_grid()        # survives a clear
        t.set_density_grid(rho, lo, hi)
        assert all(bitwise_equal(g, w).all() for g, w in zip(t.grid_probe(0.7, rays, tmax, st, return_steps=True), want))
        t.set_majorant_block(0)       # applied to the current grid at once
        want0 = grid_probe_host(rho, lo, hi, 0.7, rays, tmax, st, return_steps=True)
        assert all(bitwise_equal(g, w).all() for g, w in zip(t.grid_probe(0.7, rays, tmax, st, return_steps=True), want0))
        assert (want0[3] != want[3]).any()
        # a rejected grid leaves the grid and the block size as they were
        with pytest.raises(VPTError) as ei:
            t.set_density_grid(np.full((2, 2, 2), np.nan), (0, 0, 0), (1, 1, 1), majorant_block=2)
        assert ei.value.code == _lib.VPT_E_INVALID
        assert all(bitwise_equal(g, w).all() for g, w in zip(t.grid_probe(0.7, rays, tmax, st, return_steps=True), want0))
        t.set_density_grid(rho, lo, hi, majorant_block=2)  # grid and block in one call, a grid already set
        assert all(bitwise_equal(g, w).all() for g, w in zip(t.grid_probe(0.7, rays, tmax, st, return_steps=True), want))
    finally:
        t.close()
