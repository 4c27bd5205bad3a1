"""Stage A's decide() with the launch's camera table (all-fresh batches cast from PoolParams::cam_oc) and, for the
free-flight estimators, the draws and loads taken before the cast: renders from a moved camera are the oracle's
bit for bit, the table follows each launch's scene and camera, and the log in two halves is lm_log.

The oracle's render fixes main()'s camera origin, so the reference here is cam_model.py: the oracle's stream
start, camera direction and estimator per sample, summed in orc_render_layout's chunk order.  Shapes: 24 x 20
(padded 8 x 8 tiles), 40 spp (two chunks of the tapered layout), a non-dyadic origin inside the room."""
import ctypes
import functools
from dataclasses import dataclass

import numpy as np
import pytest

import cam_model
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import RenderConfig, lib
from minimal_volumetric_path_tracer_amd.tracer import ESTIMATORS
from scenes import ALT_SCENES, SCENES

W, H, SPP = 24, 20, 40
CAM = (3.3, -7.1, 40.7)
SCENE_FNS = {"default": SCENES["default"], "metal_walls": ALT_SCENES["alt_metal_walls"],
             "point_lights": SCENES["point_lights"]}


@dataclass
class CamConfig(RenderConfig):
    origin: tuple = CAM

    def params(self):
        p = super().params()
        for i in range(3):
            p.camera.o[i] = self.origin[i]
        return p


def _cfg(est, origin=CAM, **kw):
    base = dict(width=W, height=H, spp=SPP, estimator=est, fp64=True, origin=origin)
    base.update(kw)
    return CamConfig(**base)


_ORC = {}


def _orc():
    if "o" not in _ORC:
        from oracle.oracle import Oracle

        _ORC["o"] = Oracle(portable=True)
    return _ORC["o"]


@functools.lru_cache(maxsize=None)
def _samples(scene, origin, est, n=SPP, max_depth=0, hg_g=0.0):
    """(L per sample, tests, iterations): computed once per case, shared, never written to"""
    orc = _orc()
    orc.set_scene(SCENE_FNS[scene]())
    L, tests, iters = cam_model.sample_radiance(orc, W, H, n, origin, ESTIMATORS[est], max_depth=max_depth, hg_g=hg_g)
    L.setflags(write=False)
    return L, tests, iters


def _ref_image(scene, origin, est, **kw):
    L, _, _ = _samples(scene, origin, est, **kw)
    return cam_model.image(L, cam_model.chunk_starts(_orc(), SPP))


def _same(a, b):
    eq = bitwise_equal(a, b)
    assert eq.all(), f"{(~eq).sum()} of {eq.size} values differ"


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene", ["default", "metal_walls", "point_lights"])
@pytest.mark.parametrize("est", ["ff", "mis", "explicit_free", "implicit_free", "surface_pt"])
def test_moved_camera_estimators(gpu_tracer, est, scene):
    gpu_tracer.set_scene(SCENE_FNS[scene]())
    _same(gpu_tracer.render(_cfg(est)), _ref_image(scene, CAM, est))


@pytest.mark.parametrize("est", ["ff", "mis"])
@pytest.mark.parametrize("origin", [(-23.0, 24.3, 0.0), (23.5, 24.1, 35.7)], ids=["at_point_light", "in_sphere_light"])
def test_degenerate_origins(gpu_tracer, est, origin):
    """the table holds zeros (oc = +-0, det = 0 at the point light's own sphere) or a negative |oc|^2 - r^2"""
    gpu_tracer.set_scene(SCENE_FNS["default"]())
    _same(gpu_tracer.render(_cfg(est, origin)), _ref_image("default", origin, est))


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_depth_cap(gpu_tracer, est):
    """max_depth = 2: the kill prediction ends paths by depth, so more batches are all fresh"""
    gpu_tracer.set_scene(SCENE_FNS["default"]())
    _same(gpu_tracer.render(_cfg(est, max_depth=2)), _ref_image("default", CAM, est, max_depth=2))


def test_table_follows_scene_and_camera():
    """one Tracer: a render, another scene, another camera -- no launch may cast from an earlier launch's table"""
    from minimal_volumetric_path_tracer_amd import Tracer

    other = (-11.9, 5.3, 61.1)
    t = Tracer(0, SCENE_FNS["default"]())
    try:
        _same(t.render(_cfg("ff")), _ref_image("default", CAM, "ff"))
        t.set_scene(SCENE_FNS["point_lights"]())
        _same(t.render(_cfg("ff")), _ref_image("point_lights", CAM, "ff"))
        _same(t.render(_cfg("ff", other)), _ref_image("point_lights", other, "ff"))
        t.set_scene(SCENE_FNS["default"]())
        _same(t.render(_cfg("mis", other)), _ref_image("default", other, "mis"))
    finally:
        t.close()


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_band_shard(gpu_tracer, est):
    """rank 1 of 3 with 4-row bands: file rows 4-7 and 16-19 of the full image"""
    gpu_tracer.set_scene(SCENE_FNS["default"]())
    got = gpu_tracer.render(_cfg(est, band_rows=4, band_stride=3, band_offset=1))
    full = _ref_image("default", CAM, est)
    _same(got, np.concatenate([full[4:8], full[16:20]]))
    whole = gpu_tracer.render(_cfg(est))
    _same(got, np.concatenate([whole[4:8], whole[16:20]]))


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_accumulator_tile_subset(gpu_tracer, est):
    """one level for every tile, then a pass of two levels over a tile subset (pool_kernel's tile map): every
    pixel is the chunked sum of the levels it holds"""
    C, tiles = 8, [7, 2, 4]
    gpu_tracer.set_scene(SCENE_FNS["default"]())
    L, _, _ = _samples("default", CAM, est)
    acc = gpu_tracer.accumulator(_cfg(est, spp=SPP), chunk=C)
    try:
        assert (acc.tiles_x, acc.tiles_y) == (3, 3)
        acc.add(1)
        acc.add(2, tiles=tiles)
        got = acc.image(fp64=True)
    finally:
        acc.close()
    one = cam_model.image(L, [0, C])
    three = cam_model.image(L, [0, C, 2 * C, 3 * C])
    in_subset = np.zeros((3, 3), dtype=bool)
    in_subset.reshape(-1)[tiles] = True
    mask = np.repeat(np.repeat(in_subset, 8, axis=0), 8, axis=1)[:H, :W]
    _same(got, np.where(mask[..., None], three, one))


@pytest.mark.parametrize("est", ["ff", "mis"])
def test_count_work(gpu_tracer, est):
    gpu_tracer.set_scene(SCENE_FNS["default"]())
    _, tests, iters = _samples("default", CAM, est)
    assert gpu_tracer.count_work(_cfg(est)) == (tests, iters)


def test_log_in_two_halves(gpu_tracer, orc_vm):
    """math probe 23 (gm_log_pair_of, then gm_log_finish) against lm_log (probe 2) and the oracle's log: both
    paths' boundaries (|x - 1| < 0x1.09p-4 is [0x1.fbdp-1, 0x1.109p0)), the sweep below 1, draws 1 - k / 2^48,
    and the rare arguments (zero, negative, subnormal, inf, NaN)"""
    rng = np.random.default_rng(23)
    lo, hi = float.fromhex("0x1.fbdp-1"), float.fromhex("0x1.109p0")
    edges = []
    for v in (lo, hi, 1.0, 0.5, 2.0, float.fromhex("0x1p-1022"), 1 - 2.0 ** -48, 2.0 ** -48):
        edges += [np.nextafter(v, 0), v, np.nextafter(v, np.inf)]
    rare = [0.0, -0.0, -1.0, 5e-324, float.fromhex("0x0.fffffffffffffp-1022"), np.inf, -np.inf, np.nan, 1e308]
    sweep = 1.0 - np.arange(1, 2 ** 16 + 2 ** 15, dtype=np.float64) * 2.0 ** -17   # 98303 points in (0.25, 1)
    k = rng.integers(0, 2 ** 48, size=2 ** 16, dtype=np.uint64)
    draws = 1.0 - k.astype(np.float64) * 2.0 ** -48                                # erand48's 1 - xi, exactly
    k_small = rng.integers(1, 2 ** 20, size=4096, dtype=np.uint64)                 # 1 - xi next to 1: the B path
    near_one = 1.0 - k_small.astype(np.float64) * 2.0 ** -48
    x = np.concatenate([np.array(edges + rare), sweep, draws, near_one])
    two = gpu_tracer.math_probe(23, x)
    _same(two, gpu_tracer.math_probe(2, x))
    _same(two, orc_vm.math(2, x))
