"""Estimators 10 and 11 on the GPU against the oracle's independent statement of them (oracle/vpt_oracle_grid.h,
trace_hetero in oracle/vpt_oracle.c), sample for sample: where every transmittance segment lies in a non-uniform
field, on every grid configuration, on the other scenes, with the HG phase function and the depth cap, through the
chunked sums of the render kernels, and in the work counters.

The bars.  End states are equal on every sample.  Estimator 11's radiances are bitwise equal: nothing in it is an
optical depth.  Estimator 10's are bitwise too: the oracle's optical depth equals the host build's bit for bit
(tests/test_oracle_hetero.py::test_optical_depth counts 0 differing values), and the GPU's equals the host build's
(tests/test_gpu_hetero.py, tests/test_gpu_trilinear.py), so no rounding of tau is left between the two sides.  The
largest deviation is printed all the same.

The inputs (tests/hetero_cloud.py) are chosen on the CPU so that each class of mistake would show
(tests/test_oracle_hetero.py).  Shapes are small: 2048 camera samples (64 x 32 x 1), 1024 on the other scenes,
12 x 10 and 16 x 16 images; most of the wall time is the oracle on the CPU."""
import numpy as np
import pytest

import cam_model
import hetero_cloud as hc
import test_gpu_hetero as T
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import RenderConfig, Tracer
from oracle.oracle import default_chunk
from scenes import default_scene, dielectric_scene, mat3_scene, no_emitter_scene, point_lights_scene

pytestmark = pytest.mark.gpu

SCENES = {"mat3": mat3_scene, "point_lights": point_lights_scene, "dielectric": dielectric_scene}


@pytest.fixture(scope="module")
def ot():
    """a tracer of this module's own: its grids and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")
    t.close()


def _reset(ot, orc_vm):
    """the oracle is shared by the session: no grid, no fault, the default scene"""
    orc_vm.set_hetero_fault(0)
    orc_vm.clear_density_grid()
    orc_vm.set_scene(default_scene())
    ot.set_scene(default_scene())


def _samples(orc_vm, w, h):
    rays, st = T._camera_samples(orc_vm, w, h, 1, hc.SEED)
    return rays.reshape(-1), st.reshape(-1)


def _compare(ot, orc_vm, est, rays, st, what, **medium):
    """Tracer.trace against Oracle.trace on the grids both sides hold: end states on every sample, radiances bitwise"""
    got, got_st = ot.trace(est, rays, st, hc.SA, hc.SS, **medium)
    want, want_st, counters = orc_vm.trace(hc.ESTIMATORS[est], rays, st, hc.SA, hc.SS, counters=True, **medium)
    assert (got_st == want_st).all(), f"{what}: {(got_st != want_st).sum()} of {len(st)} end states differ"
    with np.errstate(invalid="ignore"):
        dev = np.nanmax(np.abs(got - want))
    print(f"{what}: largest |L_gpu - L_oracle| = {dev:.3e}, largest L = {np.nanmax(want):.3e}, "
          f"{(~bitwise_equal(got, want)).sum()} values differ")
    assert bitwise_equal(got, want).all(), f"{what}: {(~bitwise_equal(got, want)).sum()} radiance values differ, worst {dev:.3e}"
    return want, counters


@pytest.mark.parametrize("block,interp,emit", hc.CONFIGS)
@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_per_sample_parity(ot, orc_vm, est, block, interp, emit):
    rays, st = _samples(orc_vm, 64, 32)
    try:
        _reset(ot, orc_vm)
        hc.set_cloud(ot, block, interp, emit)
        hc.set_cloud(orc_vm, block, interp, emit)
        L, (_, iters, surface, medium) = _compare(ot, orc_vm, est, rays, st, f"{est}, block {block}, {interp}, emission {emit}")
        # the inputs' conditions (tests/hetero_cloud.py), from the oracle's counters
        assert 4 * surface >= iters and 4 * medium >= iters and 2 * np.count_nonzero(L.any(axis=1)) >= len(L)
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_other_scenes(ot, orc_vm, est, scene):
    """the material-3 sphere around the point light (multipleT stays homogeneous), point lights only (MISv2's light
    loop is empty, every medium event takes the shadow-ray path), the dielectric (its draw inside MISv2's light loop)"""
    rays, st = _samples(orc_vm, 32, 32)
    try:
        _reset(ot, orc_vm)
        ot.set_scene(SCENES[scene]())
        orc_vm.set_scene(SCENES[scene]())
        hc.set_cloud(ot, *hc.MAIN)
        hc.set_cloud(orc_vm, *hc.MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {scene}")
        assert np.count_nonzero(L.any(axis=1)) > 400
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_no_emitter_scene(ot, orc_vm, est):
    """without an emitter the path ends before the track: zero radiance (the emission grid included), the oracle's states"""
    rays, st = _samples(orc_vm, 32, 32)
    try:
        _reset(ot, orc_vm)
        ot.set_scene(no_emitter_scene())
        orc_vm.set_scene(no_emitter_scene())
        hc.set_cloud(ot, *hc.MAIN)
        hc.set_cloud(orc_vm, *hc.MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, no emitter")
        assert (L == 0).all()
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("medium", [dict(hg_g=0.6), dict(max_depth=3), dict(hg_g=0.6, max_depth=3)],
                         ids=["hg", "depth", "hg_depth"])
@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_extensions(ot, orc_vm, est, medium):
    rays, st = _samples(orc_vm, 64, 32)
    try:
        _reset(ot, orc_vm)
        hc.set_cloud(ot, *hc.MAIN)
        hc.set_cloud(orc_vm, *hc.MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {medium}", **medium)
        assert np.count_nonzero(L.any(axis=1)) > 1000
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("spp,config", [(72, hc.MAIN), (8, (0, "nearest", False))], ids=["above_32", "in_order"])
@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_render_parity(ot, orc_vm, est, spp, config):
    """the persistent-wave kernel's image against the oracle's render, fp64 and fp32.  The kernels of estimators 10 and
    11 ignore chunk_spp (include/vpt.h): a lane sums its pixel's samples in order at any count, and Oracle.render's
    default for them is that order.  72 spp is a count at which estimators 0-5 sum in chunks (8, then the tapered 22,
    14, 10, 6, 4, 3, 2, 1, 1, 1): the oracle's samples summed in that layout give another image, so a kernel that
    chunked would fail here.  8 spp is test_gpu_hetero.test_kernels_agree's in-order sum, here tied to the oracle."""
    w, h = 12, 10
    try:
        _reset(ot, orc_vm)
        hc.set_cloud(ot, *config)
        hc.set_cloud(orc_vm, *config)
        want = orc_vm.render(w, h, spp, hc.ESTIMATORS[est], hc.SA, hc.SS, seed=T.SEED)
        if spp == 72:
            # the oracle's render is the in-order sum of its own samples, and the chunked layout is told apart from it
            starts = cam_model.chunk_starts(orc_vm, spp)
            assert default_chunk(spp) == 32 and len(starts) > 3 and starts[-1] == spp
            rays, st = T._camera_samples(orc_vm, w, h, spp, T.SEED)
            L, _ = orc_vm.trace(hc.ESTIMATORS[est], rays.reshape(-1), st.reshape(-1), hc.SA, hc.SS)
            L = L.reshape(h, w, spp, 3)
            assert bitwise_equal(cam_model.image(L, [0, spp]), want).all()
            assert (~bitwise_equal(cam_model.image(L, starts), want)).sum() > 100
        for fp64 in (True, False):
            got = ot.render(RenderConfig(width=w, height=h, spp=spp, estimator=est, sigma_a=hc.SA, sigma_s=hc.SS, seed=T.SEED, fp64=fp64))
            ref = want if fp64 else want.astype(np.float32)
            print(f"{est}, {spp} spp, fp64 {fp64}: largest deviation {np.abs(got - ref).max():.3e}, {(~bitwise_equal(got, ref)).sum()} values differ")
            assert bitwise_equal(got, ref).all(), f"{(~bitwise_equal(got, ref)).sum()} of {ref.size} values differ"
        assert np.count_nonzero(want) > w * h
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio"])
def test_work_counters(ot, orc_vm, est):
    """count_work of a 16 x 16 x 4 render of the cloud: the oracle's (sphere tests, iterations) of the same render"""
    try:
        _reset(ot, orc_vm)
        hc.set_cloud(ot, *hc.MAIN)
        hc.set_cloud(orc_vm, *hc.MAIN)
        _, c = orc_vm.render(16, 16, 4, hc.ESTIMATORS[est], hc.SA, hc.SS, seed=T.SEED, counters=True)
        got = ot.count_work(RenderConfig(width=16, height=16, spp=4, estimator=est, sigma_a=hc.SA, sigma_s=hc.SS, seed=T.SEED))
        assert got == (c.tests, c.iterations)
        assert c.surface > 200 and c.medium > 200
    finally:
        _reset(ot, orc_vm)
