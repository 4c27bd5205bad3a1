"""Estimators 12, 13 and 14 on the GPU against the oracle's independent statement of them (the decisions of
oracle/vpt_oracle_grid.h; trace_hetero_eqa, trace_hetero_mis and trace_hetero_chroma in oracle/vpt_oracle.c), sample
for sample: the throughput after a medium vertex, the segment of every transmittance factor, T carried or walked
again, ws and w in their places, and the per-channel branches of the shared helpers -- on a non-uniform field at
q = 0.5 with a coloured medium, on every grid configuration, on the other scenes, with the HG phase function and the
depth cap, through the sums of the render kernels, and in the work counters.

The bars.  End states are equal on every sample, and radiances and images are bitwise equal: the GPU's probes equal
the host build's bit for bit (tests/test_gpu_hetero_eqa.py, test_gpu_hetero_mis.py, test_gpu_hetero_chroma.py), the
oracle's probes equal the host build's bit for bit (tests/test_oracle_hetero_ext.py), and estimator 1's path
arithmetic is held bitwise by tests/test_gpu_parity.py, so nothing is left to round differently.  The largest
deviation is printed all the same.

The inputs (tests/hetero_cloud.py) are chosen on the CPU so that each class of mistake would show
(tests/test_oracle_hetero_ext.py).  Shapes are small: 2048 camera samples (64 x 32 x 1), 1024 on the other scenes,
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
ESTS = list(hc.EXT_ESTIMATORS)
# (estimator, block, interpolation, track fraction, colour): the three estimators on the four grid configurations, and
# at the main one two more fractions for estimator 13 and a colour with a pair of equal extinctions for estimator 14
PARITY = [(est, block, interp, hc.Q, hc.COLOUR) for est in ESTS for block, interp in hc.EXT_CONFIGS]
PARITY += [("hetero_mis", *hc.EXT_MAIN, q, hc.COLOUR) for q in (0.25, 1.0)]
PARITY += [("hetero_chromatic", *hc.EXT_MAIN, hc.Q, hc.COLOUR_PAIR)]
PARITY_IDS = [f"{e}-{b}-{i}-q{q}-{'pair' if c is hc.COLOUR_PAIR else 'colour'}" for e, b, i, q, c in PARITY]


@pytest.fixture(scope="module")
def ot():
    """a tracer of this module's own: its grid and its settings never reach the other modules' tracers"""
    t = Tracer(0, default_scene())
    yield t
    t.set_majorant_block(0)
    t.set_grid_interpolation("nearest")
    t.close()


def _reset(ot, orc_vm):
    """the oracle is shared by the session: no grid, no fault, the default fraction, colour and scene"""
    orc_vm.set_hetero_fault(0)
    for owner in (orc_vm, ot):
        hc.reset_ext(owner)
        owner.set_scene(default_scene())


def _set(ot, orc_vm, block, interp, q=hc.Q, colour=hc.COLOUR):
    for owner in (ot, orc_vm):
        hc.set_ext_cloud(owner, block, interp, q, colour)


def _samples(orc_vm, w, h):
    rays, st = T._camera_samples(orc_vm, w, h, 1, hc.SEED)
    return rays.reshape(-1), st.reshape(-1)


def _compare(ot, orc_vm, est, rays, st, what, **medium):
    """Tracer.trace against Oracle.trace on the grids and settings both sides hold: end states on every sample,
    radiances bitwise"""
    got, got_st = ot.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS, **medium)
    want, want_st, counters = orc_vm.trace(hc.ESTIMATORS[est], rays, st, hc.EXT_SA, hc.EXT_SS, counters=True, **medium)
    assert (got_st == want_st).all(), f"{what}: {(got_st != want_st).sum()} of {len(st)} end states differ"
    with np.errstate(invalid="ignore"):
        dev = np.nanmax(np.abs(got - want))
    print(f"{what}: largest |L_gpu - L_oracle| = {dev:.3e}, largest L = {np.nanmax(want):.3e}, "
          f"{(~bitwise_equal(got, want)).sum()} values differ")
    assert bitwise_equal(got, want).all(), f"{what}: {(~bitwise_equal(got, want)).sum()} radiance values differ, worst {dev:.3e}"
    return want, counters


@pytest.mark.parametrize("est,block,interp,q,colour", PARITY, ids=PARITY_IDS)
def test_per_sample_parity(ot, orc_vm, est, block, interp, q, colour):
    rays, st = _samples(orc_vm, 64, 32)
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, block, interp, q, colour)
        L, (_, iters, surface, medium) = _compare(ot, orc_vm, est, rays, st, f"{est}, block {block}, {interp}, q {q}, colour {colour}")
        # the inputs' conditions (tests/hetero_cloud.py), from the oracle's counters
        assert 4 * surface >= iters and 4 * medium >= iters and 2 * np.count_nonzero(L.any(axis=1)) >= len(L)
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("est", ESTS)
def test_other_scenes(ot, orc_vm, est, scene):
    """the material-3 sphere around the point light (multipleT stays homogeneous), point lights only (MISv2's light
    loop is empty and every medium vertex takes the shadow-ray or the cone path: the configuration estimator 12 exists
    for), the dielectric (its draw inside MISv2's light loop)"""
    rays, st = _samples(orc_vm, 32, 32)
    try:
        _reset(ot, orc_vm)
        ot.set_scene(SCENES[scene]())
        orc_vm.set_scene(SCENES[scene]())
        _set(ot, orc_vm, *hc.EXT_MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {scene}")
        # of 1024: about 500 with the sphere lights; point lights alone light about 230 -- the cone ray of a point
        # light scores Ls * (1 / inf) = 0 wherever it reaches the light, as in the reference
        assert np.count_nonzero(L.any(axis=1)) > 200
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("est", ESTS)
def test_no_emitter_scene(ot, orc_vm, est):
    """without an emitter the path ends before the decision: zero radiance, the oracle's states"""
    rays, st = _samples(orc_vm, 32, 32)
    try:
        _reset(ot, orc_vm)
        ot.set_scene(no_emitter_scene())
        orc_vm.set_scene(no_emitter_scene())
        _set(ot, orc_vm, *hc.EXT_MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, no emitter")
        assert (L == 0).all()
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("medium", [dict(hg_g=0.6), dict(max_depth=3), dict(hg_g=0.6, max_depth=3)],
                         ids=["hg", "depth", "hg_depth"])
@pytest.mark.parametrize("est", ESTS)
def test_extensions(ot, orc_vm, est, medium):
    rays, st = _samples(orc_vm, 64, 32)
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, *hc.EXT_MAIN)
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {medium}", **medium)
        assert np.count_nonzero(L.any(axis=1)) > 1000
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("spp,config", [(72, hc.EXT_MAIN), (8, (0, "nearest"))], ids=["above_32", "in_order"])
@pytest.mark.parametrize("est", ESTS)
def test_render_parity(ot, orc_vm, est, spp, config):
    """the persistent-wave kernel's image against the oracle's render, fp64 and fp32.  The kernels of estimators 12-14
    ignore chunk_spp as those of 10 and 11 do (include/vpt.h): a lane sums its pixel's samples in order at any count,
    and Oracle.render's default for them is that order.  72 spp is a count at which estimators 0-5 sum in chunks: the
    oracle's samples summed in that layout give another image, so a kernel that chunked would fail here.  8 spp is the
    in-order sum of one chunk."""
    w, h = 12, 10
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, *config)
        want = orc_vm.render(w, h, spp, hc.ESTIMATORS[est], hc.EXT_SA, hc.EXT_SS, seed=T.SEED)
        if spp == 72:
            # the oracle's render is the in-order sum of its own samples, and the chunked layout is told apart from it
            starts = cam_model.chunk_starts(orc_vm, spp)
            assert default_chunk(spp) == 32 and len(starts) > 3 and starts[-1] == spp
            rays, st = T._camera_samples(orc_vm, w, h, spp, T.SEED)
            L, _ = orc_vm.trace(hc.ESTIMATORS[est], rays.reshape(-1), st.reshape(-1), hc.EXT_SA, hc.EXT_SS)
            L = L.reshape(h, w, spp, 3)
            assert bitwise_equal(cam_model.image(L, [0, spp]), want).all()
            assert (~bitwise_equal(cam_model.image(L, starts), want)).sum() > 100
        for fp64 in (True, False):
            got = ot.render(RenderConfig(width=w, height=h, spp=spp, estimator=est, sigma_a=hc.EXT_SA, sigma_s=hc.EXT_SS,
                                         seed=T.SEED, fp64=fp64))
            ref = want if fp64 else want.astype(np.float32)
            print(f"{est}, {spp} spp, fp64 {fp64}: largest deviation {np.abs(got - ref).max():.3e}, {(~bitwise_equal(got, ref)).sum()} values differ")
            assert bitwise_equal(got, ref).all(), f"{(~bitwise_equal(got, ref)).sum()} of {ref.size} values differ"
        assert np.count_nonzero(want) > w * h
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("est", ESTS)
def test_work_counters(ot, orc_vm, est):
    """count_work of a 16 x 16 x 4 render of the cloud: the oracle's (sphere tests, iterations) of the same render"""
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, *hc.EXT_MAIN)
        _, c = orc_vm.render(16, 16, 4, hc.ESTIMATORS[est], hc.EXT_SA, hc.EXT_SS, seed=T.SEED, counters=True)
        got = ot.count_work(RenderConfig(width=16, height=16, spp=4, estimator=est, sigma_a=hc.EXT_SA, sigma_s=hc.EXT_SS,
                                         seed=T.SEED))
        assert got == (c.tests, c.iterations)
        assert c.surface > 200 and c.medium > 200
    finally:
        _reset(ot, orc_vm)
