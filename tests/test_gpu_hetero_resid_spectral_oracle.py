"""Estimators 15 and 16 on the GPU against the oracle's independent statement of them (og_residual, og_spectral_ratio and
og_spectral_track in oracle/vpt_oracle_grid.h; trace_hetero at ratio = 2 and trace_hetero_spectral in
oracle/vpt_oracle.c), sample for sample: the residual estimate at all four factor sites with every piece of the control
optical depth, W multiplied into the throughput before the decision is classified, the albedo vector at a medium
vertex, the vector T at the same four sites and the order in which the point-light and the cone factor draw -- on a
field with a density floor (estimator 15) and under three colours (estimator 16), on every grid configuration, on the
other scenes, with the HG phase function and the depth cap, through the sums of the render kernels, and in the work
counters.

The bars.  End states are equal on every sample, and radiances and images are bitwise equal: the GPU's probes equal the
host build's bit for bit (tests/test_gpu_residual.py, tests/test_gpu_hetero_spectral.py), the oracle's probes equal the
host build's bit for bit (tests/test_oracle_hetero_resid_spectral.py), and estimator 11's path arithmetic is held
bitwise by tests/test_gpu_hetero_oracle.py, so nothing is left to round differently.  The largest deviation is printed
all the same.

The inputs (tests/hetero_cloud.py) are chosen on the CPU so that each class of mistake would show
(tests/test_oracle_hetero_resid_spectral.py).  Shapes are small: 2048 camera samples (64 x 32 x 1), 1024 on the other
scenes, 12 x 10 and 16 x 16 images; most of the wall time is the oracle on the CPU."""
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
ESTS = ("hetero_residual", "hetero_spectral")
# (estimator, block, interpolation, colour): estimator 15 on the floor cloud at its five configurations; estimator 16 on
# the cloud at the four configurations under each of the three colours
PARITY = [("hetero_residual", block, interp, "grey") for block, interp in hc.RES_CONFIGS]
PARITY += [("hetero_spectral", block, interp, colour) for colour in hc.SPECTRAL_COLOURS for block, interp in hc.EXT_CONFIGS]
PARITY_IDS = [f"{e}-{b}-{i}-{c}" for e, b, i, c in PARITY]
MAIN = {"hetero_residual": hc.RES_MAIN, "hetero_spectral": hc.SPECTRAL_MAIN}
# the 8 spp render runs the trilinear kernels: the 72 spp one runs the nearest ones at the main configuration
OTHER = {"hetero_residual": (1, "trilinear"), "hetero_spectral": (0, "trilinear")}
MEDIUM = {"hetero_residual": (hc.RES_SA, hc.RES_SS), "hetero_spectral": (hc.EXT_SA, hc.EXT_SS)}


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


def _set(ot, orc_vm, est, block, interp, colour="colour"):
    for owner in (ot, orc_vm):
        if est == "hetero_residual":
            hc.set_floor_cloud(owner, block, interp)
        else:
            hc.set_ext_cloud(owner, block, interp, colour=hc.SPECTRAL_COLOURS[colour])


def _samples(orc_vm, w, h):
    rays, st = T._camera_samples(orc_vm, w, h, 1, hc.SEED)
    return rays.reshape(-1), st.reshape(-1)


def _compare(ot, orc_vm, est, rays, st, what, **medium):
    """Tracer.trace against Oracle.trace on the grids and settings both sides hold: end states on every sample,
    radiances bitwise with NaN equal to NaN"""
    sa, ss = MEDIUM[est]
    got, got_st = ot.trace(est, rays, st, sa, ss, **medium)
    want, want_st, counters = orc_vm.trace(hc.ESTIMATORS[est], rays, st, sa, ss, counters=True, **medium)
    assert (got_st == want_st).all(), f"{what}: {(got_st != want_st).sum()} of {len(st)} end states differ"
    with np.errstate(invalid="ignore"):
        dev = np.nanmax(np.abs(got - want))
    print(f"{what}: largest |L_gpu - L_oracle| = {dev:.3e}, largest L = {np.nanmax(want):.3e}, "
          f"{(~bitwise_equal(got, want)).sum()} values differ")
    assert bitwise_equal(got, want).all(), f"{what}: {(~bitwise_equal(got, want)).sum()} radiance values differ, worst {dev:.3e}"
    return want, counters


@pytest.mark.parametrize("est,block,interp,colour", PARITY, ids=PARITY_IDS)
def test_per_sample_parity(ot, orc_vm, est, block, interp, colour):
    rays, st = _samples(orc_vm, 64, 32)
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, est, block, interp, colour)
        L, (_, iters, surface, medium) = _compare(ot, orc_vm, est, rays, st, f"{est}, block {block}, {interp}, {colour}")
        # the inputs' conditions (tests/hetero_cloud.py), from the oracle's counters
        assert 4 * surface >= iters and 4 * medium >= iters and 2 * np.count_nonzero(L.any(axis=1)) >= len(L)
        assert np.isfinite(L).all()
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("est", ESTS)
def test_other_scenes(ot, orc_vm, est, scene):
    """the material-3 sphere around the point light (multipleT stays homogeneous), point lights only (MISv2's light
    loop is empty and every medium vertex takes the shadow-ray or the cone path, whose two factors draw in a fixed
    order), the dielectric (its draw inside MISv2's light loop, between the per-light factors' draws)"""
    rays, st = _samples(orc_vm, 32, 32)
    try:
        _reset(ot, orc_vm)
        ot.set_scene(SCENES[scene]())
        orc_vm.set_scene(SCENES[scene]())
        _set(ot, orc_vm, est, *MAIN[est])
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {scene}")
        # of 1024: point lights alone light few samples -- the cone ray of a point light scores Ls * (1 / inf) = 0
        # wherever it reaches the light, as in the reference -- and the ratio estimates are 0.0 on some more
        assert np.count_nonzero(L.any(axis=1)) > 100
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
        _set(ot, orc_vm, est, *MAIN[est])
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
        _set(ot, orc_vm, est, *MAIN[est])
        L, _ = _compare(ot, orc_vm, est, rays, st, f"{est}, {medium}", **medium)
        assert np.count_nonzero(L.any(axis=1)) > 800
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("spp,which", [(72, MAIN), (8, OTHER)], ids=["above_32", "in_order"])
@pytest.mark.parametrize("est", ESTS)
def test_render_parity(ot, orc_vm, est, spp, which):
    """the persistent-wave kernel's image against the oracle's render, fp64 and fp32.  The kernels of estimators 15 and
    16 ignore chunk_spp as those of 10-14 do (include/vpt.h): a lane sums its pixel's samples in order at any count, and
    Oracle.render's default for them is that order.  72 spp is a count at which estimators 0-5 sum in chunks: the
    oracle's samples summed in that layout give another image, so a kernel that chunked would fail here.  8 spp is the
    in-order sum of one chunk, on the trilinear kernels."""
    w, h = 12, 10
    sa, ss = MEDIUM[est]
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, est, *which[est])
        want = orc_vm.render(w, h, spp, hc.ESTIMATORS[est], sa, ss, seed=T.SEED)
        if spp == 72:
            # the oracle's render is the in-order sum of its own samples, and the chunked layout is told apart from it
            starts = cam_model.chunk_starts(orc_vm, spp)
            assert default_chunk(spp) == 32 and len(starts) > 3 and starts[-1] == spp
            rays, st = T._camera_samples(orc_vm, w, h, spp, T.SEED)
            L, _ = orc_vm.trace(hc.ESTIMATORS[est], rays.reshape(-1), st.reshape(-1), sa, ss)
            L = L.reshape(h, w, spp, 3)
            assert bitwise_equal(cam_model.image(L, [0, spp]), want).all()
            assert (~bitwise_equal(cam_model.image(L, starts), want)).sum() > 100
        for fp64 in (True, False):
            got = ot.render(RenderConfig(width=w, height=h, spp=spp, estimator=est, sigma_a=sa, sigma_s=ss, seed=T.SEED, fp64=fp64))
            ref = want if fp64 else want.astype(np.float32)
            print(f"{est}, {spp} spp, fp64 {fp64}: largest deviation {np.abs(got - ref).max():.3e}, {(~bitwise_equal(got, ref)).sum()} values differ")
            assert bitwise_equal(got, ref).all(), f"{(~bitwise_equal(got, ref)).sum()} of {ref.size} values differ"
        assert np.count_nonzero(want) > w * h
    finally:
        _reset(ot, orc_vm)


@pytest.mark.parametrize("est", ESTS)
def test_work_counters(ot, orc_vm, est):
    """count_work of a 16 x 16 x 4 render: the oracle's (sphere tests, iterations) of the same render"""
    sa, ss = MEDIUM[est]
    try:
        _reset(ot, orc_vm)
        _set(ot, orc_vm, est, *MAIN[est])
        _, c = orc_vm.render(16, 16, 4, hc.ESTIMATORS[est], sa, ss, seed=T.SEED, counters=True)
        got = ot.count_work(RenderConfig(width=16, height=16, spp=4, estimator=est, sigma_a=sa, sigma_s=ss, seed=T.SEED))
        assert got == (c.tests, c.iterations)
        assert c.surface > 200 and c.medium > 200
    finally:
        _reset(ot, orc_vm)
