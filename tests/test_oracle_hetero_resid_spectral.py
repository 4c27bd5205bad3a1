"""The oracle's statement of estimators 15 and 16 (the walkers at the end of oracle/vpt_oracle_grid.h: og_residual,
og_spectral_ratio, og_spectral_track; trace_hetero at ratio = 2 and trace_hetero_spectral in oracle/vpt_oracle.c),
pinned on the CPU: its two probes against the host build of csrc/vpt_grid.h's residual walker and of
csrc/vpt_grid_spectral.h bit for bit, its tracers against the pinned estimator 11 where the new code is inert, what the
library refuses, and the sensitivity of the inputs of tests/test_gpu_hetero_resid_spectral_oracle.py to each class of
mistake a path test is there to catch (orc_hetero_set_fault 11-18).  No GPU.

The oracle's grid, fault and medium colour are state of the library that the session's fixtures share: every test that
sets one resets it in a `finally`."""
import numpy as np
import pytest

import chroma_model as cm
import grid_model as gm
import hetero_cloud as hc
import majorant_model as mm
import residual_model as rs
import test_grid_residual as tgr
import test_grid_spectral as tgs
import test_gpu_hetero as T
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import grid_residual_probe_host
from scenes import default_scene
from test_grid_chroma import CASE_IDS, CASES
from test_oracle_hetero_ext import _same

SPECTRAL_NAMES = ("t_coll", "w", "steps", "states", "T", "ratio_steps", "ratio_states")


def _reset(orc):
    orc.set_hetero_fault(0)
    hc.reset_ext(orc)
    orc.ext_counters()


def _samples(orc_vm, h=64):
    """64 x h camera samples as records and start states: 4096 here, the GPU tests' 2048 at h = 32"""
    rays, st = T._camera_samples(orc_vm, 64, h, 1, hc.SEED)
    return rays.reshape(-1), st.reshape(-1)


# ---------------------------------------------------------------------------------------------- the probes
RESIDUAL_CASES = [(b, "nearest") for b in (1, 2, 8)] + [(b, "trilinear") for b in (1, 2, 8)]


def test_residual_probe_equals_the_host_build(orc):
    """tests/test_grid_residual.py's inputs (the sparse field with and without the density floor, 4096 rays through its
    box, a thick and a thin medium) at blocks 1, 2 and 8 under both lookups: the estimate, tauc, the end state and the
    draws, bit for bit with the sign of zeros.  Each outcome occurs more than 100 times: the +0.0 exit (under the nearest
    lookup at blocks 2 and 8; the trilinear field seldom reaches a dilated block's majorant), "none" with a product of
    weights (everywhere but at block 1 under the nearest lookup, where no block has a candidate), and "none" with the
    analytic part alone (in every case)"""
    rays, tmax = mm.box_rays(tgr.LO, tgr.HI)
    st = gm.states(11, len(rays))
    try:
        for block, interp in RESIDUAL_CASES:
            seen = dict(zero=0, product=0, analytic=0)
            for rho in (mm.sparse_field() + np.float32(0.5), mm.sparse_field()):
                for sigma_t in (0.7, 0.05):
                    kw = dict(majorant_block=block, interpolation=interp)
                    want = grid_residual_probe_host(rho, tgr.LO, tgr.HI, sigma_t, rays, tmax, st, **kw)
                    got = orc.grid_residual_probe(rho, tgr.LO, tgr.HI, sigma_t, rays, tmax, st, **kw)
                    _same(("That", "tauc", "states", "steps"), got, want, (block, interp, sigma_t))
                    that, tauc, _, steps = got
                    assert not np.isnan(that).any()
                    tc = tgr._tc(sigma_t, tauc)
                    seen["zero"] += int((that == 0).sum())
                    seen["product"] += int(((that > 0) & (that < tc)).sum())
                    seen["analytic"] += int(((that > 0) & (that == tc) & (tauc > 0)).sum())
            print(f"block {block}, {interp}: {seen}")
            assert seen["analytic"] > 100
            if (block, interp) == (1, "nearest"):
                assert seen["product"] == seen["zero"] == 0
            else:
                assert seen["product"] > 100
                assert seen["zero"] > 100 or interp == "trilinear"
    finally:
        _reset(orc)


def _betas(n):
    """test_grid_spectral's throughputs: one per ray, every third with a channel at zero, every seventh all zero"""
    betas = np.random.default_rng(5).uniform(-1.0, 2.0, (n, 3))
    betas[::3, 2] = 0.0
    betas[::7] = 0.0
    return betas


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_spectral_probe_equals_the_host_build(orc, case):
    """tests/test_grid_spectral.py's cases (the coloured medium, no density at all, one extinction 2^14 times the others';
    both lookups; blocks 0, 1 and 2) with beta = None and with a throughput per ray that has zero channels: the track's
    distance, weights, steps and end state and the ratio walk's T, draws and end state, bit for bit with the sign of
    zeros.  Collisions, "none", and a T strictly inside (0, 1) in some channel each occur more than 100 times"""
    name, interp, block = case
    rho, sigma_a, sigma_s, ca, cs = tgs._medium(name)
    rays, tmax, st = tgs._inputs(name)
    try:
        for beta in (None, _betas(len(rays))):
            want = tgs.probe(case, beta)
            got = orc.grid_spectral_probe(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st, absorption=ca, scattering=cs,
                                          majorant_block=block, interpolation=interp, beta=beta)
            _same(SPECTRAL_NAMES, got, want, (case, beta is None))
            tc, _, _, _, Tk, _, _ = got
            assert not np.isnan(tc).any() and not np.isnan(Tk).any()
            coll, none, part = tc >= 0, tc == -1, ((Tk > 0) & (Tk < 1)).any(axis=0)
            print(f"{case}, beta {'ones' if beta is None else 'per ray'}: collisions {coll.sum()}, none {none.sum()}, "
                  f"0 < T < 1 {part.sum()}")
            if name == "zero":
                assert none.all() and not part.any()
            else:
                assert coll.sum() > 100 and none.sum() > 100 and part.sum() > 100
    finally:
        _reset(orc)


def test_spectral_probe_on_grey_extinction(orc):
    """equal extinctions under a coloured albedo, with a throughput: the host build's outputs bit for bit (the scalar
    track under st[0] and W = 1; every T the scalar walker's)"""
    rays, tmax, st = tgs._inputs()
    args = (cm.field(), cm.LO, cm.HI, 0.25, 0.25, rays, tmax, st)
    kw = dict(absorption=(1.5, 1.0, 0.5), scattering=(0.5, 1.0, 1.5), majorant_block=2, interpolation="trilinear", beta=(1.0, 0.25, 0.0))
    try:
        from minimal_volumetric_path_tracer_amd import grid_spectral_probe_host
        got = orc.grid_spectral_probe(*args, **kw)
        _same(SPECTRAL_NAMES, got, grid_spectral_probe_host(*args, **kw), "grey extinction")
        assert bitwise_equal(got[4][0], got[4][1]).all() and bitwise_equal(got[4][1], got[4][2]).all()
        assert (got[0] >= 0).sum() > 100 and (got[0] == -1).sum() > 100
    finally:
        _reset(orc)


# ---------------------------------------------------------------------------------------------- the inputs
def test_the_floor_cloud_has_the_blocks_it_is_there_for():
    """residual_model.control (the Python model, not the code under test) on hetero_cloud.floor_cloud(): at blocks 1 and 2
    under both lookups there are blocks with mn == 0, and -- but at block 1 under the nearest lookup, where every block is
    uniform -- blocks with 0 < mn < mu.  The shared cloud has neither at EXT_MAIN: every minimum is 0 there"""
    rho = hc.floor_cloud()
    assert rho.dtype == np.float32 and rho.shape == hc.cloud()[0].shape
    for block, interp in hc.RES_CONFIGS:
        mn, mu = rs.control(rho, block, interp), rs.majorants(rho, block, interp)
        between = int(((mn > 0) & (mn < mu)).sum())
        print(f"block {block}, {interp}: {mn.size} blocks, mn == 0 in {(mn == 0).sum()}, 0 < mn < mu in {between}")
        if block > max(rho.shape) - 1:
            assert mn.size == 1
            continue
        assert (mn == 0).sum() >= 4
        if (block, interp) == (1, "nearest"):
            assert (mn == mu).all() and (mn > 0).sum() > 50
        else:
            assert between >= 4
    assert (rs.control(hc.cloud()[0], *hc.EXT_MAIN) == 0).all()


def test_the_colours_order_their_extinctions_as_said():
    sa, ss = hc.EXT_SA, hc.EXT_SS
    st = {n: [sa * ca[k] + ss * cs[k] for k in range(3)] for n, (ca, cs) in hc.SPECTRAL_COLOURS.items()}
    assert len(set(st["colour"])) == 3 and int(np.argmax(st["colour"])) == 2
    assert len(set(st["first"])) == 3 and int(np.argmax(st["first"])) == 0
    assert st["top_pair"][0] == st["top_pair"][1] > st["top_pair"][2] and st["top_pair"][0] / max(st["top_pair"]) == 1.0


def test_the_inputs_meet_their_conditions(orc_vm):
    """the 2048 samples of tests/test_gpu_hetero_resid_spectral_oracle.py, estimator 15 on the floor cloud at every
    configuration and estimator 16 on the cloud at every configuration under every colour: surface events and medium
    events are each at least a quarter of the estimator iterations, at least half the samples carry light, every
    radiance is finite (tests/hetero_cloud.py).  Measured: estimator 15 -- surface 0.322-0.334, medium 0.263-0.277, lit
    0.516-0.557; estimator 16 -- surface 0.284-0.305, medium 0.298-0.318, lit 0.504-0.552"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm, 32)
    runs = [(15, hc.RES_SA, hc.RES_SS, cfg, "grey") for cfg in hc.RES_CONFIGS]
    runs += [(16, hc.EXT_SA, hc.EXT_SS, cfg, name) for name in hc.SPECTRAL_COLOURS for cfg in hc.EXT_CONFIGS]
    try:
        for est, sa, ss, (block, interp), colour in runs:
            if est == 15:
                hc.set_floor_cloud(orc_vm, block, interp)
            else:
                hc.set_ext_cloud(orc_vm, block, interp, colour=hc.SPECTRAL_COLOURS[colour])
            L, _, (_, iters, surface, medium) = orc_vm.trace(est, rays, st, sa, ss, counters=True)
            lit = np.count_nonzero(L.any(axis=1))
            print(f"estimator {est}, block {block}, {interp}, {colour}: {iters} iterations, surface {surface / iters:.3f}, "
                  f"medium {medium / iters:.3f}, lit {lit / len(L):.3f}")
            assert 4 * surface >= iters and 4 * medium >= iters and 2 * lit >= len(L)
            assert np.isfinite(L).all()
    finally:
        _reset(orc_vm)


def test_the_inputs_reach_every_new_branch(orc_vm):
    """on the 4096 samples of the sensitivity test every branch the new statements have is taken at least 200 times
    where it can occur at all.  Estimator 15, floor cloud: residual walks with both parts at work (tauc > 0 and a product
    of weights other than 1) at RES_MAIN -- measured 3667; walks that pass a block with a control and no residual only at
    block 1 under the nearest lookup -- 10541 there, 0 at RES_MAIN.  Estimator 16 at SPECTRAL_MAIN under COLOUR: decisions
    whose three W differ at a collision 3985 and on a surface 811, ratio walks that went on past rho >= mu 4781,
    collisions that entered with three different beta 1618.  Real collisions without a draw (a_n == 0: a beta whose
    channels below the largest are zero, at rho >= mu) are reported, 48 here, and not bounded"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        orc_vm.ext_counters()
        hc.set_floor_cloud(orc_vm, *hc.RES_MAIN)
        orc_vm.trace(15, rays, st, hc.RES_SA, hc.RES_SS)
        main = orc_vm.ext_counters()
        hc.set_floor_cloud(orc_vm, 1, "nearest")
        orc_vm.trace(15, rays, st, hc.RES_SA, hc.RES_SS)
        flat = orc_vm.ext_counters()
        hc.set_ext_cloud(orc_vm, *hc.SPECTRAL_MAIN, colour=hc.COLOUR)
        orc_vm.trace(16, rays, st, hc.EXT_SA, hc.EXT_SS)
        spec = orc_vm.ext_counters()
        print(f"estimator 15: both parts {main['residual_both']}, flat blocks {flat['residual_flat_block']} (block 1 nearest), "
              f"{main['residual_flat_block']} (main); estimator 16: {({k: v for k, v in spec.items() if v and not isinstance(v, tuple)})}")
        assert main["residual_both"] >= 200 and main["residual_flat_block"] == 0
        assert flat["residual_flat_block"] >= 200 and flat["residual_both"] == 0  # every weight product is 1: no candidate
        for name in ("W_differ_collision", "W_differ_surface", "ratio_went_on", "beta_differ_collision"):
            assert spec[name] >= 200, (name, spec[name])
        assert "no_draw_collision" in spec and spec["no_draw_collision"] >= 0
        print(f"collisions without a draw: {spec['no_draw_collision']}")
    finally:
        _reset(orc_vm)


def test_the_old_counter_entry_point_writes_six_values(orc):
    """orc_ext_counters keeps its contract -- six values into the caller's six-element buffer, whatever estimators 15 and
    16 count -- and orc_ext_counters_15_16 writes seven: the values behind either stay as they were"""
    guard = 0xA5A5A5A5A5A5A5A5
    for fn, n in ((orc.L.orc_ext_counters, 6), (orc.L.orc_ext_counters_15_16, 7)):
        buf = np.full(n + 4, guard, dtype=np.uint64)
        fn(buf.ctypes.data, 0)
        assert (buf[n:] == guard).all() and (buf[:n] != guard).all()
    assert len([v for v in orc.ext_counters(reset=False).values() if not isinstance(v, tuple)]) + 3 == 13


# ---------------------------------------------------------------------------------------------- identities inside the oracle
def _equal(a, b):
    (La, sa, ca), (Lb, sb, cb) = a, b
    return (sa == sb).all() and ca == cb and bitwise_equal(La, Lb).all()


def test_zero_control_is_estimator_11(orc_vm):
    """the shared cloud at EXT_MAIN: every block minimum is 0 (asserted from the Python model), so mr == mu, no piece of
    tauc is other than 0 and exp(-0) == 1: estimator 15 is estimator 11 bit for bit -- radiances, end states, the work
    counters, and no residual walk with both parts at work.  On the floor cloud the two differ: the control is felt"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    assert (rs.control(hc.cloud()[0], *hc.EXT_MAIN) == 0).all()
    try:
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN, colour=hc.GREY)
        r11 = orc_vm.trace(11, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        orc_vm.ext_counters()
        r15 = orc_vm.trace(15, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        ext = orc_vm.ext_counters()
        assert _equal(r15, r11)
        assert ext["residual_both"] == 0 and ext["residual_flat_block"] == 0
        assert np.count_nonzero(r11[0].any(axis=1)) > 1500 and r11[2][2] > 1000 and r11[2][3] > 1000
        for cfg in (hc.EXT_MAIN, hc.RES_MAIN):  # the project's bar for "felt": 200 of 4096 samples
            hc.set_floor_cloud(orc_vm, *cfg)
            r11 = orc_vm.trace(11, rays, st, hc.RES_SA, hc.RES_SS)
            r15 = orc_vm.trace(15, rays, st, hc.RES_SA, hc.RES_SS)
            print(f"floor cloud, {cfg}: {(r15[1] != r11[1]).sum()} end states differ from estimator 11's")
            assert (r15[1] != r11[1]).sum() >= 200 and (~bitwise_equal(r15[0], r11[0]).all(axis=1)).sum() >= 200
    finally:
        _reset(orc_vm)


def test_uniform_blocks_take_one_draw_per_factor(orc_vm, orc):
    """block 1 under the nearest lookup: no block has a candidate, so a factor over a segment inside the box is one draw
    and exp(-sigma_t tauc) exactly.  On the probe: every ray through the floor cloud's box takes one draw and returns the
    analytic part bit for bit.  In the tracer: no residual walk multiplies a weight in, every walk passes a flat block;
    at block 2 the walks do draw more (the setting is felt)"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    brays, btmax = mm.box_rays(hc.EXT_LO, hc.EXT_HI)
    bst = gm.states(11, len(brays))
    sigma_t = hc.RES_SA + hc.RES_SS
    try:
        that, tauc, so, steps = orc.grid_residual_probe(hc.floor_cloud(), hc.EXT_LO, hc.EXT_HI, sigma_t, brays, btmax, bst, majorant_block=1)
        assert (steps == 1).all() and (tauc > 0).sum() > 1000
        assert bitwise_equal(that, tgr._tc(sigma_t, tauc)).all() and ((that > 0) & (that < 1)).sum() > 1000
        again = orc.grid_residual_probe(hc.floor_cloud(), hc.EXT_LO, hc.EXT_HI, sigma_t, brays, btmax, gm.states(12, len(brays)), majorant_block=1)
        assert bitwise_equal(again[0], that).all() and bitwise_equal(again[1], tauc).all()  # zero variance: no draw is read
        _, _, _, steps2 = orc.grid_residual_probe(hc.floor_cloud(), hc.EXT_LO, hc.EXT_HI, sigma_t, brays, btmax, bst, majorant_block=2)
        assert (steps2 > 1).sum() > 1000
        hc.set_floor_cloud(orc_vm, 1, "nearest")
        orc_vm.ext_counters()
        L, _, c = orc_vm.trace(15, rays, st, hc.RES_SA, hc.RES_SS, counters=True)
        ext = orc_vm.ext_counters()
        assert ext["residual_both"] == 0 and ext["residual_flat_block"] > 1000 and np.isfinite(L).all()
    finally:
        _reset(orc_vm)
        _reset(orc)


@pytest.mark.parametrize("block,interp", hc.EXT_CONFIGS)
def test_default_colour_is_estimator_11(orc_vm, block, interp):
    """the default colour: the track is estimator 10's with W = 1, every T_k is the scalar walker's, alb_k is
    sigma_s / sigma_t: estimator 16 is estimator 11 bit for bit, counters included.  Under COLOUR it is not"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        hc.set_ext_cloud(orc_vm, block, interp, colour=hc.GREY)
        r11 = orc_vm.trace(11, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        orc_vm.ext_counters()
        r16 = orc_vm.trace(16, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        ext = orc_vm.ext_counters()
        assert _equal(r16, r11)
        assert ext["W_differ_collision"] == ext["W_differ_surface"] == ext["ratio_went_on"] == 0
        assert np.count_nonzero(r11[0].any(axis=1)) > 1000  # not vacuous: a quarter of the samples carry light
        orc_vm.set_medium_colour(*hc.COLOUR)
        assert (orc_vm.trace(16, rays, st, hc.EXT_SA, hc.EXT_SS)[1] != r11[1]).sum() > 1000  # the colour is felt
    finally:
        _reset(orc_vm)


@pytest.mark.parametrize("block,interp", hc.EXT_CONFIGS)
def test_coloured_albedo_on_grey_extinction_is_estimator_11_per_channel(orc_vm, block, interp):
    """dyadic multipliers on sigma_a == sigma_s, so st_k is one double: the track is the scalar one, every channel's T is
    the scalar walker's and only alb_k = ss_k / st differs: channel k is estimator 11's channel k at (sigma_a ca_k,
    sigma_s cs_k) bit for bit, with equal end states.  The three channels do differ"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    s_, ca, cs = 0.015625, (1.5, 1.0, 0.5), (0.5, 1.0, 1.5)
    try:
        hc.set_ext_cloud(orc_vm, block, interp, colour=(ca, cs))
        L16, s16 = orc_vm.trace(16, rays, st, s_, s_)
        for k in range(3):
            assert s_ * ca[k] + s_ * cs[k] == 2 * s_
            Lk, sk = orc_vm.trace(11, rays, st, s_ * ca[k], s_ * cs[k])
            assert (sk == s16).all() and bitwise_equal(L16[:, k], Lk[:, k]).all(), k
        assert (L16[:, 0] != L16[:, 2]).sum() > 1000
    finally:
        _reset(orc_vm)


# ---------------------------------------------------------------------------------------------- what the library refuses
def test_what_the_library_refuses_the_oracle_refuses(orc_vm):
    """estimator 15 without a majorant block; estimators 15 and 16 with an emission grid; estimator 16 with a channel
    without extinction; either without a grid -- trace and render raise ValueError, and so do the probes on a block 0 or
    a channel without extinction.  Estimator 11 is not refused in any of these states but the last"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    rays, st = rays[:64], st[:64]

    def refused(est, sa=hc.EXT_SA, ss=hc.EXT_SS):
        with pytest.raises(ValueError):
            orc_vm.trace(est, rays, st, sa, ss)
        with pytest.raises(ValueError):
            orc_vm.render(4, 4, 1, est, sa, ss)

    try:
        for est in (15, 16):
            refused(est)  # no grid
        hc.set_floor_cloud(orc_vm, 0, "nearest")
        refused(15)
        orc_vm.trace(16, rays, st, hc.EXT_SA, hc.EXT_SS)
        orc_vm.trace(11, rays, st, hc.EXT_SA, hc.EXT_SS)
        hc.set_floor_cloud(orc_vm, 2, "nearest")
        orc_vm.trace(15, rays, st, hc.EXT_SA, hc.EXT_SS)
        orc_vm.set_medium_colour((1.0, 0.0, 1.0), (1.0, 0.0, 1.0))
        refused(16)
        orc_vm.trace(15, rays, st, hc.EXT_SA, hc.EXT_SS)  # estimator 15 does not read the colour
        refused(16, 0.0, 0.0)
        orc_vm.set_medium_colour(*hc.COLOUR)
        orc_vm.set_emission_grid(hc.cloud()[1], hc.RGB)
        for est in (15, 16):
            refused(est)
        orc_vm.trace(11, rays, st, hc.EXT_SA, hc.EXT_SS)
        brays, btmax = mm.box_rays(hc.EXT_LO, hc.EXT_HI, n=8)
        bst = gm.states(1, len(brays))
        with pytest.raises(ValueError):
            orc_vm.grid_residual_probe(hc.floor_cloud(), hc.EXT_LO, hc.EXT_HI, 0.1, brays, btmax, bst, majorant_block=0)
        with pytest.raises(ValueError):
            orc_vm.grid_spectral_probe(hc.floor_cloud(), hc.EXT_LO, hc.EXT_HI, 0.1, 0.1, brays, btmax, bst,
                                       absorption=(1.0, 0.0, 1.0), scattering=(1.0, 0.0, 1.0))
    finally:
        _reset(orc_vm)


# ---------------------------------------------------------------------------------------------- the deliberate mistakes
# fault: (its estimator, what it is, whether it changes draws: True, False, or None -- only through beta, see the test)
FAULTS = {
    11: (15, "tauc without the piece up to tend where the boundary test rejects the point", False),
    12: (15, "the residual weight against mu, not mr", False),
    13: (15, "the cone factor is estimator 11's ratio estimate", True),
    14: (16, "W applied at a collision only", None),
    15: (16, "the scalar sigma_s / sigma_t at the medium vertex, not alb", None),
    16: (16, "MISv2's per-light factor is the largest channel's T in every channel", False),
    17: (16, "h = W without |beta|", True),
    18: (16, "the ratio walk returns (0, 0, 0) at the first rho >= mu", True),
}


def _set_main(orc_vm, est):
    if est == 15:
        hc.set_floor_cloud(orc_vm, *hc.RES_MAIN)
        return hc.RES_SA, hc.RES_SS
    if est == 16:
        hc.set_ext_cloud(orc_vm, *hc.SPECTRAL_MAIN, colour=hc.COLOUR)
    elif est in (10, 11):
        hc.set_cloud(orc_vm, *hc.MAIN)
    else:
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN)
    return hc.EXT_SA, hc.EXT_SS


@pytest.mark.parametrize("kind", list(FAULTS))
def test_the_inputs_expose_each_class_of_mistake(orc_vm, kind):
    """a condition on the inputs, not a measurement: each of the oracle's deliberate mistakes 11-18 moves at least 200
    of 4096 samples of its estimator beyond the bar the GPU is held to (a radiance outside
    test_gpu_hetero._radiance_bound, or another end state), at RES_MAIN on the floor cloud (estimator 15) or at
    SPECTRAL_MAIN under COLOUR (estimator 16), and leaves every other estimator 10-16 untouched bit for bit.
    Measured, moved (of them with another end state): 11 -- 411 (0); 12 -- 1137 (0); 13 -- 1467 (1055); 14 -- 597 (22);
    15 -- 1879 (28); 16 -- 867 (0); 17 -- 1034 (166); 18 -- 1694 (1639).  At block 2 under the trilinear lookup fault 11
    moves 112 and fault 18 none: the reason for the nearest lookup (tests/hetero_cloud.py).
    End states.  Faults 11, 12 and 16 change a factor's value and no draw: every end state is the same.  Faults 13, 17
    and 18 change draws.  Faults 14 and 15 change no draw where they are committed, but they change beta, and the
    spectral track's h_k = |beta_k| W_k reads beta at every later decision: a few tens of paths take another branch
    there.  For these two the test asks that 200 samples move with the SAME end state -- the radiance itself shows the
    mistake -- and that some end states differ, which is what the specification implies"""
    est, what, draws = FAULTS[kind]
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        sa, ss = _set_main(orc_vm, est)
        L, s = orc_vm.trace(est, rays, st, sa, ss)
        orc_vm.set_hetero_fault(kind)
        Lf, sf = orc_vm.trace(est, rays, st, sa, ss)
        orc_vm.set_hetero_fault(0)
        out = ~T._radiance_bound(Lf, L).all(axis=1)
        moved = int((out | (sf != s)).sum())
        print(f"estimator {est}, fault {kind} ({what}): {moved} samples moved, {(sf != s).sum()} end states differ")
        assert moved >= 200, f"fault {kind} ({what}) moves only {moved} samples of estimator {est}"
        if draws is None:
            assert int((out & (sf == s)).sum()) >= 200 and (sf != s).any()
        else:
            assert (sf != s).any() if draws else (sf == s).all()
        assert bitwise_equal(orc_vm.trace(est, rays, st, sa, ss)[0], L).all()  # the switch is off again
        for other in {10, 11, 12, 13, 14, 15, 16} - {est}:  # and it concerns no other estimator
            sa, ss = _set_main(orc_vm, other)
            L, s = orc_vm.trace(other, rays[:512], st[:512], sa, ss)
            orc_vm.set_hetero_fault(kind)
            Lf, sf = orc_vm.trace(other, rays[:512], st[:512], sa, ss)
            orc_vm.set_hetero_fault(0)
            assert (sf == s).all() and bitwise_equal(Lf, L).all(), other
            hc.reset_ext(orc_vm)
    finally:
        _reset(orc_vm)
