"""The oracle's statement of estimators 12, 13 and 14 (the decisions at the end of oracle/vpt_oracle_grid.h;
trace_hetero_eqa, trace_hetero_mis and trace_hetero_chroma in oracle/vpt_oracle.c), pinned on the CPU: its three
probes against the host build of csrc/vpt_grid_eqa.h, vpt_grid_mis.h and vpt_grid_chroma.h bit for bit, its tracers
against the pinned estimators they reduce to where the new code is inert, and the sensitivity of the inputs of
tests/test_gpu_hetero_ext_oracle.py to each class of mistake a path test is there to catch (orc_hetero_set_fault 5-10).
No GPU.

The oracle's grid, fault, track fraction and medium colour are state of the library that the session's fixtures share:
every test that sets one resets it in a `finally`."""
import functools

import numpy as np
import pytest

import chroma_model as cm
import eqa_model as em
import grid_model as gm
import hetero_cloud as hc
import test_grid_chroma as tgc
import test_grid_mis as tgm
import test_gpu_hetero as T
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import grid_chroma_probe_host, grid_eqa_probe_host, grid_mis_probe_host
from scenes import default_scene
from test_grid_eqa import _fields

INTERPS = ("nearest", "trilinear")


def _reset(orc):
    orc.set_hetero_fault(0)
    hc.reset_ext(orc)
    orc.ext_counters()


@functools.lru_cache(maxsize=None)
def _inputs(light, sigma_t):
    """test_grid_mis._inputs with more rays of the same generator: grid_model's rays without those whose line holds the
    light.  The thin medium scatters a sixth of its rays and the trilinear sparse field is empty at a seventh of the
    sampled points; every outcome is to occur more than 100 times (8000 rays give 65 empty points, 32 000 give 180)"""
    rays, tmax = gm.tau_rays(n=4000 if sigma_t > 0.1 else 32000)
    st = gm.states(3, len(rays))
    D = np.array([em.geometry(rays["o"][i], rays["d"][i], tgm.LIGHTS[light])[0] for i in range(len(rays))])
    keep = D != 0
    return rays[keep], tmax[keep], st[keep]


def _same(names, got, want, case):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name} ({case})"
        assert bitwise_equal(g, w).all(), f"{name} ({case}): {(~bitwise_equal(g, w)).sum()} of {g.size} differ"
        if g.dtype == np.float64:  # and the sign of a zero
            assert (np.signbit(g) == np.signbit(w)).all(), f"{name} ({case}): signs differ"


@pytest.mark.parametrize("case", tgm.CASES, ids=tgm.CASE_IDS)
def test_equiangular_probe_equals_the_host_build(orc, case):
    """test_grid_eqa.py's inputs (the tau grid and the sparse field, a light inside and one outside the box, both
    lookups, a thick and a thin medium): psurf, dist, pdf, T, rho_t and the end state, bit for bit"""
    light, field, sigma_t, interp = case
    rays, tmax, st = _inputs(light, sigma_t)
    args = (_fields()[field], gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, tgm.LIGHTS[light], st)
    try:
        want = grid_eqa_probe_host(*args, interpolation=interp)
        got = orc.grid_eqa_probe(*args, interpolation=interp)
        _same(("psurf", "dist", "pdf", "T", "rho_t", "states"), got, want, case)
        _, dist, _, _, rho_t, _ = got
        surface, medium, empty = dist == -1, (dist != -1) & (rho_t > 0), (dist != -1) & (rho_t == 0)
        print(f"{case}: surface {surface.sum()}, medium {medium.sum()}, empty {empty.sum()}")
        assert surface.sum() > 100 and medium.sum() > 100
        assert empty.sum() > 100 if field == "sparse" else empty.sum() == 0
    finally:
        _reset(orc)


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("case", tgm.CASES, ids=tgm.CASE_IDS)
def test_mis_probe_equals_the_host_build(orc, case, block):
    """the same inputs at q = 0, 0.5 and 1 on the global and the local majorant: psurf, strategy, dist, pdf, pe, T,
    rho_t, steps and the end state, bit for bit; at q = 0.5 each of the four outcomes occurs more than 100 times"""
    light, field, sigma_t, interp = case
    rays, tmax, st = _inputs(light, sigma_t)
    args = (_fields()[field], gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, tgm.LIGHTS[light], st)
    try:
        for q in (0.0, 0.5, 1.0):
            kw = dict(q=q, majorant_block=block, interpolation=interp)
            want = grid_mis_probe_host(*args, **kw)
            got = orc.grid_mis_probe(*args, **kw)
            _same(("psurf", "strategy", "dist", "pdf", "pe", "T", "rho_t", "steps", "states"), got, want, (case, q, block))
            assert not np.isnan(got[2]).any()
            if q == 0.5:
                counts = [int(m.sum()) for m in tgm._outcomes(got)]
                print(f"{case} block {block}: track/surface {counts[0]}, track/medium {counts[1]}, eqa/surface {counts[2]}, "
                      f"eqa/medium {counts[3]}")
                assert min(counts) > 100, counts
            else:
                assert (got[1] == int(q)).all()  # one strategy only
    finally:
        _reset(orc)


@pytest.mark.parametrize("case", tgc.CASES, ids=tgc.CASE_IDS)
def test_chromatic_probe_equals_the_host_build(orc, case):
    """test_grid_chroma.py's cases (the coloured medium, no density at all, one extinction 2^14 times the others'; both
    lookups; blocks 0, 1 and 2): hero, distance, optical depth, weights, steps and the end state, bit for bit"""
    name, interp, block = case
    rho, sigma_a, sigma_s, ca, cs = tgc._medium(name)
    rays, tmax, st = tgc._inputs()
    try:
        want = tgc.probe(case)
        got = orc.grid_chroma_probe(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st, absorption=ca, scattering=cs,
                                    majorant_block=block, interpolation=interp)
        _same(cm.NAMES, got, want, case)
        hero, tc, _, _, _, _ = got
        assert all((hero == k).sum() > 1000 for k in range(3))
        if name != "zero":
            assert (tc >= 0).sum() > 500 and (tc == -1).sum() > 500
    finally:
        _reset(orc)


def test_chromatic_probe_grey_takes_no_hero_draw(orc):
    """equal extinctions under a coloured albedo: the host build's outputs bit for bit, hero 0 on every ray"""
    rays, tmax, st = tgc._inputs()
    kw = dict(absorption=(1.5, 1.0, 0.5), scattering=(0.5, 1.0, 1.5), majorant_block=2, interpolation="trilinear")
    try:
        want = grid_chroma_probe_host(cm.field(), cm.LO, cm.HI, 0.25, 0.25, rays, tmax, st, **kw)
        got = orc.grid_chroma_probe(cm.field(), cm.LO, cm.HI, 0.25, 0.25, rays, tmax, st, **kw)
        _same(cm.NAMES, got, want, "grey extinction")
        assert (got[0] == 0).all() and len({float(got[3][c][got[1] >= 0][0]) for c in range(3)}) == 3
    finally:
        _reset(orc)


def _samples(orc_vm, h=64):
    """64 x h camera samples as records and start states: 4096 here, the GPU tests' 2048 at h = 32"""
    rays, st = T._camera_samples(orc_vm, 64, h, 1, hc.SEED)
    return rays.reshape(-1), st.reshape(-1)


@pytest.mark.parametrize("rho", [1.0, 2.0])
def test_uniform_grid_walks_estimator_1(orc, orc_vm, rho):
    """uniform rho on [-4096, 4096]^3: [a, b] is [0, t], rho(xt) is rho and every factor is the homogeneous one but for
    the rounding of tau, so estimator 12 at (sigma_a, sigma_s) walks the pinned estimator 1 at (rho sigma_a,
    rho sigma_s) draw for draw -- equal end states, radiances within the rounding of tau"""
    orc.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    L1, s1, c1 = orc.trace(1, rays, st, rho * T.SA, rho * T.SS, counters=True)
    try:
        for interp in INTERPS:
            orc.set_density_grid(np.full((4, 4, 4), rho, np.float32), T.BIG_LO, T.BIG_HI, 2, interp)
            L12, s12, c12 = orc.trace(12, rays, st, T.SA, T.SS, counters=True)
            assert (s12 == s1).all(), f"{(s12 != s1).sum()} end states differ"
            assert c12 == c1
            ok = T._radiance_bound(L12, L1)
            print(f"rho {rho}, {interp}: max |L12 - L1| = {np.abs(L12 - L1).max():.3e}")
            assert ok.all(), f"{(~ok).sum()} channels beyond the bound, worst {np.abs(L12 - L1).max():.3e}"
        assert np.count_nonzero(L1.any(axis=1)) > 2000 and c1[2] > 200 and c1[3] > 2000
    finally:
        _reset(orc)


@pytest.mark.parametrize("block,interp", hc.EXT_CONFIGS)
def test_fraction_zero_is_estimator_12(orc_vm, block, interp):
    """q = 0 on the cloud: the coin never chooses the track, (c - 0) / (1 - 0) is c and 0 pff + 1 pe is pe, and the T
    that the decision carries is the T estimator 12 walks again: radiances and end states bit for bit"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        hc.set_ext_cloud(orc_vm, block, interp, q=0.0)
        L12, s12, c12 = orc_vm.trace(12, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        L13, s13, c13 = orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        assert (s13 == s12).all() and c13 == c12 and bitwise_equal(L13, L12).all()
        assert np.count_nonzero(L12.any(axis=1)) > 1500 and c12[3] > 1000
        orc_vm.set_hetero_mis_fraction(hc.Q)
        assert (orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS)[1] != s12).sum() > 1000  # the fraction is felt
    finally:
        _reset(orc_vm)


def test_fraction_one_always_tracks(orc_vm):
    """q = 1: every decision runs a track, so no medium vertex comes from the equi-angular strategy, and 1 - q = 0
    never divides (every radiance is finite)"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN, q=1.0)
        orc_vm.ext_counters()
        L, _, c = orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        ext = orc_vm.ext_counters()
        assert ext["equiangular"] == 0 and ext["track"] == c[3] and c[3] > 1000
        assert np.isfinite(L).all()
    finally:
        _reset(orc_vm)


@pytest.mark.parametrize("block,interp", hc.EXT_CONFIGS)
def test_grey_extinction_is_estimator_10(orc_vm, block, interp):
    """the default colour: estimator 14 is estimator 10 bit for bit.  Equal extinctions under a coloured albedo (dyadic
    multipliers on sigma_a == sigma_s, so st_k is one double): no hero draw, and channel k is estimator 10's channel k
    at (sigma_a ca_k, sigma_s cs_k) bit for bit -- the same extinction, the albedo ss_k / st"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    s_, ca, cs = 0.015625, (1.5, 1.0, 0.5), (0.5, 1.0, 1.5)
    try:
        hc.set_ext_cloud(orc_vm, block, interp, colour=hc.GREY)
        L10, s10, c10 = orc_vm.trace(10, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        L14, s14, c14 = orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
        assert (s14 == s10).all() and c14 == c10 and bitwise_equal(L14, L10).all()
        assert np.count_nonzero(L10.any(axis=1)) > 1500
        orc_vm.set_medium_colour(ca, cs)
        orc_vm.ext_counters()
        L14, s14 = orc_vm.trace(14, rays, st, s_, s_)
        assert orc_vm.ext_counters()["hero"][1:] == (0, 0)
        for k in range(3):
            assert s_ * ca[k] + s_ * cs[k] == 2 * s_
            Lk, sk = orc_vm.trace(10, rays, st, s_ * ca[k], s_ * cs[k])
            assert (sk == s14).all() and bitwise_equal(L14[:, k], Lk[:, k]).all(), k
        assert (L14[:, 0] != L14[:, 2]).sum() > 1000
        orc_vm.set_medium_colour(*hc.COLOUR)
        assert (orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS)[1] != s10).sum() > 1000  # the colour is felt
    finally:
        _reset(orc_vm)


def test_settings_are_validated_as_the_library_validates_them(orc_vm):
    """the track fraction in [0, 1] and finite; colour multipliers finite and >= 0; a refused value leaves the setting;
    estimators 12-14 with an emission grid, without a grid, and estimator 14 with a channel without extinction"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    rays, st = rays[:256], st[:256]
    try:
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN, q=0.25)
        base = orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS)
        for q in (-0.1, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                orc_vm.set_hetero_mis_fraction(q)
        got = orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS)
        assert (got[1] == base[1]).all() and bitwise_equal(got[0], base[0]).all()
        base = orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS)
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                orc_vm.set_medium_colour((1.0, bad, 1.0), (1.0, 1.0, 1.0))
            with pytest.raises(ValueError):
                orc_vm.set_medium_colour((1.0, 1.0, 1.0), (1.0, 1.0, bad))
        with pytest.raises(ValueError):
            orc_vm.set_medium_colour((1.0, 1.0), (1.0, 1.0, 1.0))
        got = orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS)
        assert (got[1] == base[1]).all() and bitwise_equal(got[0], base[0]).all()
        orc_vm.set_medium_colour((1.0, 0.0, 1.0), (1.0, 0.0, 1.0))  # accepted by the setter, refused by the trace
        with pytest.raises(ValueError):
            orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS)
        orc_vm.trace(12, rays, st, hc.EXT_SA, hc.EXT_SS)  # the other estimators do not read it
        orc_vm.set_medium_colour(*hc.COLOUR)
        orc_vm.set_emission_grid(hc.cloud()[1], hc.RGB)
        for est in (12, 13, 14):
            with pytest.raises(ValueError):
                orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS)
            with pytest.raises(ValueError):
                orc_vm.render(4, 4, 1, est, hc.EXT_SA, hc.EXT_SS)
        orc_vm.trace(10, rays, st, hc.EXT_SA, hc.EXT_SS)
        orc_vm.clear_density_grid()
        for est in (12, 13, 14):
            with pytest.raises(ValueError):
                orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS)
    finally:
        _reset(orc_vm)


def test_the_inputs_meet_their_conditions(orc_vm):
    """the 2048 samples of tests/test_gpu_hetero_ext_oracle.py on the cloud, every estimator on every configuration:
    surface events and medium events are each at least a quarter of the estimator iterations, at least half the
    samples carry light, every radiance is finite (tests/hetero_cloud.py).  On the 4096 samples of the sensitivity
    test: both strategies of estimator 13 sample more than 200 medium vertices; estimator 14 picks each hero channel
    more than 500 times and the three channels of w differ at more than 200 vertices"""
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm, 32)
    try:
        for est in (12, 13, 14):
            for block, interp in hc.EXT_CONFIGS:
                hc.set_ext_cloud(orc_vm, block, interp)
                L, _, (tests, iters, surface, medium) = orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS, counters=True)
                lit = np.count_nonzero(L.any(axis=1))
                print(f"estimator {est}, block {block}, {interp}: {iters} iterations, surface {surface / iters:.3f}, "
                      f"medium {medium / iters:.3f}, lit {lit / len(L):.3f}")
                assert 4 * surface >= iters and 4 * medium >= iters and 2 * lit >= len(L)
                assert np.isfinite(L).all()
        rays, st = _samples(orc_vm)
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN)
        orc_vm.ext_counters()
        orc_vm.trace(13, rays, st, hc.EXT_SA, hc.EXT_SS)
        e13 = orc_vm.ext_counters()
        orc_vm.trace(14, rays, st, hc.EXT_SA, hc.EXT_SS)
        e14 = orc_vm.ext_counters()
        print(f"estimator 13: medium vertices equi-angular {e13['equiangular']}, track {e13['track']}; estimator 14: heroes "
              f"{e14['hero']}, vertices whose three w differ {e14['w_differ']}")
        assert e13["equiangular"] > 200 and e13["track"] > 200
        assert min(e14["hero"]) > 500 and e14["w_differ"] > 200
    finally:
        _reset(orc_vm)


# fault: (the estimators it concerns, what it is, whether a draw or a branch depends on what it changes)
FAULTS = {
    5: ((12, 13), "sigma_s without rho(xt) at the vertex", False),
    6: ((12, 13), "the equi-angular interval [0, t], not [a, b]", True),
    7: ((13,), "the combined pdf's tracking term without T", False),
    8: ((13,), "the medium step's T over the segment behind xt", False),
    9: ((14,), "ws not applied on the surface branch", False),
    10: ((14,), "the hero's scalar transmittance as MISv2's per-light factor", False),
}


@pytest.mark.parametrize("kind", list(FAULTS))
def test_the_inputs_expose_each_class_of_mistake(orc_vm, kind):
    """a condition on the inputs, not a measurement: with the cloud, the box, the medium, the fraction and the colour of
    tests/hetero_cloud.py each of the oracle's deliberate mistakes 5-10 moves at least 200 of 4096 samples beyond the
    bar the GPU is held to (a radiance outside test_gpu_hetero._radiance_bound, or another end state).  Measured
    (block 2, trilinear): fault 5 -- 1950 (12), 1931 (13); 6 -- 2008, 1959; 7 -- 1931; 8 -- 1931; 9 -- 1108; 10 -- 1074.
    In ROOM_LO .. ROOM_HI fault 6 moves 42 and 44: the reason for the smaller box."""
    ests, what, draws = FAULTS[kind]
    orc_vm.set_scene(default_scene())
    rays, st = _samples(orc_vm)
    try:
        hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN)
        for est in ests:
            L, s = orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS)
            orc_vm.set_hetero_fault(kind)
            Lf, sf = orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS)
            orc_vm.set_hetero_fault(0)
            moved = int((~T._radiance_bound(Lf, L).all(axis=1) | (sf != s)).sum())
            print(f"estimator {est}, fault {kind} ({what}): {moved} samples moved, {(sf != s).sum()} end states differ")
            assert moved >= 200, f"fault {kind} ({what}) moves only {moved} samples of estimator {est}"
            assert (sf != s).any() if draws else (sf == s).all()
            assert bitwise_equal(orc_vm.trace(est, rays, st, hc.EXT_SA, hc.EXT_SS)[0], L).all()  # the switch is off again
        for est in {10, 11, 12, 13, 14} - set(ests):  # and it concerns no other estimator
            if est in (10, 11):
                hc.set_cloud(orc_vm, *hc.MAIN)
            else:
                hc.set_ext_cloud(orc_vm, *hc.EXT_MAIN)
            L, s = orc_vm.trace(est, rays[:512], st[:512], hc.EXT_SA, hc.EXT_SS)
            orc_vm.set_hetero_fault(kind)
            Lf, sf = orc_vm.trace(est, rays[:512], st[:512], hc.EXT_SA, hc.EXT_SS)
            orc_vm.set_hetero_fault(0)
            assert (sf == s).all() and bitwise_equal(Lf, L).all(), est
    finally:
        _reset(orc_vm)
