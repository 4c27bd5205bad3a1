"""The two walkers of spectral tracking on the CPU (vpt_grid_spectral_probe_host: csrc/vpt_grid_spectral.h compiled for the
host): the probe against a plain-Python restatement bit for bit, the grey identities against the scalar probes of
estimators 10 and 11, the largest channel against ratio tracking under the bounding extinction, the expectation of every
weight from the inputs alone, the bound that the conservation of the weights gives, and the argument checks.  No GPU."""
import functools
import math

import numpy as np
import pytest

import chroma_model as cm
import grid_model as gm
import ratio_model as rm
import spectral_model as sm
from minimal_volumetric_path_tracer_amd import (VPTError, _lib, grid_probe_host, grid_ratio_probe_host,
                                                grid_spectral_probe_host)
from test_grid_chroma import CASE_IDS, CASES, MEDIA


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


N_MODEL = 384  # the rays of the model comparison: the first of chroma_model's 4096, every kind of them among these


def _medium(name):
    scale, sigma_a, sigma_s, ca, cs = MEDIA[name]
    return (cm.field() * np.float32(scale)).astype(np.float32), sigma_a, sigma_s, ca, cs


# "steep": the largest extinction is 16384.5 on a field of up to 4, so a ray through the box has a majorant optical depth
# of 1e5 and more -- and spectral tracking takes that many tentative steps, in every walker (seconds per ray in the Python
# model, half a minute per 4096 rays on the host).  Its rays are chroma_model's with the surface moved up: ray i ends
# where the majorant optical depth sb rho_max (tmax - t_entry) is STEEP_DEPTHS[i % 4], formed from the inputs alone
STEEP_DEPTHS = (0.25, 1.0, 4.0, 400.0)


@functools.lru_cache(maxsize=None)
def _inputs(name="field", n=4096):
    rays, tmax = cm.rays()
    st = gm.states(7, len(rays))
    if name == "steep":
        rho, sigma_a, sigma_s, ca, cs = _medium(name)
        per_length = max(cm.coefficients(sigma_a, sigma_s, ca, cs)[2]) * float(rho.max())
        tmax = tmax.copy()
        for i in range(len(rays)):
            iv = rm._slab([float(v) for v in cm.LO], [float(v) for v in cm.HI], [float(v) for v in rays["o"][i]],
                          [float(v) for v in rays["d"][i]])
            if iv is not None:
                tmax[i] = min(tmax[i], iv[0] + STEEP_DEPTHS[i % 4] / per_length)
    return rays[:n], tmax[:n], st[:n]


def probe(case, beta=None, n=4096):
    """the host probe on a case of test_grid_chroma's CASES; tests/test_gpu_hetero_spectral.py compares the device probe
    with it"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = _medium(name)
    rays, tmax, st = _inputs(name, n)
    return grid_spectral_probe_host(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st, absorption=ca, scattering=cs,
                                    majorant_block=block, interpolation=ip, beta=beta)


def _same(names, got, want):
    for nm, g, w in zip(names, got, want):
        if g.dtype == np.float64:
            assert (_bits(g) == _bits(w)).all(), f"{nm}: {(_bits(g) != _bits(w)).sum()} of {g.size} differ"
        else:
            assert (g == w).all(), f"{nm}: {(g != w).sum()} of {g.size} differ"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_probe_equals_the_python_model(case):
    """384 rays around the 2 x 3 x 2 field (they miss the box, start inside it, end inside it, run on without a surface,
    have no length): t_coll, W, T, the steps and the end states of both walkers bit for bit, with beta = 1 and with a
    throughput that differs per ray and has a channel at zero"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = _medium(name)
    rays, tmax, st = _inputs(name, N_MODEL)
    sa, ss, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
    assert len(set(stk)) == 3
    betas = np.random.default_rng(5).uniform(-1.0, 2.0, (N_MODEL, 3))
    betas[::3, 2] = 0.0
    betas[::7] = 0.0  # nothing carried: h = (1, 1, 1)
    for beta in (None, betas):
        want = sm.spectral_rays(rho, cm.LO, cm.HI, sa, ss, rays, tmax, st, ip, block, beta=beta)
        got = probe(case, beta, N_MODEL)
        _same(sm.NAMES, got, want)
    tc, w, steps, _, T, rsteps, _ = got
    assert not np.isnan(tc).any() and not np.isnan(T).any()  # no walk reaches the step cap
    coll, none = tc >= 0, tc == -1
    assert (coll | none).all() and np.isfinite(w).all() and (w >= 0).all() and (T >= 0).all() and (T <= 1).all()
    inside = (rays["o"] > np.array(cm.LO)).all(axis=1) & (rays["o"] < np.array(cm.HI)).all(axis=1)
    print(f"{case}: collisions {coll.sum()}, none {none.sum()}, start inside {inside.sum()}, max steps {steps.max()}, "
          f"{rsteps.max()}")
    assert inside.sum() > 30 and (~inside).sum() > 100
    if name == "zero":
        assert none.all() and (_bits(w) == _bits(np.ones_like(w))).all() and (_bits(T) == _bits(np.ones_like(T))).all()
        assert (steps == 0).all() and (rsteps == 0).all()
    else:
        assert coll.sum() > 50 and none.sum() > 50
        assert (none & (steps > 1)).sum() >= 3  # a track that met null collisions and found nothing
        assert ((T > 0) & (T < 1)).any(axis=0).sum() > 50


GREY_MEDIA = ((0.3, 0.9, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)), (0.5, 0.9, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)),
              (0.25, 0.25, (1.5, 1.0, 0.5), (0.5, 1.0, 1.5)))


@pytest.mark.parametrize("block", [0, 1, 2])
@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
def test_grey_is_the_scalar_walkers(interpolation, block):
    """equal extinctions: the ratio walk is grid_ratio_probe_host's in all three channels with its state and steps, the
    track is grid_probe_host's t_coll, state and steps, W at "none" is exactly 1.0 and at a collision ss_c / st in the
    bits of chroma_model's grey weight: with the default multipliers and with a coloured albedo on a grey extinction.  A
    throughput changes nothing"""
    rho = cm.field()
    rays, tmax, st = _inputs()
    for sigma_a, sigma_s, ca, cs in GREY_MEDIA:
        _, ss, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
        assert stk[0] == stk[1] == stk[2] == sigma_a + sigma_s
        that, rso11, rsteps11 = grid_ratio_probe_host(rho, cm.LO, cm.HI, stk[0], rays, tmax, st, majorant_block=block,
                                                      interpolation=interpolation)
        _, tc10, so10, steps10 = grid_probe_host(rho, cm.LO, cm.HI, stk[0], rays, tmax, st, majorant_block=block,
                                                 return_steps=True, interpolation=interpolation)
        for beta in (None, (1.0, 0.25, 0.0)):
            tc, w, steps, so, T, rsteps, rso = grid_spectral_probe_host(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st,
                                                                        absorption=ca, scattering=cs, majorant_block=block,
                                                                        interpolation=interpolation, beta=beta)
            for c in range(3):
                assert (_bits(T[c]) == _bits(that)).all()
            assert (rso == rso11).all() and (rsteps == rsteps11).all()
            assert (_bits(tc) == _bits(tc10)).all() and (so == so10).all() and (steps == steps10).all()
            coll = tc >= 0
            assert coll.sum() > 500 and (~coll).sum() > 500
            grey_w = cm.w_of(ss, stk, 0.37)  # chroma_model's grey weight: whatever tau is
            for c in range(3):
                assert (_bits(w[c][coll]) == _bits(np.float64(grey_w[c]))).all()
                assert grey_w[c] == ss[c] / stk[0]
                assert (_bits(w[c][~coll]) == _bits(np.float64(1.0))).all()
        assert (that > 0).sum() > 500 and (that < 1).sum() > 500  # the estimate moves, and rays pass
    assert len({ss[c] / stk[0] for c in range(3)}) == 3  # the coloured albedo: the three channels differ


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "zero"], ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] != "zero"])
def test_largest_channel_is_ratio_tracking_under_sb(case):
    """coloured coefficients: on every ray where ratio tracking under sigma_t = sb returns a non-zero value, the largest
    channel's T and the end state are that walk's bit for bit -- at least half of the rays"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = _medium(name)
    rays, tmax, st = _inputs(name)
    _, _, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
    big = int(np.argmax(stk))
    sb = max(stk)
    assert sorted(stk)[1] < sb
    that, so11, steps11 = grid_ratio_probe_host(rho, cm.LO, cm.HI, sb, rays, tmax, st, majorant_block=block, interpolation=ip)
    _, _, _, _, T, rsteps, rso = probe(case)
    nz = that != 0
    print(f"{case}: {nz.sum()} of {len(rays)} rays with a non-zero estimate; channel {big}")
    assert nz.sum() >= len(rays) // 2
    assert (_bits(T[big][nz]) == _bits(that[nz])).all() and (rso[nz] == so11[nz]).all() and (rsteps[nz] == steps11[nz]).all()
    assert (T[big][~nz] == 0).all() and (rsteps[~nz] >= steps11[~nz]).all()
    if name == "field":
        assert (rsteps[~nz] > steps11[~nz]).sum() > 20  # the walk goes on for the other two channels
        small = int(np.argmin(stk))
        assert (T[small][~nz] > 0).sum() > 20


# the expectation test: grid_model's ray down the axis of rho = (1, 3), tau = 4, with the numpy check's extinctions
# (0.030, 0.012, 0.0045) scaled so that sb * tau = 1.65 as there
EX_SCALE = 1.65 / (0.030 * 4.0)
EX_SA, EX_SS = (0.010 * EX_SCALE, 0.002 * EX_SCALE, 0.0005 * EX_SCALE), (0.020 * EX_SCALE, 0.010 * EX_SCALE, 0.0040 * EX_SCALE)


@pytest.mark.parametrize("block", [0, 1])
def test_expectation_in_every_channel(block):
    """65 536 states down the axis of the non-uniform field rho = (1, 3) (tau = 4, sb tau = 1.65).  The mean of T_c against
    exp(-st_c tau), the mean of W_c over "none" (zero elsewhere) against the same, the mean of w_c over collisions against
    (ss_c / st_c)(1 - exp(-st_c tau)): each within 4.5 of the sample's own standard errors (7e-6 two-sided).  So that the
    test cannot pass vacuously: the bound is at most 5 % of the target, and the target of either other channel lies
    outside it.  block 1: the local walk, whose majorant is the voxel's own density -- every collision with
    q = 1"""
    rays, tmax = gm.ks_rays()
    st = gm.states(gm.KS_SEED, len(rays))
    n = len(rays)
    assert n == 65536
    tau = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays[:1], 1e30, st[:1])[0][0]
    assert tau == 4.0
    stk = [a + s for a, s in zip(EX_SA, EX_SS)]
    sb = max(stk)
    assert 1.0 < sb * tau < 3.0 and len(set(stk)) == 3
    tc, w, _, _, T, _, _ = grid_spectral_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, 1.0, rays, tmax, st, absorption=EX_SA,
                                                    scattering=EX_SS, majorant_block=block)
    coll = tc >= 0
    assert not np.isnan(tc).any() and 1000 < coll.sum() < n - 1000
    want_T = [math.exp(-stk[c] * tau) for c in range(3)]
    want_w = [(EX_SS[c] / stk[c]) * (1 - math.exp(-stk[c] * tau)) for c in range(3)]
    for name, vals, want in (("T", T, want_T), ("W none", np.where(~coll, w, 0.0), want_T), ("w coll", np.where(coll, w, 0.0), want_w)):
        for c in range(3):
            v = vals[c]
            bound = 4.5 * float(v.std(ddof=1)) / math.sqrt(n)
            others = [want[k] for k in range(3) if k != c]
            print(f"block {block} {name}_{c}: mean {v.mean():.6f}, target {want[c]:.6f}, |diff| {abs(v.mean() - want[c]):.2e}, "
                  f"bound {bound:.2e} ({bound / want[c]:.4f} of it), rel. deviation {v.std(ddof=1) / v.mean():.3f}, max "
                  f"{v.max():.4f}, the other channels' {others[0]:.6f}, {others[1]:.6f}")
            assert bound <= 0.05 * want[c]
            assert all(abs(o - want[c]) > bound for o in others)
            assert abs(v.mean() - want[c]) <= bound


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "zero"], ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] != "zero"])
def test_weights_are_bounded(case):
    """the conservation of csrc/vpt_grid_spectral.h, derived and not measured: with beta = 1 the three weights sum to 3 on
    every branch, so max_c W_c <= 3 (1 + 2^-40); with beta = (1, 0.25, 0), sum_c |beta_c| W_c <= (sum_c |beta_c|)(1 + 2^-40).
    W before the albedo: at "none" the probe returns it; at a collision it returns fl(W_c alb_c), and the bound is
    multiplied by alb_c (one rounding of 2^-53 against the slack of 2^-40).  All 4096 rays"""
    name, ip, block = case
    _, sigma_a, sigma_s, ca, cs = _medium(name)
    _, ss, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
    alb = np.array([ss[c] / stk[c] for c in range(3)])
    slack = 1.0 + 2.0 ** -40
    for beta in ((1.0, 1.0, 1.0), (1.0, 0.25, 0.0)):
        tc, w, _, _, _, _, _ = probe(case, beta)
        coll = tc >= 0
        b = np.abs(np.array(beta))
        total = b.sum()
        # sum_c |beta_c| W_c, with W_c alb_c <= alb_c X  <=>  W_c <= X where alb_c > 0
        wn, wc = w[:, ~coll], w[:, coll]
        assert ((b[:, None] * wn).sum(axis=0) <= total * slack).all()
        assert ((b[:, None] * wc / alb[:, None]).sum(axis=0) <= total * slack * (1.0 + 2.0 ** -50)).all()
        if beta == (1.0, 1.0, 1.0):
            assert (wn.max(axis=0) <= 3.0 * slack).all()
            assert (wc <= 3.0 * slack * alb[:, None]).all()
            s = wn.sum(axis=0)
            print(f"{case}: max W {wn.max():.6f} (none), {(wc / alb[:, None]).max():.6f} (collision); sum at none in "
                  f"[{s.min()!r}, {s.max()!r}]")
            assert np.abs(s - 3.0).max() <= 3.0 * 2.0 ** -40
            if name == "field":
                assert wn.max() > 1.5  # the weights do move


def test_argument_errors():
    """NULLs, n < 0, a channel without extinction, a bad block, a bad mode, a coefficient that is negative or not finite"""
    rays, tmax = gm.ks_rays(4)
    st = gm.states(1, 4)
    args = (gm.KS_RHO, gm.KS_LO, gm.KS_HI, 0.5, 0.5, rays, tmax, st)
    for bad in (-0.5, float("nan"), float("inf")):
        for kw in ({"absorption": (1.0, bad, 1.0)}, {"scattering": (1.0, 1.0, bad)}):
            with pytest.raises(VPTError) as ei:
                grid_spectral_probe_host(*args, **kw)
            assert ei.value.code == _lib.VPT_E_INVALID, (bad, kw)
    with pytest.raises(VPTError) as ei:
        grid_spectral_probe_host(*args, absorption=(1.0, 0.0, 1.0), scattering=(1.0, 0.0, 1.0))  # st_1 == 0
    assert ei.value.code == _lib.VPT_E_INVALID
    grid_spectral_probe_host(*args, absorption=(0.0, 0.0, 0.0))  # no absorption is a medium
    grid_spectral_probe_host(*args, scattering=(0.0, 0.0, 0.0))  # and so is no scattering: every collision's w is +0
    for kw in ({"majorant_block": -1}, {"interpolation": "cubic"}, {"absorption": (1.0, 1.0)}):
        with pytest.raises(VPTError) as ei:
            grid_spectral_probe_host(*args, **kw)
        assert ei.value.code == _lib.VPT_E_INVALID
    # the C entry point itself: NULL arrays and a negative count
    import ctypes

    from minimal_volumetric_path_tracer_amd.tracer import _grid_args
    d, r = _grid_args(gm.KS_RHO, gm.KS_LO, gm.KS_HI)
    sa, ss = np.full(3, 0.5), np.full(3, 0.5)
    fn = _lib.lib().vpt_grid_spectral_probe_host
    tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, float), (4,)))
    good = [ctypes.byref(d), r.ctypes.data, 0, 0, sa.ctypes.data, ss.ctypes.data, rays.ctypes.data, tm.ctypes.data, None,
            st.ctypes.data, 4] + [None] * 7
    assert fn(*good) == _lib.VPT_OK  # every output may be NULL, and beta
    for k in (0, 1, 4, 5, 6, 7, 9):
        bad = list(good)
        bad[k] = None
        assert fn(*bad) == _lib.VPT_E_INVALID, k
    bad = list(good)
    bad[10] = -1
    assert fn(*bad) == _lib.VPT_E_INVALID
    assert _lib.HETERO_SPECTRAL == 16
