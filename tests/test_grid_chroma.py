"""The distance decision of the chromatic medium on the CPU (vpt_grid_chroma_probe_host: csrc/vpt_grid_chroma.h compiled
for the host): the probe against a plain-Python restatement bit for bit, the bounds of the weights, unbiasedness of the
decision in every channel from the inputs alone, the grey identities against the plain grid probe, and the argument
checks.  No GPU."""
import functools
import math

import numpy as np
import pytest

import chroma_model as cm
import grid_model as gm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_chroma_probe_host, grid_probe_host


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# (field, sigma_a, sigma_s, absorption, scattering).  "steep": one channel's extinction is 2^14 times the others', so
# where another channel is the hero st_0 * tau reaches 1e4 and beyond, on the field scaled by 4
MEDIA = {
    "field": (1.0, 0.3, 0.9, cm.CA, cm.CS),
    "zero": (0.0, 0.3, 0.9, cm.CA, cm.CS),
    "steep": (4.0, 1.0, 0.5, (16384.0, 1.0, 0.25), (1.0, 1.0, 1.0)),
}
CASES = [(m, ip, block) for m in MEDIA for ip in ("nearest", "trilinear") for block in (0, 1, 2)]
CASE_IDS = ["-".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs():
    rays, tmax = cm.rays()
    return rays, tmax, gm.states(7, len(rays))


def _medium(name):
    scale, sigma_a, sigma_s, ca, cs = MEDIA[name]
    return (cm.field() * np.float32(scale)).astype(np.float32), sigma_a, sigma_s, ca, cs


def probe(case):
    """the host probe on a case of CASES; tests/test_gpu_hetero_chroma.py compares the device probe with it"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = _medium(name)
    rays, tmax, st = _inputs()
    return grid_chroma_probe_host(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st, absorption=ca, scattering=cs,
                                  majorant_block=block, interpolation=ip)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_host_probe_equals_the_python_model(case):
    """4096 rays around the 2 x 3 x 2 field (they miss the box, start inside it, end inside it, run on without a
    surface): hero, distance, optical depth, weights, steps and end state bit for bit; every weight finite and within
    its bound, w_c <= 3 ss_c / st_c at a collision and ws_c <= 3 at none, on every ray"""
    name, ip, block = case
    rho, sigma_a, sigma_s, ca, cs = _medium(name)
    rays, tmax, st = _inputs()
    assert len(rays) == 4096
    sa, ss, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
    want = cm.chroma_rays(rho, cm.LO, cm.HI, sa, ss, rays, tmax, st, ip, block)
    got = probe(case)
    for nm, g, w in zip(cm.NAMES, got, want):
        if g.dtype == np.float64:
            assert (_bits(g) == _bits(w)).all(), f"{nm}: {(_bits(g) != _bits(w)).sum()} of {g.size} differ"
        else:
            assert (g == w).all(), f"{nm}: {(g != w).sum()} of {g.size} differ"
    hero, tc, tau, w, steps, _ = got
    assert not np.isnan(tc).any()  # no track reaches the step cap
    coll, none = tc >= 0, tc == -1
    assert (coll | none).all() and np.isfinite(w).all() and (w >= 0).all()
    assert all((hero == k).sum() > 1000 for k in range(3))
    for c in range(3):
        assert (w[c][coll] <= 3 * ss[c] / stk[c]).all(), f"w_{c}: max {w[c][coll].max()!r} of {3 * ss[c] / stk[c]!r}"
        assert (w[c][none] <= 3.0).all(), f"ws_{c}: max {w[c][none].max()!r}"
    x_max = float((max(stk) * tau).max())
    print(f"{case}: collisions {coll.sum()}, none {none.sum()}, max st_k tau {x_max:.4g}, max w {w[:, coll].max(initial=0):.6f}, "
          f"max ws {w[:, none].max(initial=0):.6f}")
    if name == "zero":
        assert none.all() and (_bits(tau) == 0).all() and (_bits(w) == _bits(np.ones_like(w))).all() and (steps == 0).all()
    else:
        assert coll.sum() > 500 and none.sum() > 500
        assert (none & (tau > 0)).sum() > 50  # a track that crossed medium and found nothing
    if name == "steep":
        assert x_max > 1e4
        assert (w[0][hero != 0] == 0).sum() > 100  # the steep channel's weight underflows to +0, and nothing is 0 / 0


# the unbiasedness test's medium: the coloured multipliers on (0.1, 0.3)
UB_SA, UB_SS = 0.1, 0.3


def test_unbiased_in_every_channel():
    """65 536 decisions down the axis of rho = (1, 3) (grid_model's ray: tau_max = 4) with the coloured multipliers.  The
    collision density of hero h is st_h rho T_h and "none" has the probability T_h(tau_max), so under the balance
    heuristic E[w_c [collision]] = (ss_c / st_c)(1 - exp(-st_c tau_max)) and E[ws_c [none]] = exp(-st_c tau_max) in each
    channel c.  Each sample mean lies within 4.5 of its own standard errors of that value (7e-6 two-sided).  So that the
    test cannot pass vacuously: the bound is at most 5 % of the analytic value, and the analytic value of either other
    channel -- what a grey medium of that channel's coefficients gives -- lies outside it"""
    rays, tmax = gm.ks_rays()
    st = gm.states(gm.KS_SEED, len(rays))
    n = len(rays)
    assert n == 65536
    tau_max = grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays[:1], 1e30, st[:1])[0][0]
    assert tau_max == 4.0
    _, ss, stk = cm.coefficients(UB_SA, UB_SS)
    assert len(set(stk)) == 3
    hero, tc, tau, w, _, _ = grid_chroma_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, UB_SA, UB_SS, rays, tmax, st,
                                                    absorption=cm.CA, scattering=cm.CS)
    coll = tc >= 0
    assert not np.isnan(tc).any() and 1000 < coll.sum() < n - 1000
    assert all(abs((hero == k).mean() - 1 / 3) <= 4.5 * math.sqrt(2 / 9 / n) for k in range(3))
    want_w = [(ss[c] / stk[c]) * (1 - math.exp(-stk[c] * tau_max)) for c in range(3)]
    want_ws = [math.exp(-stk[c] * tau_max) for c in range(3)]
    for name, mask, want in (("w", coll, want_w), ("ws", ~coll, want_ws)):
        for c in range(3):
            v = np.where(mask, w[c], 0.0)
            bound = 4.5 * float(v.std(ddof=1)) / math.sqrt(n)
            others = [want[k] for k in range(3) if k != c]
            print(f"{name}_{c}: mean {v.mean():.6f}, analytic {want[c]:.6f}, |diff| {abs(v.mean() - want[c]):.2e}, bound "
                  f"{bound:.2e} ({bound / want[c]:.4f} of it), the other channels' {others[0]:.6f}, {others[1]:.6f}")
            assert bound <= 0.05 * want[c]
            assert all(abs(o - want[c]) > bound for o in others)
            assert abs(v.mean() - want[c]) <= bound


@pytest.mark.parametrize("block", [0, 2])
@pytest.mark.parametrize("interpolation", ["nearest", "trilinear"])
def test_grey_identities(interpolation, block):
    """equal extinctions: no hero draw -- hero 0, and distance, steps and end state are grid_probe_host's on the same
    rays -- and w_c == ss_c / st, ws_c == 1.0 bitwise: with the default multipliers (any medium), and with a coloured
    albedo on a grey extinction (dyadic multipliers on sigma_a == sigma_s)"""
    rho = cm.field()
    rays, tmax, st = _inputs()
    s = 0.5 + 0.9
    assert ((s + s) + s) / 3.0 != s  # an extinction whose rounded mean of three is not itself
    for sigma_a, sigma_s, ca, cs in ((0.3, 0.9, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)), (0.5, 0.9, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)),
                                     (0.25, 0.25, (1.5, 1.0, 0.5), (0.5, 1.0, 1.5))):
        _, ss, stk = cm.coefficients(sigma_a, sigma_s, ca, cs)
        assert stk[0] == stk[1] == stk[2] == sigma_a + sigma_s
        hero, tc, tau, w, steps, so = grid_chroma_probe_host(rho, cm.LO, cm.HI, sigma_a, sigma_s, rays, tmax, st, absorption=ca,
                                                             scattering=cs, majorant_block=block, interpolation=interpolation)
        _, tc10, so10, steps10 = grid_probe_host(rho, cm.LO, cm.HI, sigma_a + sigma_s, rays, tmax, st, majorant_block=block,
                                                 return_steps=True, interpolation=interpolation)
        assert (hero == 0).all() and (so == so10).all() and (steps == steps10).all()
        assert (_bits(tc) == _bits(tc10)).all()
        coll = tc >= 0
        assert coll.sum() > 500 and (~coll).sum() > 500
        upto = np.where(coll, tc, tmax)
        assert (_bits(tau) == _bits(grid_probe_host(rho, cm.LO, cm.HI, 1.0, rays, upto, st, interpolation=interpolation)[0])).all()
        for c in range(3):
            assert (_bits(w[c][coll]) == _bits(np.float64(ss[c] / stk[0]))).all()
            assert (_bits(w[c][~coll]) == _bits(np.float64(1.0))).all()
    assert len({ss[c] / stk[0] for c in range(3)}) == 3  # the coloured albedo: the three channels differ


def test_three_equal_terms_do_not_average_to_themselves():
    """why grey extinction takes den = st[0] (csrc/vpt_grid_chroma.h): ((s + s) + s) / 3.0 != s for a share of all
    doubles -- four million random values between 1e-300 and 1e300, every one of the misses one ulp away --, while
    three ones do average to 1.0, which is all ws needs"""
    rng = np.random.default_rng(3)
    s = rng.uniform(1.0, 2.0, 1 << 22) * 10.0 ** rng.integers(-300, 300, 1 << 22)
    m = ((s + s) + s) / 3.0
    miss = m != s
    print(f"{miss.sum()} of {len(s)} ({miss.mean():.4f})")
    assert 0.05 < miss.mean() < 0.3
    assert ((m[miss] == np.nextafter(s[miss], np.inf)) | (m[miss] == np.nextafter(s[miss], 0))).all()
    assert ((1.0 + 1.0) + 1.0) / 3.0 == 1.0


def test_argument_errors():
    """the setter's rule through the host-only path: a multiplier that is negative or not finite, a channel without
    extinction, and what is not three numbers"""
    rays, tmax = gm.ks_rays(4)
    st = gm.states(1, 4)
    args = (gm.KS_RHO, gm.KS_LO, gm.KS_HI, 0.5, 0.5, rays, tmax, st)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        for kw in ({"absorption": (1.0, bad, 1.0)}, {"scattering": (1.0, 1.0, bad)}):
            with pytest.raises(VPTError) as ei:
                grid_chroma_probe_host(*args, **kw)
            assert ei.value.code == _lib.VPT_E_INVALID, (bad, kw)
    with pytest.raises(VPTError) as ei:
        grid_chroma_probe_host(*args, absorption=(1.0, 0.0, 1.0), scattering=(1.0, 0.0, 1.0))  # st_1 == 0
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_chroma_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 0.0, 0.0, rays, tmax, st)  # no medium at all
    assert ei.value.code == _lib.VPT_E_INVALID
    grid_chroma_probe_host(*args, absorption=(0.0, 0.0, 0.0))  # no absorption is a medium
    grid_chroma_probe_host(*args, scattering=(0.0, 0.0, 0.0))  # and so is no scattering: every w is +0
    for kw in ({"absorption": (1.0, 1.0)}, {"scattering": 1.0}, {"absorption": np.ones((3, 1))}):
        with pytest.raises(VPTError) as ei:
            grid_chroma_probe_host(*args, **kw)
        assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_chroma_probe_host(*args, majorant_block=-1)
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(VPTError) as ei:
        grid_chroma_probe_host(*args, interpolation="cubic")
    assert ei.value.code == _lib.VPT_E_INVALID
    with pytest.raises(ValueError):
        grid_chroma_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 0.5, 0.5, rays, tmax, st[:3])  # states of another length
    assert _lib.HETERO_CHROMATIC == 14
