"""A plain-Python restatement of one distance decision of estimator 14 (csrc/vpt_grid_chroma.h: vpt_grid_chroma_one) and
of its weights, for tests/test_grid_chroma.py: the hero draw, the track under the hero's extinction, the optical depth up
to the collision or to tmax, and e, w, ws and T -- one IEEE double operation per Python operation, in the header's order,
with math.exp.  The optical depths and the delta tracks come from grid_probe_host (the walkers, which
tests/test_grid_host.py, test_grid_majorants.py and test_grid_trilinear.py pin against models of their own); a track
starts from the state after the hero draw.  The module also holds the inputs the CPU and the GPU tests share."""
import math

import numpy as np

import grid_model as gm
from minimal_volumetric_path_tracer_amd import grid_probe_host

NAMES = ("hero", "t_coll", "tau", "w", "steps", "states")

# the 2 x 3 x 2 field of the probe tests, in a box of its own with no two extents equal
SHAPE = (2, 3, 2)  # [nz, ny, nx]
LO, HI = (-1.0, 0.5, -2.0), (2.0, 3.0, 1.5)
# the coloured multipliers of the issue, and a medium under which the three extinctions differ
CA, CS = (0.5, 1.0, 2.0), (2.0, 1.0, 0.5)


def field(seed=41):
    return np.random.default_rng(seed).uniform(0.2, 1.0, SHAPE).astype(np.float32)


def coefficients(sigma_a, sigma_s, ca=CA, cs=CS):
    """(sa, ss, st) per channel, formed as the library forms them"""
    sa = [float(sigma_a) * float(c) for c in ca]
    ss = [float(sigma_s) * float(c) for c in cs]
    return sa, ss, [a + s for a, s in zip(sa, ss)]


def rays(n=4096, seed=13):
    """segments around the box LO, HI as (rays, tmax): random ones (start outside, cross, miss), every third ending
    inside the box (tmax inside), every sixth starting inside too, every eleventh missing the box, every fifth along an
    axis, every 97th of zero length, and every fourth running on without a surface (tmax = 1e30)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(LO), np.array(HI)
    ext = hi - lo
    a = lo - 0.6 * ext + rng.uniform(0, 1, (n, 3)) * 2.2 * ext
    b = lo - 0.6 * ext + rng.uniform(0, 1, (n, 3)) * 2.2 * ext
    k = np.arange(n)
    inside = k % 3 == 0
    b[inside] = lo + rng.uniform(0.01, 0.99, (int(inside.sum()), 3)) * ext
    both = k % 6 == 0
    a[both] = lo + rng.uniform(0.01, 0.99, (int(both.sum()), 3)) * ext
    far = k % 11 == 0
    a[far] = hi + 1.0 + rng.uniform(0, 1, (int(far.sum()), 3)) * ext
    b[far] = a[far] + rng.uniform(0, 1, (int(far.sum()), 3)) * ext
    for i in np.nonzero(k % 5 == 0)[0]:
        ax = i % 3
        b[i] = a[i]
        b[i, ax] = a[i, ax] + rng.uniform(-2.0, 2.0) * ext[ax]
    zero = k % 97 == 0
    b[zero] = a[zero]
    seg = b - a
    tmax = np.sqrt((seg * seg).sum(axis=1))
    out = np.zeros(n, dtype=gm.RAY_DTYPE)
    out["o"] = a
    with np.errstate(invalid="ignore", divide="ignore"):
        d = seg / tmax[:, None]
    d[tmax == 0] = (1.0, 0.0, 0.0)
    out["d"] = d
    tmax[(k % 4 == 1) & ~zero] = 1e30
    return out, tmax


def hero(st, state):
    """(h, the state after the draw): no draw where the three extinctions are equal"""
    if st[0] == st[1] and st[1] == st[2]:
        return 0, int(state)
    x, xi = gm.erand48_step(state)
    h = int(xi * 3)
    return (h if h < 2 else 2), x


def e_of(st, tau):
    x0, x1, x2 = st[0] * tau, st[1] * tau, st[2] * tau
    mn = x0 if x0 < x1 else x1
    mn = mn if mn < x2 else x2
    return [math.exp((x0 - mn) * -1.0), math.exp((x1 - mn) * -1.0), math.exp((x2 - mn) * -1.0)]


def w_of(ss, st, tau):
    e = e_of(st, tau)
    grey = st[0] == st[1] and st[1] == st[2]  # the mean of three equal terms, exactly (csrc/vpt_grid_chroma.h)
    den = st[0] if grey else ((st[0] * e[0] + st[1] * e[1]) + st[2] * e[2]) / 3.0
    return [(ss[k] * e[k]) / den for k in range(3)]


def ws_of(st, tau):
    e = e_of(st, tau)
    den = ((e[0] + e[1]) + e[2]) / 3.0
    return [e[k] / den for k in range(3)]


def T_of(st, tau):
    return [math.exp(st[k] * tau * -1.0) for k in range(3)]


def chroma_rays(rho, lo, hi, sa, ss, rays, tmax, states, interpolation="nearest", majorant_block=0):
    """the model over arrays, in grid_chroma_probe_host's order: (hero, t_coll, tau, w (3, n), steps, end states)"""
    n = len(rays)
    st = [float(a) + float(s) for a, s in zip(sa, ss)]
    ss = [float(s) for s in ss]
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, float), (n,)))
    h = np.zeros(n, dtype=np.int32)
    so = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        h[i], so[i] = hero(st, states[i])
    tc, steps = np.zeros(n), np.zeros(n, dtype=np.uint32)
    for k in range(3):  # the tracks under st[k], from the state after the hero draw
        idx = np.nonzero(h == k)[0]
        if len(idx):
            _, tc[idx], so[idx], steps[idx] = grid_probe_host(rho, lo, hi, st[k], rays[idx], tmax[idx], so[idx],
                                                              majorant_block=majorant_block, return_steps=True,
                                                              interpolation=interpolation)
    cap = tc != tc
    upto = np.where(tc >= 0, tc, tmax)
    upto[cap] = 0.0
    tau = grid_probe_host(rho, lo, hi, 1.0, rays, upto, states, interpolation=interpolation)[0]
    tau[cap] = 0.0
    w = np.zeros((3, n))
    for i in range(n):
        if cap[i]:
            continue
        w[:, i] = w_of(ss, st, float(tau[i])) if tc[i] >= 0 else ws_of(st, float(tau[i]))
    return h, tc, tau, w, steps, so
