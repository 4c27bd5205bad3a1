"""A plain-Python restatement of ratio tracking with the global majorant (csrc/vpt_grid.h: vpt_grid_ratio), for
tests/test_grid_ratio.py: the slab test, the tentative step -log(1 - xi) / (rho_max sigma_t), the voxel index
min(n - 1, floor((p - lo) * inv_cell)) and the weight That * (1 - rho / rho_max), one IEEE double operation per
Python operation in the header's order."""
import math

import numpy as np

import majorant_model as mm

BIG = 1.7976931348623157e+308
MAX_STEPS = 1 << 22


def _slab(lo, hi, o, d):
    """vpt_grid_slab: (t0, t1) or None"""
    a0, a1 = 0.0, BIG
    for a in range(3):
        if d[a] == 0.0:
            if not (lo[a] <= o[a] < hi[a]):
                return None
            continue
        inv = 1.0 / d[a]
        ta, tb = (lo[a] - o[a]) * inv, (hi[a] - o[a]) * inv
        if ta > tb:
            ta, tb = tb, ta
        if ta > a0:
            a0 = ta
        if tb < a1:
            a1 = tb
        if ta != ta or tb != tb:
            return None
    return (a0, a1) if a0 < a1 else None


def _axis_index(n, lo, inv_cell, p):
    v = (p - lo) * inv_cell
    f = float(math.floor(v)) if math.isfinite(v) else v
    if not f >= 0.0:
        return 0
    return int(f) if f < float(n) else n - 1


def ratio_global(rho, lo, hi, sigma_t, o, d, tmax, state):
    """one ray: (That, end state, draws)"""
    nz, ny, nx = rho.shape
    n = (nx, ny, nz)
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    o, d = [float(v) for v in o], [float(v) for v in d]
    inv_cell = [float(n[a]) / (hi[a] - lo[a]) for a in range(3)]
    rho_max = float(np.float32(rho.max()))
    x = int(state) & 0xFFFFFFFFFFFF
    if not rho_max > 0.0:
        return 1.0, x, 0
    iv = _slab(lo, hi, o, d)
    if iv is None:
        return 1.0, x, 0
    t, t1 = iv
    that = 1.0
    for k in range(MAX_STEPS):
        xs, xi = mm.erand48_steps(np.array([x], dtype=np.uint64))
        x, xi = int(xs[0]), float(xi[0])
        t = t + (-math.log(1 - xi) / (rho_max * sigma_t))
        if t > tmax or t >= t1 or t != t:
            return that, x, k + 1
        idx = [_axis_index(n[a], lo[a], inv_cell[a], o[a] + d[a] * t) for a in range(3)]
        r = float(rho[idx[2], idx[1], idx[0]])
        if r >= rho_max:
            return 0.0, x, k + 1
        that = that * (1.0 - r / rho_max)
    return math.nan, x, MAX_STEPS


def ratio_global_rays(rho, lo, hi, sigma_t, rays, tmax, states):
    """ratio_global over arrays: (That, end states, draws)"""
    tmax = np.broadcast_to(np.asarray(tmax, float), (len(rays),))
    out = [ratio_global(rho, lo, hi, sigma_t, rays["o"][i], rays["d"][i], float(tmax[i]), states[i]) for i in range(len(rays))]
    return (np.array([v[0] for v in out]), np.array([v[1] for v in out], dtype=np.uint64),
            np.array([v[2] for v in out], dtype=np.uint32))
