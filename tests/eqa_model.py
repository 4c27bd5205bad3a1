"""A plain-Python restatement of one equi-angular distance decision in the density grid (csrc/vpt_grid_eqa.h:
vpt_grid_eqa_one), for tests/test_grid_eqa.py: the interval [a, b] from the slab test, the two draws, the surface
coin, D / proj / ta / tb / s / dist / pdf with math.sqrt / atan2 / tan, the density at the sampled point (the voxel,
or the nested lerps of the trilinear lookup) and T = exp(sigma_t * tau * -1.0) -- one IEEE double operation per Python
operation, in the header's order.  The optical depths tau come from grid_probe_host (the deterministic walker, which
tests/test_grid_host.py and tests/test_grid_trilinear.py check against models of their own)."""
import math

import numpy as np

import grid_model as gm
from minimal_volumetric_path_tracer_amd import grid_probe_host
from ratio_model import _axis_index, _slab


def _tl_axis(n, lo, inv_cell, p):
    u = (p - lo) * inv_cell - 0.5
    if not u > 0.0:
        u = 0.0
    if u > float(n - 1):
        u = float(n - 1)
    i = int(math.floor(u))
    i = max(0, min(i, max(n - 2, 0)))
    return i, min(i + 1, n - 1), u - float(i)


def _lerp(a, b, f):
    return a + f * (b - a)


def lookup(rho, lo, hi, interpolation, p):
    """vpt_grid_lookup at the point p of the box (clamped like the code: the caller has clipped)"""
    nz, ny, nx = rho.shape
    n = (nx, ny, nz)
    inv_cell = [float(n[a]) / (hi[a] - lo[a]) for a in range(3)]
    if interpolation == "nearest":
        ix, iy, iz = (_axis_index(n[a], lo[a], inv_cell[a], p[a]) for a in range(3))
        return float(rho[iz, iy, ix])
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = (_tl_axis(n[a], lo[a], inv_cell[a], p[a]) for a in range(3))
    r = lambda z, y, x: float(rho[z, y, x])
    c00 = _lerp(r(z0, y0, x0), r(z0, y0, x1), fx)
    c01 = _lerp(r(z0, y1, x0), r(z0, y1, x1), fx)
    c10 = _lerp(r(z1, y0, x0), r(z1, y0, x1), fx)
    c11 = _lerp(r(z1, y1, x0), r(z1, y1, x1), fx)
    return _lerp(_lerp(c00, c01, fy), _lerp(c10, c11, fy), fz)


def interval(lo, hi, o, d, t):
    """step 2: (a, b)"""
    iv = _slab(lo, hi, o, d)
    if iv is None:
        return 0.0, t
    t0, t1 = iv
    return (t0 if t0 > 0.0 else 0.0), (t if t < t1 else t1)


def geometry(o, d, lp):
    """(D, proj) as equiangular_setup forms them"""
    dv = [lp[k] - o[k] for k in range(3)]
    dvn = math.sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2])
    proj = (dv[0] * d[0] + dv[1] * d[1] + dv[2] * d[2]) / (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return math.sqrt(dvn * dvn - proj * proj), proj


def eqa_rays(rho, lo, hi, sigma_t, rays, tmax, light, states, interpolation="nearest"):
    """the model over arrays: (psurf, dist, pdf, T, rho_t, end states) and, beside the probe's outputs, (a, b)"""
    n = len(rays)
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    tmax = np.broadcast_to(np.asarray(tmax, float), (n,))
    light = np.broadcast_to(np.asarray(light, float), (n, 3))
    tau_s = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, states, interpolation=interpolation)[0]
    out = np.zeros((n, 7))
    so = np.zeros(n, dtype=np.uint64)
    med = []
    for i in range(n):
        o, d = [float(v) for v in rays["o"][i]], [float(v) for v in rays["d"][i]]
        t = float(tmax[i])
        a, b = interval(lo, hi, o, d, t)
        x1, x = gm.erand48_step(states[i])
        psurf = math.exp(sigma_t * float(tau_s[i]) * -1.0)
        x2, coin = gm.erand48_step(x1)
        so[i] = x2
        out[i] = (psurf, -1.0, 0.0, 0.0, 0.0, a, b)
        if coin < psurf:
            continue
        lp = [float(v) for v in light[i]]
        D, proj = geometry(o, d, lp)
        ta = math.atan2(a - proj, D)
        tb = math.atan2(b - proj, D)
        s = D * math.tan((1 - x) * ta + x * tb)
        dist = s + proj
        pdf = D / math.fabs(tb - ta) / (s * s + D * D) * (1 - psurf)
        rho_t = lookup(rho, lo, hi, interpolation, [o[k] + d[k] * dist for k in range(3)])
        out[i, 1:3] = dist, pdf
        out[i, 4] = rho_t
        if rho_t != 0.0:
            med.append(i)
    if med:  # T over [0, dist] for the rays that go on
        med = np.array(med)
        tau_d = grid_probe_host(rho, lo, hi, sigma_t, rays[med], out[med, 1], states[med], interpolation=interpolation)[0]
        out[med, 3] = [math.exp(sigma_t * float(v) * -1.0) for v in tau_d]
    return (out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], so), (out[:, 5], out[:, 6])
