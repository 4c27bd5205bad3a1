"""A plain-Python restatement of residual ratio tracking (csrc/vpt_grid.h: vpt_grid_residual_lm_m) and of the two
control builders beside the two majorant builders, for tests/test_grid_residual.py: the slab test, the DDA over the
super-voxels with vpt_grid_block_plane's planes, the eager draw rem = -log(1 - xi), the residual majorant mu - mn, the
control optical depth's pieces and the weight That * (1 - (rho - mn) / (mu - mn)) -- one IEEE double operation per
Python operation, in the order the header comment of csrc/vpt_grid.h writes down.  The lookup at a tentative point is
eqa_model.lookup (the voxel, or the nested lerps)."""
import math

import numpy as np

import majorant_model as mm
from eqa_model import lookup
from ratio_model import BIG, MAX_STEPS, _axis_index, _slab


def counts(shape, block):
    """(nbx, nby, nbz) of a [nz, ny, nx] grid"""
    nz, ny, nx = shape
    return tuple((n - 1) // block + 1 for n in (nx, ny, nz))


def _blocks(rho, block, dilate, op, start):
    nz, ny, nx = rho.shape
    nbx, nby, nbz = counts(rho.shape, block)
    out = np.full((nbz, nby, nbx), start, dtype=np.float32)
    e = 1 if dilate else 0
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                z0, z1 = max(bz * block - e, 0), min((bz + 1) * block + e, nz)
                y0, y1 = max(by * block - e, 0), min((by + 1) * block + e, ny)
                x0, x1 = max(bx * block - e, 0), min((bx + 1) * block + e, nx)
                out[bz, by, bx] = op(rho[z0:z1, y0:y1, x0:x1])
    return out


def majorants(rho, block, interpolation="nearest"):
    """the block maxima [nbz, nby, nbx]; under the trilinear field over each block dilated by one voxel on every side"""
    return _blocks(np.asarray(rho, np.float32), block, interpolation == "trilinear", np.max, 0.0)


def control(rho, block, interpolation="nearest"):
    """the block minima, the same blocks"""
    return _blocks(np.asarray(rho, np.float32), block, interpolation == "trilinear", np.min, np.inf)


def _plane(lo, hi, cell, nb, block, a, kb):
    """vpt_grid_block_plane"""
    if kb <= 0:
        return lo[a]
    if kb >= nb[a]:
        return hi[a]
    return lo[a] + float(kb * block) * cell[a]


def _next_axis(tn):
    if tn[0] <= tn[1]:
        return 0 if tn[0] <= tn[2] else 2
    return 1 if tn[1] <= tn[2] else 2


def residual(rho, maj, ctl, lo, hi, block, interpolation, sigma_t, o, d, tmax, state):
    """one ray: (That, tauc, end state, draws)"""
    nz, ny, nx = rho.shape
    n = (nx, ny, nz)
    nb = counts(rho.shape, block)
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    o, d = [float(v) for v in o], [float(v) for v in d]
    tmax = float(tmax)
    inv_cell = [float(n[a]) / (hi[a] - lo[a]) for a in range(3)]
    cell = [(hi[a] - lo[a]) / float(n[a]) for a in range(3)]
    rho_max = float(np.float32(rho.max()))
    x = int(state) & 0xFFFFFFFFFFFF
    if not rho_max > 0.0:
        return 1.0, 0.0, x, 0
    iv = _slab(lo, hi, o, d)
    if iv is None:
        return 1.0, 0.0, x, 0
    t0, t1 = iv
    tend = t1 if t1 < tmax else tmax
    i, step, tn, inv = [0] * 3, [0] * 3, [0.0] * 3, [0.0] * 3
    for a in range(3):
        i[a] = _axis_index(n[a], lo[a], inv_cell[a], o[a] + d[a] * t0) // block
        step[a] = 1 if d[a] > 0.0 else (-1 if d[a] < 0.0 else 0)
        inv[a] = 1.0 / d[a] if step[a] else 0.0
        tn[a] = (_plane(lo, hi, cell, nb, block, a, i[a] + (step[a] > 0)) - o[a]) * inv[a] if step[a] else BIG
    max_cross = nb[0] + nb[1] + nb[2] + 4
    t, that, tauc = t0, 1.0, 0.0
    a = _next_axis(tn)
    te = tn[a]
    mu = mn = 0.0
    if te > t:
        mu, mn = float(maj[i[2], i[1], i[0]]), float(ctl[i[2], i[1], i[0]])

    def none():
        return that * math.exp(sigma_t * tauc * -1.0), tauc, x, k + 1

    for k in range(MAX_STEPS):
        xs, xi = mm.erand48_steps(np.array([x], dtype=np.uint64))
        x, xi = int(xs[0]), float(xi[0])
        rem = -math.log(1 - xi)
        tc = 0.0
        found = False
        for _ in range(max_cross):
            if te > t:
                mr = mu - mn
                if mr > 0.0:
                    s = mr * sigma_t
                    tc = t + (rem / s)
                    if tc < te:
                        found = True
                        break
                    rem = rem - s * (te - t)
                e = te if te < tend else tend
                if e > t:
                    tauc = tauc + mn * (e - t)
                t = te
            if not (te < t1) or te > tmax:
                return none()
            i[a] += step[a]
            if i[a] < 0 or i[a] >= nb[a]:
                return none()
            tn[a] = (_plane(lo, hi, cell, nb, block, a, i[a] + (step[a] > 0)) - o[a]) * inv[a]
            a = _next_axis(tn)
            te = tn[a]
            mu = mn = 0.0
            if te > t:
                mu, mn = float(maj[i[2], i[1], i[0]]), float(ctl[i[2], i[1], i[0]])
        if not found:
            return none()
        if tc > tmax or tc >= t1:
            if tend > t:
                tauc = tauc + mn * (tend - t)
            return none()
        tauc = tauc + mn * (tc - t)
        r = lookup(rho, lo, hi, interpolation, [o[q] + d[q] * tc for q in range(3)])
        if r >= mu:
            return 0.0, tauc, x, k + 1
        if r > mn:
            that = that * (1.0 - (r - mn) / (mu - mn))
        t = tc
    return math.nan, tauc, x, MAX_STEPS


def residual_rays(rho, lo, hi, sigma_t, rays, tmax, states, majorant_block, interpolation="nearest"):
    """residual over arrays, on the grids the builders above give: (That, tauc, end states, draws)"""
    rho = np.asarray(rho, np.float32)
    maj, ctl = majorants(rho, majorant_block, interpolation), control(rho, majorant_block, interpolation)
    tmax = np.broadcast_to(np.asarray(tmax, float), (len(rays),))
    out = [residual(rho, maj, ctl, lo, hi, majorant_block, interpolation, sigma_t, rays["o"][i], rays["d"][i], tmax[i], states[i])
           for i in range(len(rays))]
    return (np.array([v[0] for v in out]), np.array([v[1] for v in out]), np.array([v[2] for v in out], dtype=np.uint64),
            np.array([v[3] for v in out], dtype=np.uint32))
