"""Independent numpy model of volumetric emission on the density grid (csrc/vpt_grid.h, "Emission") for
tests/test_grid_emission.py and tests/test_gpu_emission.py.

The quantity the emitting track estimates is sigma_t * integral of T(t) rho(t) eps(t) dt over the tracked segment,
T = exp(-sigma_t tau(t)).  Nothing here walks voxels or draws: the segment is cut at every analytic plane crossing
(grid_model / trilinear_model), and each piece is integrated in closed form (nearest: rho and eps are constant on it)
or by a 16-point Gauss-Legendre rule (trilinear: the integrand is smooth inside an interpolation cell)."""
import numpy as np

import grid_model as gm
import trilinear_model as tm

# tests 1 and 2: 6 x 5 x 4 voxels, no two dimensions equal, an off-centre box
SHAPE = (4, 5, 6)  # [nz, ny, nx]
LO, HI = (-1.0, 2.0, -3.0), (5.0, 4.5, 7.0)
# the expectation test: two densities, eps different in every voxel, one oblique ray that enters the box from outside
EX_LO, EX_HI = (0.0, 0.0, 0.0), (4.0, 2.0, 2.0)
EX_SIGMA_T, EX_N, EX_SEED = 0.3, 65536, 20250307
EX_O = (-0.5, 0.3, 0.45)
EX_D = np.array([0.9, 0.3, 0.25]) / np.sqrt(0.9 * 0.9 + 0.3 * 0.3 + 0.25 * 0.25)


def fields(seed=11):
    """(rho, eps) of SHAPE: random, about a quarter of the voxels of each zero (not the same ones)"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.1, 3.0, SHAPE) * (rng.uniform(0, 1, SHAPE) > 0.25)
    eps = rng.uniform(0.0, 2.0, SHAPE) * (rng.uniform(0, 1, SHAPE) > 0.25)
    return rho.astype(np.float32), eps.astype(np.float32)


def expectation_fields():
    """(rho, eps) of shape [2, 2, 8]: rho is 3 in the x slabs 3, 4, 5 and 1 elsewhere -- with super-voxels of two voxels
    the second one holds both densities, so its collisions can be null -- and eps differs voxel by voxel"""
    rho = np.ones((2, 2, 8), dtype=np.float32)
    rho[:, :, 3:6] = 3.0
    eps = (0.25 + 0.0625 * np.arange(32, dtype=np.float32)).reshape(2, 2, 8)[::-1, :, ::-1].copy()
    return rho, eps


def rays(n=400, seed=23):
    """n rays with tmax: origins inside the box (even) and outside, aimed at a point of the box (odd); every seventh
    along an axis, every fifth cut short inside the box"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(LO), np.array(HI)
    ext = hi - lo
    a = lo + rng.uniform(0.02, 0.98, (n, 3)) * ext
    out = np.arange(n) % 2 == 1
    side = rng.integers(0, 2, (n, 3)) * 2 - 1
    a[out] = (0.5 * (lo + hi) + side * (0.6 + rng.uniform(0, 1, (n, 3))) * ext)[out]
    b = lo + rng.uniform(0.02, 0.98, (n, 3)) * ext
    axis = np.arange(n) % 7 == 0
    for i in np.nonzero(axis)[0]:
        k = i % 3
        a[i] = lo + rng.uniform(0.02, 0.98, 3) * ext
        b[i] = a[i]
        b[i, k] = a[i, k] + (1 if i % 2 else -1) * ext[k]
    seg = b - a
    length = np.sqrt((seg * seg).sum(axis=1))
    r = np.zeros(n, dtype=gm.RAY_DTYPE)
    r["o"] = a
    r["d"] = seg / length[:, None]
    tmax = np.where(np.arange(n) % 5 == 0, length, 1e30)
    return r, tmax


def voxel_value(field, lo, hi, p):
    """the field's value in the voxel of each point p (m x 3), indices held to the grid (a point the rounding left a
    hair outside the box reads the border voxel, as the walkers do)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    nz, ny, nx = field.shape
    n = np.array([nx, ny, nz])
    idx = np.clip(np.floor((p - lo) * (n / (hi - lo))).astype(np.int64), 0, n - 1)
    return field[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64)


def reference_nearest(rho, eps, lo, hi, o, d, tmax, sigma_t):
    """sigma_t int T rho eps dt for the piecewise constant fields: per voxel piece eps T0 (1 - exp(-sigma_t rho len))"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    o, d = np.asarray(o, float), np.asarray(d, float)
    nz, ny, nx = rho.shape
    cuts = [0.0, float(tmax)]
    for a, n in enumerate((nx, ny, nz)):
        if d[a] == 0.0:
            continue
        planes = lo[a] + (hi[a] - lo[a]) * np.arange(n + 1) / n
        t = (planes - o[a]) / d[a]
        cuts.extend(t[(t > 0.0) & (t < tmax)].tolist())
    cuts = np.sort(np.array(cuts))
    mid = o[None, :] + d[None, :] * (0.5 * (cuts[1:] + cuts[:-1]))[:, None]
    r = gm.density_at(rho, lo, hi, mid)
    e = gm.density_at(eps, lo, hi, mid)
    depth = sigma_t * r * (cuts[1:] - cuts[:-1])
    t0 = np.exp(-np.concatenate(([0.0], np.cumsum(depth)[:-1])))
    return float(np.sum(e * t0 * -np.expm1(-depth)))


def reference_trilinear(rho, eps, lo, hi, o, d, tmax, sigma_t, order=16):
    """the same integral for the trilinear fields: Gauss-Legendre of `order` points on every piece between two cuts"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    o, d = np.asarray(o, float), np.asarray(d, float)
    cuts = tm._cuts(np.shape(rho), lo, hi, o, d, tmax)
    gx, gw = np.polynomial.legendre.leggauss(order)
    a, b = cuts[:-1], cuts[1:]
    t = (0.5 * (a + b))[:, None] + (0.5 * (b - a))[:, None] * gx[None, :]
    p = o[None, :] + d[None, :] * t.reshape(-1, 1)
    f = tm.density_at(rho, lo, hi, p) * tm.density_at(eps, lo, hi, p) * np.exp(-sigma_t * tm.tau_along(rho, lo, hi, o, d, t.reshape(-1)))
    return float(sigma_t * np.sum((0.5 * (b - a))[:, None] * f.reshape(t.shape) * gw[None, :]))


def reference(rho, eps, lo, hi, o, d, tmax, sigma_t, interpolation):
    f = reference_trilinear if interpolation == "trilinear" else reference_nearest
    return f(rho, eps, lo, hi, o, d, tmax, sigma_t)
