"""Independent numpy model of the trilinear density field (csrc/vpt_grid.h, "Trilinear interpolation") for
tests/test_grid_trilinear.py.

Nothing here is shaped like the code under test.  The lookup is the weights form sum w_x w_y w_z rho, not nested
lerps.  The optical depth does not walk cells: it cuts the segment at every analytic crossing of a voxel-centre
plane or a box face, sorts the cuts, and integrates each piece with a 4-point Gauss-Legendre rule (exact for the
cubic a trilinear field is along a line inside one interpolation cell)."""
import numpy as np

# 4-point Gauss-Legendre on [-1, 1]
_GX = np.array([-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526])
_GW = np.array([0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538])


def _axis_weights(x, lo, hi, n):
    """per point: the two voxel indices of one axis and their weights (field clamped at the border)"""
    u = np.clip((x - lo) / (hi - lo) * n - 0.5, 0.0, n - 1.0)
    i0 = np.minimum(np.floor(u).astype(np.int64), max(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = u - i0
    return i0, i1, 1.0 - w1, w1


def density_at(rho, lo, hi, p):
    """the trilinear field at the points p (m x 3), 0 outside the box; rho may be float32 or float64"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    rho = np.asarray(rho, dtype=np.float64)
    nz, ny, nx = rho.shape
    inside = np.all((p >= lo) & (p < hi), axis=1)
    ax = [_axis_weights(p[:, a], lo[a], hi[a], n) for a, n in enumerate((nx, ny, nz))]
    out = np.zeros(len(p))
    for kz in (0, 1):
        for ky in (0, 1):
            for kx in (0, 1):
                w = ax[0][2 + kx] * ax[1][2 + ky] * ax[2][2 + kz]
                out += w * rho[ax[2][kz], ax[1][ky], ax[0][kx]]
    return np.where(inside, out, 0.0)


def _cuts(rho_shape, lo, hi, o, d, tmax):
    nz, ny, nx = rho_shape
    cuts = [0.0, float(tmax)]
    for a, n in enumerate((nx, ny, nz)):
        if d[a] == 0.0:
            continue
        centres = lo[a] + (hi[a] - lo[a]) * (np.arange(n) + 0.5) / n
        planes = np.concatenate(([lo[a]], centres, [hi[a]]))
        t = (planes - o[a]) / d[a]
        cuts.extend(t[(t > 0.0) & (t < tmax)].tolist())
    return np.sort(np.array(cuts))


def _gauss(rho, lo, hi, o, d, a, b):
    """the integral of the field over [a[k], b[k]] of o + d t for every k (each piece inside one cell)"""
    half, mid = 0.5 * (b - a), 0.5 * (a + b)
    t = mid[:, None] + half[:, None] * _GX[None, :]
    p = o[None, None, :] + d[None, None, :] * t[:, :, None]
    f = density_at(rho, lo, hi, p.reshape(-1, 3)).reshape(t.shape)
    return half * (f * _GW[None, :]).sum(axis=1)


def tau_model(rho, lo, hi, o, d, tmax):
    """optical depth of the trilinear field over o + d t, t in [0, tmax] (one ray; d a unit vector)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    o, d = np.asarray(o, float), np.asarray(d, float)
    if not tmax > 0.0:
        return 0.0
    cuts = _cuts(np.shape(rho), lo, hi, o, d, tmax)
    return float(_gauss(rho, lo, hi, o, d, cuts[:-1], cuts[1:]).sum())


def tau_along(rho, lo, hi, o, d, ts):
    """tau(t) of one ray for every t of the array ts (t >= 0): whole pieces summed, the last one up to t"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    o, d = np.asarray(o, float), np.asarray(d, float)
    ts = np.asarray(ts, float)
    top = float(ts.max()) if len(ts) else 0.0
    if not top > 0.0:
        return np.zeros(len(ts))
    cuts = _cuts(np.shape(rho), lo, hi, o, d, top)
    cum = np.concatenate(([0.0], np.cumsum(_gauss(rho, lo, hi, o, d, cuts[:-1], cuts[1:]))))
    k = np.clip(np.searchsorted(cuts, ts, side="right") - 1, 0, len(cuts) - 2)
    return cum[k] + _gauss(rho, lo, hi, o, d, cuts[k], ts)
