"""Independent numpy model of the density grid (csrc/vpt_grid.h) and the inputs the grid tests share
(tests/test_grid_host.py on the CPU, tests/test_gpu_hetero.py on the GPU).

The optical-depth model does not walk voxels: it cuts the segment at every analytic crossing with a grid plane
inside the box, sorts the cuts, and looks each piece up at its midpoint (rho = 0 outside the box)."""
import numpy as np

from scenes import stream_state

RAY_DTYPE = np.dtype([("o", "<f8", 3), ("d", "<f8", 3)])

# test 1: no two dimensions equal, an off-centre box
TAU_SHAPE = (5, 3, 4)  # [nz, ny, nx]: 4 x 3 x 5 voxels
TAU_LO, TAU_HI = (-1.0, 2.0, -3.0), (5.0, 4.5, 7.0)
# test 3: one axis-parallel ray through two voxels
KS_RHO = np.array([[[1.0, 3.0]]], dtype=np.float32)  # 2 x 1 x 1
KS_LO, KS_HI = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
KS_SIGMA_T, KS_SEED, KS_N = 1.0, 20240611, 65536


def tau_grid(seed=5):
    return np.random.default_rng(seed).uniform(0.0, 3.0, TAU_SHAPE).astype(np.float32)


def density_at(rho, lo, hi, p):
    """rho at the points p (n x 3), 0 outside the box"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    nz, ny, nx = rho.shape
    n = np.array([nx, ny, nz])
    inside = np.all((p >= lo) & (p < hi), axis=1)
    idx = np.clip(np.floor((p - lo) * (n / (hi - lo))).astype(np.int64), 0, n - 1)
    return np.where(inside, rho[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64), 0.0)


def tau_model(rho, lo, hi, o, d, tmax):
    """optical depth of o + d t, t in [0, tmax] (one ray; d a unit vector)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    nz, ny, nx = rho.shape
    cuts = [0.0, float(tmax)]
    for a, n in enumerate((nx, ny, nz)):
        if d[a] == 0.0:
            continue
        planes = lo[a] + (hi[a] - lo[a]) * np.arange(n + 1) / n
        t = (planes - o[a]) / d[a]
        cuts.extend(t[(t > 0.0) & (t < tmax)].tolist())
    cuts = np.sort(np.array(cuts))
    mid = 0.5 * (cuts[1:] + cuts[:-1])
    rho_mid = density_at(rho, lo, hi, o[None, :] + d[None, :] * mid[:, None])
    return float(np.sum(rho_mid * (cuts[1:] - cuts[:-1])))


def tau_rays(n=2000, seed=9):
    """segments a -> b as (rays, tmax): random ones around the box (start outside, end inside, miss it), every
    fifth along an axis (zero direction components), every 97th of zero length, and the rest inside the box"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(TAU_LO), np.array(TAU_HI)
    ext = hi - lo
    a = lo - 0.6 * ext + rng.uniform(0, 1, (n, 3)) * 2.2 * ext
    b = lo - 0.6 * ext + rng.uniform(0, 1, (n, 3)) * 2.2 * ext
    inside = np.arange(n) % 3 == 0
    b[inside] = lo + rng.uniform(0.01, 0.99, (int(inside.sum()), 3)) * ext          # end inside
    both = np.arange(n) % 6 == 0
    a[both] = lo + rng.uniform(0.01, 0.99, (int(both.sum()), 3)) * ext              # start inside too
    far = np.arange(n) % 11 == 0
    a[far] = hi + 1.0 + rng.uniform(0, 1, (int(far.sum()), 3)) * ext                # miss the box
    b[far] = a[far] + rng.uniform(0, 1, (int(far.sum()), 3)) * ext
    axis = np.arange(n) % 5 == 0
    for i in np.nonzero(axis)[0]:                                                   # along an axis
        k = i % 3
        b[i] = a[i]
        b[i, k] = a[i, k] + rng.uniform(-2.0, 2.0) * ext[k]
    zero = np.arange(n) % 97 == 0
    b[zero] = a[zero]                                                               # zero length
    seg = b - a
    tmax = np.sqrt((seg * seg).sum(axis=1))
    rays = np.zeros(n, dtype=RAY_DTYPE)
    rays["o"] = a
    with np.errstate(invalid="ignore", divide="ignore"):
        d = seg / tmax[:, None]
    d[tmax == 0] = (1.0, 0.0, 0.0)
    rays["d"] = d
    return rays, tmax


def states(seed, n):
    return np.array([stream_state(seed, i, 0) for i in range(n)], dtype=np.uint64)


def ks_rays(n=KS_N):
    rays = np.zeros(n, dtype=RAY_DTYPE)
    rays["o"] = (0.0, 0.5, 0.5)
    rays["d"] = (1.0, 0.0, 0.0)
    return rays, np.full(n, 1e30)


def erand48_step(x):
    """one step of the erand48 recurrence (csrc/vpt_rng.h): (new state, the draw)"""
    x = (int(x) * 0x5DEECE66D + 0xB) & 0xFFFFFFFFFFFF
    return x, x / float(1 << 48)


def ks_statistic(t_coll, exit_t, cdf):
    """Kolmogorov distance between the empirical law of t_coll ("none" = an atom at exit_t) and the CDF
    cdf(t) on [0, exit_t), which jumps to 1 at exit_t"""
    t = np.sort(np.where(t_coll < 0, exit_t, t_coll))
    n = len(t)
    body = t < exit_t
    F = np.where(body, cdf(np.minimum(t, exit_t)), 1.0)
    hi_ = np.arange(1, n + 1) / n
    lo_ = np.arange(0, n) / n
    # at the atom the model jumps from cdf(exit_t-) to 1: compare the empirical mass below the atom with it
    d_body = np.max(np.maximum(np.abs(hi_ - F), np.abs(F - lo_))[body]) if body.any() else 0.0
    d_atom = abs(body.sum() / n - cdf(np.array([exit_t]))[0])
    return max(d_body, d_atom)
