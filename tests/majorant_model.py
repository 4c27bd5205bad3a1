"""Inputs and small models the local-majorant tests share (tests/test_grid_majorants.py on the CPU,
tests/test_gpu_majorants.py on the GPU): the sparse field, rays through a box, the erand48 step on arrays and
the free path's optical depth -log(1 - xi)."""
import numpy as np

import grid_model as gm

# the sparse field: 8 x 6 x 4 voxels, about half of them empty, in grid_model's off-centre box
SPARSE_SHAPE = (4, 6, 8)  # [nz, ny, nx]
SPARSE_LO, SPARSE_HI = gm.TAU_LO, gm.TAU_HI
SIGMA_T = 0.7
MASK48 = np.uint64(0xFFFFFFFFFFFF)


def sparse_field(shape=SPARSE_SHAPE, seed=31):
    """about half the voxels zero, the rest in [0.2, 3]"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.2, 3.0, shape)
    rho[rng.uniform(0, 1, shape) < 0.5] = 0.0
    return rho.astype(np.float32)


def resample2(rho):
    """every voxel repeated 2 x 2 x 2"""
    return np.repeat(np.repeat(np.repeat(rho, 2, axis=0), 2, axis=1), 2, axis=2)


def box_rays(lo, hi, n=4096, seed=17):
    """n rays that all cross the box [lo, hi] (rays, tmax): from a point around the box (every third inside it)
    towards a point inside it; tmax ends every fourth ray inside the box, the others run on"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    ext = hi - lo
    a = lo - 0.6 * ext + rng.uniform(0, 1, (n, 3)) * 2.2 * ext
    inside = np.arange(n) % 3 == 0
    a[inside] = lo + rng.uniform(0.01, 0.99, (int(inside.sum()), 3)) * ext
    b = lo + rng.uniform(0.01, 0.99, (n, 3)) * ext
    seg = b - a
    dist = np.sqrt((seg * seg).sum(axis=1))
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"] = a
    rays["d"] = seg / dist[:, None]
    tmax = np.where(np.arange(n) % 4 == 0, dist, 1e30)
    return rays, tmax


def erand48_steps(x):
    """one step of the erand48 recurrence on an array of states: (new states, the draws)"""
    x = (np.asarray(x, dtype=np.uint64) * np.uint64(0x5DEECE66D) + np.uint64(0xB)) & MASK48
    return x, x.astype(np.float64) / float(1 << 48)


def free_depth(xi):
    """-log(1 - xi): the optical depth a tentative step has to cover"""
    return -np.log(1 - xi)


def same_ray(o, d, n):
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"] = o
    rays["d"] = np.asarray(d, float) / np.linalg.norm(d)
    return rays
