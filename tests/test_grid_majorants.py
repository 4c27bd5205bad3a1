"""Local majorants for delta tracking on the CPU (vpt_grid_probe_host_lm: csrc/vpt_grid.h's vpt_grid_track_lm
compiled for the host): the reduction to the global-majorant track with one super-voxel, analytic inversion
at block size 1, the distribution at block size 2, the step counts, and the rays and grids that stress the
super-voxel walker.  No GPU."""
import numpy as np
import pytest

import grid_model as gm
import majorant_model as mm
from minimal_volumetric_path_tracer_amd import VPTError, _lib, grid_probe_host

SIGMA_T = mm.SIGMA_T
REL = 1e-10


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def sparse():
    """the sparse field, its 4096 rays and start states, and the tracks at block sizes 0, 1 and 2 (computed once,
    read-only)"""
    rho = mm.sparse_field()
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI)
    st = gm.states(11, len(rays))
    out = {"rho": rho, "rays": rays, "tmax": tmax, "st": st}
    for b in (0, 1, 2):
        out[b] = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st, majorant_block=b, return_steps=True)
    for v in out.values():
        for arr in (v if isinstance(v, tuple) else (v,)):
            arr.setflags(write=False)
    return out


def _reduction_sets():
    rho = gm.tau_grid()
    rays, tmax = gm.tau_rays()
    for sigma_t in (0.7, 0.05):
        yield rho, gm.TAU_LO, gm.TAU_HI, sigma_t, rays, tmax, gm.states(3, len(rays))
    rays, tmax = gm.ks_rays()
    yield gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, gm.states(gm.KS_SEED, gm.KS_N)


def test_one_super_voxel_is_the_global_track():
    """block >= max(n): t_coll and end states bitwise those of vpt_grid_probe_host, steps the global track's"""
    coll = none = 0
    for rho, lo, hi, sigma_t, rays, tmax, st in _reduction_sets():
        tau0, tc0, so0 = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st)
        steps0 = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, return_steps=True)[3]
        assert (steps0[so0 != st] >= 1).all() and (steps0[so0 == st] == 0).all()
        for b in (max(rho.shape), max(rho.shape) + 3):
            tau, tc, so, steps = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, st, majorant_block=b, return_steps=True)
            assert (_bits(tau) == _bits(tau0)).all()
            assert (_bits(tc) == _bits(tc0)).all(), f"block {b}: {(_bits(tc) != _bits(tc0)).sum()} t_coll differ"
            assert (so == so0).all(), f"block {b}: {(so != so0).sum()} end states differ"
            assert (steps == steps0).all(), f"block {b}: {(steps != steps0).sum()} step counts differ"
        if len(rho.shape) == 3 and rho.shape == gm.TAU_SHAPE and sigma_t == 0.7:
            coll, none = int((tc0 >= 0).sum()), int((tc0 == -1).sum())
    assert coll > 200 and none > 200


def test_block_1_inverts_the_optical_depth(sparse):
    """block 1: the majorant is the voxel's density, so no collision is null: one draw per track, and the
    collision lies where sigma_t tau reaches -log(1 - xi).  The bound is the rounding argument of
    test_optical_depth_matches_the_numpy_model: at most nx + ny + nz + 1 pieces, each off by a few ulps."""
    rho, rays, tmax, st = sparse["rho"], sparse["rays"], sparse["tmax"], sparse["st"]
    tau_end, tc, so, steps = sparse[1]
    assert abs((rho == 0).mean() - 0.5) < 0.15 and rho[rho > 0].min() >= 0.2 and rho.max() <= 3.0
    stepped, xi = mm.erand48_steps(st)
    assert (so == stepped).all()  # every ray of the set crosses the box: exactly one draw
    assert (steps == 1).all()
    assert not np.isnan(tc).any()
    want = mm.free_depth(xi)
    hit = tc >= 0
    assert hit.sum() > 1000 and (~hit).sum() > 200
    tau_c = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays[hit], tc[hit], st[hit])[0]
    ratio = np.abs(SIGMA_T * tau_c - want[hit]) / want[hit]
    print(f"worst |sigma_t tau(t_coll) - (-log(1 - xi))| / (-log(1 - xi)) = {ratio.max():.3e} over {hit.sum()} collisions")
    assert (ratio <= REL).all(), f"{(ratio > REL).sum()} collisions off, worst {ratio.max():.3e}"
    assert (tc[hit] <= tmax[hit]).all()
    # none: the depth up to min(tmax, t1) (the probe's tau stops at the box) does not reach the free depth
    over = SIGMA_T * tau_end[~hit] - want[~hit]
    print(f"none: largest (sigma_t tau - free depth) / free depth = {(over / want[~hit]).max():.3e}")
    assert (over <= REL * want[~hit]).all()
    # a ray that misses the box: the start state, no step
    miss = np.zeros(3, dtype=gm.RAY_DTYPE)
    miss["o"] = [(10, 10, 10), (-5, 3, 0), (2, 3, 20)]
    miss["d"] = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    _, tcm, som, stm = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, miss, 1e30, st[:3], majorant_block=1,
                                       return_steps=True)
    assert (tcm == -1).all() and (som == st[:3]).all() and (stm == 0).all()


def _diagonal():
    """one oblique ray from outside the box through its whole diagonal, and its slab interval"""
    lo, hi = np.array(mm.SPARSE_LO), np.array(mm.SPARSE_HI)
    ext = hi - lo
    a = lo + ext * np.array([-0.05, 0.07, 0.03])
    b = lo + ext * np.array([1.02, 0.91, 0.96])
    d = (b - a) / np.linalg.norm(b - a)
    with np.errstate(divide="ignore"):
        ta, tb = (lo - a) / d, (hi - a) / d
    t0 = max(np.minimum(ta, tb).max(), 0.0)
    t1 = np.maximum(ta, tb).min()
    return a, d, t0, t1


def test_block_2_distribution():
    """65 536 tracks along one oblique ray at block 2: Kolmogorov distance to F(t) = 1 - exp(-sigma_t tau(t)) below
    the alpha = 0.001 critical value 1.95 / sqrt(N) of test_delta_tracking_distribution; the CDF of the
    homogeneous medium at the global majorant is rejected by the same statistic"""
    rho = mm.sparse_field()
    o, d, t0, t1 = _diagonal()
    sigma_t = 0.3
    rays = mm.same_ray(o, d, gm.KS_N)
    st = gm.states(gm.KS_SEED, gm.KS_N)
    _, tc, _, steps = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays, 1e30, st, majorant_block=2,
                                      return_steps=True)
    assert not np.isnan(tc).any() and ((tc == -1) | ((tc > t0) & (tc < t1))).all()
    assert (tc == -1).sum() > 500 and (tc >= 0).sum() > 50000
    assert steps.max() > 1  # null collisions exist at this block size
    crit = 1.95 / np.sqrt(gm.KS_N)

    def hetero(t):
        tau = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, sigma_t, rays[:len(t)], np.asarray(t, float), st[:len(t)])[0]
        return 1 - np.exp(-sigma_t * tau)

    def homogeneous(t):
        return 1 - np.exp(-sigma_t * float(rho.max()) * np.maximum(np.asarray(t, float) - t0, 0.0))

    d_het = gm.ks_statistic(tc, t1, hetero)
    d_hom = gm.ks_statistic(tc, t1, homogeneous)
    print(f"D_N = {d_het:.5f} (critical {crit:.5f}); against the homogeneous majorant CDF: {d_hom:.5f}")
    assert d_het < crit
    assert d_hom > crit


def test_fewer_steps_with_smaller_blocks(sparse):
    s0, s1, s2 = (int(sparse[b][3].sum()) for b in (0, 1, 2))
    print(f"tentative steps over {len(sparse['rays'])} tracks: block 0 {s0}, block 2 {s2}, block 1 {s1}")
    assert s2 < s0
    assert s2 >= s1


def test_empty_super_voxels_take_one_draw_and_no_more():
    """a field whose x < 2 slab (one column of 2^3 super-voxels) is empty, in the box [0, n]: rays inside the slab
    end as "none" after exactly one draw; a missed box takes none"""
    rho = mm.sparse_field().copy()
    rho[:, :, :2] = 0.0
    nz, ny, nx = rho.shape
    lo, hi = (0.0, 0.0, 0.0), (float(nx), float(ny), float(nz))
    n = 64
    rng = np.random.default_rng(3)
    rays = np.zeros(n, dtype=gm.RAY_DTYPE)
    rays["o"] = np.stack([rng.uniform(0.1, 1.9, n), np.full(n, -1.0), rng.uniform(0.1, nz - 0.1, n)], axis=1)
    rays["d"] = (0.0, 1.0, 0.0)
    rays["o"][n // 2:, 1] = ny + 1.0  # the other half runs down the slab
    rays["d"][n // 2:] = (0.0, -1.0, 0.0)
    st = gm.states(5, n)
    stepped, _ = mm.erand48_steps(st)
    for b in (1, 2):
        _, tc, so, steps = grid_probe_host(rho, lo, hi, SIGMA_T, rays, 1e30, st, majorant_block=b, return_steps=True)
        assert (tc == -1).all() and (so == stepped).all() and (steps == 1).all()
    miss = rays.copy()
    miss["o"][:, 0] = -3.0
    _, tc, so, steps = grid_probe_host(rho, lo, hi, SIGMA_T, miss, 1e30, st, majorant_block=2, return_steps=True)
    assert (tc == -1).all() and (so == st).all() and (steps == 0).all()
    # an all-zero field: rho_max == 0, no draw even inside the box
    _, tc, so, steps = grid_probe_host(np.zeros_like(rho), lo, hi, SIGMA_T, rays, 1e30, st, majorant_block=2, return_steps=True)
    assert (tc == -1).all() and (so == st).all() and (steps == 0).all()


def test_axis_parallel_rays_in_a_plane_between_super_voxels():
    """rays along y and z that lie exactly in the plane x = 2k between two super-voxels of block 2 (and along x
    in the planes y = 2k), box [0, n] so the planes are exact.  The field is constant on every 2^3 block, so the
    block's majorant is its density, no collision is null and the inversion property of block 1 must hold."""
    coarse = mm.sparse_field((2, 3, 4), seed=32)
    rho = mm.resample2(coarse)
    nz, ny, nx = rho.shape
    lo, hi = (0.0, 0.0, 0.0), (float(nx), float(ny), float(nz))
    rays = []
    for k in range(0, nx + 1, 2):  # x = 0 and x = nx included: the box faces (lo <= o < hi decides)
        for z in (0.5, 1.0, 2.0, 3.5):
            rays.append(((float(k), -1.0, z), (0.0, 1.0, 0.0)))
            rays.append(((float(k), ny + 1.0, z), (0.0, -1.0, 0.0)))
        for y in (0.5, 2.0, 4.0, 5.5):
            rays.append(((float(k), y, -0.5), (0.0, 0.0, 1.0)))
            rays.append(((float(k), y, nz + 0.5), (0.0, 0.0, -1.0)))
    for k in range(0, ny + 1, 2):
        for z in (0.5, 2.0):
            rays.append(((-1.0, float(k), z), (1.0, 0.0, 0.0)))
            rays.append(((nx + 1.0, float(k), z), (-1.0, 0.0, 0.0)))
    r = np.zeros(len(rays), dtype=gm.RAY_DTYPE)
    r["o"] = [a for a, _ in rays]
    r["d"] = [b for _, b in rays]
    reps = 16  # every ray with 16 states
    r = np.repeat(r, reps)
    st = gm.states(7, len(r))
    stepped, xi = mm.erand48_steps(st)
    want = mm.free_depth(xi)
    tau_all = grid_probe_host(rho, lo, hi, SIGMA_T, r, 1e30, st)[0]
    inside = ((r["o"] >= np.array(lo)) & (r["o"] < np.array(hi)) | (r["d"] != 0)).all(axis=1)  # the slab test's rule
    assert inside.sum() > 200 and (~inside).sum() >= reps and (tau_all[~inside] == 0).all()
    for b in (2, 1):
        _, tc, so, steps = grid_probe_host(rho, lo, hi, SIGMA_T, r, 1e30, st, majorant_block=b, return_steps=True)
        assert (so[inside] == stepped[inside]).all() and (steps[inside] == 1).all()
        assert (so[~inside] == st[~inside]).all() and (tc[~inside] == -1).all()
        hit = tc >= 0
        assert hit.sum() > 100
        tau_c = grid_probe_host(rho, lo, hi, SIGMA_T, r[hit], tc[hit], st[hit])[0]
        ratio = np.abs(SIGMA_T * tau_c - want[hit]) / want[hit]
        print(f"block {b}: worst relative depth error {ratio.max():.3e} over {hit.sum()} collisions")
        assert (ratio <= REL).all()
        none = inside & ~hit
        assert (SIGMA_T * tau_all[none] - want[none] <= REL * want[none]).all()


@pytest.mark.parametrize("block", [2, 4])
def test_partial_last_block_equals_the_resampled_field(block):
    """7 x 5 x 3 voxels (no dimension a multiple of the block) against the same field resampled 2 x with the block
    doubled: the super-voxels cover the same voxels of the same box, so end states are equal and t_coll agrees to
    rounding"""
    rho = mm.sparse_field((3, 5, 7), seed=33)
    rays, tmax = mm.box_rays(mm.SPARSE_LO, mm.SPARSE_HI, n=2048, seed=19)
    st = gm.states(13, len(rays))
    _, tca, soa, sta = grid_probe_host(rho, mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st, majorant_block=block,
                                       return_steps=True)
    _, tcb, sob, stb = grid_probe_host(mm.resample2(rho), mm.SPARSE_LO, mm.SPARSE_HI, SIGMA_T, rays, tmax, st,
                                       majorant_block=2 * block, return_steps=True)
    assert (soa == sob).all() and (sta == stb).all()
    assert ((tca >= 0) == (tcb >= 0)).all() and (tca >= 0).sum() > 500 and (tca == -1).sum() > 100
    hit = tca >= 0
    rel = np.abs(tca[hit] - tcb[hit]) / tca[hit]
    print(f"block {block}: worst relative |t_coll - resampled| = {rel.max():.3e}")
    assert (rel <= REL).all()
    assert sta.max() > 1  # null collisions: the blocks are not uniform


def test_negative_block_is_invalid():
    rays, tmax = gm.ks_rays(1)
    with pytest.raises(VPTError) as ei:
        grid_probe_host(gm.KS_RHO, gm.KS_LO, gm.KS_HI, 1.0, rays, tmax, gm.states(1, 1), majorant_block=-1)
    assert ei.value.code == _lib.VPT_E_INVALID
