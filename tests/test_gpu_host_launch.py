"""The host side of the per-ray entry points and of the density-grid launches (csrc/vpt_kernels.hip's staging helper and
unit selector, csrc/vpt_hetero_launch.h): what a copy of the wrong length, a wrong grid size, a mishandled optional
output or a wrong slot of a unit's table would change.  One 8^3 grid with majorant block 2 in the default scene;
257 rays: one full workgroup and one lane.  And the branches of the kernels' LDS prologue (csrc/vpt_hetero_lds.h), on
grids at and around the 16 384-float budget."""
import ctypes

import numpy as np
import pytest

import test_gpu_hetero as T
from conftest import bitwise_equal
from minimal_volumetric_path_tracer_amd import (RenderConfig, Tracer, _lib, grid_emission_probe_host, grid_eqa_probe_host,
                                                grid_probe_host, grid_ratio_probe_host)
from scenes import default_scene
from test_gpu_ratio import _camera_batch

pytestmark = pytest.mark.gpu

N = 257
LO, HI = T.ROOM_LO, T.ROOM_HI
BLOCK = 2
SIGMA_T = 0.03
LIGHT = (1.5, 3.1, 1.5)
RHO = np.random.default_rng(41).uniform(0.0, 1.0, (8, 8, 8)).astype(np.float32)
RHO[RHO < 0.3] = 0.0  # empty voxels: the majorant blocks differ
EPS = np.random.default_rng(42).uniform(0.0, 2.0, (8, 8, 8)).astype(np.float32)
RGB = (0.9, 0.5, 0.2)
RAYS, STATES = _camera_batch(17, 1, 7)  # 289 camera rays through the box
RAYS, STATES = np.ascontiguousarray(RAYS[:N]), np.ascontiguousarray(STATES[:N])
TMAX = np.linspace(40.0, 400.0, N)  # some rays end inside the box


@pytest.fixture(scope="module")
def lt():
    """a tracer of this module's own, with the grid, its majorant grid and an emission grid"""
    t = Tracer(0, default_scene())
    t.set_density_grid(RHO, LO, HI, majorant_block=BLOCK, emission=EPS, emission_rgb=RGB)
    yield t
    t.close()


def _out(n, dtype=np.float64, k=1):
    """an output of n rows and one row more, every byte 0xA5: the row behind the end must stay as it is"""
    a = np.empty((n + 1, k), dtype=dtype)
    a.view(np.uint8)[...] = 0xA5
    return a


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _x3(n):
    return np.ascontiguousarray(RAYS["o"][:n] + 30.0 * RAYS["d"][:n])


# every call: (tracer, n, with the optional outputs) -> (status, {name: output array of n + 1 rows})
def _grid_probe(t, n, opt):
    o = {"tau": _out(n), "t_coll": _out(n), "states": _out(n, np.uint64)}
    return _lib.lib().vpt_grid_probe(t._ctx, SIGMA_T, _ptr(RAYS), _ptr(TMAX), _ptr(STATES), n, *map(_ptr, o.values())), o


def _grid_probe_lm(t, n, opt):
    o = {"tau": _out(n), "t_coll": _out(n), "states": _out(n, np.uint64)}
    steps = _out(n, np.uint32) if opt else None
    rc = _lib.lib().vpt_grid_probe_lm(t._ctx, SIGMA_T, _ptr(RAYS), _ptr(TMAX), _ptr(STATES), n, *map(_ptr, o.values()), _ptr(steps))
    return rc, dict(o, **({"steps": steps} if opt else {}))


def _grid_ratio_probe(t, n, opt):
    o = {"that": _out(n), "states": _out(n, np.uint64)}
    steps = _out(n, np.uint32) if opt else None
    rc = _lib.lib().vpt_grid_ratio_probe(t._ctx, SIGMA_T, _ptr(RAYS), _ptr(TMAX), _ptr(STATES), n, *map(_ptr, o.values()), _ptr(steps))
    return rc, dict(o, **({"steps": steps} if opt else {}))


def _grid_eqa_probe(t, n, opt):
    light = np.ascontiguousarray(np.broadcast_to(np.asarray(LIGHT), (N, 3)))
    o = {k: _out(n) for k in ("psurf", "dist", "pdf", "T", "rho_t")}
    o["states"] = _out(n, np.uint64)
    return _lib.lib().vpt_grid_eqa_probe(t._ctx, SIGMA_T, _ptr(RAYS), _ptr(TMAX), _ptr(light), _ptr(STATES), n,
                                         *map(_ptr, o.values())), o


def _grid_emission_probe(t, n, opt):
    o = {"t_coll": _out(n), "esum": _out(n), "states": _out(n, np.uint64)}
    steps = _out(n, np.uint32) if opt else None
    rc = _lib.lib().vpt_grid_emission_probe(t._ctx, SIGMA_T, _ptr(RAYS), _ptr(TMAX), _ptr(STATES), n, *map(_ptr, o.values()),
                                            _ptr(steps))
    return rc, dict(o, **({"steps": steps} if opt else {}))


def _trace_batch(t, n, opt, est="ff"):
    m = RenderConfig(estimator=est, sigma_a=T.SA, sigma_s=T.SS).medium()
    rgb, states = _out(n, k=3), _out(n, np.uint64) if opt else None
    rc = _lib.lib().vpt_trace_batch(t._ctx, ctypes.byref(m), _ptr(RAYS), _ptr(STATES), n, _ptr(rgb), _ptr(states))
    return rc, dict({"rgb": rgb}, **({"states": states} if opt else {}))


def _punctual_volumetric(t, n, opt):
    rgb = _out(n, k=3)
    return _lib.lib().vpt_punctual_volumetric(t._ctx, 7, _ptr(_x3(N)), n, 0.07, 0.0135, 0.0125, _ptr(rgb)), {"rgb": rgb}


def _ray_marching_batch(t, n, opt):
    rgb, states = _out(n, k=3), _out(n, np.uint64) if opt else None
    x_new, ids = _out(n, k=3), _out(n, np.int32)
    x_new[:] = 0.25  # in and out
    ids[:] = -1
    rc = _lib.lib().vpt_ray_marching_batch(t._ctx, 0.0135, 0.0125, 16.0, _ptr(RAYS), _ptr(STATES), n, _ptr(rgb), _ptr(x_new),
                                           _ptr(ids), _ptr(states))
    o = {"rgb": rgb, "x_new": x_new[:n], "idsource": ids[:n]}  # the inputs have no row behind the end to keep
    return rc, dict(o, **({"states": states} if opt else {}))


def _math_probe(t, n, opt):
    x, out = np.linspace(-3.0, 3.0, N), _out(n)
    return _lib.lib().vpt_math_probe(t._ctx, 1, _ptr(x), _ptr(x), _ptr(out), n), {"exp": out}


def _phase_probe(t, n, opt):
    """n states and n - 1 directions (none at n == 0), so that the two counts differ"""
    nw = max(n - 1, 0)
    din = np.array([0.0, 0.6, -0.8])
    wl = np.ascontiguousarray(RAYS["d"])
    o = {"dirs": _out(n, k=3), "states": _out(n, np.uint64), "values": _out(nw)}
    rc = _lib.lib().vpt_phase_probe(t._ctx, 0.4, _ptr(din), _ptr(STATES), n, _ptr(o["dirs"]), _ptr(o["states"]), _ptr(wl), nw,
                                    _ptr(o["values"]))
    return rc, o


CALLS = {f.__name__[1:]: f for f in (_grid_probe, _grid_probe_lm, _grid_ratio_probe, _grid_eqa_probe, _grid_emission_probe,
                                     _trace_batch, _punctual_volumetric, _ray_marching_batch, _math_probe, _phase_probe)}
OPTIONAL = {"grid_probe_lm": "steps", "grid_ratio_probe": "steps", "grid_emission_probe": "steps", "trace_batch": "states",
            "ray_marching_batch": "states"}


def _host(name):
    """the grid probes on the host, in the order of the call's outputs"""
    if name == "grid_probe":
        return grid_probe_host(RHO, LO, HI, SIGMA_T, RAYS, TMAX, STATES)
    if name == "grid_probe_lm":
        return grid_probe_host(RHO, LO, HI, SIGMA_T, RAYS, TMAX, STATES, majorant_block=BLOCK, return_steps=True)
    if name == "grid_ratio_probe":
        return grid_ratio_probe_host(RHO, LO, HI, SIGMA_T, RAYS, TMAX, STATES, majorant_block=BLOCK)
    if name == "grid_eqa_probe":
        return grid_eqa_probe_host(RHO, LO, HI, SIGMA_T, RAYS, TMAX, LIGHT, STATES)
    if name == "grid_emission_probe":
        return grid_emission_probe_host(RHO, EPS, LO, HI, SIGMA_T, RAYS, TMAX, STATES, majorant_block=BLOCK)
    return None


def _rows(a, n):
    return a[:n].tobytes()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_staging(lt, name):
    """(a) n == 0 is VPT_OK and writes nothing; (b) 257 rays give on their first 256 the bits of a 256-ray call, leave
    the row behind the end alone and, for the grid probes, equal the host build; (c) without the optional outputs the
    other outputs keep their bits"""
    call = CALLS[name]
    rc, o = call(lt, 0, True)
    assert rc == _lib.VPT_OK, _lib.lib().vpt_last_error()
    assert all((a.view(np.uint8) == 0xA5).all() for a in o.values())
    rc, full = call(lt, N, True)
    assert rc == _lib.VPT_OK, _lib.lib().vpt_last_error()
    rc, part = call(lt, N - 1, True)
    assert rc == _lib.VPT_OK, _lib.lib().vpt_last_error()
    for k in full:
        n_k = N - 1 if (name, k) == ("phase_probe", "values") else N  # that call's second count
        assert _rows(full[k], n_k - 1) == _rows(part[k], n_k - 1), k
        assert _rows(full[k], n_k) != _rows(_out(n_k, full[k].dtype, full[k].shape[1]), n_k), k  # written
        if len(full[k]) > n_k:
            assert (full[k][n_k:].view(np.uint8) == 0xA5).all(), f"{k}: written behind the end"
    host = _host(name)
    if host is not None:
        assert len(host) == len(full)
        for (k, g), w in zip(full.items(), host):
            assert bitwise_equal(g[:N, 0], w).all(), f"{k}: {(~bitwise_equal(g[:N, 0], w)).sum()} differ from the host build"
    if name in OPTIONAL:
        rc, bare = call(lt, N, False)
        assert rc == _lib.VPT_OK, _lib.lib().vpt_last_error()
        assert set(bare) == set(full) - {OPTIONAL[name]}
        for k in bare:
            assert _rows(bare[k], N) == _rows(full[k], N), k


W, H, SPP, SEED = 8, 8, 2, 5
SETTINGS = [(ip, em) for ip in ("nearest", "trilinear") for em in (False, True)]


def _cfg(est):
    return RenderConfig(width=W, height=H, spp=SPP, estimator=est, sigma_a=T.SA, sigma_s=T.SS, seed=SEED, fp64=True)


NO_EMISSION = ("hetero_equiangular", "hetero_mis", "hetero_chromatic")  # estimators that take no emission grid
MIS_FRACTION = 0.3  # strictly between 0 (estimator 12's draws) and 1
COLOUR = ((1.0, 0.7, 0.4), (0.9, 1.0, 0.6))  # absorption, scattering: no two channels alike


@pytest.mark.parametrize("est", ["hetero", "hetero_ratio", "hetero_equiangular", "hetero_mis", "hetero_chromatic"])
def test_every_setting_reaches_its_unit(lt, orc_vm, monkeypatch, est):
    """Each (interpolation, emission) setting of one context -- estimators 12 to 14 take no emission grid: the
    interpolation alone -- through the persistent-wave render, render_kernel_simple (VPT_SIMPLE_KERNEL=1) and the in-order
    sum of the per-sample call: the three are one image bit for bit, and no two settings give the same image.  Estimator
    13 runs with a track fraction of its own and estimator 14 with unequal channels, so that a launch that dropped either
    would show"""
    rays, st = T._camera_samples(orc_vm, W, H, SPP, SEED)
    m = _cfg(est).medium()
    imgs = {}
    try:
        lt.set_hetero_mis_fraction(MIS_FRACTION)
        lt.set_medium_colour(*COLOUR)
        for ip, em in SETTINGS if est not in NO_EMISSION else [(ip, False) for ip in ("nearest", "trilinear")]:
            lt.set_grid_interpolation(ip)
            if em:
                lt.set_emission_grid(EPS, RGB)
            else:
                lt.clear_emission_grid()
            img = imgs[ip, em] = lt.render(_cfg(est))
            with monkeypatch.context() as mp:
                mp.setenv("VPT_SIMPLE_KERNEL", "1")
                simple = lt.render(_cfg(est))
            assert bitwise_equal(img, simple).all(), f"{ip}, emission {em}: {(~bitwise_equal(img, simple)).sum()} differ"
            L, _ = lt.trace(est, rays.reshape(-1), st.reshape(-1), m.sigma_a, m.sigma_s)
            L = L.reshape(H, W, SPP, 3)
            acc = np.zeros((H, W, 3))
            for s in range(SPP):
                acc = L[:, :, s] + acc
            assert bitwise_equal(img, acc * (1 / float(SPP))).all(), f"{ip}, emission {em}: the sample sum differs"
        keys = list(imgs)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not bitwise_equal(imgs[a], imgs[b]).all(), f"{a} and {b} give one image"
    finally:
        lt.set_grid_interpolation("nearest")
        lt.set_emission_grid(EPS, RGB)
        lt.set_hetero_mis_fraction(0.5)
        lt.set_medium_colour()


# ---- the LDS prologue's branches (csrc/vpt_hetero_lds.h) ----
CAP = 16384  # the budget in floats
# (shape [nz, ny, nx], majorant block): every branch of the prologue by its condition on nv and nbv
LDS_GRIDS = {
    "both_staged": ((15, 32, 32), 4),       # nv < cap, nbv = 256 <= cap - nv = 1024: majorants behind the density
    "maj_global": ((15, 32, 32), 2),        # nv < cap, nbv = 2048 > cap - nv: density staged, majorants global
    "nv_is_cap": ((16, 32, 32), 2),         # nv == cap: the <= boundary, nothing left for majorants
    "maj_at_zero": ((17, 32, 32), 2),       # nv > cap, nbv = 2304 <= cap: density global, majorants staged at 0
    "nothing_staged": ((17, 32, 32), 1),    # nv > cap, nbv = nv > cap
    "no_majorants": ((17, 32, 32), 0),      # nv > cap, LM = false: density global
}
LDS_ESTIMATORS = ["hetero", "hetero_ratio", "hetero_equiangular", "hetero_mis", "hetero_chromatic"]
EQA_GRIDS = ("both_staged", "nv_is_cap", "no_majorants")  # estimator 12 ignores the majorants: one grid per nv case


def _nbv(shape, block):
    return int(np.prod([-(-n // block) for n in shape])) if block else 0


def test_lds_grids_meet_their_conditions():
    """the grids above are what their names say (no GPU work, but it belongs with them)"""
    nv = {k: int(np.prod(sh)) for k, (sh, _) in LDS_GRIDS.items()}
    nbv = {k: _nbv(sh, b) for k, (sh, b) in LDS_GRIDS.items()}
    assert nv["both_staged"] < CAP and 0 < nbv["both_staged"] <= CAP - nv["both_staged"]
    assert nv["maj_global"] < CAP and nbv["maj_global"] > CAP - nv["maj_global"]
    assert nv["nv_is_cap"] == CAP and nbv["nv_is_cap"] > 0
    assert nv["maj_at_zero"] > CAP and 0 < nbv["maj_at_zero"] <= CAP
    assert nv["nothing_staged"] > CAP and nbv["nothing_staged"] > CAP
    assert nv["no_majorants"] > CAP and nbv["no_majorants"] == 0
    assert {nv[k] for k in EQA_GRIDS} == set(nv.values())


def _sparse_field(shape, seed):
    rho = np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(np.float32)
    rho[rho < 0.3] = 0.0  # empty voxels: the majorant blocks differ
    return rho


@pytest.fixture(scope="module")
def pt():
    """a tracer of the prologue tests' own: they replace the grid"""
    t = Tracer(0, default_scene())
    t.set_hetero_mis_fraction(MIS_FRACTION)
    t.set_medium_colour(*COLOUR)
    yield t
    t.close()


def _lds_cases():
    for k in LDS_GRIDS:
        for est in LDS_ESTIMATORS:
            if est != "hetero_equiangular" or k in EQA_GRIDS:
                yield pytest.param(k, est, "nearest", id=f"{k}-{est}")
    for est in LDS_ESTIMATORS:
        yield pytest.param("both_staged", est, "trilinear", id=f"both_staged-{est}-trilinear")


@pytest.mark.parametrize("grid,est,ip", list(_lds_cases()))
def test_lds_prologue_branches(pt, monkeypatch, grid, est, ip):
    """The persistent-wave render, whose prologue stages the density and the majorants in LDS or leaves either in global
    memory, equals render_kernel_simple's (VPT_SIMPLE_KERNEL=1), which reads global memory only, bit for bit -- on a grid
    for every branch of the prologue"""
    shape, block = LDS_GRIDS[grid]
    try:
        pt.set_density_grid(_sparse_field(shape, 43), LO, HI, majorant_block=block, interpolation=ip)
        img = pt.render(_cfg(est))
        with monkeypatch.context() as mp:
            mp.setenv("VPT_SIMPLE_KERNEL", "1")
            simple = pt.render(_cfg(est))
        assert np.isfinite(img).all() and (img > 0).any()
        assert bitwise_equal(img, simple).all(), f"{(~bitwise_equal(img, simple)).sum()} differ"
    finally:
        pt.set_majorant_block(0)
        pt.set_grid_interpolation("nearest")
        pt.clear_density_grid()
