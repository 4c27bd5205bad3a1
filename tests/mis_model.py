"""A plain-Python restatement of one distance decision of estimator 13 (csrc/vpt_grid_mis.h: vpt_grid_mis_one), for
tests/test_grid_mis.py.  It builds on eqa_model.py (the interval, the geometry, the lookup): the two draws, the coin
that picks the strategy, the rescaled surface coin, the equi-angular distance or the track's, pe at a tracked distance
from s = dist - proj, and pdf = q * (sigma_t * rho_t * T) + (1 - q) * pe -- one IEEE double operation per Python operation,
in the header's order, with math.sqrt / atan2 / tan.  The optical depths and the delta tracks come from grid_probe_host
(the walkers, which tests/test_grid_host.py, test_grid_majorant.py and test_grid_trilinear.py pin against models of their
own); a track starts from the state after the two draws."""
import math

import numpy as np

import eqa_model as em
import grid_model as gm
from minimal_volumetric_path_tracer_amd import grid_probe_host

NAMES = ("psurf", "strategy", "dist", "pdf", "pe", "T", "rho_t", "steps")


def mis_rays(rho, lo, hi, sigma_t, q, rays, tmax, light, states, interpolation="nearest", majorant_block=0):
    """the model over arrays, in grid_mis_probe_host's order: (psurf, strategy, dist, pdf, pe, T, rho_t, steps, end
    states)"""
    n = len(rays)
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    q = float(q)
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, float), (n,)))
    light = np.broadcast_to(np.asarray(light, float), (n, 3))
    tau_s = grid_probe_host(rho, lo, hi, sigma_t, rays, tmax, states, interpolation=interpolation)[0]
    psurf = np.array([math.exp(sigma_t * float(v) * -1.0) for v in tau_s])
    xs, cs = np.zeros(n), np.zeros(n)
    so = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        x1, xs[i] = gm.erand48_step(states[i])
        so[i], cs[i] = gm.erand48_step(x1)
    strategy = (cs < q).astype(np.int32)
    steps = np.zeros(n, dtype=np.uint32)
    tc = np.zeros(n)
    trk = np.nonzero(strategy == 1)[0]
    if len(trk):  # the tracks, from the state after the coin
        _, tc[trk], so[trk], steps[trk] = grid_probe_host(rho, lo, hi, sigma_t, rays[trk], tmax[trk], so[trk],
                                                          majorant_block=majorant_block, return_steps=True,
                                                          interpolation=interpolation)
    dist, pdf, pe, T, rho_t = np.full(n, -1.0), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    med = []
    for i in range(n):
        o, d = [float(v) for v in rays["o"][i]], [float(v) for v in rays["d"][i]]
        a, b = em.interval(lo, hi, o, d, float(tmax[i]))
        lp = [float(v) for v in light[i]]
        ps = float(psurf[i])
        if strategy[i]:
            if tc[i] != tc[i]:  # the step cap
                dist[i] = tc[i]
                continue
            if tc[i] < 0:
                continue
            dist[i] = tc[i]
            D, proj = em.geometry(o, d, lp)
            ta = math.atan2(a - proj, D)
            tb = math.atan2(b - proj, D)
            s = float(dist[i]) - proj
            pe[i] = D / math.fabs(tb - ta) / (s * s + D * D) * (1 - ps)
        else:
            cc = (float(cs[i]) - q) / (1 - q)
            if cc < ps:
                continue
            D, proj = em.geometry(o, d, lp)
            ta = math.atan2(a - proj, D)
            tb = math.atan2(b - proj, D)
            x = float(xs[i])
            s = D * math.tan((1 - x) * ta + x * tb)
            dist[i] = s + proj
            pe[i] = D / math.fabs(tb - ta) / (s * s + D * D) * (1 - ps)
        ds = float(dist[i])
        rho_t[i] = em.lookup(rho, lo, hi, interpolation, [o[k] + d[k] * ds for k in range(3)])
        med.append(i)
    if med:
        med = np.array(med)
        go = med[rho_t[med] != 0.0]  # T over [0, dist] for the rays that go on; +0 where the path ends
        if len(go):
            tau_d = grid_probe_host(rho, lo, hi, sigma_t, rays[go], dist[go], states[go], interpolation=interpolation)[0]
            T[go] = [math.exp(sigma_t * float(v) * -1.0) for v in tau_d]
        for i in med:
            pff = sigma_t * float(rho_t[i]) * float(T[i])
            pdf[i] = q * pff + (1 - q) * float(pe[i])
    return psurf, strategy, dist, pdf, pe, T, rho_t, steps, so
