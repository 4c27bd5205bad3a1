"""A plain-Python restatement of the two walkers of estimator 16 (csrc/vpt_grid_spectral.h: chromatic ratio tracking and
the spectral delta track, under the global and under local majorants) for tests/test_grid_spectral.py: the launch
constants sb, f and alb, the slab test, the free-path step under sb (or the DDA over the super-voxels with the eager
draw rem = -log(1 - xi)), the lookup at a tentative point (eqa_model.lookup: the voxel, or the nested lerps), the three
products of the ratio walk and the track's decision r, n, h, a_r, a_n, c with its one draw -- one IEEE double operation
per Python operation, in the order the header comment writes down.  Nothing of the library is called: the grey branch of
the track is restated too (estimator 10's decision xi' * mu < rho)."""
import math

import numpy as np

import majorant_model as mm
from eqa_model import lookup
from ratio_model import BIG, MAX_STEPS, _axis_index, _slab
from residual_model import _next_axis, _plane, counts, majorants

NAMES = ("t_coll", "w", "steps", "states", "T", "ratio_steps", "ratio_states")


def consts(ss, st):
    """(sb, f, alb, grey): vpt_grid_spectral_consts"""
    sb = st[0] if st[0] > st[1] else st[1]
    sb = sb if sb > st[2] else st[2]
    return sb, [st[k] / sb for k in range(3)], [ss[k] / st[k] for k in range(3)], st[0] == st[1] and st[1] == st[2]


class _Walk:
    """the tentative points of the walk under sb, vpt_grid_track_m's / vpt_grid_track_lm_m's: next() returns (t, mu) of a
    point that passed the boundary test, or None where the walker returns "none"; x is the stream state, steps the draws
    of free paths"""

    def __init__(self, rho, maj, lo, hi, block, o, d, tmax, sb, state):
        nz, ny, nx = rho.shape
        self.n = (nx, ny, nz)
        self.lo, self.hi = [float(v) for v in lo], [float(v) for v in hi]
        self.o, self.d = [float(v) for v in o], [float(v) for v in d]
        self.tmax, self.sb, self.block, self.maj = float(tmax), sb, block, maj
        self.x = int(state) & 0xFFFFFFFFFFFF
        self.steps = 0
        self.rho_max = float(np.float32(rho.max()))
        self.dead = not self.rho_max > 0.0
        if self.dead:
            return
        iv = _slab(self.lo, self.hi, self.o, self.d)
        if iv is None:
            self.dead = True
            return
        self.t, self.t1 = iv
        if block:
            n, lo, hi, o, d = self.n, self.lo, self.hi, self.o, self.d
            self.nb = counts(rho.shape, block)
            inv_cell = [float(n[a]) / (hi[a] - lo[a]) for a in range(3)]
            self.cell = [(hi[a] - lo[a]) / float(n[a]) for a in range(3)]
            self.i, self.step, self.tn, self.inv = [0] * 3, [0] * 3, [0.0] * 3, [0.0] * 3
            for a in range(3):
                self.i[a] = _axis_index(n[a], lo[a], inv_cell[a], o[a] + d[a] * self.t) // block
                self.step[a] = 1 if d[a] > 0.0 else (-1 if d[a] < 0.0 else 0)
                self.inv[a] = 1.0 / d[a] if self.step[a] else 0.0
                self.tn[a] = (self._pl(a) - o[a]) * self.inv[a] if self.step[a] else BIG
            self.a = _next_axis(self.tn)
            self.te = self.tn[self.a]
            self.mu = self._maj() if self.te > self.t else 0.0

    def _pl(self, a):
        return _plane(self.lo, self.hi, self.cell, self.nb, self.block, a, self.i[a] + (self.step[a] > 0))

    def _maj(self):
        return float(self.maj[self.i[2], self.i[1], self.i[0]])

    def draw(self):
        xs, xi = mm.erand48_steps(np.array([self.x], dtype=np.uint64))
        self.x = int(xs[0])
        return float(xi[0])

    def point(self, t):
        return [self.o[q] + self.d[q] * t for q in range(3)]

    def next(self):
        if self.dead:
            return None
        self.steps += 1
        if not self.block:
            self.t = self.t + (-math.log(1 - self.draw()) / (self.rho_max * self.sb))
            if self.t > self.tmax or self.t >= self.t1 or self.t != self.t:
                self.dead = True
                return None
            return self.t, self.rho_max
        rem = -math.log(1 - self.draw())
        tc, found = 0.0, False
        for _ in range(self.nb[0] + self.nb[1] + self.nb[2] + 4):
            if self.te > self.t:
                if self.mu > 0.0:
                    s = self.mu * self.sb
                    tc = self.t + (rem / s)
                    if tc < self.te:
                        found = True
                        break
                    rem = rem - s * (self.te - self.t)
                self.t = self.te
            a = self.a
            if not (self.te < self.t1) or self.te > self.tmax:
                break
            self.i[a] += self.step[a]
            if self.i[a] < 0 or self.i[a] >= self.nb[a]:
                break
            self.tn[a] = (self._pl(a) - self.o[a]) * self.inv[a]
            self.a = _next_axis(self.tn)
            self.te = self.tn[self.a]
            self.mu = self._maj() if self.te > self.t else 0.0
        if not found or tc > self.tmax or tc >= self.t1:
            self.dead = True
            return None
        self.t = tc
        return tc, self.mu


def ratio(rho, maj, lo, hi, block, interpolation, sb, f, o, d, tmax, state):
    """chromatic ratio tracking, one ray: (T[3], end state, draws)"""
    w = _Walk(rho, maj, lo, hi, block, o, d, tmax, sb, state)
    T = [1.0, 1.0, 1.0]
    for _ in range(MAX_STEPS):
        p = w.next()
        if p is None:
            return T, w.x, w.steps
        t, mu = p
        r = lookup(rho, w.lo, w.hi, interpolation, w.point(t))
        if r >= mu:
            T = [T[k] * (1.0 - f[k]) for k in range(3)]
            if T[0] == 0.0 and T[1] == 0.0 and T[2] == 0.0:
                return T, w.x, w.steps
        else:
            q = r / mu
            T = [T[k] * (1.0 - f[k] * q) for k in range(3)]
    return [math.nan] * 3, w.x, w.steps


def collide(f, beta, r, mu, W, w):
    """vpt_grid_spectral_collide: True for a real collision; W is updated in place, the draw comes from the walk w"""
    q = 1.0 if r >= mu else r / mu
    rr = [f[k] * q for k in range(3)]
    nn = [1.0 - rr[k] for k in range(3)]
    h = [abs(beta[k]) * W[k] for k in range(3)]
    hs = (h[0] + h[1]) + h[2]
    if not hs > 0.0 or not hs <= BIG:
        h = [1.0, 1.0, 1.0]
    a_r = (h[0] * rr[0] + h[1] * rr[1]) + h[2] * rr[2]
    a_n = (h[0] * nn[0] + h[1] * nn[1]) + h[2] * nn[2]
    c = a_r + a_n
    real = True
    if not a_n == 0.0:
        real = w.draw() * c < a_r
    if real:
        g = c / a_r
        W[:] = [W[k] * (rr[k] * g) for k in range(3)]
        return True
    g = c / a_n
    W[:] = [W[k] * (nn[k] * g) for k in range(3)]
    return False


def track(rho, maj, lo, hi, block, interpolation, sb, f, grey, beta, o, d, tmax, state):
    """the spectral delta track, one ray: (t_coll, W[3], end state, steps); grey: estimator 10's track, W = 1.0"""
    w = _Walk(rho, maj, lo, hi, block, o, d, tmax, sb, state)
    W = [1.0, 1.0, 1.0]
    for _ in range(MAX_STEPS):
        p = w.next()
        if p is None:
            return -1.0, W, w.x, w.steps
        t, mu = p
        r = lookup(rho, w.lo, w.hi, interpolation, w.point(t))
        if grey:
            if r >= mu or w.draw() * mu < r:
                return t, W, w.x, w.steps
        elif collide(f, beta, r, mu, W, w):
            return t, W, w.x, w.steps
    return math.nan, W, w.x, w.steps


def spectral_rays(rho, lo, hi, sa, ss, rays, tmax, states, interpolation="nearest", majorant_block=0, beta=None):
    """the model over arrays, in grid_spectral_probe_host's order: (t_coll, w (3, n), steps, end states, T (3, n), the ratio
    walk's draws, its end states)"""
    n = len(rays)
    rho = np.asarray(rho, np.float32)
    st = [float(a) + float(s) for a, s in zip(sa, ss)]
    ss = [float(s) for s in ss]
    sb, f, alb, grey = consts(ss, st)
    maj = majorants(rho, majorant_block, interpolation) if majorant_block else None
    tmax = np.broadcast_to(np.asarray(tmax, float), (n,))
    bt = np.broadcast_to(np.ones(3) if beta is None else np.asarray(beta, float), (n, 3))
    tc, w, steps, so = np.zeros(n), np.zeros((3, n)), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    T, rsteps, rso = np.zeros((3, n)), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    for i in range(n):
        o, d = rays["o"][i], rays["d"][i]
        t, W, so[i], steps[i] = track(rho, maj, lo, hi, majorant_block, interpolation, sb, f, grey, [float(v) for v in bt[i]],
                                      o, d, tmax[i], states[i])
        tc[i] = t
        if t != t:
            w[:, i] = 0.0
        elif t >= 0:
            w[:, i] = [W[k] * alb[k] for k in range(3)]
        else:
            w[:, i] = W
        T[:, i], rso[i], rsteps[i] = ratio(rho, maj, lo, hi, majorant_block, interpolation, sb, f, o, d, tmax[i], states[i])
    return tc, w, steps, so, T, rsteps, rso
