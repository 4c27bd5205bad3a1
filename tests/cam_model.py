"""A render from a camera origin other than main()'s, stated with the oracle's own pieces (oracle/vpt_oracle.c):
the oracle's render entry points fix the origin of src/rt.cpp:755, but the jittered direction of a camera ray does
not depend on the origin (orc_camera_ray), and orc_trace takes any ray.  Per sample: the stream's start state
(orc_stream_state_c), the jitter pair and the direction (orc_camera_ray), the estimator on (origin, direction) from
the state after the jitter (orc_trace).  The per-pixel sums are the chunked sums of orc_render_layout, in numpy
float64 (acc = L + acc inside a chunk, tot = acc + tot over chunks, times 1 / (double)spp)."""
import ctypes
from ctypes import byref

import numpy as np

from oracle.oracle import Counters, Medium, default_chunk


def chunk_starts(orc, spp, chunk=0):
    """sample ranges of a pixel's chunks: the GPU's auto layout (chunk 0) or uniform chunks"""
    taper = 0
    if chunk == 0:
        chunk, taper = default_chunk(spp), 1
    buf = (ctypes.c_int * (spp + 2))()
    n = orc.L.orc_chunk_layout(ctypes.c_int(spp), ctypes.c_int(chunk), ctypes.c_int(taper), buf, ctypes.c_int(spp + 2))
    assert n > 0
    return list(buf[: n + 1])


def sample_radiance(orc, w, h, n, origin, est, seed=0x5EED0001, sigma_a=0.001, sigma_s=0.009, hg_g=0.0, max_depth=0):
    """L[file row, x, sample, 3] of samples 0..n-1 of every pixel, and the summed (tests, iterations) counters"""
    m = Medium(sigma_a, sigma_s, hg_g, max_depth, est, 0.1, 7)
    L = np.zeros((h, w, n, 3))
    ray = (ctypes.c_double * 6)()
    out = (ctypes.c_double * 3)()
    c = Counters()
    tests = iters = 0
    cam, trace, start = orc.L.orc_camera_ray, orc.L.orc_trace, orc.L.orc_stream_state_c
    for y in range(h):  # camera row; file row h - 1 - y
        for x in range(w):
            idx = (h - y - 1) * w + x
            for i in range(n):
                st = cam(w, h, x, y, start(seed, idx, i), ray)
                ray[0], ray[1], ray[2] = origin
                trace(ray, st, byref(m), out, byref(c))
                L[h - 1 - y, x, i] = out[0], out[1], out[2]
                tests += c.tests
                iters += c.iterations
    return L, tests, iters


def pixel_sums(L, starts):
    """the chunk sums combined in chunk order: orc_render_layout's `tot` per pixel"""
    tot = np.zeros(L.shape[:2] + (3,))
    for c0, c1 in zip(starts[:-1], starts[1:]):
        acc = np.zeros_like(tot)
        for i in range(c0, c1):
            acc = L[:, :, i] + acc
        tot = acc + tot
    return tot


def image(L, starts):
    spp = starts[-1]
    return pixel_sums(L[:, :, :spp], starts) * (1 / float(spp))
