"""CPU model of the grid accumulator (vpt_accum_create_grid, Tracer.grid_accumulator; numpy only).

The input is the per-sample radiances L[rows, w, cap, 3] of a shard.  Per pixel the model keeps
  sum     acc = L + acc over the samples the pixel holds, in order from zero (NOT the sum of the chunk sums);
  s1, s2  folded from the chunk sums c_k (samples [kC, kC + C) summed as c = L + c from zero): y = lum(c_k),
          s1 = y + s1, s2 = y*y + s2, the lines of csrc/vpt_accum.h;
and per 8x8 tile a level count and an error.  add, refine, the tile maximum, the maps and the resolve are
accum_model.AccumModel's (lum, pixel_err, active, to_pixels): only the way a level arrives differs.  Every numpy
operation rounds once, in the kernel's order, so the tests compare bits.
"""
from __future__ import annotations

import numpy as np

import accum_model as am


def radiances(trace, rays, states, file_rows=None):
    """L[rows, w, spp, 3] from a per-sample call trace(rays, states) -> (L, end states) on the camera samples
    [file row, x, sample] of test_gpu_hetero._camera_samples; file_rows: the shard's rows (None: all)"""
    if file_rows is not None:
        rays, states = rays[list(file_rows)], states[list(file_rows)]
    L, _ = trace(np.ascontiguousarray(rays).reshape(-1), np.ascontiguousarray(states).reshape(-1))
    L = np.asarray(L, dtype=np.float64).reshape(states.shape + (3,))
    L.setflags(write=False)
    return L


def chunk_sums(L, C):
    """csum[levels, rows, w, 3]: level k = samples [kC, kC + C) summed as c = L + c from zero"""
    rows, w, cap, _ = L.shape
    assert cap % C == 0
    out = np.zeros((cap // C, rows, w, 3))
    with np.errstate(all="ignore"):
        for k in range(cap // C):
            c = np.zeros((rows, w, 3))
            for s in range(k * C, (k + 1) * C):
                c = L[:, :, s] + c
            out[k] = c
    return out


class GridAccumModel(am.AccumModel):
    """the grid accumulator on per-sample radiances L[rows, w, cap, 3] with levels of C samples"""

    def __init__(self, L, C, lum_floor=0.01):
        super().__init__(chunk_sums(L, C), C, lum_floor)
        self.L = L

    def _add_tile(self, t, n):
        assert self.levels[t] + n <= self.max_levels
        r, c = self._slice(t)
        k0 = int(self.levels[t])
        with np.errstate(all="ignore"):
            for s in range(k0 * self.C, (k0 + n) * self.C):  # the pixel's sum: sample by sample, in order
                self.sum[r, c] = self.L[r, c, s] + self.sum[r, c]
            for k in range(k0, k0 + n):  # the statistic: level by level
                y = am.lum(self.csum[k, r, c])
                self.s1[r, c] = y + self.s1[r, c]
                self.s2[r, c] = y * y + self.s2[r, c]
        self.levels[t] += n
        e = am.pixel_err(self.s1[r, c], self.s2[r, c], int(self.levels[t]), float(self.C) * self.lum_floor)
        self.tile_err[t] = np.max(e)  # np.max lets a NaN win, like vpt_accum_max
