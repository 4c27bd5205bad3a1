"""CPU model of the progressive accumulator (numpy only): csrc/vpt_accum.h restated.

Per-sample radiance comes from the oracle exactly as the renderer defines it (Oracle.stream_state ->
Oracle.camera_ray -> Oracle.trace); chunk sums are formed as acc = L + acc; from them the model keeps sum, s1,
s2 per pixel and a level count and error per 8x8 tile, runs the refine policy and resolves the image.  Every
numpy operation below rounds once (no contraction), in the header's order, so every value is exact and the
tests compare bits.
"""
from __future__ import annotations

import numpy as np

LUM = (0.2126, 0.7152, 0.0722)


def shard_file_rows(h, band_rows=0, band_stride=1, band_offset=0):
    """file rows of a shard in the order vpt_render writes them (include/vpt.h, band_*)"""
    band_rows = band_rows or h
    nb = -(-h // band_rows)
    rows = []
    for b in range(band_offset, nb, band_stride):
        rows += list(range(b * band_rows, min(h, (b + 1) * band_rows)))
    return rows


def chunk_sums(orc, w, h, C, levels, est, seed, file_rows=None, **medium):
    """csum[levels, rows, w, 3]: level k of a pixel = its samples [kC, kC + C) summed as acc = L + acc"""
    file_rows = list(range(h)) if file_rows is None else list(file_rows)
    n = len(file_rows) * w
    xs = np.tile(np.arange(w), len(file_rows))
    frs = np.repeat(np.asarray(file_rows), w)
    out = np.zeros((levels, n, 3))
    rays = np.zeros((n, 6))
    st = np.zeros(n, dtype=np.uint64)
    for k in range(levels):
        acc = np.zeros((n, 3))
        for s in range(k * C, (k + 1) * C):
            for i in range(n):
                fr, x = int(frs[i]), int(xs[i])
                s0 = orc.stream_state(seed, fr * w + x, s)
                rays[i], st[i] = orc.camera_ray(w, h, x, h - 1 - fr, s0)
            L, _ = orc.trace(est, rays, st, **medium)
            acc = L + acc
        out[k] = acc
    return out.reshape(levels, len(file_rows), w, 3)


_CACHE = {}


def cached_chunk_sums(orc, scene_name, scene, w, h, C, levels, est, seed, bands=(0, 1, 0), **medium):
    """chunk_sums computed once per configuration and shared by the tests (read-only)"""
    key = (scene_name, w, h, C, levels, est, seed, bands, tuple(sorted(medium.items())))
    if key not in _CACHE:
        orc.set_scene(scene)
        cs = chunk_sums(orc, w, h, C, levels, est, seed, shard_file_rows(h, *bands), **medium)
        cs.setflags(write=False)
        _CACHE[key] = cs
    return _CACHE[key]


def lum(c):
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def pixel_err(s1, s2, m, cfloor):
    """vpt_accum_err, elementwise; m scalar"""
    s1 = np.asarray(s1, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    if m < 2:
        return np.full(s1.shape, np.inf)
    with np.errstate(all="ignore"):
        mean = s1 / float(m)
        var = (s2 - s1 * mean) / float(m - 1)
        var = np.where(var > 0, var, 0.0)
        se = np.sqrt(var / float(m))
        den = np.where(mean > cfloor, mean, cfloor)
        return se / den


def stat(csum, C, lum_floor=0.01):
    """vpt_accum_stat_host: csum[m, npix, 3] -> sum[npix, 3], s12[npix, 2], err[npix]"""
    m = csum.shape[0]
    s = np.zeros(csum.shape[1:])
    s1 = np.zeros(csum.shape[1])
    s2 = np.zeros(csum.shape[1])
    with np.errstate(all="ignore"):
        for k in range(m):
            y = lum(csum[k])
            s = csum[k] + s
            s1 = y + s1
            s2 = y * y + s2
    return s, np.stack([s1, s2], axis=-1), pixel_err(s1, s2, m, float(C) * lum_floor)


def active(levels, err, target, min_levels, max_levels):
    """the refine policy: ascending indices of the active tiles (NaN > target is False)"""
    levels = np.asarray(levels)
    with np.errstate(invalid="ignore"):
        a = (levels < max_levels) & ((levels < min_levels) | (np.asarray(err) > target))
    return [int(t) for t in np.nonzero(a)[0]]


class AccumModel:
    """the accumulator on precomputed chunk sums csum[max_levels, rows, w, 3]"""

    def __init__(self, csum, C, lum_floor=0.01):
        self.csum, self.C, self.lum_floor = csum, C, lum_floor
        self.max_levels, self.rows, self.w = csum.shape[0], csum.shape[1], csum.shape[2]
        self.tiles_x, self.tiles_y = -(-self.w // 8), -(-self.rows // 8)
        self.ntiles = self.tiles_x * self.tiles_y
        self.levels = np.zeros(self.ntiles, dtype=np.int32)
        self.sum = np.zeros((self.rows, self.w, 3))
        self.s1 = np.zeros((self.rows, self.w))
        self.s2 = np.zeros((self.rows, self.w))
        self.tile_err = np.full(self.ntiles, np.inf)

    def _slice(self, t):
        ty, tx = divmod(t, self.tiles_x)
        return slice(ty * 8, min(self.rows, ty * 8 + 8)), slice(tx * 8, min(self.w, tx * 8 + 8))

    def add(self, levels=1, tiles=None):
        tiles = range(self.ntiles) if tiles is None else tiles
        for t in tiles:
            self._add_tile(int(t), levels)

    def _add_tile(self, t, n):
        assert self.levels[t] + n <= self.max_levels
        r, c = self._slice(t)
        with np.errstate(all="ignore"):
            for k in range(self.levels[t], self.levels[t] + n):
                ch = self.csum[k, r, c]
                y = lum(ch)
                self.sum[r, c] = ch + self.sum[r, c]
                self.s1[r, c] = y + self.s1[r, c]
                self.s2[r, c] = y * y + self.s2[r, c]
        self.levels[t] += n
        e = pixel_err(self.s1[r, c], self.s2[r, c], int(self.levels[t]), float(self.C) * self.lum_floor)
        self.tile_err[t] = np.max(e)  # np.max lets a NaN win, like vpt_accum_max

    def refine(self, target, lum_floor=0.01, min_levels=4, levels_per_pass=1):
        """returns the active sets of the passes made"""
        if lum_floor != self.lum_floor:
            self.lum_floor = lum_floor
            for t in range(self.ntiles):
                self._add_tile(t, 0)
        sets = []
        while True:
            act = active(self.levels, self.tile_err, target, min_levels, self.max_levels)
            if not act:
                return sets
            sets.append(act)
            for t in act:
                self._add_tile(t, min(levels_per_pass, self.max_levels - int(self.levels[t])))

    def to_pixels(self, per_tile):
        g = np.asarray(per_tile).reshape(self.tiles_y, self.tiles_x)
        return np.repeat(np.repeat(g, 8, axis=0), 8, axis=1)[:self.rows, :self.w]

    def spp_map(self):
        return self.to_pixels(self.levels.astype(np.int64) * self.C)

    def image(self, fp64=True):
        spp = self.spp_map()
        with np.errstate(all="ignore"):
            scale = np.where(spp > 0, 1.0 / np.maximum(spp, 1).astype(np.float64), 0.0)
            img = np.where(spp[..., None] > 0, self.sum * scale[..., None], 0.0)
        return img if fp64 else img.astype(np.float32)
