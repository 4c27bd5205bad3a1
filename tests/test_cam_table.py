"""The pool kernel's camera table (vpt_int_cam_table, through vpt_debug_cam_table; no GPU): (o - centre, |o - centre|^2)
per sphere, bit for bit what numpy float64 gives for Sphere::intersect's expression order -- three differences,
then ocx*ocx + ocy*ocy + ocz*ocz summed left to right, every product and sum rounded on its own (no fused
multiply-add: the host unit is built with -ffp-contract=off like the device code that reads the table)."""
import ctypes

import numpy as np
import pytest

from minimal_volumetric_path_tracer_amd import lib
from scenes import ALT_SCENES, SCENES, SPHERE_DTYPE

ORIGINS = [(0.0, 11.2, 214.0), (3.3, -7.1, 40.7), (-23.0, 24.3, 0.0), (23.5, 24.1, 35.7), (1e5 + 49.1, -0.3, 7e-3)]


def _table(spheres, o):
    f = lib().vpt_debug_cam_table
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    s = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE)
    oo = np.array(o, dtype=np.float64)
    out = np.full((len(s), 4), np.nan)
    assert f(s.ctypes.data, len(s), oo.ctypes.data, out.ctypes.data) == 0
    return out


def _numpy_table(spheres, o):
    p = np.asarray(spheres["p"], dtype=np.float64)
    oc = np.float64(o)[None, :] - p
    sq = oc * oc
    cc = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    return np.concatenate([oc, cc[:, None]], axis=1)


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("scene", ["default", "mat3", "alt_metal_walls", "alt_open_space"])
def test_cam_table_bits(scene, origin):
    spheres = dict(SCENES, **ALT_SCENES)[scene]()
    got, want = _table(spheres, origin), _numpy_table(spheres, origin)
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()  # the bits: -0.0 is not +0.0 here


def test_cam_table_contraction_would_show():
    """the cases are able to tell a fused multiply-add from the separate roundings"""
    import math

    differ = 0
    for scene in ("default", "alt_open_space"):
        s = dict(SCENES, **ALT_SCENES)[scene]()
        for o in ORIGINS:
            t = _numpy_table(s, o)
            for ocx, ocy, ocz, cc in t:
                if hasattr(math, "fma"):
                    fused = math.fma(ocz, ocz, math.fma(ocy, ocy, ocx * ocx))
                else:  # exact rational arithmetic stands in for the fused operations
                    from fractions import Fraction as Fr

                    fused = float(Fr(float(Fr(ocy) * Fr(ocy) + Fr(ocx * ocx))) + Fr(ocz) * Fr(ocz))
                differ += fused != cc
    assert differ > 0


def test_cam_table_rejects_bad_arguments():
    f = lib().vpt_debug_cam_table
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    o = np.zeros(3)
    out = np.zeros(4 * 65)
    s = np.zeros(65, dtype=SPHERE_DTYPE)
    assert f(s.ctypes.data, 65, o.ctypes.data, out.ctypes.data) != 0
    assert f(None, 1, o.ctypes.data, out.ctypes.data) != 0
