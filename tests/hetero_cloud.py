"""The inputs that tests/test_oracle_hetero.py (CPU: the sensitivity of these inputs to each class of mistake) and
tests/test_gpu_hetero_oracle.py (GPU: estimators 10 and 11 against the oracle) share: a non-uniform, non-cubic cloud
inside the room, its emission, the medium, and the four grid configurations.

Why these coefficients.  A path test sees a transmittance segment only at a surface event (Trs, MISv2's per-light
factors) or a medium event (the point-light factor, the cone factor), so both have to be common, and the roulette
ends 40 % of all iterations before either.  At bench.py's dense medium (0.003, 0.027) the cloud (mean density about
1.2) makes 48 % of the iterations medium events and 11 % surface events; at a fifth of it the two are 26-28 % and
32-35 %, and each of the oracle's four deliberate mistakes (orc_hetero_set_fault) changes more than 200 of 4096
samples (tests/test_oracle_hetero.py asserts both)."""
import numpy as np

import emission_model as em

ROOM_LO, ROOM_HI = (-60.0, -50.0, -100.0), (60.0, 50.0, 230.0)  # test_gpu_hetero's: contains the room and the camera
SA, SS = 0.0006, 0.0054  # a fifth of test_gpu_hetero's (0.003, 0.027)
RGB = (0.9, 0.5, 0.25)
SEED = 3
# (majorant block, interpolation, emission): the full matrix, and the one configuration of the other tests
CONFIGS = [(block, interp, emit) for block in (0, 2) for interp in ("nearest", "trilinear") for emit in (False, True)]
MAIN = (2, "trilinear", True)
ESTIMATORS = {"hetero": 10, "hetero_ratio": 11}


def cloud():
    """(rho, eps): emission_model's 6 x 5 x 4 fields, some voxels of each zero; eps scaled as test_gpu_emission._cloud
    scales it, so that the glow is of the order of the lit room"""
    rho, eps = em.fields()
    return rho, eps * np.float32(40.0)


def set_cloud(owner, block, interp, emit):
    """the cloud in the room on a Tracer or an Oracle (both take these arguments)"""
    rho, eps = cloud()
    owner.set_density_grid(rho, ROOM_LO, ROOM_HI, majorant_block=block, interpolation=interp)
    if emit:
        owner.set_emission_grid(eps, RGB)
