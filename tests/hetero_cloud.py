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


# ---- estimators 12, 13 and 14 (tests/test_oracle_hetero_ext.py, tests/test_gpu_hetero_ext_oracle.py): the same cloud,
# no emission grid (the library refuses these estimators with one).
#
# Why another box.  In ROOM_LO .. ROOM_HI the camera and every wall lie inside the grid, so the equi-angular interval
# [a, b] is [0, t] on all but the rays that hit nothing, and a kernel that sampled [0, t] would differ on 42 of 4096
# samples.  In EXT_LO .. EXT_HI the camera stands outside the box (a > 0 on every camera ray) and the walls lie
# outside it (b < t on most later rays): that mistake moves more than 1000 samples.  The three lights are inside.
#
# Why these coefficients.  The smaller box holds less medium; at (0.0026, 0.0234) the 2048 samples of the GPU tests
# have at least 27 % surface events, 25 % medium events and 50 % lit samples under each of the three estimators on
# each of the four grid configurations, and each of the oracle's deliberate mistakes 5-10 (orc_hetero_set_fault)
# changes more than 1000 of 4096 samples (tests/test_oracle_hetero_ext.py asserts both).
EXT_LO, EXT_HI = (-40.0, -35.0, -70.0), (40.0, 38.0, 120.0)
EXT_SA, EXT_SS = 0.0026, 0.0234
Q = 0.5  # estimator 13's track fraction
# estimator 14's colour: three different extinctions and three different albedos
COLOUR = ((1.0, 0.6, 0.3), (0.7, 1.0, 1.4))
# one pair of equal extinctions (channels 0 and 1 take the same multipliers, so the pair is equal bit for bit) and a
# third that differs: two of three hero choices run the same track, and the weights' mean has two equal terms
COLOUR_PAIR = ((1.0, 1.0, 0.3), (1.0, 1.0, 1.4))
GREY = ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
EXT_CONFIGS = [(block, interp) for block in (0, 2) for interp in ("nearest", "trilinear")]
EXT_MAIN = (2, "trilinear")
ESTIMATORS.update({"hetero_equiangular": 12, "hetero_mis": 13, "hetero_chromatic": 14})
EXT_ESTIMATORS = ("hetero_equiangular", "hetero_mis", "hetero_chromatic")


def set_ext_cloud(owner, block, interp, q=Q, colour=COLOUR):
    """the cloud in EXT_LO .. EXT_HI, the track fraction and the medium colour on a Tracer or an Oracle"""
    owner.set_density_grid(cloud()[0], EXT_LO, EXT_HI, majorant_block=block, interpolation=interp)
    owner.set_hetero_mis_fraction(q)
    owner.set_medium_colour(*colour)


def reset_ext(owner):
    """the defaults of what set_ext_cloud set, and no grid"""
    owner.clear_density_grid()
    owner.set_hetero_mis_fraction(0.5)
    owner.set_medium_colour(*GREY)


# ---- estimators 15 and 16 (tests/test_oracle_hetero_resid_spectral.py, tests/test_gpu_hetero_resid_spectral_oracle.py):
# the box EXT_LO .. EXT_HI, no emission grid.
#
# Estimator 16 takes the cloud and the medium of estimators 12-14 as they are, under three colours.  COLOUR has three
# different extinctions, channel 2 the largest.  COLOUR_FIRST is COLOUR's absorption reversed under a scattering that
# falls with the channel: channel 0 is the largest, so a statement that reads "the last channel" for "the largest" shows.
# COLOUR_TOP_PAIR gives channels 0 and 1 the same multipliers and the largest extinction: both have f == x / x == 1.0 and
# both are 0.0 after a rho >= mu point, the third still estimates.
COLOUR_FIRST = ((0.3, 0.6, 1.0), (1.4, 1.0, 0.7))
COLOUR_TOP_PAIR = ((1.0, 1.0, 0.3), (1.4, 1.4, 0.7))
SPECTRAL_COLOURS = {"colour": COLOUR, "first": COLOUR_FIRST, "top_pair": COLOUR_TOP_PAIR}
#
# Estimator 15 needs a field of its own.  On cloud() every block minimum is 0 at the main configuration (block 2,
# trilinear) and under the nearest lookup 4 of 18 are positive with a mean mn / mu of 0.05: the control grid is inert and
# the estimator is estimator 11, so a test on it would pass whatever the residual code did.  floor_cloud() lays the
# density FLOOR under the x slabs FLOOR_SLABS of the same cloud.  At blocks 1 and 2 under both lookups it has blocks with
# mn == 0 and -- but at block 1 under the nearest lookup, where every block is uniform (mn == mu: the one-draw branch) --
# blocks with 0 < mn < mu (tests/test_oracle_hetero_resid_spectral.py asserts it from residual_model.control).
# Why this floor and these coefficients.  The roulette ends 40 % of the iterations, so surface and medium events share
# less than 60 % and each is to have 25 %; and at block 2 under the nearest lookup a candidate in a block's densest voxel
# makes the estimate 0.0, which costs lit samples in proportion to the candidates' rate mr sigma_t.  A floor of 0.5 under
# three slabs lights 48 % of the samples at the sigma_t that gives 25 % medium events.  A high floor under four of the
# six slabs at a quarter of (EXT_SA, EXT_SS) keeps the collisions (their rate has the floor in it) and thins the
# candidates (theirs has not): at least 32 % surface events, 26 % medium events and 51 % lit samples on every
# configuration.  A block >= max(n) is one super-voxel, the global control; its minimum is 0 here.
FLOOR = np.float32(3.0)
FLOOR_SLABS = slice(0, 4)
RES_SA, RES_SS = 0.00065, 0.00585  # a quarter of (EXT_SA, EXT_SS)
RES_CONFIGS = [(block, interp) for block in (1, 2) for interp in ("nearest", "trilinear")] + [(6, "trilinear")]
# The configuration of the sensitivity tests, the other scenes, the extensions and the 72 spp render is block 2 under the
# NEAREST lookup for both estimators, not EXT_MAIN.  Under the trilinear lookup a block's majorant is taken over the block
# dilated by a voxel, so a looked-up rho >= mu is rare (1 of 4096 samples meets one): the branch that tells chromatic ratio
# tracking from the scalar walker is not taken, and a walker that returned (0, 0, 0) there moves no sample.  Under the
# nearest lookup 4800 ratio walks of 4096 samples go on past such a point.  For estimator 15, 13 of 18 block minima are
# positive under the nearest lookup against 7 under the dilation, and a missing piece of tauc moves 411 samples, not 112.
RES_MAIN = (2, "nearest")
SPECTRAL_MAIN = (2, "nearest")
ESTIMATORS.update({"hetero_residual": 15, "hetero_spectral": 16})


def floor_cloud():
    """cloud()'s density with FLOOR added to the voxels of the x slabs FLOOR_SLABS"""
    rho = cloud()[0].copy()
    rho[:, :, FLOOR_SLABS] += FLOOR
    return rho


def set_floor_cloud(owner, block, interp):
    """estimator 15's field in EXT_LO .. EXT_HI on a Tracer or an Oracle"""
    owner.set_density_grid(floor_cloud(), EXT_LO, EXT_HI, majorant_block=block, interpolation=interp)
    owner.set_medium_colour(*GREY)
