"""csrc/vpt_grid_mis.h's host side under AddressSanitizer and UndefinedBehaviorSanitizer: writes the ray sets of
scripts/grid_sanitize.py (the tau and KS sets of tests/grid_model.py, and the tau set on a 1 x 1 x 1 grid) and the sparse
field of the equi-angular tests to files, builds scripts/grid_mis_sanitize.cpp with -fsanitize=address,undefined and runs
it on each.  CPU only; exits non-zero on any report.
usage: python scripts/grid_mis_sanitize.py [--cxx g++] [--dir DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]


def main():
    import grid_model as gm
    import majorant_model as mm
    from grid_sanitize import write

    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    d = args.dir or tempfile.mkdtemp(prefix="grid_mis_sanitize_")
    os.makedirs(d, exist_ok=True)
    rays, tmax = gm.tau_rays()
    st = gm.states(3, len(rays))
    write(os.path.join(d, "tau.bin"), gm.tau_grid(), gm.TAU_LO, gm.TAU_HI, 0.7, rays, tmax, st)
    sparse = mm.sparse_field()
    sparse[:, :, :4] = 0.0  # a region where the trilinear field too is exactly zero: the rho_t == 0 exit
    write(os.path.join(d, "sparse.bin"), sparse, gm.TAU_LO, gm.TAU_HI, 0.7, rays, tmax, st)
    write(os.path.join(d, "one.bin"), np.full((1, 1, 1), 0.7, np.float32), gm.TAU_LO, gm.TAU_HI, 0.05, rays, tmax, st)
    rays, tmax = gm.ks_rays(4096)
    write(os.path.join(d, "ks.bin"), gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, gm.states(gm.KS_SEED, 4096))
    exe = os.path.join(d, "grid_mis_sanitize")
    subprocess.run([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "minimal_volumetric_path_tracer_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "grid_mis_sanitize.cpp"), "-o", exe], check=True)
    for name in ("tau.bin", "sparse.bin", "one.bin", "ks.bin"):
        subprocess.run([exe, os.path.join(d, name)], check=True)
    print("clean")


if __name__ == "__main__":
    sys.exit(main())
