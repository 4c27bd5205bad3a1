"""csrc/vpt_grid.h's host side under AddressSanitizer and UndefinedBehaviorSanitizer: writes the tau and KS ray sets of
tests/grid_model.py (and the tau set on a 1 x 1 x 1 grid) to files, builds scripts/grid_sanitize.cpp with
-fsanitize=address,undefined and runs it on each.  CPU only; exits non-zero on any report.
usage: python scripts/grid_sanitize.py [--cxx g++] [--dir DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def write(path, rho, lo, hi, sigma_t, rays, tmax, states):
    nz, ny, nx = rho.shape
    with open(path, "wb") as f:
        f.write(np.array([nx, ny, nz, len(rays)], np.int32).tobytes())
        f.write(np.array(list(lo) + list(hi) + [sigma_t], np.float64).tobytes())
        f.write(np.ascontiguousarray(rho, np.float32).tobytes())
        f.write(np.concatenate([rays["o"], rays["d"]], axis=1).astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float64), (len(rays),))).tobytes())
        f.write(np.ascontiguousarray(states, np.uint64).tobytes())


def main():
    import grid_model as gm

    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    d = args.dir or tempfile.mkdtemp(prefix="grid_sanitize_")
    os.makedirs(d, exist_ok=True)
    rays, tmax = gm.tau_rays()
    write(os.path.join(d, "tau.bin"), gm.tau_grid(), gm.TAU_LO, gm.TAU_HI, 0.7, rays, tmax, gm.states(3, len(rays)))
    write(os.path.join(d, "one.bin"), np.full((1, 1, 1), 0.7, np.float32), gm.TAU_LO, gm.TAU_HI, 0.05, rays, tmax,
          gm.states(3, len(rays)))
    rays, tmax = gm.ks_rays(4096)
    write(os.path.join(d, "ks.bin"), gm.KS_RHO, gm.KS_LO, gm.KS_HI, gm.KS_SIGMA_T, rays, tmax, gm.states(gm.KS_SEED, 4096))
    exe = os.path.join(d, "grid_sanitize")
    subprocess.run([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "minimal_volumetric_path_tracer_amd", "csrc"),
                    os.path.join(ROOT, "scripts", "grid_sanitize.cpp"), "-o", exe], check=True)
    for name in ("tau.bin", "one.bin", "ks.bin"):
        subprocess.run([exe, os.path.join(d, name)], check=True)
    print("clean")


if __name__ == "__main__":
    sys.exit(main())
