"""What the heterogeneous medium (estimator 10: density grid, delta tracking) costs, at 1024^2 x 64 spp in the
dense medium of bench.py's CONFIGS["dense"] (sigma 0.003 / 0.027, 8 bounces), default scene.  GPU events on the
default stream, best and all of --reps repetitions after one untimed run.  Rows:
  a          estimator 0 (the pool kernel)
  b          estimator 10 on a uniform rho = 1 grid (4^3 voxels on [-4096, 4096]^3): a's paths draw for draw, so
             b - a is the cost of the grid machinery and of leaving the pool kernel
  c          estimator 10 on a 64^3 procedural cloud in the room (rho_max / mean about 10: most collisions are
             null), with the mean tentative delta-tracking steps per track (65 536 camera samples)
  b16, c16   b and c on 16^3 grids (64 KiB of LDS hold them)
each of b, c, b16, c16 with hetero_kernel and with VPT_SIMPLE_KERNEL=1 (render_kernel_simple_hetero), and with
hetero_kernel on --nolds-lib, a build that reads every grid from global memory
(bash scripts/build_variant.sh hetero_nolds -DVPT_HETERO_LDS=0; the default stages grids of at most 64 KiB -- b, b16
and c16 -- in LDS).
  c_B<k>, c16_B<k>   c and c16 with local majorants on super-voxels of k = 2, 4, 8, 16 voxels per axis
             (Tracer.set_majorant_block; hetero_kernel only), with the steps per track; and, where
             --noldsmaj-lib is built (bash scripts/build_variant.sh hetero_noldsmaj -DVPT_HETERO_LDS_MAJ=0), the same
             rows on that build, which reads the majorant grid from global memory (the default stages it in what
             the density left of the 64 KiB of LDS)
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
--only takes a comma-separated subset of the row groups base (a, b, c, b16, c16), simple, nolds, lm, noldsmaj.
usage: python scripts/hetero_time.py [--reps N] [--size WxH] [--spp N] [--only GROUPS] [--nolds-lib PATH]
       [--noldsmaj-lib PATH]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA = dict(sigma_a=0.003, sigma_s=0.027, max_depth=8)
BLOCKS = (2, 4, 8, 16)
ROOM_LO, ROOM_HI = (-60.0, -50.0, -100.0), (60.0, 50.0, 230.0)
BIG_LO, BIG_HI = (-4096.0,) * 3, (4096.0,) * 3


def cloud(n):
    """a procedural cloud on n^3 voxels: a few Gaussian puffs, scaled so that rho_max / mean is about 10 and the
    mean density is 1 (the mean extinction is then the dense medium's)"""
    rng = np.random.default_rng(7)
    z, y, x = np.meshgrid(*(3 * [(np.arange(n) + 0.5) / n]), indexing="ij")
    rho = np.zeros((n, n, n))
    for _ in range(12):
        c = rng.uniform(0.15, 0.85, 3)
        s = rng.uniform(0.05, 0.12)
        rho += rng.uniform(0.5, 1.0) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    rho += 0.02 * rho.max()
    k = 1.0
    for _ in range(40):  # a power sharpens or flattens the field until max / mean is 10
        r = rho ** k
        k *= (np.log(10.0) / np.log(r.max() / r.mean())) ** 0.5
    r = rho ** k
    return (r / r.mean()).astype(np.float32)


def grids(row):
    if row in ("b", "b16"):
        n = 4 if row == "b" else 16
        return np.ones((n, n, n), np.float32), BIG_LO, BIG_HI
    return cloud(64 if row == "c" else 16), ROOM_LO, ROOM_HI


def camera_samples(n, w, h, seed=3):
    """n camera samples of the default camera (the arithmetic of src/rt.cpp:758-787 in numpy; statistics only)"""
    import minimal_volumetric_path_tracer_amd as vpt

    p = vpt.RenderConfig(width=w, height=h).params()
    rng = np.random.default_rng(seed)
    o, cd = np.array(p.camera.o[:]), np.array(p.camera.d[:])
    cx = np.array([w * p.fov_scale / h, 0.0, 0.0])
    cy = np.cross(cx, cd)
    cy = cy / np.linalg.norm(cy) * p.fov_scale
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    jx, jy = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    d = cx * (((x + jx - 0.5) / w - 0.5))[:, None] + cy * (((y + jy - 0.5) / h - 0.5))[:, None] + cd
    rays = np.zeros(n, dtype=vpt.RAY_DTYPE)
    rays["o"] = o
    rays["d"] = d / np.linalg.norm(d, axis=1)[:, None]
    return rays, rng.integers(0, 1 << 48, n, dtype=np.uint64)


def step(args):
    import ctypes

    import torch

    import minimal_volumetric_path_tracer_amd as vpt
    from minimal_volumetric_path_tracer_amd import _lib

    w, h = (int(v) for v in args.size.split("x"))
    tr = vpt.Tracer(0)
    res = {"row": args.step, "build_id": vpt.build_id(), "lib": os.path.relpath(_lib.LIB_PATH, ROOT),
           "simple_kernel": bool(os.environ.get("VPT_SIMPLE_KERNEL"))}
    if args.step == "a":
        cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator="ff", seed=0x5EED0001, **SIGMA)
    else:
        rho, lo, hi = grids(args.step)
        if args.block:
            tr.set_majorant_block(args.block)
            res["majorant_block"] = args.block
        tr.set_density_grid(rho, lo, hi)
        cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator="hetero", seed=0x5EED0001, **SIGMA)
        res.update(grid=list(rho.shape), rho_max_over_mean=round(float(rho.max() / rho.mean()), 3))
        if args.step in ("c", "c16") and not res["simple_kernel"]:
            rays, st = camera_samples(65536, w, h)
            f = vpt.lib().vpt_debug_hetero_steps
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_lib.vpt_medium)] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + \
                [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 2
            out = np.zeros((len(rays), 3))
            tracks, steps = ctypes.c_uint64(), ctypes.c_uint64()
            m = cfg.medium()
            _lib.check(f(tr._ctx, ctypes.byref(m), rays.ctypes.data, st.ctypes.data, len(rays), out.ctypes.data,
                         ctypes.byref(tracks), ctypes.byref(steps)))
            res.update(tracks=tracks.value, tentative_steps=steps.value,
                       steps_per_track=round(steps.value / max(tracks.value, 1), 3))
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    ms = []
    for i in range(args.reps + 1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.render_device(cfg, out.data_ptr())
        b.record()
        torch.cuda.synchronize()
        if i > 0:  # the first run pays for buffers and code objects
            ms.append(a.elapsed_time(b))
    res.update(gpu_ms=round(min(ms), 3), gpu_ms_all=[round(x, 3) for x in ms],
               msamples_per_s=round(w * h * args.spp / min(ms) / 1e3, 1), image_mean=float(out.mean()),
               image_finite=bool(torch.isfinite(out).all()))
    tr.close()
    print(json.dumps(res))


def child(args, row, simple=False, lib=None, block=0, timeout=240):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    if simple:
        env["VPT_SIMPLE_KERNEL"] = "1"
    if lib:
        env["VPT_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--step", row, "--reps", str(args.reps), "--size", args.size,
           "--spp", str(args.spp), "--block", str(block)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"row {row} failed with status {r.returncode}: {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["a", "b", "c", "b16", "c16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--only", default="base,simple,nolds,lm,noldsmaj")
    ap.add_argument("--block", type=int, default=0, help="with --step: the majorant block size (0: off)")
    ap.add_argument("--nolds-lib", default=os.path.join(ROOT, "build_variants", "libvpt_hetero_nolds.so"))
    ap.add_argument("--noldsmaj-lib", default=os.path.join(ROOT, "build_variants", "libvpt_hetero_noldsmaj.so"))
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"command": "python scripts/hetero_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    groups = set(args.only.split(","))
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        if "base" in groups:
            out["a"] = child(args, "a")
        for row in ("b", "c", "b16", "c16"):
            if "base" in groups:
                out[row] = child(args, row)
            if "simple" in groups:
                out[row + "_simple"] = child(args, row, simple=True)
        if "nolds" in groups and os.path.exists(args.nolds_lib):
            for row in ("b", "c", "b16", "c16"):
                out[row + "_nolds"] = child(args, row, lib=args.nolds_lib)
        elif "nolds" in groups:
            out["nolds"] = f"{os.path.relpath(args.nolds_lib, ROOT)} is not built"
        if "lm" in groups:
            for row in ("c", "c16"):
                for b in BLOCKS:
                    out[f"{row}_B{b}"] = child(args, row, block=b)
        if "noldsmaj" in groups and os.path.exists(args.noldsmaj_lib):
            for row in ("c", "c16"):
                for b in BLOCKS:
                    out[f"{row}_B{b}_noldsmaj"] = child(args, row, lib=args.noldsmaj_lib, block=b)
        elif "noldsmaj" in groups:
            out["noldsmaj"] = f"{os.path.relpath(args.noldsmaj_lib, ROOT)} is not built"
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
