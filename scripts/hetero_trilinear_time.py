"""What trilinear density interpolation (Tracer.set_grid_interpolation, csrc/vpt_grid.h) costs: rows (b), (c) and (c16) of
scripts/hetero_time.py -- the uniform 4^3 grid, the 64^3 and the 16^3 cloud -- at 1024^2 x 64 spp in the dense medium,
for estimators 10 ("hetero") and 11 ("hetero_ratio"), nearest and trilinear, with majorant blocks 0 and 8.  GPU events
on the default stream, best and all of --reps repetitions after one untimed run, and for estimator 10 the mean
tentative delta-tracking steps per track over 65 536 camera samples.  Every figure is a measurement: no threshold.
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
usage: python scripts/hetero_trilinear_time.py [--reps N] [--size WxH] [--spp N] [--rows b,c,c16]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import hetero_time as ht  # noqa: E402  (the grids, the medium and the camera samples of that table)

BLOCKS = (0, 8)
ESTIMATORS = ("hetero", "hetero_ratio")
MODES = ("nearest", "trilinear")


def step(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt
    from minimal_volumetric_path_tracer_amd import _lib

    w, h = (int(v) for v in args.size.split("x"))
    rho, lo, hi = ht.grids(args.step)
    tr = vpt.Tracer(0)
    tr.set_density_grid(rho, lo, hi, majorant_block=args.block, interpolation=args.interp)
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=args.est, seed=0x5EED0001, **ht.SIGMA)
    res = {"row": args.step, "estimator": args.est, "interpolation": args.interp, "majorant_block": args.block,
           "build_id": vpt.build_id(), "grid": list(rho.shape)}
    if args.est == "hetero":
        rays, st = ht.camera_samples(65536, w, h)
        f = vpt.lib().vpt_debug_hetero_steps
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(_lib.vpt_medium)] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + \
            [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 2
        out = np.zeros((len(rays), 3))
        tracks, steps = ctypes.c_uint64(), ctypes.c_uint64()
        m = cfg.medium()
        _lib.check(f(tr._ctx, ctypes.byref(m), rays.ctypes.data, st.ctypes.data, len(rays), out.ctypes.data,
                     ctypes.byref(tracks), ctypes.byref(steps)))
        res.update(tracks=tracks.value, tentative_steps=steps.value, steps_per_track=round(steps.value / max(tracks.value, 1), 3))
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
    res.update(gpu_ms=round(min(ms), 3), gpu_ms_all=[round(x, 3) for x in ms], image_mean=float(out.mean()),
               image_finite=bool(torch.isfinite(out).all()))
    tr.close()
    print(json.dumps(res))


def child(args, row, est, interp, block, timeout=300):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", row, "--est", est, "--interp", interp, "--block", str(block),
           "--reps", str(args.reps), "--size", args.size, "--spp", str(args.spp)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"row {row} {est} {interp} B{block} failed with status {r.returncode}: {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["b", "c", "c16"])
    ap.add_argument("--est", choices=ESTIMATORS, default="hetero")
    ap.add_argument("--interp", choices=MODES, default="nearest")
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rows", default="b,c,c16")
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"command": "python scripts/hetero_trilinear_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        for row in args.rows.split(","):
            for est in ESTIMATORS:
                for block in BLOCKS:
                    for interp in MODES:
                        out[f"{row}_{est}_B{block}_{interp}"] = child(args, row, est, interp, block)
                    near, tri = out[f"{row}_{est}_B{block}_nearest"], out[f"{row}_{est}_B{block}_trilinear"]
                    out[f"{row}_{est}_B{block}_ratio"] = round(tri["gpu_ms"] / near["gpu_ms"], 3)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
