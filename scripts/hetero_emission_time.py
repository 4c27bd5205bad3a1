"""What volumetric emission (Tracer.set_emission_grid, csrc/vpt_grid.h) costs: rows (c) and (c16) of
scripts/hetero_time.py -- the 64^3 and the 16^3 cloud -- at 1024^2 x 64 spp in the dense medium, for estimators 10
("hetero") and 11 ("hetero_ratio"), without and with an emission grid (the cloud's own density, squared and scaled:
the dense cores glow).  GPU events on the default stream, best and all of --reps repetitions after one untimed run,
and the spread (max - min) / min of the repetitions.  Every figure is a measurement: no threshold.
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
usage: python scripts/hetero_emission_time.py [--reps N] [--size WxH] [--spp N] [--rows c,c16] [--block B]
       [--interp nearest|trilinear]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import hetero_time as ht  # noqa: E402  (the grids and the medium of that table)

ESTIMATORS = ("hetero", "hetero_ratio")
RGB = (1.0, 0.55, 0.2)


def emission_of(rho):
    r = rho.astype(np.float64) / float(rho.max())
    return (40.0 * r * r).astype(np.float32)


def step(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt

    w, h = (int(v) for v in args.size.split("x"))
    rho, lo, hi = ht.grids(args.step)
    tr = vpt.Tracer(0)
    tr.set_density_grid(rho, lo, hi, majorant_block=args.block, interpolation=args.interp)
    if args.emission:
        tr.set_emission_grid(emission_of(rho), RGB)
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=args.est, seed=0x5EED0001, **ht.SIGMA)
    res = {"row": args.step, "estimator": args.est, "emission": bool(args.emission), "interpolation": args.interp,
           "majorant_block": args.block, "build_id": vpt.build_id(), "grid": list(rho.shape)}
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
               spread=round((max(ms) - min(ms)) / min(ms), 5), image_mean=float(out.mean()),
               image_finite=bool(torch.isfinite(out).all()))
    tr.close()
    print(json.dumps(res))


def child(args, row, est, emission, timeout=300):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--step", row, "--est", est, "--emission", str(int(emission)),
           "--block", str(args.block), "--interp", args.interp, "--reps", str(args.reps), "--size", args.size,
           "--spp", str(args.spp)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"row {row} {est} emission {int(emission)} failed with status {r.returncode}: {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["c", "c16"])
    ap.add_argument("--est", choices=ESTIMATORS, default="hetero")
    ap.add_argument("--emission", type=int, default=0)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--interp", choices=["nearest", "trilinear"], default="nearest")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rows", default="c,c16")
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"command": "python scripts/hetero_emission_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        for row in args.rows.split(","):
            for est in ESTIMATORS:
                for emission in (False, True):
                    out[f"{row}_{est}_{'emission' if emission else 'plain'}"] = child(args, row, est, emission)
                plain, lit = out[f"{row}_{est}_plain"], out[f"{row}_{est}_emission"]
                out[f"{row}_{est}_ratio"] = round(lit["gpu_ms"] / plain["gpu_ms"], 3)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
