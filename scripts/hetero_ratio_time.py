"""Whether ratio tracking pays: estimator 11 (VPT_HETERO_RATIO) against estimator 10 on the grids of
scripts/hetero_time.py (rows b, c, c16; its medium, scene and image size), with the global majorant and with local
majorants on super-voxels of 2 and 8 voxels per axis.
  time rows    <row>_e<10|11>_B<k>: kernel ms at 1024^2 x 64 spp, GPU events on the default stream, best and all of
               --reps repetitions after one untimed run
  error rows   err_<row> for c and c16: a 256^2 x 16 384 spp estimator-10 image (block 0, a seed of its own) as the
               reference, then for each estimator and block a 256^2 x 64 spp image: kernel ms (best of --reps), the
               per-pixel RMSE against the reference over the three channels, and time x MSE, the figure that says
               which estimator reaches an error sooner (the reference's own noise, MSE_10 / 256, is inside every
               MSE alike)
  c128 rows    row c on a 128^3 cloud (the same puffs at twice the resolution; global majorant and B = 8), time only:
               estimator 10's transmittance walks grow with the resolution, estimator 11's do not
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
usage: python scripts/hetero_ratio_time.py [--reps N] [--size WxH] [--spp N] [--ref-spp N] [--only time,error,c128]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import hetero_time as ht  # noqa: E402  (the grids, the medium)

BLOCKS = (0, 2, 8)
ESTIMATORS = {10: "hetero", 11: "hetero_ratio"}
ERR_SIZE, ERR_SPP = 256, 64


def grids(row):
    if row == "c128":
        return ht.cloud(128), ht.ROOM_LO, ht.ROOM_HI
    return ht.grids(row)


def _timed(tr, cfg, reps, dtype):
    """(best ms, all ms, the image) of reps renders after one untimed one"""
    import torch

    out = torch.empty((cfg.height, cfg.width, 3), dtype=dtype, device="cuda")
    ms = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.render_device(cfg, out.data_ptr())
        b.record()
        torch.cuda.synchronize()
        if i > 0:  # the first run pays for buffers and code objects
            ms.append(a.elapsed_time(b))
    return min(ms), ms, out


def step_time(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt

    w, h = (int(v) for v in args.size.split("x"))
    tr = vpt.Tracer(0)
    rho, lo, hi = grids(args.step)
    tr.set_density_grid(rho, lo, hi, majorant_block=args.block)
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=ESTIMATORS[args.est], seed=0x5EED0001, **ht.SIGMA)
    best, ms, out = _timed(tr, cfg, args.reps, torch.float32)
    res = {"row": args.step, "estimator": args.est, "majorant_block": args.block, "build_id": vpt.build_id(),
           "grid": list(rho.shape), "gpu_ms": round(best, 3), "gpu_ms_all": [round(x, 3) for x in ms],
           "msamples_per_s": round(w * h * args.spp / best / 1e3, 1), "image_mean": float(out.mean()),
           "image_finite": bool(torch.isfinite(out).all())}
    tr.close()
    print(json.dumps(res))


def step_error(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt

    tr = vpt.Tracer(0)
    rho, lo, hi = grids(args.step)
    tr.set_density_grid(rho, lo, hi, majorant_block=0)
    common = dict(width=ERR_SIZE, height=ERR_SIZE, fp64=True, **ht.SIGMA)
    ref = torch.empty((ERR_SIZE, ERR_SIZE, 3), dtype=torch.float64, device="cuda")
    tr.render_device(vpt.RenderConfig(spp=args.ref_spp, estimator="hetero", seed=0xC10D5EED, **common), ref.data_ptr())
    torch.cuda.synchronize()
    res = {"row": args.step, "build_id": vpt.build_id(), "grid": list(rho.shape), "size": ERR_SIZE, "spp": ERR_SPP,
           "ref_spp": args.ref_spp, "ref_mean": float(ref.mean()), "ref_finite": bool(torch.isfinite(ref).all()), "cases": []}
    for block in BLOCKS:
        tr.set_majorant_block(block)
        for est, name in ESTIMATORS.items():
            cfg = vpt.RenderConfig(spp=ERR_SPP, estimator=name, seed=0x5EED0001, **common)
            best, ms, img = _timed(tr, cfg, args.reps, torch.float64)
            mse = float(((img - ref) ** 2).mean())
            res["cases"].append({"estimator": est, "majorant_block": block, "gpu_ms": round(best, 3),
                                 "gpu_ms_all": [round(x, 3) for x in ms], "rmse": float(np.sqrt(mse)), "mse": mse,
                                 "ms_x_mse": best * mse, "image_mean": float(img.mean()),
                                 "image_finite": bool(torch.isfinite(img).all())})
    tr.close()
    print(json.dumps(res))


def child(args, extra, timeout):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--size", args.size, "--spp", str(args.spp),
           "--ref-spp", str(args.ref_spp)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(extra)} failed with status {r.returncode}: {r.stderr[-2000:]}")
    print("done:", " ".join(extra), file=sys.stderr, flush=True)  # progress; the result line goes to stdout alone
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["b", "c", "c16", "c128"])
    ap.add_argument("--mode", choices=["time", "error"], default="time")
    ap.add_argument("--est", type=int, choices=sorted(ESTIMATORS), default=11)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--only", default="time,error,c128")
    args = ap.parse_args()
    if args.step:
        return step_time(args) if args.mode == "time" else step_error(args)
    out = {"command": "python scripts/hetero_ratio_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    groups = set(args.only.split(","))
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        if "time" in groups:
            for row in ("b", "c", "c16"):
                for est in ESTIMATORS:
                    for b in BLOCKS:
                        out[f"{row}_e{est}_B{b}"] = child(args, ["--step", row, "--est", str(est), "--block", str(b)], 240)
        if "c128" in groups:
            for est in ESTIMATORS:
                for b in (0, 8):
                    out[f"c128_e{est}_B{b}"] = child(args, ["--step", "c128", "--est", str(est), "--block", str(b)], 240)
        if "error" in groups:
            for row in ("c", "c16"):
                out[f"err_{row}"] = child(args, ["--step", row, "--mode", "error"], 600)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
