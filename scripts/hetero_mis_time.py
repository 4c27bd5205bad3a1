"""What the one-sample combination of delta tracking and equi-angular sampling costs and buys: estimator 13
(VPT_HETERO_MIS) at the track fraction --q against estimators 10 and 12 on the grids of scripts/hetero_time.py (rows b, c16,
c; its medium and image size) in the default scene, on the model of scripts/hetero_eqa_time.py.
  time rows    <row>_e<10|12|13>: kernel ms at 1024^2 x 64 spp, GPU events on the default stream, best and all of --reps
               repetitions after one untimed run
  error rows   err_<row>: a 256^2 x --ref-spp estimator-10 image (a seed of its own) as the reference, then for each
               estimator and each of two seeds a 256^2 x 64 spp image: kernel ms (best of --reps), the per-pixel RMSE
               against the reference over the three channels, and time x MSE
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
usage: python scripts/hetero_mis_time.py [--q Q] [--reps N] [--size WxH] [--spp N] [--ref-spp N] [--only time,error]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import hetero_ratio_time as hr  # noqa: E402  (the timed render)
import hetero_time as ht  # noqa: E402  (the grids, the medium)

ROWS = ("b", "c16", "c")
ESTIMATORS = {10: "hetero", 12: "hetero_equiangular", 13: "hetero_mis"}
ERR_SIZE, ERR_SPP = 256, 64
SEEDS = (0x5EED0001, 0x5EED0002)


def _tracer(args):
    import minimal_volumetric_path_tracer_amd as vpt

    tr = vpt.Tracer(0)
    rho, lo, hi = ht.grids(args.step)
    tr.set_density_grid(rho, lo, hi)
    tr.set_hetero_mis_fraction(args.q)
    return vpt, tr, rho


def step_time(args):
    import torch

    w, h = (int(v) for v in args.size.split("x"))
    vpt, tr, rho = _tracer(args)
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=ESTIMATORS[args.est], seed=SEEDS[0], **ht.SIGMA)
    best, ms, out = hr._timed(tr, cfg, args.reps, torch.float32)
    res = {"row": args.step, "estimator": args.est, "q": args.q, "build_id": vpt.build_id(), "grid": list(rho.shape),
           "gpu_ms": round(best, 3), "gpu_ms_all": [round(x, 3) for x in ms],
           "msamples_per_s": round(w * h * args.spp / best / 1e3, 1), "image_mean": float(out.mean()),
           "image_finite": bool(torch.isfinite(out).all())}
    tr.close()
    print(json.dumps(res))


def step_error(args):
    import torch

    vpt, tr, rho = _tracer(args)
    common = dict(width=ERR_SIZE, height=ERR_SIZE, fp64=True, **ht.SIGMA)
    ref = torch.empty((ERR_SIZE, ERR_SIZE, 3), dtype=torch.float64, device="cuda")
    tr.render_device(vpt.RenderConfig(spp=args.ref_spp, estimator="hetero", seed=0xC10D5EED, **common), ref.data_ptr())
    torch.cuda.synchronize()
    res = {"row": args.step, "q": args.q, "build_id": vpt.build_id(), "grid": list(rho.shape), "size": ERR_SIZE,
           "spp": ERR_SPP, "ref_spp": args.ref_spp, "ref_mean": float(ref.mean()),
           "ref_finite": bool(torch.isfinite(ref).all()), "cases": []}
    for est, name in ESTIMATORS.items():
        for seed in SEEDS:
            cfg = vpt.RenderConfig(spp=ERR_SPP, estimator=name, seed=seed, **common)
            best, ms, img = hr._timed(tr, cfg, args.reps, torch.float64)
            mse = float(((img - ref) ** 2).mean())
            res["cases"].append({"estimator": est, "seed": seed, "gpu_ms": round(best, 3),
                                 "gpu_ms_all": [round(x, 3) for x in ms], "rmse": float(np.sqrt(mse)), "mse": mse,
                                 "ms_x_mse": best * mse, "image_mean": float(img.mean()),
                                 "image_max": float(img.max()), "image_finite": bool(torch.isfinite(img).all())})
    tr.close()
    print(json.dumps(res))


def child(args, extra, timeout):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--q", str(args.q), "--reps", str(args.reps), "--size", args.size,
           "--spp", str(args.spp), "--ref-spp", str(args.ref_spp)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(extra)} failed with status {r.returncode}: {r.stderr[-2000:]}")
    print("done:", " ".join(extra), file=sys.stderr, flush=True)  # progress; the result line goes to stdout alone
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=ROWS)
    ap.add_argument("--mode", choices=["time", "error"], default="time")
    ap.add_argument("--est", type=int, choices=sorted(ESTIMATORS), default=13)
    ap.add_argument("--q", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--only", default="time,error")
    args = ap.parse_args()
    if args.step:
        return step_time(args) if args.mode == "time" else step_error(args)
    out = {"command": "python scripts/hetero_mis_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp,
           "q": args.q}
    groups = set(args.only.split(","))
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        if "time" in groups:
            for row in ROWS:
                for est in ESTIMATORS:
                    out[f"{row}_e{est}"] = child(args, ["--step", row, "--est", str(est)], 240)
        if "error" in groups:
            for row in ROWS:
                out[f"err_{row}"] = child(args, ["--step", row, "--mode", "error"], 600)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
