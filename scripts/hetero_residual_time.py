"""Whether residual ratio tracking pays: estimator 15 (VPT_HETERO_RESIDUAL) against estimators 10 and 11 at the same
majorant block, on the timing clouds of scripts/hetero_time.py (rows c and c16; its medium, scene and image size) and on
each of them over a density floor (cloud + 0.25 rho_max: rows cf and c16f -- the case the estimator is for), with blocks
of 2, 4 and 8 voxels per axis, nearest and trilinear lookup.
  per field and lookup, one child process:
    time   e<10|11|15>_B<k>: kernel ms at 1024^2 x 64 spp, GPU events on the default stream, best and all of --reps
           repetitions after one untimed run
    error  a 256^2 x --ref-spp estimator-10 image (block 0, a seed of its own) as the reference, then for each estimator
           and block a 256^2 x 64 spp image: kernel ms (best of --reps), the per-pixel MSE against the reference over
           the three channels, and time x MSE, the figure that says which estimator reaches an error sooner (the
           reference's own noise, MSE_10 x 64 / ref-spp, is inside every MSE alike)
  --variant-lib PATH: estimator 15's time rows once more on another build of the library (the out-of-line walker,
           -DVPT_RESIDUAL_NOINLINE=1), this build and the variant in a child each, one after the other
Every child runs under a timeout, and the driver stops at the first failure.  Prints one JSON line.
usage: python scripts/hetero_residual_time.py [--reps N] [--size WxH] [--spp N] [--ref-spp N] [--fields c,cf,c16,c16f]
       [--interps nearest,trilinear] [--only time,error] [--variant-lib PATH]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import hetero_time as ht  # noqa: E402  (the clouds, the medium)

BLOCKS = (2, 4, 8)
ESTIMATORS = {10: "hetero", 11: "hetero_ratio", 15: "hetero_residual"}
FIELDS = ("c", "cf", "c16", "c16f")
ERR_SIZE, ERR_SPP = 256, 64


def field(name):
    """the cloud of hetero_time's row c or c16; with the suffix f on a floor of a quarter of its maximum"""
    rho, lo, hi = ht.grids(name.rstrip("f"))
    if name.endswith("f"):
        rho = (rho + np.float32(0.25) * rho.max()).astype(np.float32)
    return rho, lo, hi


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


def step(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt

    w, h = (int(v) for v in args.size.split("x"))
    ests = [int(e) for e in args.ests.split(",")]
    tr = vpt.Tracer(0)
    rho, lo, hi = field(args.step)
    tr.set_density_grid(rho, lo, hi, majorant_block=0, interpolation=args.interp)
    res = {"field": args.step, "interpolation": args.interp, "build_id": vpt.build_id(), "lib": os.path.relpath(os.environ["VPT_LIB"], ROOT) if os.environ.get("VPT_LIB") else "",
           "grid": list(rho.shape), "rho_min": float(rho.min()), "rho_max": float(rho.max()), "rho_mean": float(rho.mean())}
    groups = set(args.only.split(","))
    if "time" in groups:
        res["time"] = []
        for block in BLOCKS:
            tr.set_majorant_block(block)
            for est in ests:
                cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=ESTIMATORS[est], seed=0x5EED0001, **ht.SIGMA)
                best, ms, out = _timed(tr, cfg, args.reps, torch.float32)
                res["time"].append({"estimator": est, "majorant_block": block, "gpu_ms": round(best, 3),
                                    "gpu_ms_all": [round(x, 3) for x in ms],
                                    "msamples_per_s": round(w * h * args.spp / best / 1e3, 1),
                                    "image_mean": float(out.mean()), "image_finite": bool(torch.isfinite(out).all())})
    if "error" in groups:
        tr.set_majorant_block(0)
        common = dict(width=ERR_SIZE, height=ERR_SIZE, fp64=True, **ht.SIGMA)
        ref = torch.empty((ERR_SIZE, ERR_SIZE, 3), dtype=torch.float64, device="cuda")
        tr.render_device(vpt.RenderConfig(spp=args.ref_spp, estimator="hetero", seed=0xC10D5EED, **common), ref.data_ptr())
        torch.cuda.synchronize()
        res.update({"size": ERR_SIZE, "spp": ERR_SPP, "ref_spp": args.ref_spp, "ref_mean": float(ref.mean()),
                    "ref_finite": bool(torch.isfinite(ref).all()), "error": []})
        for block in BLOCKS:
            tr.set_majorant_block(block)
            for est in ests:
                cfg = vpt.RenderConfig(spp=ERR_SPP, estimator=ESTIMATORS[est], seed=0x5EED0001, **common)
                best, ms, img = _timed(tr, cfg, args.reps, torch.float64)
                mse = float(((img - ref) ** 2).mean())
                res["error"].append({"estimator": est, "majorant_block": block, "gpu_ms": round(best, 3),
                                     "gpu_ms_all": [round(x, 3) for x in ms], "rmse": float(np.sqrt(mse)), "mse": mse,
                                     "ms_x_mse": best * mse, "image_mean": float(img.mean()),
                                     "image_finite": bool(torch.isfinite(img).all())})
    tr.close()
    print(json.dumps(res))


def child(args, extra, timeout, lib=None):
    env = dict(os.environ)
    env.pop("VPT_SIMPLE_KERNEL", None)
    if lib:
        env["VPT_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--size", args.size, "--spp", str(args.spp),
           "--ref-spp", str(args.ref_spp)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(extra)} failed with status {r.returncode}: {r.stderr[-2000:]}")
    print("done:", " ".join(extra), lib or "", file=sys.stderr, flush=True)  # progress; the result line goes to stdout alone
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=FIELDS)
    ap.add_argument("--interp", choices=["nearest", "trilinear"], default="nearest")
    ap.add_argument("--ests", default="10,11,15")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--fields", default=",".join(FIELDS))
    ap.add_argument("--interps", default="nearest,trilinear")
    ap.add_argument("--only", default="time,error")
    ap.add_argument("--variant-lib", default="")
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"command": "python scripts/hetero_residual_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        for name in args.fields.split(","):
            for interp in args.interps.split(","):
                out[f"{name}_{interp}"] = child(args, ["--step", name, "--interp", interp, "--only", args.only], 900)
                if args.variant_lib:  # estimator 15 alone, this build and the variant in turn
                    extra = ["--step", name, "--interp", interp, "--only", "time", "--ests", "15"]
                    out[f"{name}_{interp}_e15_again"] = child(args, extra, 600)
                    out[f"{name}_{interp}_e15_variant"] = child(args, extra, 600, args.variant_lib)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
