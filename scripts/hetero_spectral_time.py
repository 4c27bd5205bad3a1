"""What spectral tracking costs and gains: estimator 16 (VPT_HETERO_SPECTRAL) against estimators 14 (VPT_HETERO_CHROMATIC) and
11 (VPT_HETERO_RATIO) on the timing clouds of scripts/hetero_time.py (rows c16 and c: 16^3 and 64^3; its medium and image
size) and on a finer one (row c128: the same cloud on 128^3 voxels) in the default scene, on the model of
scripts/hetero_chroma_time.py.  Two medium colours: grey (the default multipliers: estimator 16 renders estimator 11's
image) and the coloured set absorption (0.5, 1, 2), scattering (2, 1, 0.5).  Every row under the global majorant and with
local majorants (--blocks, default 0 and 8).
  time rows    <row>_b<block>_<case>, case = e11, e14_coloured, e16_grey, e16_coloured: kernel ms at 1024^2 x 64 spp, GPU events on
               the default stream, best and all of --reps repetitions after one untimed run
  error rows   err_<row>_b<block>: a 256^2 x --ref-spp estimator-14 image of the coloured medium (a seed of its own) as the
               reference, then for each of two seeds a 256^2 x 64 spp image of estimators 14 and 16: kernel ms (best of
               --reps), the per-pixel MSE of the luminance against the reference, and time x MSE
Every row runs in a child process of its own under a timeout, and the driver stops at the first failure.
Prints one JSON line.
usage: python scripts/hetero_spectral_time.py [--reps N] [--size WxH] [--spp N] [--ref-spp N] [--blocks 0,8] [--only time,error]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

import hetero_chroma_time as hc  # noqa: E402  (the colours, the seeds, the luminance)
import hetero_ratio_time as hr  # noqa: E402  (the timed render)
import hetero_time as ht  # noqa: E402  (the grids, the medium)

ROWS = ("c16", "c", "c128")
CASES = {"e11": ("hetero_ratio", "grey"), "e14_coloured": ("hetero_chromatic", "coloured"),
         "e16_grey": ("hetero_spectral", "grey"), "e16_coloured": ("hetero_spectral", "coloured")}
ERR_CASES = ("e14_coloured", "e16_coloured")


def _grid(row):
    if row == "c128":
        return ht.cloud(128), ht.ROOM_LO, ht.ROOM_HI
    return ht.grids(row)


def _tracer(args):
    import minimal_volumetric_path_tracer_amd as vpt

    tr = vpt.Tracer(0)
    rho, lo, hi = _grid(args.step)
    tr.set_density_grid(rho, lo, hi, majorant_block=args.block)
    return vpt, tr, rho


def step_time(args):
    import torch

    w, h = (int(v) for v in args.size.split("x"))
    vpt, tr, rho = _tracer(args)
    est, colour = CASES[args.case]
    tr.set_medium_colour(*hc.COLOURS[colour])
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=est, seed=hc.SEEDS[0], **ht.SIGMA)
    best, ms, out = hr._timed(tr, cfg, args.reps, torch.float32)
    res = {"row": args.step, "block": args.block, "case": args.case, "build_id": vpt.build_id(), "grid": list(rho.shape),
           "gpu_ms": round(best, 3), "gpu_ms_all": [round(x, 3) for x in ms],
           "msamples_per_s": round(w * h * args.spp / best / 1e3, 1),
           "image_mean": [float(v) for v in out.reshape(-1, 3).mean(dim=0)], "image_finite": bool(torch.isfinite(out).all())}
    tr.close()
    print(json.dumps(res))


def step_error(args):
    import torch

    vpt, tr, rho = _tracer(args)
    common = dict(width=hc.ERR_SIZE, height=hc.ERR_SIZE, fp64=True, **ht.SIGMA)
    lum = torch.tensor(hc.LUM, dtype=torch.float64, device="cuda")
    res = {"row": args.step, "block": args.block, "build_id": vpt.build_id(), "grid": list(rho.shape), "size": hc.ERR_SIZE,
           "spp": hc.ERR_SPP, "ref_spp": args.ref_spp, "cases": []}
    tr.set_medium_colour(*hc.COLOURS["coloured"])
    ref = torch.empty((hc.ERR_SIZE, hc.ERR_SIZE, 3), dtype=torch.float64, device="cuda")
    tr.render_device(vpt.RenderConfig(spp=args.ref_spp, estimator="hetero_chromatic", seed=0xC10D5EED, **common), ref.data_ptr())
    torch.cuda.synchronize()
    res["ref_mean"] = [float(v) for v in ref.reshape(-1, 3).mean(dim=0)]
    res["ref_finite"] = bool(torch.isfinite(ref).all())
    for case in ERR_CASES:
        for seed in hc.SEEDS:
            cfg = vpt.RenderConfig(spp=hc.ERR_SPP, estimator=CASES[case][0], seed=seed, **common)
            best, ms, img = hr._timed(tr, cfg, args.reps, torch.float64)
            mse = float((((img - ref) @ lum) ** 2).mean())
            res["cases"].append({"case": case, "seed": seed, "gpu_ms": round(best, 3), "gpu_ms_all": [round(x, 3) for x in ms],
                                 "lum_mse": mse, "ms_x_mse": best * mse, "image_mean": [float(v) for v in img.reshape(-1, 3).mean(dim=0)],
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
    ap.add_argument("--step", choices=ROWS)
    ap.add_argument("--mode", choices=["time", "error"], default="time")
    ap.add_argument("--case", choices=sorted(CASES), default="e16_coloured")
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--blocks", default="0,8")
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--only", default="time,error")
    args = ap.parse_args()
    if args.step:
        return step_time(args) if args.mode == "time" else step_error(args)
    out = {"command": "python scripts/hetero_spectral_time.py " + " ".join(sys.argv[1:]), "size": args.size, "spp": args.spp}
    groups = set(args.only.split(","))
    rows = [r for r in args.rows.split(",") if r]
    blocks = [int(b) for b in args.blocks.split(",")]
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        if "time" in groups:
            for row in rows:
                for block in blocks:
                    for case in CASES:
                        out[f"{row}_b{block}_{case}"] = child(args, ["--step", row, "--block", str(block), "--case", case], 240)
        if "error" in groups:
            for row in rows:
                for block in blocks:
                    out[f"err_{row}_b{block}"] = child(args, ["--step", row, "--block", str(block), "--mode", "error"], 600)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
