"""What the grid accumulator (Tracer.grid_accumulator, estimators 10 to 16) costs against the one-shot render of the same
build, on the timing cloud of scripts/hetero_time.py (its row c16: the 16^3 procedural cloud in the room, staged in LDS;
dense medium, 8 bounces) at 1024^2 with N = 64 spp in levels of C = 8.  For estimators 10 and 11, four runs:
  a  the one-shot render: Tracer.render_device(spp = N)
  b  the accumulator adding N / C levels in one call (Accumulator.add(N / C)), then the resolve
  c  the same in N / C calls of one level (Accumulator.add(1) x N / C), then the resolve
  d  Accumulator.refine to a target that stops some tiles early, then the resolve; the target comes from --target, or
     from an untimed scan over a grid of targets (the one whose mean spp is nearest 55 % of the cap, within 40-70 %)
An estimator's four runs share one child process: each is run once untimed (code objects, buffers), then --reps rounds
alternate a, b, c, d, so that a drift of the machine meets all four alike.  Timed with GPU events on the default stream
and with the host's clock around the same calls, which end in a synchronisation; creating and reading the accumulator
are outside the timed window.  b against a is the state traffic (40 B per pixel each way) and the tail kernel; c against
b is N / C - 1 further launches, LDS prologues and synchronisations.  Each child runs under a timeout and the driver stops
at the first failure.  Prints one JSON line.
usage: python scripts/hetero_accum_time.py [--reps N] [--size WxH] [--spp N] [--chunk C] [--target E] [--min-levels M]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ESTIMATORS = ("hetero", "hetero_ratio")
SCAN_TARGETS = [2.0 ** (-k / 4) for k in range(-4, 25)]  # 2 ... 1/64 in steps of 2^(1/4)


def step(args):
    import torch

    import hetero_time as ht
    import minimal_volumetric_path_tracer_amd as vpt

    w, h = (int(v) for v in args.size.split("x"))
    levels = args.spp // args.chunk
    tr = vpt.Tracer(0)
    rho, lo, hi = ht.grids("c16")
    tr.set_density_grid(rho, lo, hi)
    cfg = vpt.RenderConfig(width=w, height=h, spp=args.spp, estimator=args.step, seed=0x5EED0001, **ht.SIGMA)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    res = {"estimator": args.step, "build_id": vpt.build_id(), "width": w, "height": h, "spp": args.spp, "chunk": args.chunk,
           "levels": levels, "grid": list(rho.shape)}

    def info(acc):
        return {"samples": int(acc.spp_map().sum()), "max_tile_err": float(acc.state()["tile_err"].max())}

    target = args.target
    if target is None:  # untimed: the target whose refine spends nearest 55 % of the cap
        table = []
        for t in SCAN_TARGETS:
            acc = tr.grid_accumulator(cfg, chunk=args.chunk)
            rep = acc.refine(t, min_levels=args.min_levels)
            table.append({"target": t, "mean_spp_frac": round(info(acc)["samples"] / (w * h * args.spp), 4), "passes": rep["passes"]})
            acc.close()
        ok = [r for r in table if 0.40 <= r["mean_spp_frac"] <= 0.70]
        res["scan"] = table
        if not ok:
            print(json.dumps(dict(res, error="no target of the scan puts the mean spp between 40 % and 70 % of the cap")))
            return 1
        target = min(ok, key=lambda r: abs(r["mean_spp_frac"] - 0.55))["target"]

    def one_call(acc):
        acc.add(levels)

    def per_level(acc):
        for _ in range(levels):
            acc.add(1)

    reports = []

    def refine(acc):
        reports.append(acc.refine(target, min_levels=args.min_levels))

    runs = {"a_one_shot": None, "b_one_call": one_call, "c_per_level": per_level, "d_refine": refine}
    times = {k: {"gpu_ms_all": [], "wall_ms_all": []} for k in runs}
    images = {}
    for i in range(args.reps + 1):  # round 0 is untimed: it pays for buffers and code objects
        for name, work in runs.items():
            acc = tr.grid_accumulator(cfg, chunk=args.chunk) if work else None
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            if work:
                work(acc)
                acc.resolve_device(out.data_ptr())
            else:
                tr.render_device(cfg, out.data_ptr())
            b.record()
            torch.cuda.synchronize()
            if i > 0:
                times[name]["wall_ms_all"].append(round((time.perf_counter() - t0) * 1e3, 3))
                times[name]["gpu_ms_all"].append(round(a.elapsed_time(b), 3))
            if i == args.reps:
                images[name] = out.clone()
                if work:
                    times[name].update(info(acc))
            if acc:
                acc.close()
    for name, t in times.items():
        t.update(gpu_ms=min(t["gpu_ms_all"]), wall_ms=min(t["wall_ms_all"]))
    npix = w * h
    times["a_one_shot"]["samples"] = npix * args.spp
    times["d_refine"].update(target=target, min_levels=args.min_levels, report=reports[-1],
                             mean_spp_frac=round(times["d_refine"]["samples"] / (npix * args.spp), 4))
    # when results must not change: b and c hold the one-shot render's image, bit for bit
    res["b_equals_a"] = bool(torch.equal(images["b_one_call"], images["a_one_shot"]))
    res["c_equals_a"] = bool(torch.equal(images["c_per_level"], images["a_one_shot"]))
    res["state_bytes_per_pass"] = npix * 40 * 2
    res.update(times)
    tr.close()
    print(json.dumps(res))
    return 0


def child(args, est, timeout=420):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", est, "--reps", str(args.reps), "--size", args.size, "--spp",
           str(args.spp), "--chunk", str(args.chunk), "--min-levels", str(args.min_levels)]
    if args.target is not None:
        cmd += ["--target", repr(args.target)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"estimator {est} failed with status {r.returncode}: {(r.stdout + r.stderr)[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=ESTIMATORS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", default="1024x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--target", type=float)
    ap.add_argument("--min-levels", type=int, default=2)
    args = ap.parse_args()
    if args.spp % args.chunk:
        ap.error("--spp must be a multiple of --chunk")
    if args.step:
        return step(args)
    out = {"command": "python scripts/hetero_accum_time.py " + " ".join(sys.argv[1:])}
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        for est in ESTIMATORS:
            out[est] = child(args, est)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
