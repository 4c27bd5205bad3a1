"""What progressive and adaptive rendering cost and buy, at BASELINE.json configs[1]'s scene (bench.py CONFIGS["ff"]:
1024^2, free flight) with a cap of 256 spp in chunks of 32 (8 levels).  Three runs, timed with GPU events on the
default stream (and the host's wall clock around the same calls), best and all of --reps repetitions after one
untimed run:
  a  the one-shot render: Tracer.render_device(spp 256, chunk_spp 32)
  b  eight all-tile passes of one level each (Accumulator.add(1) x 8), then the resolve
  c  Accumulator.refine at one target, then the resolve; the target comes from --target, or from a scan over a
     grid of targets (step "scan": the one whose mean spp is nearest 55 % of the cap, within 40-70 %)
Each step runs in a child process of its own under a timeout, and the driver stops at the first failure.  Prints one
JSON line.  usage: python scripts/accum_time.py [--target E] [--reps N] [--min-levels M] [--size WxH] [--cap SPP]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 32
SCAN_TARGETS = [2.0 ** (-k / 4) for k in range(0, 33)]  # 1 ... 1/256 in steps of 2^(1/4)


def _timed(work, reps, setup=lambda: None, finish=lambda state: None):
    """work(state) between two events, `reps` times after one untimed run; setup / finish are outside the events"""
    import torch

    ms, wall, last = [], [], None
    for i in range(reps + 1):
        state = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        work(state)
        b.record()
        torch.cuda.synchronize()
        if i > 0:  # the first run pays for buffers and code objects
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(a.elapsed_time(b))
        last = finish(state)
    return {"gpu_ms": round(min(ms), 3), "gpu_ms_all": [round(x, 3) for x in ms], "wall_ms": round(min(wall), 3),
            "wall_ms_all": [round(x, 3) for x in wall]}, last


def step(args):
    import torch

    import minimal_volumetric_path_tracer_amd as vpt
    from bench import CONFIGS

    c = dict(CONFIGS["ff"], spp=args.cap)
    if args.size:
        c["width"], c["height"] = (int(v) for v in args.size.split("x"))
    cfg = vpt.RenderConfig(**c, seed=0x5EED0001, chunk_spp=CHUNK)
    npix = c["width"] * c["height"]
    tr = vpt.Tracer(0)
    out = torch.empty((c["height"], c["width"], 3), dtype=torch.float32, device="cuda")
    res = {"step": args.step, "build_id": vpt.build_id(), "width": c["width"], "height": c["height"], "cap_spp": args.cap,
           "chunk": CHUNK}

    def finish(acc):  # what the accumulator holds, then free it
        info = {"samples": int(acc.spp_map().sum()), "max_tile_err": float(acc.state()["tile_err"].max())}
        acc.close()
        return info

    def accum_run(work):  # the passes and the resolve are timed; creating and reading the accumulator are not
        def timed(acc):
            work(acc)
            acc.resolve_device(out.data_ptr())
        return _timed(timed, args.reps, setup=lambda: tr.accumulator(cfg), finish=finish)

    if args.step == "a":
        t, _ = _timed(lambda _: tr.render_device(cfg, out.data_ptr()), args.reps)
        res.update(t, samples=npix * args.cap)
    elif args.step == "b":
        def passes(acc):
            for _ in range(args.cap // CHUNK):
                acc.add(1)
        t, info = accum_run(passes)
        res.update(t, **info)
    elif args.step == "scan":
        table = []
        for target in SCAN_TARGETS:
            acc = tr.accumulator(cfg)
            rep = acc.refine(target, min_levels=args.min_levels)
            info = finish(acc)
            table.append({"target": target, "mean_spp_frac": round(info["samples"] / (npix * args.cap), 4),
                          "passes": rep["passes"], "max_tile_err": info["max_tile_err"]})
        ok = [r for r in table if 0.40 <= r["mean_spp_frac"] <= 0.70]
        res.update(table=table, target=min(ok, key=lambda r: abs(r["mean_spp_frac"] - 0.55))["target"] if ok else None)
    elif args.step == "c":
        reports = []
        t, info = accum_run(lambda acc: reports.append(acc.refine(args.target, min_levels=args.min_levels)))
        res.update(t, target=args.target, min_levels=args.min_levels, mean_spp=round(info["samples"] / npix, 3),
                   mean_spp_frac=round(info["samples"] / (npix * args.cap), 4), report=reports[-1], **info)
    tr.close()
    print(json.dumps(res))


def child(args, name, extra=(), timeout=300):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps), "--min-levels",
           str(args.min_levels), "--cap", str(args.cap)] + (["--size", args.size] if args.size else []) + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"step {name} failed with status {r.returncode}: {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["a", "b", "c", "scan"])
    ap.add_argument("--target", type=float)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-levels", type=int, default=2)
    ap.add_argument("--size")
    ap.add_argument("--cap", type=int, default=256)
    args = ap.parse_args()
    if args.step:
        return step(args)
    out = {"command": "python scripts/accum_time.py " + " ".join(sys.argv[1:])}
    try:  # the first failure (or timeout) ends the run: nothing more is started on the GPU
        out["a_one_shot"] = child(args, "a")
        out["b_progressive"] = child(args, "b")
        target = args.target
        if target is None:
            out["scan"] = child(args, "scan")
            target = out["scan"]["target"]
            if target is None:
                raise RuntimeError("no target of the scan puts the mean spp between 40 % and 70 % of the cap")
        out["c_adaptive"] = child(args, "c", ["--target", repr(target)])
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        out["error"] = str(e)
        print(json.dumps(out))
        return 1
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
