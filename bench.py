#!/usr/bin/env python3
"""Benchmark of the hot path: Msamples/s of the volumetric radiance loop on MI355X.

Workload (BASELINE.json configs[1]): the reference's default scene (include/Sphere.cpp:11-22),
camera (src/rt.cpp:755-759) and homogeneous medium (sigma_a 0.001, sigma_s 0.009,
src/rt.cpp:794), free-flight estimator (iterativeVPTracerFree, include/vptShadeMethods.h:1263),
1024 x 1024 pixels x 256 samples per pixel.  One step = one full image: every rank renders its
row bands (interleaved 16-row bands, scaling "strong": the image is fixed, the work is split) with
one launch of pool_kernel (+ the chunk-sum reduce_kernel), then the float32 strips are gathered to
rank 0 over RCCL (N > 1).  Steps are independent images: --inflight D (default 3) keeps D of
them in flight, each on its own context and HIP stream, so that a launch's drain (the last, longest
paths of its last samples, ~0.5 ms) and its gather overlap the next launch (--inflight 1: serialized).
Inputs (the 1.4 KB scene) are resident in HBM before the timed region; nothing is skipped.

A plain run sets up, warms up, times the K steps and prints the result line (value, ms_per_step);
--dump-outputs DIR also writes the last timed step's image to DIR/image.npy.  Everything else is
behind --full:

With --full the line also carries the roofline object (a counting build of the kernel, serialized
launches for the kernel time, the build's committed PMC profile) and, at N > 1, every rank's kernel
time and the gather's.  With --full --config ff (the default config) the same run also measures
BASELINE.json configs[2] -- MIS + HG g=0.5, 1024^2 x 1024 spp, the north-star workload -- and
reports it in the line's "north_star" object next to the reference's MIS rate on this host
(--no-north-star skips it).  The CPU leg of --full (cpu_baseline, rank 0 at N=1; --no-cpu skips it)
times the reference program itself, built from its own sources by oracle/Makefile: with a
per-thread RNG (the fair flavour) and as written; and it checks sampled rows of the GPU image
against the reference's own functions (rmse_vs_reference_per_channel).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config ff|mis|dense|mis4k] [--inflight D]
                    [--dump-outputs DIR] [--full [--no-cpu] [--no-north-star]]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import minimal_volumetric_path_tracer_amd as vpt  # noqa: E402
from minimal_volumetric_path_tracer_amd.distributed import gather_image  # noqa: E402

METRIC = "Msamples/s (pixels×spp/s) at 1024²; per-channel RMSE vs CPU PPM"
FLOP_PER_TEST = 20          # Sphere::intersect, include/Sphere.h:27-37
FP64_PEAK_TFLOPS = 78.6     # MI355X FP64 vector (= FP64 matrix) peak, spec
BAND_ROWS = 16
NORTH_STAR = "mis"          # BASELINE.json configs[2], measured beside the headline config

CONFIGS = {
    # BASELINE.json configs[1]
    "ff": dict(width=1024, height=1024, spp=256, estimator="ff", sigma_a=0.001, sigma_s=0.009),
    # BASELINE.json configs[2] at its own size: 1024^2 x 1024 spp, MIS with HG g = 0.5 (the north-star workload)
    "mis": dict(width=1024, height=1024, spp=1024, estimator="mis", sigma_a=0.001, sigma_s=0.009, hg_g=0.5),
    # BASELINE.json configs[3]: dense medium, 8 bounces.  sigma_t 0.03 (3x the default, albedo 0.9 kept):
    # at SURVEY's proposed 0.1 the ~180 units of fog between the camera (z = 214) and the scene pass
    # exp(-18) = 1.5e-8 of the light and the image is black (mean 1.5e-8); at 0.03 the mean is 6 % of
    # the default scene's and every pixel is lit
    "dense": dict(width=2048, height=2048, spp=4096, estimator="ff", sigma_a=0.003, sigma_s=0.027, max_depth=8),
    # BASELINE.json configs[4]: meant for --gpus 8 (137 G samples per image; ~4 s per step on 8 GPUs)
    "mis4k": dict(width=4096, height=4096, spp=8192, estimator="mis", sigma_a=0.001, sigma_s=0.009),
    # the commented alternatives of main() (src/rt.cpp:791,793) on the one-lane-per-pixel kernel
    # (throughput of estimators 5 and 6; parity cases, not bench lines of the driver)
    "pt": dict(width=1024, height=1024, spp=64, estimator="surface_pt", sigma_a=0.001, sigma_s=0.009),
    "march": dict(width=1024, height=768, spp=4, estimator="ray_marching", sigma_a=0.001, sigma_s=0.0125,
                  march_step=0.1, march_light=8),
}


def cpu_port_check(img: np.ndarray, c: dict, threads: int, bands: int = 12, band: int = 16, ref_rate=None,
                   cal_spp: int = 16) -> dict:
    """The oracle restatement (oracle/liboracle.so: per-sample streams, glibc's libm called directly
    like the reference; built with the reference program's -O3 -march=x86-64-v3, contraction off)
    timed on `bands` bands of `band` camera rows of the bench image, same seed and chunk layout,
    and compared with the GPU image on those rows: per-channel RMSE of the linear float32
    framebuffer (the metric's "per-channel RMSE vs CPU"; the bar is bit-exact, RMSE 0)."""
    from oracle.oracle import Oracle  # cpu_baseline leg only

    H, W, SPP = c["height"], c["width"], c["spp"]
    o = Oracle(portable=False)
    o.set_scene(vpt.default_scene())
    from minimal_volumetric_path_tracer_amd.tracer import ESTIMATORS

    est = ESTIMATORS[c["estimator"]]
    # pinned like the reference program (its OpenMP threads inherit this mask when first created)
    saved = os.sched_getaffinity(0)
    os.sched_setaffinity(0, cpu_topology(threads)["cpus"])
    # calibration on the reference program's own workload (1024 x 768 free flight, all rows)
    t = time.time()
    o.render(1024, 768, cal_spp, 0, seed=0x5EED0001, threads=threads)
    cal = 1024 * 768 * cal_spp / (time.time() - t) / 1e6
    se, n, el = np.zeros(3), 0, 0.0
    for k in range(bands):
        y0 = (H - band) * k // max(bands - 1, 1)
        t = time.time()
        ref = o.render(W, H, SPP, est, sigma_a=c["sigma_a"], sigma_s=c["sigma_s"], hg_g=c.get("hg_g", 0.0),
                       max_depth=c.get("max_depth", 0), seed=0x5EED0001, y0=y0, y1=y0 + band, threads=threads)
        el += time.time() - t
        rows = slice(H - y0 - band, H - y0)  # file rows of camera rows [y0, y0 + band)
        d = img[rows].astype(np.float64) - ref[rows].astype(np.float32).astype(np.float64)
        se += (d * d).reshape(-1, 3).sum(0)
        n += band * W
    os.sched_setaffinity(0, saved)
    res = {"value": bands * band * W * SPP / el / 1e6, "unit": "Msamples/s", "cores": threads, "kind": "port",
           "sample": f"oracle restatement (per-sample erand48 streams, glibc libm), {bands} bands of "
                     f"{band} rows x {W} x {SPP} spp of the bench image, {threads} threads pinned as the reference, "
                     f"{el:.1f}s",
           "rmse_vs_gpu_per_channel": [float(x) for x in np.sqrt(se / n)],
           "calibration": {"value": cal, "workload": f"1024x768x{cal_spp} free flight, all rows, {threads} threads"}}
    if ref_rate:
        res["calibration"]["vs_reference_program"] = round(cal / ref_rate, 3)
    return res


def cpu_topology(threads: int) -> dict:
    """The host's CPU model, socket 0's physical core count, and `threads` CPUs to pin the CPU
    legs to: distinct physical cores of socket 0 (one hardware thread each) among the CPUs this
    process may use.  On the GPU box the job's CPU share is 16 (OMP_NUM_THREADS), less than a socket."""
    import glob

    allowed = sorted(os.sched_getaffinity(0))
    topo = {}
    for d in glob.glob("/sys/devices/system/cpu/cpu[0-9]*"):
        try:
            cpu = int(d.rsplit("cpu", 1)[1])
            pkg = int(open(os.path.join(d, "topology", "physical_package_id")).read())
            core = int(open(os.path.join(d, "topology", "core_id")).read())
        except (OSError, ValueError):
            continue
        topo[cpu] = (pkg, core)
    pkg0 = topo[allowed[0]][0] if allowed and allowed[0] in topo else 0
    socket_cores = len({c for (p, c) in topo.values() if p == pkg0}) or (os.cpu_count() or 1)
    pick, seen = [], set()
    for cpu in allowed:
        pc = topo.get(cpu, (pkg0, cpu))
        if pc[0] == pkg0 and pc[1] not in seen:
            seen.add(pc[1])
            pick.append(cpu)
    if len(pick) < threads:  # not enough distinct cores on socket 0: fill with the other allowed CPUs
        pick += [c for c in allowed if c not in pick]
    model = ""
    try:
        m = re.search(r"model name\s*:\s*(.*)", open("/proc/cpuinfo").read())
        model = m.group(1).strip() if m else ""
    except OSError:
        pass
    return {"cpus": pick[:threads], "socket_physical_cores": socket_cores, "model": model}


def run_reference_program(exe: str, spp: int, cpus: list) -> float:
    """Runs `exe <spp>` (the reference's main, 1024 x 768, src/rt.cpp:752) pinned to `cpus` with one
    OpenMP thread per CPU and returns the elapsed time it prints (src/rt.cpp:824-827; includes its
    serial PPM write).  The affinity is set on this process around the spawn, so the child inherits it."""
    saved = os.sched_getaffinity(0)
    env = dict(os.environ, OMP_NUM_THREADS=str(len(cpus)), OMP_PROC_BIND="close")
    try:
        os.sched_setaffinity(0, cpus)
        with tempfile.TemporaryDirectory() as td:
            r = subprocess.run([exe, str(spp)], cwd=td, capture_output=True, text=True, timeout=300, env=env)
    finally:
        os.sched_setaffinity(0, saved)
    m = re.search(r"elapsed time: ([0-9.eE+-]+)s", r.stdout)
    if r.returncode != 0 or not m:
        raise RuntimeError(f"{exe} {spp}: rc {r.returncode}: {r.stdout[-200:]} {r.stderr[-200:]}")
    return float(m.group(1))


def reference_estimator_rate(est: int, c: dict, cpus: list, rows_per: int = 4, spp: int = 256) -> dict:
    """The reference's own estimator `est` (oracle/_ref/libvpt_ref.so) on len(cpus) cores at once: one
    process per core (oracle/ref_rate.py; the harness drives the reference's global erand48 state),
    each pinned to its core and rendering `rows_per` file rows x width x `spp` samples of the image.
    Rate = all samples / the longest child's render time (the children start within milliseconds
    of each other; their interpreter start-up is outside the timed renders)."""
    H, W = c["height"], c["width"]
    saved = os.sched_getaffinity(0)
    procs = []
    try:
        for k, cpu in enumerate(cpus):
            rows = [(H * (k * rows_per + j)) // (len(cpus) * rows_per) for j in range(rows_per)]
            os.sched_setaffinity(0, [cpu])
            procs.append(subprocess.Popen([sys.executable, "-m", "oracle.ref_rate", str(est), str(W), str(H), str(spp),
                                           repr(c["sigma_a"]), repr(c["sigma_s"])] + [str(r) for r in rows],
                                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                          env=dict(os.environ, OMP_NUM_THREADS="1")))
    finally:
        os.sched_setaffinity(0, saved)
    times = []
    try:
        for p in procs:
            out, err = p.communicate(timeout=300)
            if p.returncode != 0:
                raise RuntimeError(f"oracle.ref_rate rc {p.returncode}: {err[-300:]}")
            times.append(float(out.strip().splitlines()[-1]))
    finally:  # a timeout or a failed child: the others must not keep pinning cores
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    n = len(cpus) * rows_per * W * spp
    return {"value": n / max(times) / 1e6, "cores": len(cpus),
            "sample": f"{len(cpus)} processes, one per core, {rows_per} file rows x {W} x {spp} spp each, "
                      f"renders {min(times):.2f}-{max(times):.2f}s"}


def reference_rows_check(img: np.ndarray, c: dict, rows=(0, 1, 2, 3)) -> dict:
    """Per-channel RMSE of the bench image's file rows `rows` (spread over the image) against the
    reference's own functions (oracle/_ref/libvpt_ref.so: the reference headers compiled in place,
    its pixel loop with the same per-sample erand48 streams), and that sample's single-core rate."""
    from oracle.oracle import Reference  # cpu_baseline leg only

    H, W, SPP = c["height"], c["width"], c["spp"]
    est = {"ff": 0, "mis": 1}[c["estimator"]]
    ref = Reference()
    ref.set_scene(ref.default_scene())
    se, n, el = np.zeros(3), 0, 0.0
    for k in rows:
        fr = (H - 1) * k // max(len(rows) - 1, 1)   # file row
        y = H - 1 - fr                              # camera row
        t = time.time()
        out = ref.render(W, H, SPP, est, c["sigma_a"], c["sigma_s"], seed=0x5EED0001, y0=y, y1=y + 1)
        el += time.time() - t
        d = img[fr].astype(np.float64) - out[fr].astype(np.float32).astype(np.float64)
        se += (d * d).sum(0)
        n += W
    return {"rmse_vs_reference_per_channel": [float(x) for x in np.sqrt(se / n)],
            "reference_rows": f"file rows {[(H - 1) * k // max(len(rows) - 1, 1) for k in rows]} x {W} x {SPP} spp, "
                              "oracle/_ref/libvpt_ref.so (the reference's own functions), one core",
            "reference_one_core_msamples_s": len(rows) * W * SPP / el / 1e6}


def socket_conservative(rates_n, rates_1, cores: int, socket: int) -> float:
    """The CPU socket figure the headline ratios are quoted against: max(fastest `cores`-core run x
    socket / cores, fastest one-core run x socket) -- perfect scaling of one core at worst, and from the
    FASTEST run of each set, so a run slowed by the box's other tenants can only lower the GPU/CPU ratio."""
    return max(max(rates_n) * socket / cores, max(rates_1) * socket)


def cpu_baseline(img: np.ndarray, c: dict, threads: int) -> dict:
    """The reference program on this host's cores, pinned to `threads` physical cores of socket 0:
    oracle/_ref/rt_tls (src/rt.cpp with its erand48 state made per-thread, oracle/ref_tls_rng.h:
    BASELINE.md's fair "per-thread RNG" flavour) at `threads` cores and at one core, and
    oracle/_ref/rt (as written: one erand48 state shared by every thread).  Both are
    built from /root/reference's sources by oracle/Makefile.  Samples are the program's own
    1024 x 768 free-flight image at a reduced spp (~5-10 s each)."""
    topo = cpu_topology(threads)
    cpus = topo["cpus"]
    tls, asis = os.path.join(ROOT, "oracle", "_ref", "rt_tls"), os.path.join(ROOT, "oracle", "_ref", "rt")
    px = 1024 * 768
    spp_n, spp_1, spp_a = 64, 4, 16
    # median of three: the box's other tenants can slow one 2-3 s run by 10-20 % (the socket estimate
    # and the north-star ratio scale with this number)
    runs_n = [run_reference_program(tls, spp_n, cpus) for _ in range(3)]
    runs_1 = [run_reference_program(tls, spp_1, cpus[:1]) for _ in range(3)]
    el_n, el_1 = float(np.median(runs_n)), float(np.median(runs_1))
    el_a = run_reference_program(asis, spp_a, cpus)
    v_n, v_1, v_a = px * spp_n / el_n / 1e6, px * spp_1 / el_1 / 1e6, px * spp_a / el_a / 1e6
    S = topo["socket_physical_cores"]
    res = {
        "value": v_n, "unit": "Msamples/s", "cores": len(cpus), "kind": "reference",
        "sample": f"reference program src/rt.cpp with a per-thread erand48 state (oracle/_ref/rt_tls), "
                  f"`rt_tls {spp_n}` = 1024x768x{spp_n} free-flight, default scene, {len(cpus)} OpenMP threads "
                  f"pinned to {len(cpus)} physical cores of socket 0, elapsed {el_n:.2f}s incl. its PPM write "
                  f"(median of 3 runs: {', '.join(f'{x:.2f}' for x in runs_n)}s)",
        "cpu_model": topo["model"],
        "socket_physical_cores": S,
        "one_core": {"value": v_1, "sample": f"rt_tls {spp_1}, 1 thread, {el_1:.2f}s (median of 3: "
                                             f"{', '.join(f'{x:.2f}' for x in runs_1)}s)"},
        "parallel_efficiency": v_n / (v_1 * len(cpus)),
        "socket_estimate": {"value": v_n * S / len(cpus),
                            "how": f"EXTRAPOLATION, not a measurement: measured {len(cpus)}-core rate x {S}/{len(cpus)} "
                                   f"(the per-thread flavour has no shared state; the job's CPU share is {len(cpus)} "
                                   f"cores, not the socket, so the other {S - len(cpus)} cores cannot be run)"},
        # the FASTEST of the three runs of each: a run slowed by the box's other tenants can only lower
        # this figure's ratio, never raise it
        "socket_estimate_conservative": {
            "value": socket_conservative([px * spp_n / x / 1e6 for x in runs_n], [px * spp_1 / x / 1e6 for x in runs_1],
                                         len(cpus), S),
            "how": f"max(fastest {len(cpus)}-core run x {S}/{len(cpus)}, fastest one-core run x {S}) of the three "
                   f"runs each: the socket at no worse than perfect scaling of one core, with host noise only ever "
                   f"lowering the ratio"},
        "as_written": {"value": v_a, "kind": "reference",
                       "sample": f"oracle/_ref/rt (src/rt.cpp unchanged: one erand48 state shared by all threads, "
                                 f"SURVEY H4), `rt {spp_a}`, {len(cpus)} threads on the same cores, {el_a:.2f}s"},
    }
    res.update(reference_rows_check(img, c))
    return res


PMC_FILES = {"ff": "pmc_pool_kernel.json", "mis": "pmc_pool_kernel_mis.json"}


def pmc_profile(config: str, world: int, build: str):
    """The committed rocprofv3 PMC summary of this same command for the dominant kernel
    (profiles/<round>/pmc_pool_kernel[_mis].json, scripts/pmc.sh + scripts/pmc_summary.py), newest round
    first -- used only when it was collected on THIS library (its build_id equals vpt.build_id()), so
    the counters in the line belong to the code that ran.  Counters cannot be read live without the
    profiler; None when no profile of this build exists."""
    if config not in PMC_FILES or world != 1:
        return None
    import glob

    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", PMC_FILES[config])), reverse=True):
        try:
            prof = json.load(open(f))
        except (OSError, ValueError):
            continue
        if prof.get("build_id") == build:
            prof["path"] = os.path.relpath(f, ROOT)
            return prof
    return None


def pmc_fields(prof, kern_ms: float, fb_bytes: int, partial_bytes: int) -> dict:
    """north_star's 'rocprof-reported achieved HBM GB/s and VALU occupancy' (BASELINE.md:71-75) from the
    build's own PMC profile: HBM GB/s = traffic / the kernel time measured in this run, SIMD VALU busy,
    VALU lane use, and the traffic over the algorithmic bytes (the framebuffer the image needs; the
    chunk partials the design writes on purpose).  Nulls without a profile of this build."""
    t = pmc_traffic(prof)
    der = (prof or {}).get("derived", {})
    return {
        "hbm_gbs": round(t / (kern_ms * 1e-3) / 1e9, 2) if t else None,
        "valu_busy": round(der["simd_valu_busy_frac"], 4) if "simd_valu_busy_frac" in der else None,
        "lane_util": round(der["valu_lane_utilization"], 4) if "valu_lane_utilization" in der else None,
        "traffic_over_framebuffer": round(t / fb_bytes, 2) if t else None,
        "traffic_over_partials": round(t / partial_bytes, 3) if t else None,
        "pmc_profile": (prof or {}).get("path"),
        "pmc_build_id": (prof or {}).get("build_id"),
    }


def fb_bytes(c: dict) -> int:
    """the float32 framebuffer of one image (what the image itself needs written)"""
    return c["width"] * c["height"] * 3 * 4


def partial_bytes(c: dict) -> int:
    """the chunk partials one launch writes (float64 RGB per pixel per chunk, csrc/vpt_chunks.h)"""
    spp = c["spp"]
    C = max(32, (spp + 127) // 128) if spp > 32 else spp
    head = spp - min(spp, 2 * C) if spp > C else spp
    n, rem = -(-head // C), spp - head
    while rem > 0:
        rem -= (rem + 2) // 3
        n += 1
    return c["width"] * c["height"] * 3 * 8 * n


def pmc_traffic(prof):
    """HBM bytes per launch: (2 * FETCH_SIZE + WRITE_SIZE) * 1 KiB -- gfx950 FETCH_SIZE reports half
    of a streamed read (MI355X_MICROARCH.md, HBM)."""
    try:
        c = prof["counters"]
        return int((2 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024)
    except (TypeError, KeyError):
        return None


def pmc_fp64_flop(prof):
    """All FP64 VALU work per launch, from the same profile: (add + mul + 2 fma + trans) wave
    instructions x 64 lanes x VALU lane utilisation (the FLOPS_FP64 counter is not usable on this
    stack).  Reported beside the intersection-only roofline of SURVEY 8(d)."""
    try:
        c = prof["counters"]
        ops = c["SQ_INSTS_VALU_ADD_F64"] + c["SQ_INSTS_VALU_MUL_F64"] + 2 * c["SQ_INSTS_VALU_FMA_F64"] + \
            c["SQ_INSTS_VALU_TRANS_F64"]
        return ops * 64 * prof["derived"]["valu_lane_utilization"]
    except (TypeError, KeyError):
        return None


def measure(c: dict, args, tracers, streams, world: int, rank: int, dev) -> dict:
    """Times args.steps images of config `c` (after args.warmup untimed ones), every rank
    rendering its row bands, strips gathered to rank 0 (N > 1); max over ranks.  Returns the
    whole-job rate and rank 0's image of the last timed step; with --full also the kernel's
    serialized launch time (HIP events on the launch stream), the gather's (N > 1) and the
    ray-sphere tests per sample of the reference algorithm on this workload, each from launches
    of its own outside the timed region."""
    import torch.distributed as tdist

    dist = tdist if world > 1 else None
    H, W, SPP = c["height"], c["width"], c["spp"]
    band = BAND_ROWS if world > 1 else H
    if world > 1 and H % (band * world):
        raise SystemExit("image height must be a multiple of 16 * world size")
    cfg = vpt.RenderConfig(**c, seed=0x5EED0001, band_rows=band, band_stride=world, band_offset=rank,
                           chunk_spp=args.chunk)
    D = len(tracers)
    tracer, stream = tracers[0], streams[0]
    rows = cfg.shard_rows()
    outs = [torch.empty((rows, W, 3), dtype=torch.float32, device=dev) for _ in range(D)]
    images = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) if rank == 0 else None for _ in range(D)]

    # ray-sphere tests per sample of the reference algorithm on this workload (counting build of
    # the same kernel, untimed; 1/16 of the spp -- the per-sample mean is what is needed): --full only
    T = None
    if args.full:
        cnt_cfg = vpt.RenderConfig(**{**c, "spp": max(1, SPP // 16)}, seed=0x5EED0001, band_rows=band,
                                   band_stride=world, band_offset=rank)
        tests, iters = tracer.count_work(cnt_cfg)
        T = tests / (rows * W * cnt_cfg.spp)

    def step(k, ev=None):
        """step k: the whole image on slot k % D -- render the rank's bands, then (N > 1) the RCCL
        gather of the strips to rank 0, all on the slot's stream (the gather of step k overlaps the
        render of step k + 1 on the next slot)"""
        j = k % D
        s = streams[j]
        with torch.cuda.stream(s):
            if ev is not None:
                ev[0].record(s)
            tracers[j].render_device(cfg, outs[j].data_ptr(), s.cuda_stream)
            if ev is not None:
                ev[1].record(s)
            if world > 1:
                # RCCL gather of the strips to rank 0 (gloo, the one-GPU test harness: through host memory)
                strip = outs[j] if args.dist_backend == "nccl" else outs[j].cpu()
                full = gather_image(strip, cfg, band_rows=band)
                if rank == 0:
                    images[j].copy_(full)
            elif rank == 0:
                images[j].copy_(outs[j])

    for k in range(max(args.warmup, D if args.warmup else 0)):
        step(k)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(args.steps if args.full and D == 1 else 0)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, evs[k] if evs else None)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    img = None
    if rank == 0:
        if args.full:
            for j in range(1, min(D, args.steps)):  # every slot rendered the same image
                assert torch.equal(images[j], images[0]), "in-flight slots disagree"
        img = images[(args.steps - 1) % D].float().cpu().numpy()  # what the last timed step computed
    if args.full and D > 1:
        # overlapping launches make per-launch events meaningless: the kernel's duration for the
        # roofline comes from serialized launches of the same render, on one stream, right after
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(min(max(args.steps, 2), 5))]
        for a, b in evs:
            a.record(stream)
            tracer.render_device(cfg, outs[0].data_ptr(), stream.cuda_stream)
            b.record(stream)
        torch.cuda.synchronize(dev)
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in evs])) if args.full else None
    gather_ms = None
    if dist and args.full:
        # the gather alone: all ranks' strips ready (barrier), rank 0's stream timed around the collective
        # and its copy into the image, serialized, a few times (outside the timed region)
        torch.cuda.synchronize(dev)
        dist.barrier()
        gts = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                strip = outs[0] if args.dist_backend == "nccl" else outs[0].cpu()
                full = gather_image(strip, cfg, band_rows=band)
                if rank == 0:
                    images[0].copy_(full)
                b.record(stream)
            torch.cuda.synchronize(dev)
            gts.append(a.elapsed_time(b))
            dist.barrier()
        gather_ms = float(np.median(gts))
    rank_elapsed, rank_kern_ms = [elapsed], [kern_ms]
    if dist:
        tdev = dev if args.dist_backend == "nccl" else torch.device("cpu")
        t = torch.tensor([elapsed, kern_ms or 0.0], dtype=torch.float64, device=tdev)
        every = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        rank_elapsed = [float(x[0].item()) for x in every]
        rank_kern_ms = [float(x[1].item()) for x in every] if args.full else [None] * world
        elapsed = max(rank_elapsed)  # the job's time is the slowest rank's
    launch_samples = rows * W * SPP
    achieved = launch_samples * FLOP_PER_TEST * T / (kern_ms * 1e-3) / 1e12 if args.full else None
    return {"value": H * W * SPP * args.steps / elapsed / 1e6, "elapsed": elapsed, "kern_ms": kern_ms, "T": T,
            "achieved": achieved, "launch_samples": launch_samples, "image": img, "band": band, "D": D,
            "nevents": len(evs), "rank_elapsed": rank_elapsed, "rank_kern_ms": rank_kern_ms, "gather_ms": gather_ms}


def workload_name(c: dict) -> str:
    return (f"{c['estimator']} {c['width']}x{c['height']}x{c['spp']}spp default scene, sigma_a {c['sigma_a']} "
            f"sigma_s {c['sigma_s']}" + (f", HG g {c['hg_g']}" if c.get("hg_g") else "")
            + (f", max depth {c['max_depth']}" if c.get("max_depth") else ""))


def shared_device_refusal(rank_pci: list, shared_device: bool):
    """None when every rank has a GPU of its own (distinct PCI ids) or --shared-device declares a test run;
    otherwise why an N-GPU line must not be printed: N ranks on fewer GPUs would time shared hardware"""
    if shared_device or len(set(rank_pci)) == len(rank_pci):
        return None
    dup = sorted({p for p in rank_pci if rank_pci.count(p) > 1})
    return (f"refusing a {len(rank_pci)}-GPU line: ranks share GPU(s) {', '.join(dup)}; "
            "--shared-device marks such a run as a test")


def _free_port() -> int:
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, cmd: list, env=None, timeout=None) -> int:
    """`bench.py --gpus N` started without a launcher (no WORLD_SIZE in the environment): starts N rank
    processes of `cmd`, one per GPU, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set the way
    `torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` sets them, and waits
    for all of them.  The parent never touches the GPU (no HIP call, no libvpt): the ranks are children
    started by fork + exec of a fresh interpreter, not a re-exec of this process.  Returns 0 when every
    rank exits 0; otherwise the first failing rank's status, after stopping the others -- a failed rank
    fails the run, it never falls back to fewer GPUs.  (The reference's parallelism this replaces: the
    OpenMP row loop, src/rt.cpp:767.)"""
    base = dict(os.environ if env is None else env)
    port = str(_free_port())
    procs = []
    for r in range(n):
        e = dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                 GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(cmd, env=e))
    rc, t0 = 0, time.time()
    pending = list(range(n))
    try:
        while pending:
            for r in list(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.remove(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 128 - code
                    print(f"bench.py: rank {r} exited with status {code}; stopping the other ranks", file=sys.stderr)
                    for q in pending:
                        procs[q].terminate()
            if pending and timeout is not None and time.time() - t0 > timeout:
                print(f"bench.py: ranks {pending} still running after {timeout}s; stopping them", file=sys.stderr)
                for q in pending:
                    procs[q].kill()
                rc = rc or 124
            if pending:
                time.sleep(0.05)
    finally:
        # an exception or ^C in the launcher must not orphan ranks that hold GPUs and a rendezvous:
        # terminate what still runs, then kill what ignores it (exactly these child PIDs)
        live = [p for p in procs if p.poll() is None]
        for p in live:
            p.terminate()
        t1 = time.time()
        for p in live:
            try:
                p.wait(timeout=max(0.1, 10 - (time.time() - t1)))
            except subprocess.TimeoutExpired:
                p.kill()
        for p in procs:
            p.wait()
    return rc


DUMP_LIMIT = 60_000_000  # bytes of array data --dump-outputs writes at most (64 MB with room to spare)


def dump_outputs(directory: str, img: np.ndarray) -> None:
    """--dump-outputs: the float32 image (file rows x width x RGB) that rank 0 holds after the last timed
    step -- what a caller of the timed path receives -- as <directory>/image.npy.  The inputs are fixed
    (scene, camera, medium, seed 0x5EED0001), so two builds run with the same arguments write comparable
    files.  An image above DUMP_LIMIT is written as a sample of whole rows: the sorted choice of a
    generator seeded with a constant, the same rows in every run."""
    os.makedirs(directory, exist_ok=True)
    img = np.ascontiguousarray(img, dtype=np.float32)
    keep = DUMP_LIMIT // max(1, img[0].nbytes)
    if keep < img.shape[0]:
        img = img[np.sort(np.random.default_rng(0x5EED0001).choice(img.shape[0], size=keep, replace=False))]
    np.save(os.path.join(directory, "image.npy"), img)


def roofline(m: dict, c: dict, prof, D: int) -> dict:
    """The line's `roofline` object (--full): the reference-equivalent intersection flops over the kernel's
    serialized launch time, and what the build's PMC profile adds (pmc_fields, pmc_fp64_flop)"""
    kern_ms, T = m["kern_ms"], m["T"]
    full = pmc_fp64_flop(prof)
    return {
        "bound": "fp64_valu",
        "achieved": round(m["achieved"], 4),
        "peak": FP64_PEAK_TFLOPS,
        "unit": "TFLOP/s",
        "frac": round(m["achieved"] / FP64_PEAK_TFLOPS, 5),
        "peak_no_fma": FP64_PEAK_TFLOPS / 2,
        "frac_of_no_fma_peak": round(m["achieved"] / (FP64_PEAK_TFLOPS / 2), 5),
        "traffic": pmc_traffic(prof),
        **pmc_fields(prof, kern_ms, fb_bytes(c), partial_bytes(c)),
        "kernel": (f"pool_kernel<{c['estimator']}> + reduce_kernel (one launch pair)"
                   if c["estimator"] not in ("ray_marching",) else "render_kernel_simple (one lane per pixel)"),
        "kernel_ms": round(kern_ms, 3),
        "kernel_ms_from": "HIP events around each launch of the timed steps on their stream" if D == 1 else
                          f"HIP events around {m['nevents']} serialized launches of the same render on one stream, "
                          f"right after the timed region (its {D} in-flight steps overlap)",
        "work_basis": "reference-equivalent: the ray-sphere tests the REFERENCE algorithm performs on this "
                      "workload (counting build), including the tests of rays the kernel's exact shortcuts "
                      "never cast (pLight toward a sphere light, MISv2's BSDF ray, the H5 point-light cone); "
                      "achieved/frac are therefore not executed FP64 work -- all_fp64_* is",
        "algorithmic": f"{FLOP_PER_TEST} FP64 flop x {T:.2f} ray-sphere tests per sample (SURVEY 8d) x "
                       f"{m['launch_samples']} samples per launch",
        "all_fp64_tflops": round(full / (kern_ms * 1e-3) / 1e12, 3) if full else None,
        "all_fp64_frac": round(full / (kern_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, 4) if full else None,
        "note": "FP64 VALU bound (no dense contraction exists, no MFMA): peak 78.6 TFLOP/s counts an FMA as "
                "2 flop; the path runs with contraction off (the reference's rounding), so 39.3 TFLOP/s "
                "(peak_no_fma) is the ceiling for its separately rounded mul/add. achieved/frac count "
                "intersection flops only (SURVEY 8d); all_fp64_*, traffic, hbm_gbs, valu_busy and lane_util "
                "come from the committed PMC profile of this command collected on this build "
                "(pmc_profile, pmc_build_id == build_id; null when none exists); traffic_over_* divide "
                "the HBM bytes by the float32 framebuffer and by the chunk partials the design writes",
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="ff", choices=list(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure: the roofline (counting build, serialized kernel launches, "
                         "the build's PMC profile), the per-rank kernel and gather times (N > 1), the north-star "
                         "workload (--config ff) and the CPU baseline (N = 1); a plain run does none of these")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-north-star", action="store_true",
                    help="with --full: skip the second measurement of BASELINE.json configs[2] (the north-star workload)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes what the last timed step computed to DIR/image.npy (float32 H x W x 3; "
                         "above 64 MB a fixed, seeded sample of its rows)")
    ap.add_argument("--chunk", type=int, default=0, help="samples per work unit (0 = auto: 32, more above 4096 spp, tapered; vpt_chunks.h)")
    ap.add_argument("--inflight", type=int, default=3,
                    help="steps in flight: each on its own context + HIP stream, so one launch's drain (its "
                         "last, longest paths) overlaps the next launch's start; 1 = strictly serialized")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend for N > 1 (nccl = RCCL over xGMI; gloo stages the strips "
                         "through host memory -- for the one-GPU multi-process tests only)")
    ap.add_argument("--shared-device", action="store_true",
                    help="every rank renders on cuda:0 (multi-process tests on a one-GPU box; needs gloo)")
    ap.add_argument("--size", default=None, help="WxHxSPP override of the config's image (parity tests)")
    ap.add_argument("--save-image", default=None, help="rank 0 writes the last image (float32 .npy) here")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.shared_device and args.dist_backend != "gloo":
        raise SystemExit("--shared-device needs --dist-backend gloo (RCCL wants one GPU per rank)")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: start one rank per GPU here.  torch.cuda.device_count() does not initialise HIP
        # on this image; the ranks check again after they start.
        ndev = torch.cuda.device_count()
        if args.gpus > ndev and not args.shared_device:
            print(f"bench.py: --gpus {args.gpus} but this node has {ndev} GPU(s); refusing to run on fewer",
                  file=sys.stderr)
            sys.exit(2)
        sys.exit(launch_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if not args.shared_device and world > torch.cuda.device_count():
        print(f"bench.py: WORLD_SIZE={world} but this node has {torch.cuda.device_count()} GPU(s)", file=sys.stderr)
        sys.exit(2)
    dist = None
    devi = 0 if args.shared_device else local
    torch.cuda.set_device(devi)
    dev = torch.device("cuda", devi)
    if world > 1:
        import torch.distributed as dist

        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
        if dist.get_world_size() != args.gpus:
            print(f"bench.py: the process group has {dist.get_world_size()} ranks, --gpus {args.gpus}", file=sys.stderr)
            sys.exit(2)

    # what each rank runs on, as the process group reports it (one line per rank, rank order); N ranks on
    # fewer distinct GPUs than N (a repeated PCI id) cannot give an N-GPU line unless --shared-device says so
    props = torch.cuda.get_device_properties(dev)
    pci = f"{getattr(props, 'pci_domain_id', 0):04x}:{getattr(props, 'pci_bus_id', 0):02x}:" \
          f"{getattr(props, 'pci_device_id', 0):02x}"
    me = f"rank {rank}: cuda:{dev.index} ({props.name}, PCI {pci})"
    rank_devices, rank_pci = [me], [pci]
    if dist:
        rank_devices, rank_pci = [None] * world, [None] * world
        dist.all_gather_object(rank_devices, me)
        dist.all_gather_object(rank_pci, pci)
    why = shared_device_refusal(rank_pci, args.shared_device)
    if why:
        if rank == 0:
            print(f"bench.py: {why} ({rank_devices})", file=sys.stderr)
        sys.exit(2)

    c = dict(CONFIGS[args.config])
    if args.size:
        w, h, s = (int(v) for v in args.size.lower().split("x"))
        c.update(width=w, height=h, spp=s)
    D = max(1, args.inflight)
    tracers = [vpt.Tracer(dev.index) for _ in range(D)]  # one context per slot (each its own stream state)
    streams = [torch.cuda.current_stream(dev)] if D == 1 else [torch.cuda.Stream(dev) for _ in range(D)]
    m = measure(c, args, tracers, streams, world, rank, dev)
    ns = None
    if args.full and args.config == "ff" and not args.no_north_star:
        ns = measure(CONFIGS[NORTH_STAR], args, tracers, streams, world, rank, dev)
    build = vpt.build_id()
    if rank == 0 and args.save_image:
        np.save(args.save_image, m["image"])
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, m["image"])
    if rank == 0:
        img = m["image"]
        H, W, SPP = c["height"], c["width"], c["spp"]
        res = {
            "metric": METRIC,
            "value": round(m["value"], 3),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "full": bool(args.full),
            "ms_per_step": round(m["elapsed"] / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic: the reference's default scene/camera/medium, per-sample erand48 streams (seed 0x5EED0001)",
            "config": {
                "workload": workload_name(c),
                "width": W, "height": H, "spp": SPP, "estimator": c["estimator"],
                "parallelism": f"row bands of {m['band']} interleaved over {world} GPU(s), RCCL gather to rank 0"
                if world > 1 else "1 GPU",
                "inflight": D,
                "process_group": {"backend": args.dist_backend if world > 1 else None,
                                  "world_size": dist.get_world_size() if dist else 1,
                                  "rank_devices": rank_devices,
                                  "rank_elapsed_s": [round(x, 6) for x in m["rank_elapsed"]],
                                  # each rank's serialized launch time of its shard (HIP events on its launch
                                  # stream) and rank 0's gather of one image's strips, timed serialized after
                                  # a barrier: imbalance and an exposed gather show here, not in `value`
                                  # (--full; null in a plain run)
                                  "rank_kernel_ms": [round(x, 4) for x in m["rank_kern_ms"]] if args.full else None,
                                  "gather_ms": None if m["gather_ms"] is None else round(m["gather_ms"], 4),
                                  "shared_device": bool(args.shared_device)},
            },
            "image_mean": [round(float(x), 6) for x in img.reshape(-1, 3).mean(0)],
            "build_id": build,
        }
        if args.full:
            res["roofline"] = roofline(m, c, None if args.size else pmc_profile(args.config, world, build), D)
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
        if args.full and world == 1 and not args.no_cpu:
            res["cpu_baseline"] = cpu_baseline(img, c, threads)
            res["cpu_baseline"]["port_per_sample_rng"] = cpu_port_check(img, c, threads, bands=4,
                                                                         ref_rate=res["cpu_baseline"]["value"])
            cb0 = res["cpu_baseline"]
            # ratios of this line's value to the reference program (vs_baseline stays null: BASELINE.md
            # holds no published number for this metric)
            cb0["speedup_vs_measured"] = round(m["value"] / cb0["value"], 1)
            cb0["speedup_vs_socket_estimate"] = round(m["value"] / cb0["socket_estimate"]["value"], 1)
            cb0["speedup_vs_cpu_socket_conservative"] = round(m["value"] / cb0["socket_estimate_conservative"]["value"], 1)
        if ns is not None:
            cn = CONFIGS[NORTH_STAR]
            o = {"workload": workload_name(cn) + " (BASELINE.json configs[2])",
                 "value": round(ns["value"], 3), "unit": "Msamples/s",
                 "ms_per_step": round(ns["elapsed"] / args.steps * 1e3, 3),
                 "kernel_ms": round(ns["kern_ms"], 3),
                 "tests_per_sample": round(ns["T"], 3),
                 "roofline_frac": round(ns["achieved"] / FP64_PEAK_TFLOPS, 5),
                 "pmc": pmc_fields(pmc_profile(NORTH_STAR, world, build), ns["kern_ms"], fb_bytes(cn),
                                   partial_bytes(cn)),
                 "image_mean": [round(float(x), 6) for x in ns["image"].reshape(-1, 3).mean(0)]}
            cb = res.get("cpu_baseline")
            if cb:
                # the reference's own MIS estimator (MISVPTTracerRecursive, isotropic phase: HG is an
                # extension) on rows of this image: measured on the job's cores (one process per core),
                # then scaled to the socket like the FF figure; the one-core rate beside it
                from oracle.oracle import Reference  # cpu_baseline leg only

                ref = Reference()
                ref.set_scene(ref.default_scene())
                topo = cpu_topology(threads)
                saved = os.sched_getaffinity(0)
                os.sched_setaffinity(0, topo["cpus"][:1])
                one = []
                try:
                    for _ in range(3):  # median of 3 one-core samples (8 rows x 1024 x 64 spp, ~0.4 s each)
                        t = time.time()
                        ref.render(cn["width"], cn["height"], 64, 1, cn["sigma_a"], cn["sigma_s"], seed=0x5EED0001,
                                   y0=508, y1=516)
                        one.append(8 * cn["width"] * 64 / (time.time() - t) / 1e6)
                finally:
                    os.sched_setaffinity(0, saved)
                mis1 = float(np.median(one))
                runs = [reference_estimator_rate(1, cn, topo["cpus"]) for _ in range(3)]
                misn = sorted(runs, key=lambda r: r["value"])[1]  # median of 3 runs on the job's cores
                misn["runs"] = [round(r["value"], 3) for r in runs]
                S = cb["socket_physical_cores"]
                sock = misn["value"] * S / misn["cores"]
                # fastest of the three runs of each (host noise can only lower the conservative ratio)
                sock_c = socket_conservative([r["value"] for r in runs], one, misn["cores"], S)
                o["cpu_reference"] = {"measured": misn, "one_core": mis1, "one_core_runs": [round(x, 4) for x in one],
                                      "parallel_efficiency": misn["value"] / (mis1 * misn["cores"]),
                                      "socket_estimate": sock,
                                      "socket_estimate_conservative": sock_c,
                                      "how": f"reference MISVPTTracerRecursive (oracle/_ref/libvpt_ref.so) measured on "
                                             f"{misn['cores']} cores x {S}/{misn['cores']}: an EXTRAPOLATION to the "
                                             f"{S}-core socket (the job has {misn['cores']} cores, not the socket); the "
                                             f"conservative estimate is max(fastest {misn['cores']}-core run x "
                                             f"{S}/{misn['cores']}, fastest one-core run x {S}) over the three runs "
                                             f"each, i.e. never below perfect scaling of one core",
                                      "phase": "the CPU side runs the reference's ISOTROPIC phase (it has no HG); the "
                                               "GPU side runs HG g=0.5 (the north-star extension, g=0 reduces to "
                                               "the reference bit for bit)"}
                o["speedup_vs_cpu_socket"] = round(ns["value"] / sock, 1)
                o["speedup_vs_cpu_socket_conservative"] = round(ns["value"] / sock_c, 1)
                o["target_speedup"] = 100
            res["north_star"] = o
        print(json.dumps(res))
    for t in tracers:
        t.close()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
