#!/usr/bin/env python3
"""Throughput of Guo-Hall thinning on the GPU (va_thinning.hip):
  resident  va_guo_hall_thinning_batch, inputs and outputs resident in HBM, HIP events around the call: 4096
            worm-sized masks (~100 x 40) in one call, and 64 masks at the resident limit (480 x 1024 blobs)
  single    the same worm masks through 4096 ops.guo_hall_thinning([mask]) calls, wall time on the host
  tiled     va_guo_hall_thinning_u8 on a 16 x 1080p stack of blob masks (and on one frame), for several K
            (sub-iterations per launch) and M (launches per host read): iterations, launches, host reads, and
            the bytes one launch moves (every tile's 64 x 16-word window read, every word written once)
            against the packed planes' size; the 64 at-limit masks go through it as well
  context   one 1080p frame through va_mask_thinning_u8 (the cross-erosion fallback: a different algorithm, so
            no speed claim), and the NumPy restatement of one 1080p frame on one core
With --kernels the resident and tiled legs run again in a child process under `rocprofv3 --kernel-trace --stats`
and the time is split per kernel.  Rates come from the median of the repetitions.  One JSON line per leg, appended to profiles/thinning_bench.jsonl (or --out).
Run on an MI355X:
    python tools/bench_thinning.py [--reps 15] [--kernels]"""
import argparse
import csv
import glob
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--worms", type=int, default=4096)
ap.add_argument("--large", type=int, default=64)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thinning_bench.jsonl"))
args = ap.parse_args()


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_thinning", os.path.join(ROOT, "tests", "golden", "make_golden_thinning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator()


def worm_masks(n, seed=0):
    """masks of n seeded worms (margin 5, as Polygon.get_skeleton(ret_offset=True) makes them), filled on the GPU"""
    from video.analysis.shapes import Polygon, get_masks
    rng = np.random.default_rng(seed)
    polys = [Polygon(G.POL.worm(length=float(rng.uniform(70, 110)), width=float(rng.uniform(5, 9)),
                                bend=float(rng.uniform(5, 15)), x0=float(rng.uniform(0, 1000)),
                                y0=float(rng.uniform(20, 1000)), phase=float(rng.uniform(0, 3)))) for _ in range(n)]
    return get_masks(polys, 5)


def kernel_split():
    """this script's GPU part under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "thinning", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--worms",
               str(args.worms), "--large", str(args.large), "--frames", str(args.frames)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"].replace("va::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                c0, t0 = out.get(name, (0, 0.0))
                out[name] = (c0 + int(row["Calls"]), t0 + float(row["TotalDurationNs"]) / 1e6)
        return out


def timed(call, torch):
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(args.reps):
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def wall(call, reps=None):
    call()
    ms = []
    for _ in range(reps or args.reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms), float(np.median(ms))


def resident_legs(torch, sets):
    from video import _hip, ops
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for kind, masks in sets:
        m = len(masks)
        shapes = np.array([a.shape for a in masks], np.int32)
        sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
        offsets = np.zeros(m, np.int64)
        offsets[1:] = np.cumsum(sizes)[:-1]
        total = int(sizes.sum())
        words = [ops._thin_words(a.shape) for a in masks]
        d = {k: torch.from_numpy(v).to(dev) for k, v in
             (("m", np.concatenate([a.reshape(-1) for a in masks])), ("s", shapes), ("o", offsets))}
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        it = torch.empty(m, dtype=torch.int32, device=dev)
        st = torch.empty(m, dtype=torch.int32, device=dev)

        def call():
            _hip.check(L.va_guo_hall_thinning_batch(d["m"].data_ptr(), d["s"].data_ptr(), d["o"].data_ptr(), total, m,
                                                    max(words), out.data_ptr(), it.data_ptr(), st.data_ptr(), S))
        best, med = timed(call, torch)
        assert int(st.abs().max().item()) == 0
        iters = it.cpu().numpy()
        rows.append({"leg": "resident", "masks": kind, "count": m, "pixels": total, "max_words": max(words),
                     "iterations_max": int(iters.max()), "iterations_mean": round(float(iters.mean()), 2),
                     "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
                     "masks_per_s": round(m / med * 1e3, 1),
                     "gpixel_iterations_per_s": round(float((sizes * iters).sum()) / med / 1e6, 2)})
    return rows


def tiled_call(torch, stack, k_sub, poll):
    """(call, stats, iterations) of va_guo_hall_thinning_u8 on a device-resident stack"""
    from video import _hip
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    n, h, w = stack.shape
    src = torch.from_numpy(stack).to(dev)
    need = L.va_guo_hall_thinning_scratch_bytes(n, h, w)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    iters, stats = np.zeros(n, np.int32), np.zeros(2, np.int32)

    def call():
        _hip.check(L.va_guo_hall_thinning_u8(src.data_ptr(), scratch.data_ptr(), need, dst.data_ptr(), n, h, w, k_sub,
                                             poll, iters.ctypes.data, stats.ctypes.data, S))
    return call, stats, iters


def tiled_legs(torch, stack, kind, sweep):
    rows = []
    n, h, w = stack.shape
    wpr = (w + 31) // 32
    for k_sub, poll in sweep:
        call, stats, iters = tiled_call(torch, stack, k_sub, poll)
        best, med = timed(call, torch)
        K = k_sub or 16
        tiles = -(-wpr // 14) * -(-h // (64 - 2 * K)) * n
        plane = n * h * wpr * 4
        per_launch = tiles * 1024 * 4 + plane            # every window read, every word written once
        rows.append({"leg": "tiled", "masks": kind, "frames": n, "h": h, "w": w, "sub_iterations_per_launch": K,
                     "launches_per_host_read": poll or 2, "iterations": iters.tolist() if n <= 16 else int(iters.max()),
                     "launches": int(stats[0]), "host_reads": int(stats[1]),
                     "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
                     "ms_per_frame": round(med / n, 4), "packed_plane_bytes": plane,
                     "bytes_per_iteration": int(per_launch / (K / 2)),
                     "bytes_per_iteration_over_plane": round(per_launch / (K / 2) / plane, 2)})
    return rows


def gpu_run():
    import torch
    from video import _hip, ops
    _hip.lib()
    worms = worm_masks(args.worms)
    big = [G.blob(3000 + k, 480, 1024, 6.0, -0.4) for k in range(args.large)]
    frames = np.stack([G.blob(2000 + k, 1080, 1920, 4.0, 0.0) for k in range(args.frames)])
    rows = resident_legs(torch, (("worms", worms), ("at_limit_480x1024", big)))
    sweep = [(0, 0)] if args.child else [(8, 4), (4, 4), (16, 4), (8, 1), (8, 2), (8, 8), (16, 2)]
    rows += tiled_legs(torch, frames, "1080p_blobs", sweep)
    rows += tiled_legs(torch, frames[:1], "1080p_blob", [(0, 0)] if args.child else [(8, 4), (8, 1), (16, 2)])
    rows += tiled_legs(torch, np.stack(big), "at_limit_480x1024", [(0, 0)])
    if args.child:
        return rows
    best, med = wall(lambda: [ops.guo_hall_thinning([m]) for m in worms], reps=3)
    rows.append({"leg": "single_calls", "masks": "worms", "count": len(worms), "ms_min": round(best, 2),
                 "ms_median": round(med, 2), "ms_per_mask": round(med / len(worms), 4)})
    best, med = wall(lambda: ops.guo_hall_thinning(worms), reps=3)
    rows.append({"leg": "one_call_with_copies", "masks": "worms", "count": len(worms), "ms_min": round(best, 2),
                 "ms_median": round(med, 2), "ms_per_mask": round(med / len(worms), 4)})
    best, med = wall(lambda: ops.mask_thinning(frames[0]))
    rows.append({"leg": "context_cross_erosion_va_mask_thinning_u8", "h": 1080, "w": 1920,
                 "iterations": ops.mask_thinning(frames[0])[1], "ms_min": round(best, 3), "ms_median": round(med, 3),
                 "note": "a different algorithm; wall time with copies"})
    best, med = wall(lambda: ops.guo_hall_thinning(frames[:1]))
    rows.append({"leg": "guo_hall_1080p_with_copies", "h": 1080, "w": 1920, "ms_min": round(best, 3),
                 "ms_median": round(med, 3)})
    return rows


if args.child:
    gpu_run()
    sys.exit(0)

split = kernel_split() if args.kernels else None       # (a child process: before this one opens the GPU)
rows = gpu_run()
for row in rows:
    print(json.dumps(row), flush=True)
if split:
    total = sum(t for _, t in split.values())
    rows.append({"leg": "kernels", "reps": args.reps,
                 "kernels": {k: {"calls": c, "ms_total": round(t, 3), "share": round(t / total, 4)}
                             for k, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])}})
    print(json.dumps(rows[-1]), flush=True)
if not args.no_cpu:
    frame = G.blob(2000, 1080, 1920, 4.0, 0.0)
    t = time.perf_counter()
    _, it = G.guo_hall(frame)
    row = {"leg": "cpu_numpy_restatement", "threads": os.environ.get("OMP_NUM_THREADS"), "h": 1080, "w": 1920,
           "iterations": it, "ms": round((time.perf_counter() - t) * 1e3, 1)}
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
