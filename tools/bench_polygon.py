#!/usr/bin/env python3
"""Throughput of the polygon path on the GPU (va_polygon.hip and the centre lines of video.analysis.shapes):
  fill      va_fill_poly, inputs and outputs resident in HBM, HIP events around the call: 4096 worm-sized
            polygons (~80 vertices, ~100 x 40 boxes) in one call, and 64 large ones (~1000 vertices, 1000 x 700
            boxes); bytes written = the boxes' pixels
  dt        va_distance_transform_l2_5 on the masks of the same polygons (margin 1), one workgroup per mask whose
            rows run in sequence: the longest mask bounds the call
  estimate  get_centerline_estimates of 256 worms (end points None) against 256 get_centerline_estimate calls,
            wall time on the host (uploads, geodesic calls, downloads)
  latency   Polygon.get_centerline_optimized (gentle parameters and the defaults) and get_centerline() per polygon
With --kernels the fill and dt legs run again in a child process under `rocprofv3 --kernel-trace --stats` and the
time is split per kernel.  CPU baseline on one core: the NumPy restatement (tests/golden/make_golden_polygon.py) of
the fill, the distance transform, the estimate and the optimized centre line.  One JSON line per leg, appended to
profiles/polygon_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_polygon.py [--reps 5] [--kernels]"""
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
ap.add_argument("--estimates", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygon_bench.jsonl"))
args = ap.parse_args()


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_polygon", os.path.join(ROOT, "tests", "golden", "make_golden_polygon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator()


def worms(n, seed=0):
    rng = np.random.default_rng(seed)
    return [G.worm(length=float(rng.uniform(70, 110)), width=float(rng.uniform(5, 9)), bend=float(rng.uniform(5, 15)),
                   x0=float(rng.uniform(0, 1000)), y0=float(rng.uniform(20, 1000)), phase=float(rng.uniform(0, 3)))
            for _ in range(n)]


def large(n, seed=1):
    rng = np.random.default_rng(seed)
    t = np.linspace(0, 2 * np.pi, 1000, endpoint=False)
    return [np.stack([510 + 480 * np.cos(t) * (1 + 0.05 * np.sin(k + 7 * t)),
                      360 + 330 * np.sin(t) + rng.uniform(-2, 2, len(t))], 1) for k in range(n)]


def kernel_split():
    """this script's GPU part under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "polygon", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--worms",
               str(args.worms), "--large", str(args.large)]
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


def wall(call):
    call()
    ms = []
    for _ in range(args.reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms), float(np.median(ms))


def dense_legs(torch):
    """fill and dt on device-resident tables, one call each per rep"""
    from video import _hip
    from video.analysis.shapes import Polygon
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for kind, contours in (("worms", worms(args.worms)), ("large", large(args.large))):
        polys = [Polygon(c) for c in contours]
        boxes = np.array([p.get_bounding_rect(1) for p in polys], np.int32)
        cs = [np.asarray(c).astype(np.int64) for c in contours]
        verts = np.ascontiguousarray(np.concatenate(cs), np.int32)
        vert_off = np.zeros(len(cs) + 1, np.int64)
        vert_off[1:] = np.cumsum([len(c) for c in cs])
        sizes = boxes[:, 2].astype(np.int64) * boxes[:, 3]
        out_off = np.zeros(len(cs), np.int64)
        out_off[1:] = np.cumsum(sizes)[:-1]
        total = int(sizes.sum())
        m = len(cs)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("v", verts), ("vo", vert_off), ("b", boxes), ("oo", out_off))}
        mask = torch.empty(total, dtype=torch.uint8, device=dev)
        dist = torch.empty(total, dtype=torch.float32, device=dev)
        st = torch.empty(m, dtype=torch.int32, device=dev)
        shapes = torch.from_numpy(np.ascontiguousarray(boxes[:, [3, 2]])).to(dev)

        def fill():
            _hip.check(L.va_fill_poly(d["v"].data_ptr(), d["vo"].data_ptr(), len(verts), d["b"].data_ptr(),
                                      d["oo"].data_ptr(), total, m, 1, mask.data_ptr(), st.data_ptr(), S))

        def dt():
            _hip.check(L.va_distance_transform_l2_5(mask.data_ptr(), shapes.data_ptr(), d["oo"].data_ptr(), total, m,
                                                    int(boxes[:, 2].max()), dist.data_ptr(), st.data_ptr(), S))
        best, med = timed(fill, torch)
        assert int(st.abs().max().item()) == 0
        rows.append({"leg": "fill", "polygons": kind, "count": m, "vertices": len(verts), "pixels": total,
                     "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
                     "polygons_per_s": round(m / best * 1e3, 1), "gb_per_s_written": round(total / best / 1e6, 2)})
        best, med = timed(dt, torch)
        assert int(st.abs().max().item()) == 0
        rows.append({"leg": "dt", "polygons": kind, "count": m, "pixels": total, "max_rows": int(boxes[:, 3].max()),
                     "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
                     "masks_per_s": round(m / best * 1e3, 1),
                     "gb_per_s_moved": round(total * 13 / best / 1e6, 2)})    # 1 B read, 4 B x 3 passes of the work
    return rows


def gpu_run():
    import torch
    rows = dense_legs(torch)
    if args.child:
        return rows
    from video.analysis.shapes import Polygon, get_centerline_estimates
    polys = [Polygon(c) for c in worms(args.estimates, seed=3)]
    best, med = wall(lambda: get_centerline_estimates(polys))
    rows.append({"leg": "estimate_batched", "polygons": len(polys), "ms_min": round(best, 2), "ms_median": round(med, 2),
                 "ms_per_polygon": round(best / len(polys), 3)})
    best, med = wall(lambda: [p.get_centerline_estimate() for p in polys])
    rows.append({"leg": "estimate_per_polygon", "polygons": len(polys), "ms_min": round(best, 2),
                 "ms_median": round(med, 2), "ms_per_polygon": round(best / len(polys), 3)})
    p = polys[0]
    gentle = dict(alpha=10.0, beta=100.0, gamma=0.01, spacing=5, max_iterations=60)
    for name, call in (("optimized_gentle", lambda: p.get_centerline_optimized(**gentle)),
                       ("optimized_default", lambda: p.get_centerline_optimized()),
                       ("get_centerline_default", lambda: p.get_centerline())):
        best, med = wall(call)
        rows.append({"leg": "latency", "call": name, "ms_min": round(best, 2), "ms_median": round(med, 2)})
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
    row = {"leg": "cpu_numpy_restatement", "threads": os.environ.get("OMP_NUM_THREADS")}
    sample = worms(64)
    boxes = [G.bounding_rect(c, 1) for c in sample]
    t = time.perf_counter()
    masks = [G.fill_poly(np.asarray(c).astype(np.int64), b) for c, b in zip(sample, boxes)]
    row["fill_worm_ms_per_polygon"] = round((time.perf_counter() - t) * 1e3 / len(sample), 3)
    t = time.perf_counter()
    for mk in masks:
        G.distance_transform(mk)
    row["dt_worm_ms_per_mask"] = round((time.perf_counter() - t) * 1e3 / len(sample), 3)
    big = large(2)
    t = time.perf_counter()
    bm = [G.fill_poly(np.asarray(c).astype(np.int64), G.bounding_rect(c, 1)) for c in big]
    row["fill_large_ms_per_polygon"] = round((time.perf_counter() - t) * 1e3 / len(big), 1)
    t = time.perf_counter()
    for mk in bm:
        G.distance_transform(mk)
    row["dt_large_ms_per_mask"] = round((time.perf_counter() - t) * 1e3 / len(big), 1)
    t = time.perf_counter()
    for c in sample[:8]:
        G.estimate(c)
    row["estimate_ms_per_polygon"] = round((time.perf_counter() - t) * 1e3 / 8, 1)
    t = time.perf_counter()
    G.optimized(sample[0], alpha=10.0, beta=100.0, gamma=0.01, spacing=5, max_iterations=60)
    row["optimized_gentle_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
