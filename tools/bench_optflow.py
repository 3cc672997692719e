#!/usr/bin/env python3
"""Throughput of the Farneback optical flow (va_optflow.hip) with the reference's parameters (pyr_scale 0.5,
levels 3, winsize 2, iterations 3, poly_n 5, poly_sigma 1.2): pairs per second at 640x480 and 1920x1080,
`--pairs` pairs (default 32) per call, inputs and outputs resident in HBM, HIP events around the calls.
With --kernels, the same calls run again in a child process under `rocprofv3 --kernel-trace --stats` and the
time is split per kernel.  CPU baselines: the NumPy restatement (tests/golden/make_golden_optflow.py) for one
pair, and cv2.calcOpticalFlowFarneback when OpenCV is installed.  One JSON line per size, appended to
profiles/optflow_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_optflow.py [--pairs 32] [--reps 5] [--kernels]"""
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
ap.add_argument("--pairs", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baselines")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--size", help=argparse.SUPPRESS)           # (--child: HxW)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optflow_bench.jsonl"))
args = ap.parse_args()

SIZES = ((480, 640), (1080, 1920))
PARAMS = (0.5, 3, 2, 3, 5, 1.2)


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_optflow", os.path.join(ROOT, "tests", "golden", "make_golden_optflow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator()


def kernel_split(h, w):
    """run this script's GPU part for one size under rocprofv3 and return {kernel: (calls, ms per call)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "optflow", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(args.pairs), "--reps",
               str(args.reps), "--size", "%dx%d" % (h, w)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"].replace("va::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                calls = int(row["Calls"])
                total = float(row["TotalDurationNs"]) / 1e6
                c0, t0 = out.get(name, (0, 0.0))
                out[name] = (c0 + calls, t0 + total)
        return out


def gpu_run(h, w):
    import torch
    from video import _hip
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    n = args.pairs + 1
    frames = torch.from_numpy(G.texture_frames(n, h, w, 5, step=(1, 1), cell=16)).to(dev)
    wsb = L.va_farneback_workspace_bytes(n, h, w, *PARAMS[:5])
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    mag = torch.empty((n - 1, h, w), dtype=torch.float32, device=dev)
    flow = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device=dev)

    def call():
        _hip.check(L.va_optical_flow_farneback(frames.data_ptr(), _hip.VA_U8, n, h, w, *PARAMS, 0, flow.data_ptr(),
                                               mag.data_ptr(), ws.data_ptr(), wsb, S))
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
    return ms, wsb, float(mag.float().median().item())


if args.child:
    h, w = (int(v) for v in args.size.split("x"))
    gpu_run(h, w)
    sys.exit(0)

rows = []
for h, w in SIZES:
    split = kernel_split(h, w) if args.kernels else None      # (a child process: before this one opens the GPU)
    ms, wsb, med = gpu_run(h, w)
    best = min(ms)
    row = {"size": "%dx%d" % (w, h), "pairs_per_call": args.pairs, "reps": args.reps,
           "ms_per_call_min": round(best, 3), "ms_per_call_median": round(float(np.median(ms)), 3),
           "pairs_per_s": round(args.pairs / best * 1e3, 1), "workspace_mb": round(wsb / 2 ** 20, 1),
           "median_magnitude": round(med, 4)}
    if split:
        total = sum(t for _, t in split.values())
        row["kernels"] = {k: {"calls": c, "ms_total": round(t, 3), "share": round(t / total, 4)}
                          for k, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    if not args.no_cpu:
        pair = G.texture_frames(2, h, w, 5, step=(1, 1), cell=16)
        t = time.perf_counter()
        G.farneback(pair[0], pair[1], **G.REFERENCE_PARAMS)
        row["numpy_restatement_ms_per_pair"] = round((time.perf_counter() - t) * 1e3, 1)
        try:
            import cv2
            cv2.calcOpticalFlowFarneback(pair[0], pair[1], None, *PARAMS, 0)
            t = time.perf_counter()
            for _ in range(3):
                cv2.calcOpticalFlowFarneback(pair[0], pair[1], None, *PARAMS, 0)
            row["cv2_ms_per_pair"] = round((time.perf_counter() - t) * 1e3 / 3, 2)
            row["cv2_version"] = cv2.__version__
        except ImportError:
            row["cv2_ms_per_pair"] = None
    print(json.dumps(row), flush=True)
    rows.append(row)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
