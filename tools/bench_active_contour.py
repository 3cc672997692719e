#!/usr/bin/env python3
"""Throughput of ActiveContour on the GPU (va_snake.hip), inputs and outputs resident in HBM, HIP events around
the calls:
  potential  set_potential's dense part on 64 x 1080p frames -- blur (va_gaussian_f32 / _u8) + both Sobel
             planes -- for float32 sigma = 10, float32 sigma = 1 and uint8 sigma = 10
  sobel      the Sobel pass alone, bytes moved per second (1 or 4 B read + 16 B written per pixel) beside a
             device-to-device copy of the 16 B per pixel it writes (32 B moved per pixel)
  snake      256 contours on the 1080p gradients, N = 64, 128 (matrix in LDS) and 512 (global memory), 50 and
             1000 iterations (residual tolerance 0: every iteration runs), one matrix per contour
With --kernels the same calls run again in a child process under `rocprofv3 --kernel-trace --stats` and the
time is split per kernel.  CPU baseline: the NumPy restatement (tests/golden/make_golden_active_contour.py) of
one 1080p frame's gradients and of one contour.  One JSON line per leg, appended to
profiles/active_contour_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_active_contour.py [--reps 5] [--kernels]"""
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
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--contours", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_contour_bench.jsonl"))
args = ap.parse_args()

H, W = 1080, 1920
POTENTIALS = (("f32", 10.0), ("f32", 1.0), ("u8", 10.0))
SNAKES = ((64, 50), (128, 50), (512, 50), (64, 1000), (128, 1000), (512, 1000))


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_active_contour", os.path.join(ROOT, "tests", "golden", "make_golden_active_contour.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator()


def frames_of(kind, n):
    """n 1080p potentials: a ridge along a moving ellipse plus texture"""
    y, x = np.mgrid[:H, :W].astype(np.float32)
    out = np.empty((n, H, W), np.uint8 if kind == "u8" else np.float32)
    for k in range(n):
        r = np.sqrt(((x - 960 - 7 * k) / 600) ** 2 + ((y - 540) / 400) ** 2)
        p = 200 * np.exp(-((r - 1) / 0.05) ** 2) + 20 + (G.ramp((H, W), k) & 15)
        out[k] = np.clip(p, 0, 255) if kind == "u8" else p
    return out


def kernel_split():
    """this script's GPU part under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "snake", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--frames",
               str(args.frames), "--contours", str(args.contours)]
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


def gpu_run():
    import torch
    from video import _hip
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    n = args.frames
    rows = []
    fx = torch.empty((n, H, W), dtype=torch.float64, device=dev)
    fy = torch.empty_like(fx)
    for kind, sigma in POTENTIALS:
        src = torch.from_numpy(frames_of(kind, n)).to(dev)
        tmp = torch.empty_like(src)
        dtype = _hip.VA_U8 if kind == "u8" else _hip.VA_F32
        blur = L.va_gaussian_u8 if kind == "u8" else L.va_gaussian_f32

        def potential():
            _hip.check(blur(src.data_ptr(), tmp.data_ptr(), n, H, W, 1, sigma, S))
            _hip.check(L.va_sobel5_f64(tmp.data_ptr(), dtype, fx.data_ptr(), fy.data_ptr(), n, H, W, S))

        def sobel():
            _hip.check(L.va_sobel5_f64(tmp.data_ptr(), dtype, fx.data_ptr(), fy.data_ptr(), n, H, W, S))
        best, med = timed(potential, torch)
        rows.append({"leg": "potential", "dtype": kind, "sigma": sigma, "frames": n, "size": "%dx%d" % (W, H),
                     "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
                     "frames_per_s": round(n / best * 1e3, 1)})
        if sigma == 10.0:
            best, med = timed(sobel, torch)
            moved = n * H * W * (src.element_size() + 16)
            rows.append({"leg": "sobel", "dtype": kind, "frames": n, "size": "%dx%d" % (W, H),
                         "ms_per_call_min": round(best, 3), "bytes_moved": moved,
                         "gb_per_s": round(moved / best / 1e6, 1)})
        if kind == "f32" and sigma == 10.0:
            keep = (fx.clone(), fy.clone())
    fx, fy = keep
    flat = fx.view(-1)
    dst = torch.empty_like(flat)
    best, _ = timed(lambda: dst.copy_(flat), torch)
    rows.append({"leg": "memcpy_d2d", "bytes": flat.numel() * 8, "ms_min": round(best, 3),
                 "gb_per_s_moved": round(2 * flat.numel() * 8 / best / 1e6, 1)})
    del dst
    ac = ActiveContour()                   # the reference's defaults: gamma 0.001, beta 1e2
    m = args.contours
    for N, iters in SNAKES:
        pts = np.zeros((m, N, 2))
        mats = []
        for c in range(m):
            curve = G.ellipse_curve(N, True, scale=1.0 + 0.001 * c)
            curve = curve * np.array([600 / 52.0, 400 / 38.0]) - np.array([80 * 600 / 52.0 - 960, 60 * 400 / 38.0 - 540])
            p = curves.make_curve_equidistant(curve)
            pts[c] = p
            mats.append(np.ascontiguousarray(ac.get_evolution_matrix(N, curves.curve_length(p) / (N - 1)).T))
        d_pts0 = torch.from_numpy(pts).to(dev)
        d_pts = torch.empty_like(d_pts0)
        d_n = torch.full((m,), N, dtype=torch.int32, device=dev)
        d_f = torch.arange(m, dtype=torch.int32, device=dev) % n
        d_m = torch.from_numpy(np.concatenate([a.reshape(-1) for a in mats])).to(dev)
        d_o = torch.arange(m, dtype=torch.int64, device=dev) * (N * N)
        d_it = torch.empty((m,), dtype=torch.int32, device=dev)
        d_tv = torch.empty((m,), dtype=torch.float64, device=dev)

        def snake():
            d_pts.copy_(d_pts0)
            _hip.check(L.va_active_contour(fx.data_ptr(), fy.data_ptr(), n, H, W, m, N, d_n.data_ptr(),
                                           d_f.data_ptr(), d_m.data_ptr(), d_o.data_ptr(), d_m.numel(), None, None,
                                           ac.gamma, 0.0, iters, d_pts.data_ptr(), d_it.data_ptr(),
                                           d_tv.data_ptr(), S))
        best, med = timed(snake, torch)
        assert int(d_it.min().item()) == iters
        rows.append({"leg": "snake", "contours": m, "points": N, "iterations": iters,
                     "matrix": "lds" if N <= 128 else "global", "ms_per_call_min": round(best, 3),
                     "ms_per_call_median": round(med, 3),
                     "us_per_iteration": round(best * 1e3 / iters, 2),
                     "matrix_mb": round(d_m.numel() * 8 / 2 ** 20, 1)})
        del d_m
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
    p = frames_of("f32", 1)[0]
    t = time.perf_counter()
    gx, gy = G.gradients(p, 10.0)
    row = {"leg": "cpu_numpy_restatement", "gradients_1080p_f32_sigma10_ms": round((time.perf_counter() - t) * 1e3, 1)}
    from video.analysis import curves
    from video.analysis.active_contour import ActiveContour
    ac = ActiveContour()
    for N in (128, 512):
        c = G.ellipse_curve(N, True) * np.array([600 / 52.0, 400 / 38.0]) - np.array([80 * 600 / 52.0 - 960,
                                                                                        60 * 400 / 38.0 - 540])
        pts = curves.make_curve_equidistant(c)
        P = ac.get_evolution_matrix(N, curves.curve_length(pts) / (N - 1))
        t = time.perf_counter()
        G.snake(gx, gy, pts, P, ac.gamma, 0.0, 50)
        row["snake_n%d_50it_ms_per_contour" % N] = round((time.perf_counter() - t) * 1e3, 1)
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
