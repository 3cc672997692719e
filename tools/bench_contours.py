#!/usr/bin/env python3
"""Time of every outer contour of a frame stack on the GPU (va_find_contours, va_contours.hip):
  blobs     64 x 1080p masks of the cfg#3 kind (40 moving discs of radius 8 .. 60 a frame, as bench.py's
            synth_batch places them, already thresholded and closed: no salt), resident in HBM, HIP events around
            the call; va_largest_contour on the same stack for the ratio
  salt      16 x 1080p masks with 2 % of the pixels set at random (10^4 .. 10^5 mostly one-point contours a
            frame), the same two calls
  context   oracle.find_contours_external_simple on one core for one frame of each stack
With --kernels the GPU legs run again in a child process under `rocprofv3 --kernel-trace --stats` and the time is
split per kernel.  Times are the median of the repetitions.  One JSON line per leg, appended to
profiles/contours_bench.jsonl (or --out); a leg that did not run is written "not measured".
Run on an MI355X:
    python tools/bench_contours.py [--reps 15] [--kernels]"""
import argparse
import csv
import glob
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
ap.add_argument("--blob-frames", type=int, default=64)
ap.add_argument("--salt-frames", type=int, default=16)
ap.add_argument("--salt", type=float, default=0.02)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--cpu", type=int, default=1, help="frames of the oracle leg (0: not measured)")
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_bench.jsonl"))
args = ap.parse_args()
H, W, BLOBS = 1080, 1920, 40


def blob_masks(torch, dev, n):
    """the discs of bench.py's synth_batch as masks"""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    pos = torch.rand((BLOBS, 2), generator=g, device=dev) * torch.tensor([W, H], device=dev)
    vel = (torch.rand((BLOBS, 2), generator=g, device=dev) - 0.5) * 6
    rad = 8 + torch.rand((BLOBS,), generator=g, device=dev) * 52
    t = torch.arange(n, device=dev, dtype=torch.float32).view(n, 1, 1)
    m = torch.zeros((n, H, W), dtype=torch.bool, device=dev)
    for k in range(BLOBS):
        m |= ((xx - (pos[k, 0] + vel[k, 0] * t)) ** 2 + (yy - (pos[k, 1] + vel[k, 1] * t)) ** 2) <= rad[k] ** 2
    return m.to(torch.uint8)


def salt_masks(torch, dev, n):
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    return (torch.rand((n, H, W), generator=g, device=dev) < args.salt).to(torch.uint8)


def kernel_split():
    """this script's GPU legs under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "contours", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--blob-frames",
               str(args.blob_frames), "--salt-frames", str(args.salt_frames), "--salt", str(args.salt)]
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


def gpu_leg(name, masks, torch, dev, S):
    """[row of va_find_contours, row of va_largest_contour] for one resident stack"""
    from video import _hip
    L = _hip.lib()
    n = len(masks)
    buf = lambda nbytes: torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)
    ws_bytes = L.va_find_contours_workspace_bytes(n, H, W)
    ws, nc, tot = buf(ws_bytes), buf(n * 4), torch.zeros(2, dtype=torch.int64, device=dev)

    def find(capc, capp, info, off, pts):
        _hip.check(L.va_find_contours(masks.data_ptr(), n, H, W, nc.data_ptr(), tot.data_ptr(), info.data_ptr(),
                                      off.data_ptr(), capc, pts.data_ptr(), capp, ws.data_ptr(), ws_bytes, S))
    find(0, 0, buf(8), buf(8), buf(8))                                   # the totals, then buffers with exact room
    torch.cuda.synchronize()
    k, npts = (int(v) for v in tot.tolist())
    info, off, pts = buf(k * 48), buf((k + 1) * 8), buf(npts * 8)
    best, med = timed(lambda: find(k, npts, info, off, pts), torch)
    rows = [{"leg": name + "/va_find_contours", "frames": n, "h": H, "w": W, "contours": k, "points": npts,
             "workspace_mb": round(ws_bytes / 2 ** 20, 1), "ms_per_call_min": round(best, 4),
             "ms_per_call_median": round(med, 4), "ms_per_frame": round(med / n, 4),
             "contours_per_s": round(k / med * 1e3, 1)}]
    cap = 4096
    lws_bytes = L.va_contour_workspace_bytes(n, H, W)
    lws, lp, ln, la, lc = buf(lws_bytes), buf(n * cap * 8), buf(n * 4), buf(n * 8), buf(n * 4)

    def largest():
        _hip.check(L.va_largest_contour(masks.data_ptr(), n, H, W, lp.data_ptr(), cap, ln.data_ptr(), la.data_ptr(),
                                        lc.data_ptr(), lws.data_ptr(), lws_bytes, S))
    lbest, lmed = timed(largest, torch)
    rows.append({"leg": name + "/va_largest_contour", "frames": n, "ms_per_call_min": round(lbest, 4),
                 "ms_per_call_median": round(lmed, 4), "ms_per_frame": round(lmed / n, 4),
                 "find_contours_over_largest_contour": round(med / lmed, 3)})
    return rows


def gpu_run():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    blobs, salt = blob_masks(torch, dev, args.blob_frames), salt_masks(torch, dev, args.salt_frames)
    rows = gpu_leg("blobs", blobs, torch, dev, S) + gpu_leg("salt", salt, torch, dev, S)
    return rows, blobs[0].cpu().numpy(), salt[0].cpu().numpy()


if args.child:
    gpu_run()
    sys.exit(0)

split = kernel_split() if args.kernels else None       # (a child process: before this one opens the GPU)
rows, blob0, salt0 = gpu_run()
for row in rows:
    print(json.dumps(row), flush=True)
if split:
    total = sum(t for _, t in split.values())
    rows.append({"leg": "kernels", "reps": args.reps,
                 "kernels": {k: {"calls": c, "ms_total": round(t, 3), "share": round(t / total, 4)}
                             for k, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])}})
else:
    rows.append({"leg": "kernels", "kernels": "not measured"})
print(json.dumps(rows[-1]), flush=True)
if args.cpu:
    from oracle import oracle as O
    O.build()
    for name, frame in (("blobs", blob0), ("salt", salt0)):
        O.find_contours_external_simple(frame)
        t0 = time.perf_counter()
        for _ in range(args.cpu):
            found = O.find_contours_external_simple(frame)
        ms = (time.perf_counter() - t0) * 1e3 / args.cpu
        rows.append({"leg": name + "/cpu_oracle_one_core", "frames": 1, "contours": len(found),
                     "ms_per_frame": round(ms, 3), "note": "scan and list building in C, one array per contour in Python"})
        print(json.dumps(rows[-1]), flush=True)
else:
    rows.append({"leg": "cpu_oracle_one_core", "ms_per_frame": "not measured"})
    print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
