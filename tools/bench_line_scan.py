#!/usr/bin/env python3
"""Throughput of the batched 8-bit affine warps on the GPU (va_warp.hip):
  resident  va_line_scan_u8 on 64 x 1080p frames with 256 scans each (lengths 20 .. 400, half width 5), frames,
            tables and sums resident in HBM, HIP events around the call; taps per second, and the bytes the scans
            touch (the distinct source pixels under every strip, the sums written, the tables read) against the
            time, which says whether bytes or gather latency and launch bound the kernel
  copies    the same through ops.line_scans (host tables, uploads of frames and tables, download), wall time
  single    the same scans one ops.line_scans call each (--single of them), wall time per scan
  crops     256 get_subimage crops of 200 x 200 resampled to 64 x 64: va_warp_affine_u8 resident, and
            ops.warp_affine with copies
  context   the NumPy restatement of --cpu scans on one core
With --kernels the resident legs run again in a child process under `rocprofv3 --kernel-trace --stats` and the
time is split per kernel.  Rates come from the median of the repetitions.  One JSON line per leg, appended to
profiles/line_scan_bench.jsonl (or --out); a leg that did not run is written "not measured".
Run on an MI355X:
    python tools/bench_line_scan.py [--reps 15] [--kernels]"""
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
ap.add_argument("--scans", type=int, default=256, help="scans per frame")
ap.add_argument("--crops", type=int, default=256)
ap.add_argument("--single", type=int, default=1024, help="scans of the one-call-each leg (0: not measured)")
ap.add_argument("--cpu", type=int, default=256, help="scans of the restatement leg (0: not measured)")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_scan_bench.jsonl"))
args = ap.parse_args()
H, W, HALF_WIDTH = 1080, 1920, 5


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_line_scan", os.path.join(ROOT, "tests", "golden", "make_golden_line_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def workload():
    """(frames, frame index, p1, p2) of the scans; (crop matrices, sizes, frame index) of the crops"""
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (args.frames, H, W), dtype=np.uint8)
    m = args.frames * args.scans
    length, angle = rng.uniform(20, 400, m), rng.uniform(0, 2 * np.pi, m)
    p1 = np.stack([rng.uniform(0, W, m), rng.uniform(0, H, m)], 1)
    p2 = p1 + np.stack([length * np.cos(angle), length * np.sin(angle)], 1)
    return frames, np.repeat(np.arange(args.frames), args.scans).astype(np.int32), p1, p2


def crop_tables(rng, ops):
    x0, y0 = rng.uniform(0, W - 200, args.crops), rng.uniform(0, H - 200, args.crops)
    z = np.zeros(args.crops)
    src = np.stack([np.stack([x0, y0], 1), np.stack([x0, y0 + 200], 1), np.stack([x0 + 200, y0], 1)], 1)
    dst = np.stack([np.stack([z, z], 1), np.stack([z + 64, z], 1), np.stack([z, z + 64], 1)], 1)   # get_subimage's
    return ops.affine_transforms(src, dst), np.full((args.crops, 2), 64, np.int64), \
        rng.integers(0, args.frames, args.crops).astype(np.int32)


def kernel_split():
    """this script's resident legs under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "line_scan", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--frames",
               str(args.frames), "--scans", str(args.scans), "--crops", str(args.crops)]
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


def wall(call, reps):
    call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms), float(np.median(ms))


def gpu_run():
    import torch
    from video import _hip, ops
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    frames, fidx, p1, p2 = workload()
    n, m = len(frames), len(fidx)
    mats, rows_, cols = ops.line_scan_tables(p1, p2, HALF_WIDTH)
    _, _, offsets, _, total = ops._pack_ragged(np.stack([np.ones(m, np.int64), cols], 1))
    prefix, chunks = ops._work_prefix(np.maximum(1, -(-cols // ops.WARP_CHUNK)), "bench")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fd = up(frames)
    t = {k: up(v) for k, v in (("i", fidx), ("m", mats), ("s", np.stack([rows_, cols], 1).astype(np.int32)),
                               ("o", offsets), ("p", prefix))}
    sums = torch.empty(total, dtype=torch.int32, device=dev)
    st = torch.empty(m, dtype=torch.int32, device=dev)

    def scan_call():
        _hip.check(L.va_line_scan_u8(fd.data_ptr(), n, H, W, m, t["i"].data_ptr(), t["m"].data_ptr(),
                                     t["s"].data_ptr(), t["o"].data_ptr(), t["p"].data_ptr(), chunks, total,
                                     sums.data_ptr(), st.data_ptr(), S))
    best, med = timed(scan_call, torch)
    assert int(st.abs().max().item()) == 0
    samples = int((rows_ * cols).sum())
    touched = int(((rows_ + 1) * (cols + 1)).sum())          # the distinct source pixels under a strip, about
    moved = touched + total * 4 + m * (4 + 48 + 8 + 8 + 4 + 4)
    rows = [{"leg": "line_scans_resident", "frames": n, "h": H, "w": W, "scans": m, "half_width": HALF_WIDTH,
             "columns": total, "work_items": chunks, "ms_per_call_min": round(best, 4),
             "ms_per_call_median": round(med, 4), "scans_per_s": round(m / med * 1e3, 1),
             "gtaps_per_s": round(4 * samples / med / 1e6, 2), "taps": 4 * samples,
             "bytes_touched": moved, "gbytes_per_s_touched": round(moved / med / 1e6, 2),
             "bound": "gather latency and launch, not bytes" if moved / med / 1e6 < 1000 else "see gbytes_per_s_touched"}]

    rng = np.random.default_rng(1)
    cm, csz, cf = crop_tables(rng, ops)
    k = len(cm)
    _, cshapes, coff, _, ctotal = ops._pack_ragged(csz)
    cprefix, tiles = ops._work_prefix(np.maximum(1, (-(-csz[:, 0] // ops.WARP_TILE_H)) * (-(-csz[:, 1] // ops.WARP_TILE_W))),
                                      "bench")
    c = {key: up(v) for key, v in (("i", cf), ("m", cm), ("s", cshapes), ("g", np.zeros(k, np.int32)), ("o", coff),
                                   ("p", cprefix))}
    cout = torch.empty(ctotal, dtype=torch.uint8, device=dev)
    cst = torch.empty(k, dtype=torch.int32, device=dev)

    def crop_call():
        _hip.check(L.va_warp_affine_u8(fd.data_ptr(), n, H, W, k, c["i"].data_ptr(), c["m"].data_ptr(),
                                       c["s"].data_ptr(), c["g"].data_ptr(), c["o"].data_ptr(), c["p"].data_ptr(),
                                       tiles, ctotal, cout.data_ptr(), cst.data_ptr(), S))
    best, med = timed(crop_call, torch)
    assert int(cst.abs().max().item()) == 0
    rows.append({"leg": "subimage_crops_resident", "crops": k, "source": "200x200", "destination": "64x64",
                 "work_items": tiles, "ms_per_call_min": round(best, 4), "ms_per_call_median": round(med, 4),
                 "crops_per_s": round(k / med * 1e3, 1), "gtaps_per_s": round(4 * ctotal / med / 1e6, 2)})
    if args.child:
        return rows
    del fd
    best, med = wall(lambda: ops.line_scans(frames, p1, p2, HALF_WIDTH, frame_index=fidx), 3)
    rows.append({"leg": "line_scans_with_copies", "frames": n, "scans": m, "ms_min": round(best, 2),
                 "ms_median": round(med, 2), "ms_per_scan": round(med / m, 5),
                 "note": "host tables, upload of %d MB of frames, download" % (frames.nbytes >> 20)})
    best, med = wall(lambda: ops.warp_affine(frames, cm, csz, frame_index=cf), 3)
    rows.append({"leg": "subimage_crops_with_copies", "crops": k, "ms_min": round(best, 2), "ms_median": round(med, 2)})
    if args.single:
        q = min(args.single, m)
        best, med = wall(lambda: [ops.line_scans(frames[fidx[j]], p1[j:j + 1], p2[j:j + 1], HALF_WIDTH) for j in range(q)], 2)
        rows.append({"leg": "single_calls", "scans": q, "ms_min": round(best, 2), "ms_median": round(med, 2),
                     "ms_per_scan": round(med / q, 4), "note": "each call uploads its 1080p frame"})
    else:
        rows.append({"leg": "single_calls", "ms_median": "not measured"})
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
else:
    rows.append({"leg": "kernels", "kernels": "not measured"})
print(json.dumps(rows[-1]), flush=True)
if args.cpu:
    G = generator()
    frames, fidx, p1, p2 = workload()
    q = min(args.cpu, len(fidx))
    t0 = time.perf_counter()
    for j in range(q):
        G.line_scan(frames[fidx[j]], p1[j], p2[j], HALF_WIDTH)
    ms = (time.perf_counter() - t0) * 1e3
    rows.append({"leg": "cpu_numpy_restatement", "threads": os.environ.get("OMP_NUM_THREADS"), "scans": q,
                 "ms": round(ms, 1), "ms_per_scan": round(ms / q, 3)})
else:
    rows.append({"leg": "cpu_numpy_restatement", "ms": "not measured"})
print(json.dumps(rows[-1]), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
