#!/usr/bin/env python3
"""Time of the region links between consecutive label planes on the GPU (va_region_links, va_links.hip):
  blobs     256 x 1080p frames of 40 moving discs (as bench.py's synth_batch places them), labelled by a FrameEngine
            into a resident buffer: the engine's own labels
  noise     16 x 1080p frames of 50 % noise, labelled by the same engine: about 10^5 regions a frame
Per workload, with HIP events on resident data, the median of --reps repetitions: the whole va_region_links call
with exact room; a device-to-device copy of the label stack, twice (what one read of both planes of every pair
moves), in the same run, and the ratio; need / total; ops.region_links end to end (wall clock: the call, its retry
where the first guess is short, and the download of the tables); one call with capacity 0 and the least workspace,
which counts the links a table at a time; and the path it replaces -- the download of the
label planes plus the NumPy restatement on --host-frames frames, extrapolated to the stack.  With --kernels the
calls run again in a child process under `rocprofv3 --kernel-trace --stats` and the time is split into the three
passes (count = count + scan; accumulate = clear + accumulate; place = owners, scans and records).
End to end: track_regions frames per second on resident frames, against the same loop with want=('labels',
'counts') and the links made on the host, on --host-frames frames.
One JSON line per leg, appended to profiles/region_links_bench.jsonl (or --out); a leg that did not run is written
"not measured".  Run on an MI355X:
    python tools/bench_region_links.py [--reps 15] [--kernels]"""
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
ap.add_argument("--blob-frames", type=int, default=256)
ap.add_argument("--noise-frames", type=int, default=16)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--host-frames", type=int, default=4, help="frames of the host legs (0: not measured)")
ap.add_argument("--kernels", action="store_true", help="per-pass split from a rocprofv3 run")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # the one workload a profiled child runs
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_links_bench.jsonl"))
args = ap.parse_args()
H, W, BLOBS = 1080, 1920, 40
PASSES = {"links_count_kernel": "count", "links_scan_pairs_kernel<true>": "count", "links_clear_kernel": "accumulate",
          "links_accumulate_kernel": "accumulate", "links_place_kernel<false>": "place",
          "links_scan_blocks_kernel": "place", "links_scan_pairs_kernel<false>": "place",
          "links_place_kernel<true>": "place"}


def blob_frames(torch, dev, n):
    """the discs of bench.py's synth_batch, bright on dark"""
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    yy = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    xx = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    pos = torch.rand((BLOBS, 2), generator=g, device=dev) * torch.tensor([W, H], device=dev)
    vel = (torch.rand((BLOBS, 2), generator=g, device=dev) - 0.5) * 6
    rad = 8 + torch.rand((BLOBS,), generator=g, device=dev) * 52
    out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    for first in range(0, n, 32):               # (in pieces: the float planes of 256 frames would not fit beside them)
        t = torch.arange(first, min(first + 32, n), device=dev, dtype=torch.float32).view(-1, 1, 1)
        m = torch.zeros((len(t), H, W), dtype=torch.bool, device=dev)
        for k in range(BLOBS):
            m |= ((xx - (pos[k, 0] + vel[k, 0] * t)) ** 2 + (yy - (pos[k, 1] + vel[k, 1] * t)) ** 2) <= rad[k] ** 2
        out[first:first + len(t)] = m.to(torch.uint8) * 200
    return out


def noise_frames(torch, dev, n):
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    return (torch.rand((n, H, W), generator=g, device=dev) < 0.5).to(torch.uint8) * 200


def engine(n, max_labels=0):
    from video.engine import FrameEngine
    return FrameEngine(size=(W, H), max_batch=n, thresh=100, connectivity=8, max_labels=max_labels)


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


def host_links(labels, prev=None):
    """the restatement: np.unique on the packed keys of every pair, reordered by the first pixel"""
    rows = []
    for t in range(len(labels)):
        E = labels[t - 1] if t else prev
        if E is None:
            continue
        E, L = E.ravel().astype(np.int64), labels[t].ravel().astype(np.int64)
        keys, first, count = np.unique(((E << 32) | L)[(E >= 1) & (L >= 1)], return_index=True, return_counts=True)
        order = np.argsort(first, kind="stable")
        rows.append((t, keys[order] >> 32, keys[order] & 0xffffffff, count[order]))
    return rows


def gpu_leg(name, frames, torch, dev, S):
    from video import _hip, ops
    L = _hip.lib()
    n = len(frames)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    eng = engine(n)
    try:
        eng.run_device(frames.data_ptr(), n, labels_ptr=labels.data_ptr(), counts_ptr=counts.data_ptr(), stream=S)
        torch.cuda.synchronize()
    finally:
        eng.close()
    buf = lambda nbytes: torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    nl, tot = buf(n * 4), torch.zeros(2, dtype=torch.int64, device=dev)

    def links(cap, ws, ws_bytes, rec):
        _hip.check(L.va_region_links(None, labels.data_ptr(), n, H, W, nl.data_ptr(), tot.data_ptr(), rec.data_ptr(),
                                     cap, ws.data_ptr(), ws_bytes, S))
    ws0 = L.va_region_links_workspace_bytes(n, H, W, 0)
    small, nothing = buf(ws0), buf(16)
    links(0, small, ws0, nothing)                                        # need, then buffers with exact room
    torch.cuda.synchronize()
    need = int(tot[1])
    # capacity 0 and the least workspace: nothing is stored and the links are counted a table at a time (one timed call)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    links(0, small, ws0, nothing)
    b.record()
    torch.cuda.synchronize()
    short_ms, short_total = a.elapsed_time(b), int(tot[0])
    del small
    ws_bytes = L.va_region_links_workspace_bytes(n, H, W, need)
    ws, rec = buf(ws_bytes), buf(need * 16)
    best, med = timed(lambda: links(need, ws, ws_bytes, rec), torch)
    total = int(tot[0])
    assert short_total == total
    twin = torch.empty_like(labels)

    def copy_twice():
        for _ in range(2):
            _hip.check(L.va_memcpy_d2d(twin.data_ptr(), labels.data_ptr(), labels.numel() * 4, S))
    cbest, cmed = timed(copy_twice, torch)
    del twin
    dev_labels = ops.DeviceLabels(labels.data_ptr(), n, H, W)
    ops.region_links(dev_labels)
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = ops.region_links(dev_labels)
        wall.append((time.perf_counter() - t0) * 1e3)
    assert len(got.a) == total
    rows = [{"leg": name + "/va_region_links", "frames": n, "h": H, "w": W, "regions_per_frame": round(float(counts.float().mean()), 1),
             "links": total, "need": need, "need_over_total": round(need / max(total, 1), 3),
             "workspace_mb": round(ws_bytes / 2 ** 20, 1), "ms_per_call_min": round(best, 4),
             "ms_per_call_median": round(med, 4), "ms_per_frame": round(med / n, 5),
             "copy_labels_twice_ms_median": round(cmed, 4), "call_over_copy": round(med / cmed, 3),
             "label_gb": round(labels.numel() * 4 / 1e9, 3), "capacity_0_least_workspace_ms": round(short_ms, 3),
             "least_workspace_mb": round(ws0 / 2 ** 20, 1)},
            {"leg": name + "/ops.region_links", "frames": n, "first_capacity": ops.DEFAULT_LINK_CAPACITY,
             "launches": 1 if need <= ops.DEFAULT_LINK_CAPACITY else 2, "wall_ms_median": round(float(np.median(wall)), 3)}]
    if args.host_frames and not args.child:
        k = min(args.host_frames, n)
        t0 = time.perf_counter()
        part = labels[:k].cpu().numpy()
        down = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        found = host_links(part)
        host = (time.perf_counter() - t0) * 1e3
        want = K_rows(found)
        same = np.array_equal(want, np.stack([np.repeat(np.arange(n), np.diff(got.offsets)), got.a, got.b, got.count], 1)[
            :len(want)])
        rows.append({"leg": name + "/download_and_numpy", "frames_measured": k, "download_ms_per_frame": round(down / k, 3),
                     "numpy_ms_per_pair": round(host / max(k - 1, 1), 3),
                     "extrapolated_ms_for_the_stack": round(down / k * n + host / max(k - 1, 1) * (n - 1), 1),
                     "same_links_as_the_gpu": bool(same)})
    else:
        rows.append({"leg": name + "/download_and_numpy", "ms": "not measured"})
    return rows


def K_rows(found):
    return np.concatenate([np.stack([np.full(len(a), t), a, b, c], 1) for t, a, b, c in found]
                          or [np.zeros((0, 4), np.int64)])


def end_to_end(frames, torch, dev):
    """track_regions on resident frames against the loop that downloads labels and links on the host"""
    from video import ops
    from video.analysis.tracking import RegionTracker, track_regions
    n, batch = len(frames), 64
    stack = ops.DeviceFrames.upload(frames.cpu().numpy())
    eng = engine(batch, max_labels=64)
    try:
        track_regions(eng, stack, batch)
        t0 = time.perf_counter()
        tracks = track_regions(eng, stack, batch)
        gpu_s = time.perf_counter() - t0
        row = {"leg": "end_to_end/track_regions", "frames": n, "batch": batch, "tracks": int(max(i.max(initial=-1) for i in tracks.ids) + 1),
               "frames_per_s": round(n / gpu_s, 1)}
        k = min(args.host_frames, n)
        if k:
            part = stack.gather(range(k))
            try:
                t0 = time.perf_counter()
                out = eng.run_frames(part, want=("labels", "counts"))
                found = host_links(out["labels"])
                rows = K_rows(found)
                offsets = np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0], minlength=k))])
                RegionTracker().update((offsets, rows[:, 1], rows[:, 2], rows[:, 3]), out["counts"])
                host_s = time.perf_counter() - t0
            finally:
                part.release()
            row.update(host_linking_frames_measured=k, host_linking_frames_per_s=round(k / host_s, 2),
                       speedup=round((n / gpu_s) / (k / host_s), 1))
        else:
            row["host_linking_frames_per_s"] = "not measured"
        return row
    finally:
        eng.close()
        stack.release()


def kernel_split(workload):
    """one workload's va_region_links calls under rocprofv3: {pass: ms per call}, the mean over every call of the
    child run (the run for `need` and a short first launch of ops.region_links stop after the count)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "links", "--",
               sys.executable, os.path.abspath(__file__), "--child", workload, "--reps", str(args.reps), "--blob-frames",
               str(args.blob_frames), "--noise-frames", str(args.noise_frames)]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        out, calls = {}, 0
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"].replace("va::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                if name in PASSES:
                    out[PASSES[name]] = out.get(PASSES[name], 0.0) + float(row["TotalDurationNs"]) / 1e6
                if name == "links_scan_pairs_kernel<true>":
                    calls = int(row["Calls"])                   # one launch of it per call
        return {k: v / max(calls, 1) for k, v in out.items()}


def gpu_run():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for name, make, n in (("blobs", blob_frames, args.blob_frames), ("noise", noise_frames, args.noise_frames)):
        if args.child not in (None, name):
            continue
        frames = make(torch, dev, n)
        rows += gpu_leg(name, frames, torch, dev, S)
        if name == "blobs" and not args.child:
            rows.append(end_to_end(frames, torch, dev))
        del frames
        torch.cuda.empty_cache()
    return rows


if args.child:
    gpu_run()
    sys.exit(0)

# (child processes: before this one opens the GPU)
splits = {name: kernel_split(name) for name in ("blobs", "noise")} if args.kernels else {}
rows = gpu_run()
for name in ("blobs", "noise"):
    split = splits.get(name)
    if split:
        rows.append({"leg": name + "/passes", "ms_per_call_mean": {k: round(v, 4) for k, v in split.items()},
                     "sum_ms": round(sum(split.values()), 4)})
    else:
        rows.append({"leg": name + "/passes", "ms_per_call_mean": "not measured"})
for row in rows:
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
