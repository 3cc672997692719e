#!/usr/bin/env python3
"""Time of template matching on the GPU (va_template_match_u8, va_template_match.hip), method ccoeff_normed:
  track      256 x 1080p resident frames, 40 queries a frame (one per template), templates 32 x 32, windows of
             65 x 65 positions, best records only
  track+maps the same with the float64 score maps written
  full_map   the full map of one 1080p frame with a 64 x 64 template
  tracker    TemplateTracker.update end to end (wall clock) on the resident frames, in batches of 32
Per leg, with HIP events around the call and nothing else on the device, the least and the median of --reps
repetitions, and the multiply-accumulates of S_it (positions x template pixels) per second.  Beside them, measured in
the same run: the udot4 issue rate of tools/microbench/valu_rate (built on demand with hipcc), as the multiply-
accumulates per second it would give if every issue slot held a udot4 of S_it, and the fraction of it the call reaches;
and the path the call replaces -- the download of the frames plus a NumPy restatement on one core, on --host-queries
queries, extrapolated to the leg.  One JSON line per leg, appended to profiles/template_match_bench.jsonl (or --out); a
leg that did not run is written "not measured".  Run on an MI355X:
    python tools/bench_template_match.py [--reps 9]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--per-frame", type=int, default=40)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--host-queries", type=int, default=3, help="queries of the host leg (0: not measured)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_match_bench.jsonl"))
args = ap.parse_args()
H, W, METHOD = 1080, 1920, "ccoeff_normed"
SIMDS, LANES = 256 * 4, 64


def udot4_rate():
    """multiply-accumulates per second of the whole device if every issue slot of every SIMD held a udot4, from the
    VALU microbenchmark (a child process: before this one opens the GPU); None where it cannot be built or run"""
    src = os.path.join(ROOT, "tools", "microbench", "valu_rate.hip")
    exe = os.path.join(ROOT, "tools", "microbench", "valu_rate")
    try:
        if not os.path.exists(exe):
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe],
                           check=True, timeout=600)
        said = subprocess.run([exe], check=True, timeout=120, stdout=subprocess.PIPE).stdout.decode()
        ns = float(re.search(r"v_dot4_u32_u8\s+\S+ ms\s+-> (\S+) ns per wave-instr per SIMD", said).group(1))
        return 4 * LANES * SIMDS / (ns * 1e-9)
    except Exception as e:                                              # (reported as "not measured", not hidden)
        print("udot4 microbenchmark did not run:", e, file=sys.stderr)
        return None


def host_scores(frame, templ, x0, y0, nx, ny):
    """the NumPy restatement of one query (ccoeff_normed) on one core"""
    th, tw = templ.shape
    region = frame[y0:y0 + ny + th - 1, x0:x0 + nx + tw - 1].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(region, (th, tw))
    t = templ.astype(np.int64)
    n, s_t, s_tt = t.size, t.sum(), (t * t).sum()
    s_it, s_i, s_ii = (win * t).sum(axis=(2, 3)), win.sum(axis=(2, 3)), (win * win).sum(axis=(2, 3))
    den = np.sqrt((n * s_ii - s_i * s_i).astype(np.float64) * np.float64(n * s_tt - s_t * s_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0.0, 0.0, (n * s_it - s_i * s_t).astype(np.float64) / den)


class Leg(object):
    """the device buffers of one raw call on resident frames"""

    def __init__(self, torch, dev, frames, templates, queries, maps):
        from video import _hip
        self.torch, self.L = torch, _hip.lib()
        self.queries, self.templates = np.ascontiguousarray(queries, np.int32), templates
        shapes = np.array([t.shape for t in templates], np.int32)
        sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.positions = self.queries[:, 4].astype(np.int64) * self.queries[:, 5]
        self.macs = int((self.positions * sizes[self.queries[:, 1]]).sum())
        total, nq, m = int(self.positions.sum()), len(self.queries), len(templates)
        ws_bytes = self.L.va_template_match_workspace_bytes(nq, total, m)
        up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(dev)
        room = lambda nbytes: torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        self.keep = [frames, up(np.concatenate([t.reshape(-1) for t in templates])), up(shapes), up(offsets),
                     up(self.queries), room(nq * 24), room(total * 8 if maps else 0),
                     up(np.concatenate([[0], np.cumsum(self.positions)]).astype(np.int64)), room(ws_bytes)]
        p = [b.data_ptr() for b in self.keep]
        n = frames.shape[0]
        self.args = _hip.va_match_args(C.sizeof(_hip.va_match_args), _hip.MATCH_METHODS[METHOD], p[0], n, H, W, 0, H * W,
                                       p[1], p[2], p[3], m, p[4], nq, total, p[5], p[6] if maps else None,
                                       p[7] if maps else None, p[8], ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
        self.workspace_mb, self.maps_mb = ws_bytes / 2 ** 20, total * 8 / 2 ** 20 if maps else 0.0

    def call(self):
        from video import _hip
        _hip.check(self.L.va_template_match_u8(C.byref(self.args)))

    def timed(self):
        torch = self.torch
        self.call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps):
            a.record()
            self.call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return min(ms), float(np.median(ms))

    def best(self):
        from video import _hip
        self.torch.cuda.synchronize()
        return self.keep[5][:len(self.queries) * 24].cpu().numpy().view(_hip.MATCH_BEST_DTYPE)


def row_of(name, leg, rate, frames_host=None):
    least, median = leg.timed()
    macs_per_s = leg.macs / (median * 1e-3)
    row = {"leg": name, "method": METHOD, "queries": len(leg.queries), "positions": int(leg.positions.sum()),
           "multiply_accumulates": leg.macs, "ms_per_call_min": round(least, 4), "ms_per_call_median": round(median, 4),
           "tera_mac_per_s": round(macs_per_s / 1e12, 3), "workspace_mb": round(leg.workspace_mb, 1),
           "maps_mb": round(leg.maps_mb, 1)}
    if rate:
        row.update(udot4_issue_tera_mac_per_s=round(rate / 1e12, 2), fraction_of_udot4_issue_rate=round(macs_per_s / rate, 4))
    else:
        row["udot4_issue_tera_mac_per_s"] = "not measured"
    k = min(args.host_queries, len(leg.queries)) if frames_host is not None else 0
    if k:
        best = leg.best()
        t0 = time.perf_counter()
        same = True
        for q in range(k):
            f, t, x0, y0, nx, ny = leg.queries[q].tolist()
            scores = host_scores(frames_host[f], leg.templates[t], x0, y0, nx, ny)
            j, i = divmod(int(np.argmax(scores)), nx)
            same = same and (x0 + i, y0 + j, scores[j, i]) == (best["x"][q], best["y"][q], best["score"][q])
        per_mac = (time.perf_counter() - t0) / float((leg.positions[:k] * [leg.templates[t].size for t in leg.queries[:k, 1]]).sum())
        row.update(numpy_queries_measured=k, numpy_one_core_extrapolated_ms=round(per_mac * leg.macs * 1e3, 1),
                   numpy_same_best_as_the_gpu=bool(same))
    else:
        row["numpy_one_core_extrapolated_ms"] = "not measured"
    return row


def gpu_run(rate):
    import torch
    from video import ops
    from video.analysis.tracking import TemplateTracker
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n, k = args.frames, args.per_frame
    frames = torch.randint(0, 256, (n, H, W), generator=g, device=dev, dtype=torch.uint8)
    rng = np.random.default_rng(6)
    templates = [rng.integers(0, 256, (32, 32), dtype=np.uint8) for _ in range(k)]
    corners = np.stack([rng.integers(40, W - 140, k), rng.integers(40, H - 140, k)], axis=1)
    queries = np.array([(f, t, x - 32, y - 32, 65, 65) for f in range(n) for t, (x, y) in enumerate(corners.tolist())], np.int32)
    t0 = time.perf_counter()
    few = frames[:2].cpu().numpy()
    download_ms_per_frame = (time.perf_counter() - t0) * 1e3 / 2
    rows = []
    for name, maps in (("track", False), ("track+maps", True)):
        leg = Leg(torch, dev, frames, templates, queries, maps)
        row = row_of(name, leg, rate, few if not maps else None)
        if not maps:
            row.update(download_ms_per_frame=round(download_ms_per_frame, 3),
                       download_of_the_stack_ms=round(download_ms_per_frame * n, 1))
        rows.append(row)
        del leg
        torch.cuda.empty_cache()
    big = [rng.integers(0, 256, (64, 64), dtype=np.uint8)]
    leg = Leg(torch, dev, frames[:1], big, [(0, 0, 0, 0, W - 63, H - 63)], True)
    rows.append(row_of("full_map", leg, rate))
    del leg
    # the tracker, end to end: resident frames, batches of 32, only the best records cross
    walls = []
    for _ in range(3):
        tracker = TemplateTracker(templates, corners, 32, METHOD)
        t0 = time.perf_counter()
        for first in range(0, n, 32):
            part = ops.DeviceFrames(type("Borrowed", (), {"ptr": frames[first].data_ptr(), "nbytes": 32 * H * W})(),
                                    min(32, n - first), H, W, 1)
            tracker.update(part)
        walls.append(time.perf_counter() - t0)
    rows.append({"leg": "tracker", "frames": n, "templates": k, "radius": 32, "batch": 32,
                 "frames_per_s": round(n / min(walls), 1), "wall_ms_min": round(min(walls) * 1e3, 2)})
    return rows


rate = udot4_rate()
rows = gpu_run(rate)
for row in rows:
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
