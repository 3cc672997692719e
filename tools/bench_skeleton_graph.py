#!/usr/bin/env python3
"""Throughput of skeleton graphs on the GPU (va_skeleton.hip):
  kernels   va_skeleton_graph on skeletons resident in HBM, HIP events around the call (capacities with room, so one
            run): 4096 worm skeletons (boxes of about 20 x 95) in one call, and a 16 x 1080p stack of blob skeletons;
            next to each, va_guo_hall_thinning_batch / va_guo_hall_thinning_u8 on the masks those skeletons came
            from, for scale
  calls     ops.skeleton_graphs on the same two batches, wall time with its copies and the split into per-item arrays
  polygons  256 worm polygons through shapes.get_morphological_graphs against a loop of
            Polygon.get_morphological_graph, wall time
  cpu       the restatement of the definition (tests/golden/make_golden_skeleton_graph.py) on one core, on the first
            64 worm skeletons and on one quarter-frame (540 x 960) blob skeleton
With --kernels the kernel legs run again in a child process under `rocprofv3 --kernel-trace --stats` and the time is
split per kernel.  One JSON line per leg, appended to profiles/skeleton_graph_bench.jsonl (or --out).
Run on an MI355X:
    python tools/bench_skeleton_graph.py [--reps 15] [--kernels]"""
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
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--polygons", type=int, default=256)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--kernels", action="store_true", help="per-kernel split from a rocprofv3 run")
ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_graph_bench.jsonl"))
args = ap.parse_args()


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator("make_golden_skeleton_graph")
T = G.thinning()


def worm_polygons(n, seed=0):
    from video.analysis.shapes import Polygon
    rng = np.random.default_rng(seed)
    return [Polygon(T.POL.worm(length=float(rng.uniform(70, 110)), width=float(rng.uniform(5, 9)),
                               bend=float(rng.uniform(5, 15)), x0=float(rng.uniform(0, 1000)),
                               y0=float(rng.uniform(20, 1000)), phase=float(rng.uniform(0, 3)))) for _ in range(n)]


def kernel_split():
    """this script's kernel legs under rocprofv3: {kernel: (calls, ms total)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "skeleton", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--worms",
               str(args.worms), "--frames", str(args.frames)]
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


def wall(call, reps=3):
    call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return min(ms), float(np.median(ms))


def graph_leg(torch, kind, skeletons):
    """va_skeleton_graph on device-resident skeletons"""
    from video import _hip, ops
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    flat, shapes, offsets, sizes, total = ops._pack_ragged(list(skeletons))
    m = len(shapes)
    d = {k: torch.from_numpy(v).to(dev) for k, v in (("m", flat), ("s", shapes), ("o", offsets))}
    capn, cape, capp = 1 << 20, 1 << 20, 1 << 23
    ws_bytes = L.va_skeleton_graph_workspace_bytes(total, m)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)              # noqa: E731
    ws, cnt, tot = u8(ws_bytes), u8(m * 8), torch.zeros(3, dtype=torch.int64, device=dev)
    nodes, edges, off, pts = u8(capn * 20), u8(cape * 24), u8((cape + 1) * 8), u8(capp * 8)

    def call():
        _hip.check(L.va_skeleton_graph(d["m"].data_ptr(), d["s"].data_ptr(), d["o"].data_ptr(), total, m,
                                       cnt.data_ptr(), tot.data_ptr(), nodes.data_ptr(), capn, edges.data_ptr(),
                                       off.data_ptr(), cape, pts.data_ptr(), capp, ws.data_ptr(), ws_bytes, S))
    best, med = timed(call, torch)
    totals = tot.cpu().numpy().tolist()
    assert totals[0] <= capn and totals[1] <= cape and totals[2] <= capp
    npts = np.frombuffer(edges.cpu().numpy()[:totals[1] * 24].tobytes(), ops.SKELETON_EDGE_DTYPE)["npoints"]
    return {"leg": "kernels", "skeletons": kind, "count": m, "pixels": total, "foreground": int(np.count_nonzero(flat)),
            "nodes": totals[0], "edges": totals[1], "points": totals[2],
            "longest_edge_points": int(npts.max()) if len(npts) else 0, "workspace_bytes": int(ws_bytes),
            "ms_per_call_min": round(best, 3), "ms_per_call_median": round(med, 3),
            "gpixels_per_s": round(total / med / 1e6, 2)}


def thinning_leg(torch, kind, masks):
    """the thinning call on the same batch, for scale: resident for a list, tiled for a stack"""
    from video import _hip, ops
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    if isinstance(masks, np.ndarray):
        n, h, w = masks.shape
        src = torch.from_numpy(masks).to(dev)
        need = L.va_guo_hall_thinning_scratch_bytes(n, h, w)
        scratch, dst = torch.empty(need, dtype=torch.uint8, device=dev), torch.empty_like(src)

        def call():
            _hip.check(L.va_guo_hall_thinning_u8(src.data_ptr(), scratch.data_ptr(), need, dst.data_ptr(), n, h, w, 0, 0,
                                                 None, None, S))
    else:
        flat, shapes, offsets, sizes, total = ops._pack_ragged(list(masks))
        m = len(shapes)
        d = {k: torch.from_numpy(v).to(dev) for k, v in (("m", flat), ("s", shapes), ("o", offsets))}
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        it, st = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2))
        words = max(ops._thin_words(a.shape) for a in masks)

        def call():
            _hip.check(L.va_guo_hall_thinning_batch(d["m"].data_ptr(), d["s"].data_ptr(), d["o"].data_ptr(), total, m,
                                                    words, out.data_ptr(), it.data_ptr(), st.data_ptr(), S))
    best, med = timed(call, torch)
    return {"leg": "thinning_for_scale", "masks": kind, "ms_per_call_min": round(best, 3),
            "ms_per_call_median": round(med, 3)}


def gpu_run():
    import torch
    from video import _hip, ops
    from video.analysis import shapes
    _hip.lib()
    polys = worm_polygons(args.worms)
    masks = shapes.get_masks(polys, 5)
    worms = ops.guo_hall_thinning(masks)
    frames = np.stack([T.blob(2000 + k, 1080, 1920, 4.0, 0.0) for k in range(args.frames)])
    skel_frames = ops.guo_hall_thinning(frames)
    rows = [graph_leg(torch, "worms", worms), thinning_leg(torch, "worms", masks),
            graph_leg(torch, "1080p_blob_skeletons", skel_frames), thinning_leg(torch, "1080p_blobs", frames)]
    if args.child:
        return rows
    for kind, batch in (("worms", worms), ("1080p_blob_skeletons", skel_frames)):
        best, med = wall(lambda: ops.skeleton_graphs(batch))
        rows.append({"leg": "call_with_copies", "skeletons": kind, "count": len(batch), "ms_min": round(best, 2),
                     "ms_median": round(med, 2)})
    some = polys[:args.polygons]
    best, med = wall(lambda: shapes.get_morphological_graphs(some))
    rows.append({"leg": "polygons_batched", "count": len(some), "ms_min": round(best, 2), "ms_median": round(med, 2),
                 "ms_per_polygon": round(med / len(some), 4)})
    best, med = wall(lambda: [p.get_morphological_graph() for p in some])
    rows.append({"leg": "polygons_loop", "count": len(some), "ms_min": round(best, 2), "ms_median": round(med, 2),
                 "ms_per_polygon": round(med / len(some), 4)})
    best, med = wall(lambda: ops.polygon_skeleton_graphs(
        [np.asarray(p.contour).astype(np.int64) for p in some], [p.get_bounding_rect(margin=5) for p in some]))
    rows.append({"leg": "polygons_device_part", "count": len(some), "ms_min": round(best, 2), "ms_median": round(med, 2),
                 "note": "fill + thinning + graph with copies; the rest of polygons_batched is networkx on the host"})
    if not args.no_cpu:
        t = time.perf_counter()
        for s in worms[:64]:
            G.skeleton_graph(s)
        rows.append({"leg": "cpu_restatement", "skeletons": "worms", "count": 64, "threads": 1,
                     "ms": round((time.perf_counter() - t) * 1e3, 1),
                     "pixels": int(sum(s.size for s in worms[:64]))})
        quarter = ops.guo_hall_thinning([T.blob(2000, 540, 960, 4.0, 0.0)])[0]
        t = time.perf_counter()
        G.skeleton_graph(quarter)
        rows.append({"leg": "cpu_restatement", "skeletons": "540x960_blob_skeleton", "count": 1, "threads": 1,
                     "ms": round((time.perf_counter() - t) * 1e3, 1), "pixels": int(quarter.size)})
    return rows


if args.child:
    gpu_run()
    sys.exit(0)

split = kernel_split() if args.kernels else None       # (a child process: before this one opens the GPU)
rows = gpu_run()
if split:
    total = sum(t for _, t in split.values())
    rows.append({"leg": "kernel_split", "reps": args.reps,
                 "kernels": {k: {"calls": c, "ms_total": round(t, 3), "share": round(t / total, 4)}
                             for k, (c, t) in sorted(split.items(), key=lambda kv: -kv[1][1])}})
for row in rows:
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
