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
  optimized_batch  get_centerlines_optimized of the estimate leg's 256 worms against the loop of 256
            Polygon.get_centerline_optimized calls in the same process (gentle parameters and the defaults), wall
            time on the host; where the batch's time goes (estimates, gradients with their uploads, matrix
            inversions, the snake call, the rest of the host code); and the kernels alone by HIP events on
            device-resident tables: fill + distance transform + ragged gradients, and the ragged snake
            (--only-optimized runs this leg alone)
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
ap.add_argument("--only-optimized", action="store_true", help="run the optimized_batch leg alone")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygon_bench.jsonl"))
ap.add_argument("--tag", default="", help="written into every row as \"tree\": which tree or commit was measured")
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


def optimized_batch_legs(torch, polys):
    """get_centerlines_optimized against the per-polygon loop, the batch's breakdown and its kernels"""
    from video import _hip, ops
    from video.analysis import shapes
    from video.analysis.active_contour import ActiveContour
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    m = len(polys)
    rects = [p.get_bounding_rect(margin=1) for p in polys]
    contours = [np.asarray(p.contour).astype(np.int64) for p in polys]
    rows = []
    for name, params in (("gentle", dict(alpha=10.0, beta=100.0, gamma=0.01, spacing=5, max_iterations=60)),
                         ("default", dict())):
        batch = shapes.get_centerlines_optimized(polys, **params)
        loop = [p.get_centerline_optimized(**params) for p in polys]
        assert all(np.array_equal(a, b) for a, b in zip(batch, loop)), "batch and loop differ"
        b_best, b_med = wall(lambda: shapes.get_centerlines_optimized(polys, **params))
        l_best, l_med = wall(lambda: [p.get_centerline_optimized(**params) for p in polys])
        # where the batch's time goes: its parts alone, and the spies' clocks inside one batched call
        e_best, _ = wall(lambda: shapes.get_centerline_estimates(polys))
        g_best, _ = wall(lambda: [b.free() for b in ops.centerline_gradients(contours, rects)[:2]])
        clock, seen = {"inv": 0.0, "snake": 0.0}, {}
        inv, snake = ActiveContour.get_evolution_matrix, ops.active_contour_ragged

        def spy_inv(self, N, ds):
            t = time.perf_counter()
            out = inv(self, N, ds)
            clock["inv"] += time.perf_counter() - t
            return out

        def spy_snake(*a, **kw):
            seen["args"] = a
            t = time.perf_counter()
            out = snake(*a, **kw)
            clock["snake"] += time.perf_counter() - t
            return out
        ActiveContour.get_evolution_matrix, ops.active_contour_ragged = spy_inv, spy_snake
        try:
            shapes.get_centerlines_optimized(polys, **params)
        finally:
            ActiveContour.get_evolution_matrix, ops.active_contour_ragged = inv, snake
        inv_ms, snake_ms = clock["inv"] * 1e3, clock["snake"] * 1e3
        row = {"leg": "optimized_batch", "params": name, "polygons": m, "batch_ms_min": round(b_best, 2),
               "batch_ms_median": round(b_med, 2), "loop_ms_min": round(l_best, 2), "loop_ms_median": round(l_med, 2),
               "batch_ms_per_polygon": round(b_best / m, 3), "loop_ms_per_polygon": round(l_best / m, 3),
               "speedup": round(l_best / b_best, 2), "estimates_ms": round(e_best, 2),
               "gradients_call_ms": round(g_best, 2), "matrix_inversions_ms": round(inv_ms, 2),
               "snake_call_ms": round(snake_ms, 2),
               "host_rest_ms": round(b_best - e_best - g_best - inv_ms - snake_ms, 2)}
        # the snake kernel alone, on the tables of that call
        fx, fy, shp, off, pts, npts, items, mats, moff, flags, vals, gamma, tol, max_it = seen["args"]
        t = {k: torch.from_numpy(np.ascontiguousarray(v, dt)).to(dev) for k, v, dt in (
            ("shp", shp, np.int32), ("off", off, np.int64), ("pts", pts, np.float64), ("n", npts, np.int32),
            ("it", items, np.int32), ("mats", mats, np.float64), ("moff", moff, np.int64), ("fl", flags, np.uint8),
            ("va", vals, np.float64))}
        grads = ops.centerline_gradients(contours, rects)
        total = int((grads[2][:, 0].astype(np.int64) * grads[2][:, 1]).sum())
        work, its = t["pts"].clone(), torch.empty(len(npts), dtype=torch.int32, device=dev)
        tvs = torch.empty(len(npts), dtype=torch.float64, device=dev)

        def snake_kernel():
            _hip.check(L.va_active_contour_ragged(
                grads[0].ptr, grads[1].ptr, t["shp"].data_ptr(), t["off"].data_ptr(), total, m, len(npts), pts.shape[1],
                t["n"].data_ptr(), t["it"].data_ptr(), t["mats"].data_ptr(), t["moff"].data_ptr(), t["mats"].numel(),
                t["fl"].data_ptr(), t["va"].data_ptr(), float(gamma), float(tol), int(max_it), work.data_ptr(),
                its.data_ptr(), tvs.data_ptr(), S))
        ms = []
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.reps + 1):
            work.copy_(t["pts"])
            a.record()
            snake_kernel()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        grads[0].free()
        grads[1].free()
        row.update({"snakes": len(npts), "max_points": int(pts.shape[1]), "iterations_mean": round(float(its.float().mean()), 1),
                    "snake_kernel_ms_min": round(min(ms[1:]), 3)})
        rows.append(row)
    # fill + distance transform + ragged gradients, device-resident, as centerline_gradients launches them
    verts, vert_off, bx = ops._fill_tables(contours, rects, "bench")
    _, shapes_, offsets, sizes, total = ops._pack_ragged(bx[:, [3, 2]])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (
        ("v", verts), ("vo", vert_off), ("b", bx.astype(np.int32)), ("s", shapes_), ("o", offsets))}
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    dist = torch.empty(total, dtype=torch.float32, device=dev)
    gx, gy = (torch.empty(total, dtype=torch.float64, device=dev) for _ in range(2))
    st = torch.empty(3 * m, dtype=torch.int32, device=dev)
    assert int(sizes.max()) <= ops.GRAD_CLASSES[-1], "the worms fit the resident kernel"
    launches, lo = [], 0                  # one launch per size class, as video.ops launches them
    for cap in ops.GRAD_CLASSES:
        idx = np.flatnonzero((sizes > lo) & (sizes <= cap))
        lo = cap
        if len(idx):
            launches.append((torch.from_numpy(np.ascontiguousarray(shapes_[idx])).to(dev),
                             torch.from_numpy(np.ascontiguousarray(offsets[idx])).to(dev), len(idx),
                             int(sizes[idx].max())))

    def fill():
        _hip.check(L.va_fill_poly(d["v"].data_ptr(), d["vo"].data_ptr(), len(verts), d["b"].data_ptr(), d["o"].data_ptr(),
                                  total, m, 1, mask.data_ptr(), st.data_ptr(), S))

    def dt():
        _hip.check(L.va_distance_transform_l2_5(mask.data_ptr(), d["s"].data_ptr(), d["o"].data_ptr(), total, m,
                                                int(shapes_[:, 1].max()), dist.data_ptr(), st.data_ptr() + 4 * m, S))

    def grad():
        first = 2 * m
        for sb, ob, count, max_pixels in launches:
            _hip.check(L.va_potential_gradients_ragged(dist.data_ptr(), _hip.VA_F32, sb.data_ptr(), ob.data_ptr(), total,
                                                       count, max_pixels, 1.0, gx.data_ptr(), gy.data_ptr(),
                                                       st.data_ptr() + 4 * first, S))
            first += count

    def chain():
        fill()
        dt()
        grad()
    row = {"leg": "optimized_batch_kernels", "polygons": m, "pixels": total,
           "gradient_launches": [[count, max_pixels] for _, _, count, max_pixels in launches]}
    for key, call in (("fill_ms", fill), ("dt_ms", dt), ("gradients_ms", grad), ("chain_ms", chain)):
        row[key + "_min"], row[key + "_median"] = (round(v, 4) for v in timed(call, torch))
    assert int(st.abs().max().item()) == 0
    row["gradients_gb_per_s"] = round(total * 20 / row["gradients_ms_min"] / 1e6, 2)      # 4 B read, 16 B written
    rows.append(row)
    return rows


def gpu_run():
    import torch
    if args.only_optimized:
        from video.analysis.shapes import Polygon
        return optimized_batch_legs(torch, [Polygon(c) for c in worms(args.estimates, seed=3)])
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
    rows += optimized_batch_legs(torch, polys)
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
if not args.no_cpu and not args.only_optimized:
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
        if args.tag:
            row["tree"] = args.tag
        f.write(json.dumps(row) + "\n")
