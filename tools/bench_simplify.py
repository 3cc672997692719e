#!/usr/bin/env python3
"""The batched simplifiers (va_simplify.hip, ops.simplify_curves) against the per-curve Python loops.
  edges      the edge curves of a 16 x 1080p stack of blob skeletons (ops.skeleton_graphs) through Ramer-Douglas-
             Peucker at 0.1: the kernel by HIP events on device-resident tables, the whole ops.simplify_curves call
             (pack, upload, launch, download, split), and the loop of curves.simplify_curve over --loop-curves of the
             same curves in the same process
  contours   the contours of 64 x 1080p blob masks (ops.find_contours) through both methods, at the tolerance of a
             ladder that keeps closest to a tenth of the points: kernel, ops call, and per ring the pinned
             definition in Python (ops._simplify_on_host, the restatement the tests compare with) and, for
             Ramer-Douglas-Peucker, curves.simplify_curve, over --loop-curves rings
  crossover  batch sizes 1, 2, 4, ... 256 of edge curves (rdp) and of contours (visvalingam): the device call
             against the definition in Python; the first size from which the device call stays ahead is what
             ops.SIMPLIFY_DEVICE_MIN_BATCH should be
  graphs     256 worm polygons through shapes.get_morphological_graphs with batched_simplify off and on
Medians of --reps repetitions.  One JSON line per leg, appended to profiles/simplify_bench.jsonl (or --out).
Run on an MI355X:
    python tools/bench_simplify.py [--reps 15]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--frames", type=int, default=16, help="1080p skeleton frames of the edges leg")
ap.add_argument("--mask-frames", type=int, default=64, help="1080p blob masks of the contours leg")
ap.add_argument("--loop-curves", type=int, default=2000, help="curves the Python loops are timed on")
ap.add_argument("--polygons", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.jsonl"))
args = ap.parse_args()
H, W, BLOBS = 1080, 1920, 40


def generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blob_masks(n):
    """masks of the kind of bench.py's synth_batch and tools/bench_contours.py: 40 moving discs of radius 8 .. 60 a
    frame (NumPy's generator, so not the same discs)"""
    rng = np.random.default_rng(3)
    pos = rng.random((BLOBS, 2)) * (W, H)
    vel = (rng.random((BLOBS, 2)) - 0.5) * 6
    rad = 8 + rng.random(BLOBS) * 52
    m = np.zeros((n, H, W), np.uint8)
    for t in range(n):
        for k in range(BLOBS):
            cx, cy, r = pos[k, 0] + vel[k, 0] * t, pos[k, 1] + vel[k, 1] * t, rad[k]
            x0, x1 = max(int(cx - r), 0), min(int(cx + r) + 2, W)
            y0, y1 = max(int(cy - r), 0), min(int(cy + r) + 2, H)
            if x0 < x1 and y0 < y1:
                yy, xx = np.mgrid[y0:y1, x0:x1]
                m[t, y0:y1, x0:x1] |= ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).astype(np.uint8)
    return m


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), float(np.median(ts))


def kernel_ms(curves_, tol, method, closed, reps):
    """the launch alone by HIP events, tables, outputs and workspace resident on the device: (min, median, kept)"""
    from video import _hip
    L = _hip.lib()
    arrs = [np.ascontiguousarray(c, np.float64).reshape(-1, 2) for c in curves_]
    m = len(arrs)
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    npoints = int(off[-1])
    up = [_hip.DeviceBuffer.from_array(a) for a in (np.concatenate(arrs), off, np.full(m, float(tol)))]
    need = L.va_simplify_visvalingam_workspace_bytes(npoints)
    outs = [_hip.DeviceBuffer(b) for b in (npoints, 4 * m, 4 * m, need)]

    def call():
        if method == "rdp":
            _hip.check(L.va_simplify_rdp(up[0].ptr, up[1].ptr, npoints, m, up[2].ptr, outs[0].ptr, outs[1].ptr,
                                         outs[2].ptr, None))
        else:
            _hip.check(L.va_simplify_visvalingam(up[0].ptr, up[1].ptr, npoints, m, up[2].ptr, int(closed), outs[0].ptr,
                                                 outs[1].ptr, outs[2].ptr, outs[3].ptr, need, None))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _hip.check(L.va_event_create(C.byref(e)))
    ms, one = [], C.c_float()
    for _ in range(reps + 1):
        _hip.check(L.va_event_record(ev[0], None))
        call()
        _hip.check(L.va_event_record(ev[1], None))
        _hip.check(L.va_event_sync(ev[1]))
        _hip.check(L.va_event_elapsed_ms(ev[0], ev[1], C.byref(one)))
        ms.append(one.value)
    assert not outs[2].download((m,), np.int32).any()
    kept = int(outs[1].download((m,), np.int32).astype(np.int64).sum())
    for e in ev:
        L.va_event_destroy(e)
    for b in up + outs:
        b.free()
    return min(ms[1:]), float(np.median(ms[1:])), kept


def tenth(curves_, method, closed):
    """the tolerance of a ladder whose kept fraction is closest to a tenth, and that fraction"""
    points = sum(len(c) for c in curves_)
    best = None
    for tol in (0.25, 0.5, 0.75, 1, 1.5, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
        frac = kernel_ms(curves_, tol, method, closed, 1)[2] / points
        if best is None or abs(frac - 0.1) < abs(best[1] - 0.1):
            best = (tol, frac)
    return best


def batch_row(name, curves_, tol, method, closed, loops):
    """one batch: kernel, ops call, and the per-curve loops on the first --loop-curves curves, scaled to the batch"""
    from video import ops
    m, points = len(curves_), sum(len(c) for c in curves_)
    k_min, k_med, kept = kernel_ms(curves_, tol, method, closed, args.reps)
    o_min, o_med = wall(lambda: ops.simplify_curves(curves_, tol, method=method, closed=closed), args.reps)
    some = curves_[:args.loop_curves]
    share = sum(len(c) for c in some) / points
    row = {"leg": name, "method": method, "closed": bool(closed), "tolerance": tol, "curves": m, "points": points,
           "kept_points": kept, "kept_fraction": round(kept / points, 4), "kernel_ms_min": round(k_min, 4),
           "kernel_ms_median": round(k_med, 4), "ops_call_ms_min": round(o_min, 3),
           "ops_call_ms_median": round(o_med, 3), "loop_curves": len(some), "loop_share_of_points": round(share, 4)}
    for label, fn in loops:
        l_min, l_med = wall(lambda: [fn(c) for c in some], 3)
        row[label + "_ms_median"] = round(l_med, 2)
        row[label + "_ms_scaled_to_batch"] = round(l_med / share, 1)
        row["speedup_over_" + label] = round(l_med / share / o_med, 1)
    return row


def crossover(name, curves_, tol, method, closed, monkey):
    from video import ops
    scan, first = [], None
    for b in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        monkey(1)
        d_min, _ = wall(lambda: ops.simplify_curves(curves_[:b], tol, method=method, closed=closed), args.reps)
        monkey(1 << 30)
        h_min, _ = wall(lambda: ops.simplify_curves(curves_[:b], tol, method=method, closed=closed), args.reps)
        scan.append([b, round(d_min, 4), round(h_min, 4)])
    for b, d, h in reversed(scan):
        if d >= h:
            break
        first = b
    return {"leg": "crossover", "curves": name, "method": method, "mean_points": round(float(np.mean(
        [len(c) for c in curves_[:256]])), 1), "batch_device_ms_python_ms": scan, "device_ahead_from": first}


def main():
    from video import _hip, ops
    from video.analysis import curves, shapes
    masks = blob_masks(args.mask_frames)
    _hip.lib()
    T = generator("make_golden_skeleton_graph").thinning()
    threshold = ops.SIMPLIFY_DEVICE_MIN_BATCH

    def monkey(v):
        ops.SIMPLIFY_DEVICE_MIN_BATCH = v
    rows = []
    frames = np.stack([T.blob(2000 + k, 1080, 1920, 4.0, 0.0) for k in range(args.frames)])
    edges = [c for g in ops.skeleton_graphs(ops.guo_hall_thinning(frames)) for c in g.curves]
    rows.append(batch_row("edges", edges, 0.1, "rdp", False,
                          [("simplify_curve_loop", lambda c: curves.simplify_curve(c, 0.1))]))
    rings = [c.reshape(-1, 2) for f in ops.find_contours(masks) for c in f]
    for method, closed in (("rdp", False), ("visvalingam", True)):
        tol, _ = tenth(rings, method, closed)
        loops = [("python_definition", lambda c, t=tol, me=method, cl=closed: ops._simplify_on_host(c, t, me, cl))]
        if method == "rdp":
            loops.append(("simplify_curve_loop", lambda c, t=tol: curves.simplify_curve(c, t)))
        rows.append(batch_row("contours", rings, tol, method, closed, loops))
    rows.append(crossover("edges", edges, 0.1, "rdp", False, monkey))
    rows.append(crossover("contours", rings, 2.0, "visvalingam", True, monkey))
    monkey(threshold)
    rng = np.random.default_rng(0)
    polys = [shapes.Polygon(T.POL.worm(length=float(rng.uniform(70, 110)), width=float(rng.uniform(5, 9)),
                                       bend=float(rng.uniform(5, 15)), x0=float(rng.uniform(0, 1000)),
                                       y0=float(rng.uniform(20, 1000)), phase=float(rng.uniform(0, 3))))
             for _ in range(args.polygons)]
    for on in (False, True):
        g_min, g_med = wall(lambda: shapes.get_morphological_graphs(polys, batched_simplify=on), args.reps)
        rows.append({"leg": "graphs", "polygons": len(polys), "batched_simplify": on, "ms_min": round(g_min, 2),
                     "ms_median": round(g_med, 2)})
    rows.append({"leg": "setting", "SIMPLIFY_DEVICE_MIN_BATCH": threshold, "reps": args.reps})
    with open(args.out, "a") as f:
        for row in rows:
            print(json.dumps(row))
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
