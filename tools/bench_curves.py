#!/usr/bin/env python3
"""The batched equidistant resampling (va_curves.hip, ops.curves_equidistant) against the per-curve Python loop.
  batch     256 and 4096 curves of worm-like size (8-connected pixel paths of 50-150 points, 8-27 output points)
            in spacing mode (spacing 7.5) and in count mode (count 16): the three kernels by HIP events on
            device-resident tables, the whole ops.curves_equidistant call (pack, upload, launches, download,
            split), and the loop of curves.make_curve_equidistant over the same curves in the same process
  crossover batch sizes 1, 2, 4, ... 256: the ops call against the loop, both modes; the first size from which the
            device call stays ahead is what ops.CURVES_DEVICE_MIN_BATCH should be
Count mode runs with one lane per curve, the only kernel shape the library has.  One JSON line per leg, appended to
profiles/curves_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_curves.py [--reps 7]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="*", default=[256, 4096])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curves_bench.jsonl"))
args = ap.parse_args()

SPACING, COUNT = 7.5, 16


def worm_paths(m, seed):
    """m 8-connected pixel paths of 50-150 points that mostly keep their heading"""
    rng = np.random.default_rng(seed)
    steps = np.array([(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)])
    out = []
    for _ in range(m):
        n = int(rng.integers(50, 151))
        h = (int(rng.integers(8)) + np.cumsum(rng.choice((-1, 0, 0, 0, 0, 1), n - 1))) % 8
        out.append(np.vstack([[0, 0], np.cumsum(steps[h], axis=0)]) + rng.integers(5, 400, 2))
    return out


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return min(ts), float(np.median(ts))


def kernels_ms(curves_, spacing, count, reps):
    """the three launches alone by HIP events, tables and outputs resident on the device"""
    import ctypes as C
    from video import _hip
    L = _hip.lib()
    arrs = [np.ascontiguousarray(c, np.float64) for c in curves_]
    m = len(arrs)
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    sp = np.full(m, 0.0 if spacing is None else spacing)
    ct = np.full(m, 0 if count is None else count, np.int32)
    cap = int(off[-1]) + m * (count or 0) + 8 * m
    up = [_hip.DeviceBuffer.from_array(a) for a in (np.concatenate(arrs), off, sp, ct)]
    outs = [_hip.DeviceBuffer(b) for b in (4 * m, 8 * (m + 1), 8 * m, 4 * m, 8, 16 * cap, 8 * m)]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _hip.check(L.va_event_create(C.byref(e)))
    ms, one = [], C.c_float()
    for _ in range(reps + 1):
        _hip.check(L.va_event_record(ev[0], None))
        _hip.check(L.va_curves_equidistant(up[0].ptr, up[1].ptr, int(off[-1]), m, up[2].ptr, up[3].ptr, None,
                                           outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr,
                                           outs[5].ptr, cap, outs[6].ptr, None))
        _hip.check(L.va_event_record(ev[1], None))
        _hip.check(L.va_event_sync(ev[1]))
        _hip.check(L.va_event_elapsed_ms(ev[0], ev[1], C.byref(one)))
        ms.append(one.value)
    total = int(outs[4].download((1,), np.int64)[0])
    assert total <= cap and not outs[3].download((m,), np.int32).any()
    for e in ev:
        L.va_event_destroy(e)
    for b in up + outs:
        b.free()
    return min(ms[1:]), float(np.median(ms[1:])), total


def main():
    from video import _hip, ops
    from video.analysis import curves
    _hip.lib()
    rows = [{"leg": "host", "norm_is_pinned": bool(ops.host_norm_is_pinned()),
             "threshold": ops.CURVES_DEVICE_MIN_BATCH}]
    modes = (("spacing", dict(spacing=SPACING)), ("count", dict(count=COUNT)))
    for m in args.sizes:
        cs = worm_paths(m, seed=m)
        for name, kw in modes:
            got = ops.curves_equidistant(cs, **kw)
            loop = [np.asarray(curves.make_curve_equidistant(c, **kw)) for c in cs]
            same = all(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
                       for a, b in zip(got, loop))
            k_min, k_med, total = kernels_ms(cs, kw.get("spacing"), kw.get("count"), args.reps)
            o_min, o_med = wall(lambda: ops.curves_equidistant(cs, **kw), args.reps)
            l_min, l_med = wall(lambda: [curves.make_curve_equidistant(c, **kw) for c in cs], max(3, args.reps // 2))
            sizes = [len(g) for g in got]
            rows.append({"leg": "batch", "mode": name, "curves": m, "kernel": "one lane per curve",
                         "input_points": int(sum(len(c) for c in cs)), "output_points": total,
                         "output_points_min_max": [min(sizes), max(sizes)], "bits_equal_loop": bool(same),
                         "kernels_ms_min": round(k_min, 4), "kernels_ms_median": round(k_med, 4),
                         "ops_call_ms_min": round(o_min, 3), "ops_call_ms_median": round(o_med, 3),
                         "python_loop_ms_min": round(l_min, 3), "python_loop_ms_median": round(l_med, 3),
                         "speedup": round(l_min / o_min, 2)})
    cs = worm_paths(256, seed=9)
    for name, kw in modes:
        scan, first = [], None
        for b in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            o_min, _ = wall(lambda: ops.curves_equidistant(cs[:b], **kw), args.reps)
            l_min, _ = wall(lambda: [curves.make_curve_equidistant(c, **kw) for c in cs[:b]], args.reps)
            scan.append([b, round(o_min, 4), round(l_min, 4)])
        for b, o, l in reversed(scan):
            if o >= l:
                break
            first = b
        rows.append({"leg": "crossover", "mode": name, "batch_ops_ms_loop_ms": scan, "device_ahead_from": first})
    with open(args.out, "a") as f:
        for row in rows:
            print(json.dumps(row))
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
