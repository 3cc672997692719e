#!/usr/bin/env python3
"""Time of the temporal rank planes on the GPU (va_temporal_ranks_u8, va_median.hip; DESIGN.md §9, "Temporal median").
Per workload, with HIP events on resident data, the median of --reps repetitions of the call, and beside it
va_memcpy_d2d of the same stack in the same run (one read and one write of what the call reads once) and the ratio:
  1080p monochrome, t = 25, 64, 101, 255, ranks = the medians
  1080p monochrome, t = 64, eight ranks
  1080p RGB, t = 64, the medians
  4K monochrome, t = 64, the medians
The planes of every workload are checked against np.sort on a strip of columns before they are timed.
End to end: ops.temporal_median of a 64 x 270 x 1920 host stack (upload, call and download, wall clock) against
np.median(axis=0) of the same stack on one core; both scaled by four are the 1080p figures.
One JSON line per leg, appended to profiles/temporal_median_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_temporal_median.py [--reps 15]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--host-reps", type=int, default=3, help="repetitions of the end-to-end legs (0: not measured)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_median_bench.jsonl"))
args = ap.parse_args()

WORKLOADS = (                                   # name, t, h, w, c, ranks (None: the medians)
    ("1080p_t25", 25, 1080, 1920, 1, None),
    ("1080p_t64", 64, 1080, 1920, 1, None),
    ("1080p_t101", 101, 1080, 1920, 1, None),
    ("1080p_t255", 255, 1080, 1920, 1, None),
    ("1080p_t64_8ranks", 64, 1080, 1920, 1, [0, 6, 16, 31, 32, 47, 57, 63]),
    ("1080p_rgb_t64", 64, 1080, 1920, 3, None),
    ("4k_t64", 64, 2160, 3840, 1, None),
)


def stack_of(t, px, rng):
    """t planes of px bytes: eight planes of noise, repeated with a shift of the values (the kernels' time does not
    depend on the content: the network and the counting passes are the same for every column)"""
    base = rng.integers(0, 256, (8, px), dtype=np.uint8)
    return np.stack([base[i % 8] + np.uint8((37 * (i // 8)) % 256) for i in range(t)])


def main():
    from video import _hip, ops
    L = _hip.lib()
    rng = np.random.default_rng(5)
    start, stop = C.c_void_p(), C.c_void_p()
    _hip.check(L.va_event_create(C.byref(start)))
    _hip.check(L.va_event_create(C.byref(stop)))

    def timed(call):
        call()
        _hip.check(L.va_stream_sync(None))
        ms = []
        for _ in range(args.reps):
            _hip.check(L.va_event_record(start, None))
            call()
            _hip.check(L.va_event_record(stop, None))
            _hip.check(L.va_event_sync(stop))
            one = C.c_float()
            _hip.check(L.va_event_elapsed_ms(start, stop, C.byref(one)))
            ms.append(one.value)
        return float(np.median(ms)), float(min(ms))

    rows = []
    for name, t, h, w, c, ranks in WORKLOADS:
        px = h * w * c
        ranks = sorted({(t - 1) // 2, t // 2}) if ranks is None else ranks
        rk = np.array(ranks, np.int32)
        stack = stack_of(t, px, rng)
        src, twin, out = _hip.DeviceBuffer.from_array(stack), _hip.DeviceBuffer(t * px), _hip.DeviceBuffer(len(rk) * px)
        try:
            call = lambda: _hip.check(L.va_temporal_ranks_u8(src.ptr, t, px, px, rk.ctypes.data, len(rk), out.ptr, None))
            copy = lambda: _hip.check(L.va_memcpy_d2d(twin.ptr, src.ptr, t * px, None))
            call()
            got = out.download((len(rk), px), np.uint8)
            strip = slice(px // 2, px // 2 + 4096)
            assert np.array_equal(got[:, strip], np.sort(stack[:, strip], axis=0)[ranks]), name
            ms, best = timed(call)
            copy_ms, copy_best = timed(copy)
        finally:
            for b in (src, twin, out):
                b.free()
        rows.append({"leg": name + "/va_temporal_ranks_u8", "t": t, "h": h, "w": w, "c": c, "ranks": len(rk),
                     "ms_median": round(ms, 4), "ms_min": round(best, 4), "copy_d2d_ms_median": round(copy_ms, 4),
                     "copy_d2d_ms_min": round(copy_best, 4), "ratio_to_copy": round(ms / copy_ms, 3),
                     "stack_gb_per_s": round(t * px / ms / 1e6, 1), "reps": args.reps})
        print(json.dumps(rows[-1]), flush=True)

    if args.host_reps > 0:
        stack = stack_of(64, 270 * 1920, rng).reshape(64, 270, 1920)
        ops.temporal_median(stack)                                      # warm: the pool's buffers
        wall = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            got = ops.temporal_median(stack)
            wall.append(time.perf_counter() - t0)
        host = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = np.median(stack, axis=0)
            host.append(time.perf_counter() - t0)
        assert got.tobytes() == want.tobytes()
        g, n = float(np.median(wall)), float(np.median(host))
        rows.append({"leg": "64x270x1920/ops.temporal_median vs np.median(axis=0)", "gpu_wall_ms": round(g * 1e3, 2),
                     "numpy_one_core_ms": round(n * 1e3, 1), "speedup": round(n / g, 1),
                     "scaled_to_1080p_gpu_ms": round(4 * g * 1e3, 1), "scaled_to_1080p_numpy_ms": round(4 * n * 1e3, 1),
                     "reps": args.host_reps})
    else:
        rows.append({"leg": "64x270x1920/ops.temporal_median vs np.median(axis=0)", "result": "not measured"})
    print(json.dumps(rows[-1]), flush=True)
    L.va_event_destroy(start)
    L.va_event_destroy(stop)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
