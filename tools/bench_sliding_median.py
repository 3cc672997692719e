#!/usr/bin/env python3
"""Time of the sliding-window median on the GPU (va_sliding_median_u8, va_sliding_median.hip; DESIGN.md §9, "Sliding
median").  Per workload, with HIP events on resident data, the median of --reps repetitions of one call of n frames
in the steady state (the window full, all three outputs written), and beside it in the same run
  va_memcpy_d2d of the input stack (one read and one write of what the call reads once), and
  for windows up to 255 the existing exact route: one va_temporal_ranks_u8 call with the median ranks on the W-plane
  window of an emitted frame, timed over up to eight consecutive frames and divided by their number.
The two routes alternate --rounds times; every round is reported.  Workloads:
  1080p monochrome, n = 256 a call, W = 25, 64, 101, 255, 1000, on a smooth moving scene and on noise
  1080p RGB and 4K monochrome, n = 256, W = 101, scene
  1080p monochrome, n = 32 a call, W = 101, scene (the cost of loading and storing the state per call)
The planes of every workload are checked against a sort of explicit windows on a strip of pixels before they are timed.
One JSON line per leg, appended to profiles/sliding_median_bench.jsonl (or --out).  Run on an MI355X:
    python tools/bench_sliding_median.py [--reps 15] [--rounds 3]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only", default="", help="run the legs whose name contains this")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_median_bench.jsonl"))
args = ap.parse_args()

SHAPES = {"1080p": (1080, 1920, 1), "1080p_rgb": (1080, 1920, 3), "4k": (2160, 3840, 1)}
WORKLOADS = (                                   # shape, content, frames a call, windows
    ("1080p", "scene", 256, (25, 64, 101, 255, 1000)),
    ("1080p", "noise", 256, (25, 64, 101, 255, 1000)),
    ("1080p_rgb", "scene", 256, (101,)),
    ("4k", "scene", 256, (101,)),
    ("1080p", "scene", 32, (101,)),
)
STRIP = 512


def stack_of(content, n, h, w, c, rng):
    """n frames (n, h * w * c) uint8.  noise: sixteen planes of noise, repeated with a shift of the values, so that
    every pixel's series jumps across the histogram.  scene: a smooth ground that drifts, two grey levels of sensor
    noise and a bright block that crosses the frame -- neighbouring pixels touch neighbouring bins"""
    px = h * w * c
    base = rng.integers(0, 256, (16, px), dtype=np.uint8)
    if content == "noise":
        return np.stack([base[i % 16] + np.uint8((37 * (i // 16)) % 256) for i in range(n)])
    yy, xx = np.mgrid[:h, :w]
    ground = (60 + 80 * np.sin(xx / 97.0) * np.cos(yy / 131.0) + 60).astype(np.uint8)
    ground = np.repeat(ground[:, :, None], c, axis=2)
    frames = np.empty((n, px), np.uint8)
    for i in range(n):
        f = ground + np.uint8(i // 32)
        x = (i * (w - 200)) // max(n, 1)
        f[h // 3:h // 3 + 160, x:x + 200] = 230
        frames[i] = f.reshape(px) + (base[i % 16] & 3)
    return frames


def restate(frames, window, first):
    """(lower, upper, diff) of the frames first .. of a strip, by sorting every window (all of them full)"""
    lower, upper = [], []
    for k in range(first, len(frames)):
        ordered = np.sort(frames[k - window:k], axis=0)
        lower.append(ordered[(window - 1) // 2])
        upper.append(ordered[window // 2])
    lower, upper = np.array(lower), np.array(upper)
    diff = np.abs(2 * frames[first:].astype(np.int64) - lower - upper) >> 1
    return lower, upper, np.minimum(diff, 255).astype(np.uint8)


def main():
    from video import _hip
    L = _hip.lib()
    rng = np.random.default_rng(5)
    start, stop = C.c_void_p(), C.c_void_p()
    _hip.check(L.va_event_create(C.byref(start)))
    _hip.check(L.va_event_create(C.byref(stop)))

    def timed(call, reps):
        call()
        _hip.check(L.va_stream_sync(None))
        ms = []
        for _ in range(reps):
            _hip.check(L.va_event_record(start, None))
            call()
            _hip.check(L.va_event_record(stop, None))
            _hip.check(L.va_event_sync(stop))
            one = C.c_float()
            _hip.check(L.va_event_elapsed_ms(start, stop, C.byref(one)))
            ms.append(one.value)
        return float(np.median(ms)), float(min(ms))

    rows = []
    for shape, content, n, windows in WORKLOADS:
        h, w, c = SHAPES[shape]
        px = h * w * c
        if args.only and args.only not in "%s_%s_n%d" % (shape, content, n):
            continue
        stack = stack_of(content, n, h, w, c, rng)
        src, twin = _hip.DeviceBuffer.from_array(stack), _hip.DeviceBuffer(n * px)
        outs = [_hip.DeviceBuffer(n * px) for _ in range(3)]
        ranks_out = _hip.DeviceBuffer(2 * px)
        try:
            copy_ms, copy_best = timed(lambda: _hip.check(L.va_memcpy_d2d(twin.ptr, src.ptr, n * px, None)), args.reps)
            for window in windows:
                name = "%s_%s_n%d_w%d" % (shape, content, n, window)
                nstate = int(L.va_sliding_median_state_bytes(px, window))
                state = _hip.DeviceBuffer(nstate)
                seen = [0]

                def call():
                    _hip.check(L.va_sliding_median_u8(src.ptr, n, px, px, window, seen[0], state.ptr, outs[0].ptr,
                                                      outs[1].ptr, outs[2].ptr, None))
                    seen[0] += n
                try:
                    _hip.check(L.va_memset(state.ptr, 0, nstate, None))
                    passes = (window + n - 1) // n + 1              # the stack again and again until the window is full
                    for _ in range(passes):
                        call()
                    at = px // 2
                    series = np.concatenate([stack[:, at:at + STRIP]] * passes)
                    first = len(series) - min(n, 8)
                    want = restate(series, window, first)
                    tail = len(series) - first
                    for buf, plane in zip(outs, want):
                        got = np.empty((tail, px), np.uint8)        # the last frames of the last pass
                        _hip.check(L.va_memcpy_d2h(got.ctypes.data, buf.ptr + (n - tail) * px, got.nbytes, None))
                        _hip.check(L.va_stream_sync(None))
                        assert np.array_equal(got[:, at:at + STRIP], plane), name
                    rk = np.array(sorted({(window - 1) // 2, window // 2}), np.int32)
                    emitted = min(8, n - window) if window <= 255 else 0

                    def old_route():
                        for k in range(window, window + emitted):
                            _hip.check(L.va_temporal_ranks_u8(src.ptr + (k - window) * px, window, px, px,
                                                              rk.ctypes.data, len(rk), ranks_out.ptr, None))
                    rounds = []
                    for _ in range(args.rounds):
                        ms, best = timed(call, args.reps)
                        one = {"ms_median": round(ms, 4), "ms_min": round(best, 4),
                               "us_per_frame": round(1e3 * ms / n, 3)}
                        if emitted > 0:
                            old_ms, _ = timed(old_route, args.reps)
                            one["ranks_route_us_per_frame"] = round(1e3 * old_ms / emitted, 3)
                            one["faster_than_ranks_route"] = bool(ms / n < old_ms / emitted)
                        rounds.append(one)
                finally:
                    state.free()
                ms = float(np.median([r["ms_median"] for r in rounds]))
                hist = nstate - window * ((px + 127) // 128) * 128
                # per frame and pixel: the entering byte, the leaving byte, three output bytes, the ring's byte for
                # the last `window` frames of the call; per call the histograms and trackers in and out
                traffic = n * px * 5 + min(n, window) * px + 2 * hist
                rows.append({"leg": name + "/va_sliding_median_u8", "h": h, "w": w, "c": c, "n": n, "window": window,
                             "content": content, "state_bytes": nstate, "state_bytes_per_pixel": round(nstate / px, 1),
                             "rounds": rounds, "copy_d2d_ms_median": round(copy_ms, 4),
                             "copy_d2d_ms_min": round(copy_best, 4), "ratio_to_copy": round(ms / copy_ms, 3),
                             "derived_bytes_per_call": traffic, "derived_bytes_per_frame_pixel": round(traffic / n / px, 2),
                             "derived_tb_per_s": round(traffic / ms / 1e9, 3), "reps": args.reps})
                print(json.dumps(rows[-1]), flush=True)
        finally:
            for b in [src, twin, ranks_out] + outs:
                b.free()
    L.va_event_destroy(start)
    L.va_event_destroy(stop)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
