"""Shared by tests/test_sliding_median_host.py, tests/test_gpu_sliding_median.py and
tests/golden/make_golden_sliding_median.py: two independent NumPy restatements of the sliding-window median (DESIGN.md
§9, "Sliding median"), the contents of its test clips, the fixture, the state-size formula restated, and the
stand-alone host program around va_sliding_median_math.h.

The definition, for a pixel and the absolute frame index k: the window is the frames max(0, k - W) .. k - 1, cnt =
min(k, W) values; lower[k] / upper[k] are the sorted window at ranks (cnt - 1) // 2 and cnt // 2, both 0 for the empty
window; diff[k] = min(255, |2 frame[k] - lower[k] - upper[k]| >> 1)."""
import os
import subprocess

import numpy as np

from temporal_median_checks import host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sliding_median_v1.npz")
TILE = 128                       # va_slide::kTilePixels
CONTENTS = ("noise", "ties", "alternating", "ascending", "descending", "constant", "scene")
WINDOWS = (1, 2, 3, 64, 255, 256, 300)
# (window, px, content) of every fixture case; each runs 3 W + 5 frames from the empty window
CASES = ((1, 1, "noise"), (1, 129, "ties"), (2, 17, "noise"), (2, 128, "alternating"), (3, 127, "noise"),
         (3, 260, "ascending"), (3, 16, "scene"), (64, 17, "noise"), (64, 128, "ties"), (64, 129, "alternating"),
         (64, 260, "noise"), (64, 127, "descending"), (64, 1, "scene"), (255, 17, "constant"), (255, 20, "noise"),
         (255, 17, "alternating"), (255, 1, "ties"), (256, 17, "noise"), (256, 20, "constant"),
         (256, 16, "alternating"), (300, 17, "noise"), (300, 20, "ties"), (300, 1, "ascending"),
         (300, 16, "descending"), (300, 19, "scene"))


def frames_of(window):
    return 3 * window + 5


def content(kind, n, px, rng):
    """(n, px) uint8 frames.  alternating: whole planes of 0 and 255 in turn (the median jumps between the ends of
    the histogram); constant: one value in column 0 (a counter reaches the window), a few outliers elsewhere; scene:
    a smooth drifting ground with an object that rests and moves on"""
    noise = rng.integers(0, 256, (n, px), dtype=np.uint8)
    if kind == "noise":
        return noise
    if kind == "ties":
        return (rng.integers(0, 2, (n, px)) * 255).astype(np.uint8)
    if kind == "alternating":
        out = np.zeros((n, px), np.uint8)
        out[1::2] = 255
        return out
    if kind == "ascending":
        return ((np.arange(n)[:, None] * 3 + np.arange(px)[None, :]) * 255 // max(3 * n + px, 1)).astype(np.uint8)
    if kind == "descending":
        return (255 - (np.arange(n)[:, None] * 3 + np.arange(px)[None, :]) * 255 // max(3 * n + px, 1)).astype(np.uint8)
    if kind == "constant":
        out = np.full((n, px), 200, np.uint8)
        out[rng.random((n, px)) < 0.02] = 7
        out[:, 0] = 200
        return out
    ground = 80 + 40 * np.sin(np.arange(n)[:, None] / 37.0 + np.arange(px)[None, :] / 5.0)
    out = np.clip(ground + rng.integers(0, 4, (n, px)), 0, 255).astype(np.uint8)
    out[n // 4:n // 2, :max(px // 3, 1)] = 230
    return out


def restate_sorted(frames, window):
    """(lower, upper, diff) by sorting every window: sliding_window_view + np.sort for the full windows, plain slices
    while the window grows"""
    frames = np.asarray(frames, np.uint8)
    n, px = frames.shape
    lower, upper = np.zeros((n, px), np.uint8), np.zeros((n, px), np.uint8)
    for k in range(1, min(n, window)):
        ordered = np.sort(frames[:k], axis=0)
        lower[k], upper[k] = ordered[(k - 1) // 2], ordered[k // 2]
    if n > window:
        views = np.lib.stride_tricks.sliding_window_view(frames, window, axis=0)      # (n - W + 1, px, W)
        for k in range(window, n):
            ordered = np.sort(views[k - window], axis=-1)
            lower[k], upper[k] = ordered[:, (window - 1) // 2], ordered[:, window // 2]
    mid = lower.astype(np.int64) + upper
    diff = np.minimum(255, np.abs(2 * frames.astype(np.int64) - mid) >> 1).astype(np.uint8)
    return lower, upper, diff


def restate_histogram(frames, window, ret_current=False):
    """the same from a histogram per pixel that one frame enters and one leaves; the ranks are read off its cumulative
    sums (no tracker, no walk); the difference is restated as FilterBackground's rule on the float median"""
    frames = np.asarray(frames, np.uint8)
    n, px = frames.shape
    hist = np.zeros((px, 256), np.int64)
    cols = np.arange(px)
    lower, upper = np.zeros((n + 1, px), np.uint8), np.zeros((n + 1, px), np.uint8)
    for k in range(n + 1):
        cnt = min(k, window)
        if cnt:
            cum = np.cumsum(hist, axis=1)
            lower[k] = (cum > (cnt - 1) // 2).argmax(axis=1)
            upper[k] = (cum > cnt // 2).argmax(axis=1)
        if k < n:
            hist[cols, frames[k]] += 1
            if k >= window:
                hist[cols, frames[k - window]] -= 1
    median = (lower[:n].astype(np.float64) + upper[:n]) / 2
    diff = np.minimum(np.trunc(np.abs(frames - median)), 255).astype(np.uint8)
    if ret_current:
        return lower[:n], upper[:n], diff, lower[n], upper[n]
    return lower[:n], upper[:n], diff


def trailing_medians(frames, window):
    """np.median of the window that ends with frame k, frame k included (what ops.sliding_median returns)"""
    frames = np.asarray(frames)
    return np.stack([np.median(frames[max(0, k - window + 1):k + 1], axis=0) for k in range(len(frames))])


def fixture():
    """{name: (window, frames (n, px) uint8, lower, upper, diff (n, px) uint8)}"""
    data = np.load(FIXTURE)
    out = {}
    for key in data.files:
        if key.startswith("frames_"):
            name = key[len("frames_"):]
            out[name] = (int(name.split("_")[0][1:]), data[key], data["lower_" + name], data["upper_" + name],
                         data["diff_" + name])
    return out


def state_bytes(px, window):
    """the state-size formula restated: per tile of 128 pixels a histogram of 256 counters a pixel (one byte up to a
    window of 255, two above) and four bytes of tracker a pixel; then a ring of `window` padded planes"""
    tiles = (px + TILE - 1) // TILE
    return tiles * (256 * TILE * (1 if window <= 255 else 2) + 4 * TILE) + window * tiles * TILE


def compile_shim(directory):
    """tests/sliding_median_shim.cpp with -fsanitize=address,undefined: the path of the program"""
    cxx = host_compiler()
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(directory), "sliding_median_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "sliding_median_shim.cpp"), "-o", exe])
    return exe


def run_shim(exe, runs):
    """runs: [(frames (n, px) uint8, window, stride, [frames of each call])] -> per run (lower, upper, diff (n, px),
    current lower, current upper (px), state bytes), as the program computes them in one run from zero states"""
    blob = []
    for frames, window, stride, counts in runs:
        n, px = frames.shape
        assert sum(counts) == n
        flat = np.full((n - 1) * stride + px if n else 0, 0x5A, np.uint8)
        for i in range(n):
            flat[i * stride:i * stride + px] = frames[i]
        blob += [np.array([px, stride, window, len(counts)] + list(counts), np.int64).tobytes(), flat.tobytes()]
    done = subprocess.run([exe], input=b"".join(blob), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr.decode("utf-8", "replace")[-2000:]
    out, at = [], 0
    for frames, window, _, _ in runs:
        n, px = frames.shape
        parts = []
        for shape in ((n, px), (n, px), (n, px), (px,), (px,), (state_bytes(px, window),)):
            size = int(np.prod(shape))
            parts.append(np.frombuffer(done.stdout, np.uint8, size, at).reshape(shape))
            at += size
        out.append(tuple(parts))
    assert at == len(done.stdout)
    return out
