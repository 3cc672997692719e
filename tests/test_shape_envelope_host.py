"""video.ops, the host layer, at the edges of its shape envelope, on the oracle's twin library (no GPU).

The calls the twin exports -- blur u8 and f32, morph, label, threshold, resize, region stats -- at the degenerate frames
of tests/test_gpu_shape_envelope.py (group A), at n = 0, and at the shapes with more than 65535 frames, rows or columns
(group C), against the oracle itself.  What is pinned is the host layer's own part of such a call: the reshaping of
(h, w) / (n, h, w) / (n, h, w, c) arrays, buffer sizes for tiny and empty batches, and the shape and dtype of what
comes back.  Every comparison is on dtype, shape and bytes.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libvideoanalysis_cpu.so")

DEGENERATE = [(1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 2), (3, 3), (3, 4), (4, 3), (1, 33), (33, 1), (2, 64), (64, 2)]
# (n, h, w): more than 65535 frames, rows, columns
BEYOND = [(65537, 2, 4), (65537, 4, 8), (1, 65537, 4), (1, 65537, 1), (1, 2, 65540), (1, 1, 65537)]
SHAPES = [(3,) + hw for hw in DEGENERATE] + [(0, 4, 4)] + BEYOND


class _Twin(object):
    """the bound twin; va_trim is answered with 0 (as tests/test_ops_twin.py's proxy does)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == "va_trim":
            return lambda nbytes: 0
        return getattr(self._lib, name)


@pytest.fixture
def twin(monkeypatch, oracle):
    from video import _hip, ops
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libvideoanalysis_cpu.so"],
                          stdout=subprocess.DEVNULL)
    lib = C.CDLL(CPU_LIB)
    for name, (res, args) in _hip.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.va_init(0) == 0
    ops.pool_clear()                              # whatever an earlier test pooled belongs to the real library
    proxy = _Twin(lib)
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    monkeypatch.setattr(_hip, "load_library", lambda: proxy)
    yield proxy
    ops.pool_clear()                              # the twin's buffers go back through the twin


def _same(got, want, where):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (where, g.dtype, w.dtype, g.shape, w.shape)
    assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), where      # floats: the same bits


def _frames(shape, seed=0):
    """seeded random frames; where there are three or more, frame 1 is all zero and frame 2 all 255"""
    a = np.random.default_rng(seed + shape[-1] + 7 * shape[-2]).integers(0, 256, shape, dtype=np.uint8)
    if shape[0] >= 3:
        a[1] = 0
        a[2] = 255
    return a


def _masks(shape, seed=0):
    a = (np.random.default_rng(seed + shape[-1] + 7 * shape[-2]).random(shape) < 0.5).astype(np.uint8)
    if shape[0] >= 3:
        a[1] = 0
        a[2] = 1
    return a


def _ids(shape):
    return "x".join(str(v) for v in shape)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gaussian_u8_and_f32(twin, oracle, shape):
    from video import ops
    a = _frames(shape)
    f = (a.astype(np.float32) / 64 - 1).astype(np.float32)
    for sigma in ((1.0, 5.0, 8.0) if shape[0] <= 3 else (1.0,)):
        _same(ops.gaussian_blur(a, sigma), oracle.gaussian_u8(a, sigma), ("u8", sigma))
    for sigma in ((1.0, 2.0, 9.0) if shape[0] <= 3 else (1.0,)):
        _same(ops.gaussian_blur(f, sigma), oracle.gaussian_f32(f, sigma), ("f32", sigma))
    if shape[0] <= 3:                             # colour: the channel dimension must not be taken for the width
        col = np.stack([f, f[::-1], f * 0.5], axis=-1)
        _same(ops.gaussian_blur(col, 2.0, color=True), oracle.gaussian_f32(col, 2.0), "f32 x 3")
        if shape[0]:
            _same(ops.gaussian_blur(col[0], 2.0, color=True), oracle.gaussian_f32(col[0], 2.0, layout="hwc"), "one hwc")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_threshold_morph_and_resize(twin, oracle, shape):
    from video import ops
    a = _frames(shape)
    _same(ops.threshold(a, 100), oracle.threshold_u8(a, 100), "threshold")
    elements = (("rect", oracle.RECT, 3), ("rect", oracle.RECT, 31), ("ellipse", oracle.ELLIPSE, 9),
                ("cross", oracle.CROSS, 5))
    for op, o in (("dilate", oracle.DILATE), ("erode", oracle.ERODE)):
        for name, code, k in (elements if shape[0] <= 3 else elements[:1]):
            _same(ops.morph(a, op, name, k), oracle.morph_u8(a, o, code, k), (op, name, k))
    for mode in (("nearest", "linear", "cubic", "area", "lanczos") if shape[0] <= 3 else ("linear",)):
        for size in ((1, 1), (2, 3)):             # (width, height)
            _same(ops.resize(a, size, mode), oracle.resize_u8(a, size, mode), (mode, size))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_label_and_region_stats(twin, oracle, shape):
    from video import ops
    m = _masks(shape)
    for conn in (4, 8):
        want_labels, want_counts = oracle.label_batch(m, conn)
        labels, counts = ops.label(m, conn)
        _same(labels, want_labels, ("labels", conn))
        _same(counts, want_counts, ("counts", conn))
        ml = int(want_counts.max(initial=0))
        stats = ops.region_stats(want_labels, ml)
        assert stats.dtype == np.int64 and stats.shape == (shape[0], max(ml, 1), 16)
        for f in (range(shape[0]) if shape[0] <= 3 else (0, shape[0] // 2, shape[0] - 1)):
            k = int(want_counts[f])
            _same(stats[f, :k, :14], oracle.region_stats(want_labels[f], k)[:, :14], ("stats", conn, f))


def test_single_frames_come_back_as_single_frames(twin, oracle):
    """an (h, w) array is one frame, whatever its sides: (1, 3) is not three frames of one pixel"""
    from video import ops
    for hw in DEGENERATE:
        a = _frames((1,) + hw)[0]
        _same(ops.gaussian_blur(a, 1.0), oracle.gaussian_u8(a, 1.0), hw)
        _same(ops.resize(a, (2, 3)), oracle.resize_u8(a, (2, 3)), hw)
        _same(ops.morph(a, "dilate", "rect", 3), oracle.morph_u8(a, oracle.DILATE, oracle.RECT, 3), hw)
        labels, count = ops.label(a > 127)
        want, k = oracle.label(a > 127)
        _same(labels, want, hw)
        assert isinstance(count, int) and count == k
