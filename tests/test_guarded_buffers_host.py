"""The test fill mode of the host layer (video._hip / video.ops), on the oracle's twin: no GPU.

The mode fills every device buffer with one byte and puts a guarded tail of _hip.TAIL_BYTES behind it (DESIGN.md,
"Hostile memory").  Three things are pinned here:

  control  : with the mode on, the twin's ops give the oracle's results and no violation is reported
  detector : a byte written behind the size asked for is reported, by the op for a pooled buffer and at free() for a
             buffer created directly; the tests fail when the check in ops._give or in DeviceBuffer.free is removed
  mode off : a pooled buffer is allocated as its size class, without a tail, and never filled

The negative controls write one byte inside the allocation (the slack of the size class, or the tail): nothing is ever
written outside what va_malloc returned.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libvideoanalysis_cpu.so")
FILLS = (0xA5, 0xFF)


class RecordingLib(object):
    """a bound library that records (name, args) of the calls named in `watch`; va_trim is answered with 0; `after`
    maps an entry point to a function that runs after the real call, with the call's arguments"""

    def __init__(self, lib, watch=("va_malloc", "va_memset")):
        self._lib = lib
        self.watch = tuple(watch)
        self.seen = []
        self.after = {}

    def __getattr__(self, name):
        if name == "va_trim":
            return lambda nbytes: 0
        fn = getattr(self._lib, name)               # AttributeError for what the twin lacks, as a CDLL gives it
        if name not in self.watch and name not in self.after:
            return fn

        def wrapped(*args):
            if name in self.watch:
                self.seen.append((name, args))
            rc = fn(*args)
            if name in self.after:
                self.after[name](*args)
            return rc
        return wrapped


@pytest.fixture
def twin(monkeypatch, oracle):
    """video.ops on the oracle's twin until the test ends; the mode is off and the pool empty before and after"""
    from video import _hip, ops
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libvideoanalysis_cpu.so"],
                          stdout=subprocess.DEVNULL)
    lib = C.CDLL(CPU_LIB)
    for name, (res, args) in _hip.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.va_init(0) == 0
    ops.pool_clear()                                # whatever an earlier test pooled belongs to the real library
    proxy = RecordingLib(lib)
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    monkeypatch.setattr(_hip, "load_library", lambda: proxy)
    assert _hip.fill_mode() == -1
    yield proxy
    ops.pool_clear()                                # the twin's buffers go back through the twin
    _hip.set_fill_mode(-1)
    _hip.check_guards()                             # (drained: nothing of this test is left for a later one)


_RNG = np.random.default_rng(11)
A = _RNG.integers(0, 256, (3, 20, 30), dtype=np.uint8)
F = (_RNG.random((3, 20, 30)) * 255).astype(np.float32)
MASK = np.where(_RNG.random((3, 20, 30)) < 0.4, np.uint8(255), np.uint8(0))
SQUARE = np.array([[0, 0], [4, 0], [4, 4], [0, 4]], np.int32)


def _same(got, want):
    got, want = (x if isinstance(x, (tuple, list)) else (x,) for x in (got, want))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def _cases(ops, O):
    """name -> (the call, the oracle's answer)"""
    lab, cnt = O.label_batch(MASK)
    return {
        "gaussian_u8": (lambda: ops.gaussian_blur(A, 2.0), lambda: O.gaussian_u8(A, 2.0)),
        "gaussian_f32": (lambda: ops.gaussian_blur(F, 2.0), lambda: O.gaussian_f32(F, 2.0)),
        "threshold": (lambda: ops.threshold(A, 100), lambda: O.threshold_u8(A, 100)),
        "morph": (lambda: ops.morph(MASK, "dilate", "rect", 5), lambda: O.morph_u8(MASK, O.DILATE, O.RECT, 5)),
        "label": (lambda: ops.label(MASK), lambda: (lab, cnt)),
        "region_stats": (lambda: ops.region_stats(lab[0], int(cnt[0]))[:, :14],
                         lambda: O.region_stats(lab[0], int(cnt[0]))[:, :14]),
        "resize_u8": (lambda: ops.resize(A, (17, 13)), lambda: O.resize_u8(A, (17, 13))),
        "resize_f32": (lambda: ops.resize(F, (41, 9), "cubic"), lambda: O.resize_f32(F, (41, 9), "cubic")),
        "contour_moments": (lambda: ops.contour_moments(SQUARE),
                            lambda: np.array([O.contour_moments(SQUARE)[k] for k in O.MOMENT_KEYS[:10]])),
    }


# ---------------------------------------------------------------------------------------------------- control
@pytest.mark.parametrize("fill", FILLS)
def test_filled_guarded_buffers_change_no_result(twin, oracle, fill):
    """every op twice: the second call gets recycled buffers, filled again"""
    from video import _hip, ops
    _hip.set_fill_mode(fill)
    assert _hip.fill_mode() == fill
    for name, (call, want) in sorted(_cases(ops, oracle).items()):
        expect = want()
        _same(call(), expect)
        _same(call(), expect)
    assert _hip.check_guards() == []
    ops.pool_clear()                                # free() checks every buffer once more
    assert _hip.check_guards() == []


@pytest.mark.parametrize("fill", FILLS)
def test_a_taken_buffer_is_its_size_class_and_a_tail_of_the_fill(twin, fill):
    from video import _hip, ops
    _hip.set_fill_mode(fill)
    for recycled in (False, True):
        buf = ops._take(300)
        assert (buf.nbytes, buf._asked, buf._alloc) == (512, 300, 512 + _hip.TAIL_BYTES)
        whole = np.empty(buf._alloc, np.uint8)
        assert twin.va_memcpy_d2h(whole.ctypes.data, buf.ptr, whole.nbytes, None) == 0
        assert whole.size == 512 + 256 and np.all(whole == fill), recycled
        buf.upload(np.full(300, fill ^ 0xFF, np.uint8))     # what the next user must not see
        ops._give(buf)
    assert _hip.check_guards() == []


# ---------------------------------------------------------------------------------------------------- detector
def _poke(proxy, ptr, offset, value):
    """one byte into the twin's "device" memory (host memory), through the ABI"""
    byte = np.array([value], np.uint8)
    assert proxy._lib.va_memcpy_h2d(ptr + offset, byte.ctypes.data, 1, None) == 0


@pytest.mark.parametrize("fill", FILLS)
def test_a_write_behind_a_pooled_output_makes_the_op_raise(twin, fill):
    """va_threshold_u8 of 300 elements, wrapped: after the real call the byte just behind the 300 asked for is
    overwritten.  The buffer's size class is 512, so the write stays inside the allocation.

    A write of the fill byte itself is, by construction, not detected: the same op with the same stray write passes
    when the byte written equals the fill.  That is why every test of the mode runs under two patterns."""
    from video import _hip, ops
    _hip.set_fill_mode(fill)
    src = np.arange(300, dtype=np.uint8)
    stray = [fill ^ 0x5A]
    twin.after["va_threshold_u8"] = lambda s, d, n, t, m, st: _poke(twin, d, n, stray[0])
    with pytest.raises(_hip.GuardViolation) as err:
        ops.threshold(src, 100)
    text = str(err.value)
    assert "[300, 300]" in text and "first damaged offset 300, 1 byte(s) differ" in text, text
    assert _hip.check_guards() == []                # reported once: the op raised it
    stray[0] = fill                                 # the blind spot
    assert np.array_equal(ops.threshold(src, 100), np.where(src > 100, 255, 0).astype(np.uint8))
    del twin.after["va_threshold_u8"]
    assert np.array_equal(ops.threshold(src, 100), np.where(src > 100, 255, 0).astype(np.uint8))
    assert _hip.check_guards() == []


@pytest.mark.parametrize("fill", FILLS)
def test_a_write_into_the_tail_of_a_direct_buffer_is_recorded(twin, fill):
    """the last byte of the tail of a DeviceBuffer: check_guards() finds it on the live buffer; free() records it
    (it cannot raise: __del__ swallows exceptions) and check_guards() returns what free() recorded"""
    from video import _hip
    _hip.set_fill_mode(fill)
    last = 1000 + _hip.TAIL_BYTES - 1
    live = _hip.DeviceBuffer(1000)
    _poke(twin, live.ptr, last, fill ^ 0xFF)
    found = _hip.check_guards()
    assert len(found) == 1 and "first damaged offset %d, 1 byte(s) differ" % last in found[0], found
    assert _hip.check_guards() == []
    live.free()
    assert _hip.check_guards() == []

    freed = _hip.DeviceBuffer(1000)
    _poke(twin, freed.ptr, last, fill ^ 0xFF)
    _poke(twin, freed.ptr, 1000, fill ^ 0xFF)
    freed.free()
    found = _hip.check_guards()
    assert len(found) == 1 and found[0].startswith("at free()"), found
    assert "buffer of 1000 bytes" in found[0] and "first damaged offset 1000, 2 byte(s) differ" in found[0], found
    assert _hip.check_guards() == []


def test_the_fill_byte_is_checked(twin):
    from video import _hip
    for bad in (-2, 256):
        with pytest.raises(ValueError):
            _hip.set_fill_mode(bad)
    assert _hip.fill_mode() == -1


# ---------------------------------------------------------------------------------------------------- mode off
def test_mode_off_allocates_the_size_class_and_fills_nothing(twin):
    from video import _hip, ops
    assert _hip.fill_mode() == -1
    for _ in range(2):                              # fresh, then recycled
        buf = ops._take(300)
        assert buf.nbytes == 512 and buf._fill == -1
        ops._give(buf)
    assert np.array_equal(ops.threshold(A, 100), np.where(A > 100, 255, 0).astype(np.uint8))
    sizes = [args[1] for name, args in twin.seen if name == "va_malloc"]
    assert sizes and all(s == max(256, 1 << (s - 1).bit_length()) for s in sizes), sizes
    assert sizes[0] == 512
    assert not [name for name, _ in twin.seen if name == "va_memset"]
    assert _hip.check_guards() == []
