"""GPU: every stream-taking entry point in stream order on a busy va_stream_create stream ("Stream order").

Every case of tests/stream_order_cases.py runs plain, gated and gated under the lease's zero fill on one created
(non-blocking) stream; see that module for the method.  An entry point declared asynchronous must return while the
blocker provably still holds the stream; one declared `synchronises` says so in the header (test_stream_order_host.py).
The calls go through the C ABI.  No subprocess, no thread.
"""
import ctypes as C

import numpy as np
import pytest

import pointer_offset_cases as P
import stream_order_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return P.hip_backend()


@pytest.fixture(scope="module")
def blocker(hip):
    b = S.Blocker(hip)
    yield b
    b.free()


@pytest.fixture()
def stream(hip):
    """(stream, (event, event)); destroyed afterwards, whatever the test did"""
    L = hip.lib
    s, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.check(L.va_stream_create(C.byref(s)))
    try:
        hip.check(L.va_event_create(C.byref(e0)))
        hip.check(L.va_event_create(C.byref(e1)))
        yield s, (e0, e1)
    finally:
        L.va_stream_sync(s)
        for e in (e0, e1):
            if e.value:
                L.va_event_destroy(e)
        hip.check(L.va_stream_destroy(s))


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_case_in_stream_order(hip, oracle, blocker, stream, name):
    case = S.BY_NAME[name]
    s, events = stream
    other = S.BY_NAME[S.INTERLOPERS[0] if name != S.INTERLOPERS[0] else S.INTERLOPERS[1]]
    interloper = S.Run(hip, other, oracle)
    try:
        figures = S.run_case(hip, case, oracle, s, blocker, events, interloper)
    finally:
        hip.lib.va_stream_sync(s)
        interloper.free()
    assert [mode for mode, _, _ in figures] == ["gated", "gated+fill"]
    for mode, span, busy in figures:
        print("%s %s: span %.3f ms, blocker %.3f ms" % (name, mode, span * 1e3, busy * 1e3))


@pytest.mark.parametrize("name", S.SENSITIVITY)
def test_the_runner_catches_a_call_on_the_wrong_stream(hip, oracle, blocker, stream, name):
    """the caller's mistake, made on purpose: the entry point gets the null stream while its inputs arrive on the
    created one, behind the blocker.  The call computes on the decoy (valid data: nothing can fault) and the runner
    must report a mismatch, five times out of five.  A miss means that the blocker is too short."""
    case = S.BY_NAME[name]
    s, events = stream
    run = S.Run(hip, case, oracle)
    try:
        run.setup()
        S.run_plain(run, oracle, s)
        for attempt in range(5):
            bad, span, busy = S.run_gated(run, oracle, s, blocker, events, call_stream=None)
            assert span < busy, (name, attempt, "not covered", span, busy)
            assert bad, (name, attempt, "a call on the wrong stream went unnoticed")
    finally:
        hip.lib.va_stream_sync(s)
        run.free()


def _pageable_setup(hip, nbytes):
    rng = np.random.default_rng(nbytes)
    old, new = rng.integers(0, 256, nbytes, dtype=np.uint8), rng.integers(0, 256, nbytes, dtype=np.uint8)
    assert not np.array_equal(old, new)
    dev, staged = S.Device(hip, nbytes), S.Device(hip, nbytes)
    dev.upload(old)
    staged.upload(new)
    hip.check(hip.lib.va_stream_sync(None))
    return old, new, dev, staged


def test_pageable_d2h_delivers_the_stream_ordered_bytes(hip, blocker, stream):
    """va_memcpy_d2h into a NumPy array, enqueued behind a device copy that is itself behind the blocker: it must
    deliver what that copy wrote, not what the buffer held when the call was made"""
    L = hip.lib
    s, _ = stream
    old, new, dev, staged = _pageable_setup(hip, 100003)
    try:
        blocker.enqueue(s)
        hip.check(L.va_memcpy_d2d(dev.ptr, staged.ptr, new.nbytes, s))
        got = np.zeros_like(new)
        hip.check(L.va_memcpy_d2h(got.ctypes.data, dev.ptr, got.nbytes, s))
        assert got.tobytes() == new.tobytes(), int(np.count_nonzero(got != new))
    finally:
        L.va_stream_sync(s)
        dev.free()
        staged.free()


def test_stream_wait_event_orders_a_second_stream_behind_the_first(hip, blocker, stream):
    """va_event_record behind a device copy behind the blocker on one created stream, va_stream_wait_event on a
    second: a copy enqueued on the second stream at once must see what the first stream's copy wrote"""
    L = hip.lib
    s, (e0, _) = stream
    old, new, dev, staged = _pageable_setup(hip, 100003)
    keep, second = S.Device(hip, old.nbytes), C.c_void_p()
    hip.check(L.va_stream_create(C.byref(second)))
    try:
        keep.fill(S.SENTINEL)
        hip.check(L.va_stream_sync(None))
        blocker.enqueue(s)
        hip.check(L.va_memcpy_d2d(dev.ptr, staged.ptr, new.nbytes, s))
        hip.check(L.va_event_record(e0, s))
        hip.check(L.va_stream_wait_event(second, e0))
        hip.check(L.va_memcpy_d2d(keep.ptr, dev.ptr, new.nbytes, second))
        hip.check(L.va_stream_sync(second))
        assert keep.download().tobytes() == new.tobytes()
    finally:
        L.va_stream_sync(s)
        L.va_stream_sync(second)
        hip.check(L.va_stream_destroy(second))
        for d in (dev, staged, keep):
            d.free()


def test_pageable_h2d_lands_behind_the_stream_s_earlier_work(hip, blocker, stream):
    """va_memcpy_h2d from a NumPy array, enqueued behind a device copy into the same buffer that is itself behind the
    blocker: the buffer must end up holding the host's bytes, and a later copy on the stream must see them"""
    L = hip.lib
    s, _ = stream
    old, new, dev, staged = _pageable_setup(hip, 100003)
    keep = S.Device(hip, old.nbytes)
    try:
        keep.fill(S.SENTINEL)
        hip.check(L.va_stream_sync(None))
        blocker.enqueue(s)
        hip.check(L.va_memcpy_d2d(dev.ptr, staged.ptr, new.nbytes, s))          # (new over old, on the stream)
        hip.check(L.va_memcpy_h2d(dev.ptr, old.ctypes.data, old.nbytes, s))     # (old over new, from the host)
        hip.check(L.va_memcpy_d2d(keep.ptr, dev.ptr, old.nbytes, s))
        hip.check(L.va_stream_sync(s))
        assert keep.download().tobytes() == old.tobytes()
    finally:
        L.va_stream_sync(s)
        for d in (dev, staged, keep):
            d.free()
