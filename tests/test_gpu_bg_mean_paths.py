"""Running mean of 8-bit frames: every kernel form, prefetch-group boundary and divisor range against the oracle.

The division-free kernel walks a batch in groups of eight frames held in two alternating register sets, counts its
divisor up in float64, packs and unpacks the byte lanes by hand and exists with and without a difference output,
with and without the saturation of the difference, at 16 and at 8 pixels per thread, with the reciprocals in its
arguments (up to 256 frames) or in memory.  Every case compares the difference images and the final state with
`oracle.bg_mean_u8`, bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (1, 7, 8, 9, 15, 16, 17, 255, 256, 257)     # around the group of 8, the round of 16, the 256-entry table
MAX_N = max(FRAME_COUNTS)
# (n_seen, n): the divisor crosses 2^32 inside the batch; the two-operation second quotient still on (n_seen + n <
# 2^40) and off for the batch; the last count the float64 increment reaches exactly, and beyond it (plain division)
LARGE_COUNTS = ((2 ** 32 - 130, 256), (2 ** 40 - 257, 256), (2 ** 40 - 257, 257), (2 ** 40 - 128, 256),
                (2 ** 53 - 256, 256), (2 ** 53 - 100, 256))
# name -> (frame shape, bytes by which the frame and difference buffers are entered late)
FORMS = {"wide": ((16, 24), 0),        # px % 16 == 0, 16-byte aligned: 16 px per thread
         "late8": ((16, 24), 8),       # the same, 8-byte aligned only: 8 px per thread
         "narrow": ((8, 9), 0),        # px % 8 == 0 only: 8 px per thread
         "scalar": ((5, 7), 0)}        # neither: the plain-division kernel, one px per thread (control)
SPECIALS = [0.0, 255.0, 1e-300, 254.99999999999997, 1.0 / 3.0, 5e-324]

_cache = {}


def _clip(shape):
    key = ("clip", shape)
    if key not in _cache:
        rng = np.random.default_rng(sum(shape))
        _cache[key] = rng.integers(0, 256, (MAX_N,) + shape, dtype=np.uint8)
    return _cache[key]


def _state(shape, kind):
    """'u8': random significands in [0, 255] and the special values; 'wild': values outside that range as well"""
    key = ("state", shape, kind)
    if key not in _cache:
        rng = np.random.default_rng(7 + sum(shape))
        st = rng.random(shape) * 255
        st.reshape(-1)[:len(SPECIALS)] = SPECIALS
        if kind == "wild":
            st.reshape(-1)[len(SPECIALS):len(SPECIALS) + 5] = [-3.5, 300.25, 1e6, -1e-9, 255.5]
            st.reshape(-1)[-3:] = [-200.0, 256.0, 511.75]
        _cache[key] = st
    return _cache[key]


def _reference(oracle, shape, kind, n_seen, n):
    key = ("ref", shape, kind, n_seen, n)
    if key not in _cache:
        _cache[key] = oracle.bg_mean_u8(_clip(shape)[:n], mean=_state(shape, kind), n_seen=n_seen)
    return _cache[key]


def _update(frames, state, n_seen, want_diff, late=0):
    """va_bg_update on device copies of `frames` and `state`; the frame and difference buffers start `late` bytes
    into their allocations.  Returns (difference images or None, new state)."""
    from video import _hip
    L = _hip.lib()
    src, dst, st = (_hip.DeviceBuffer(frames.nbytes + late), _hip.DeviceBuffer(frames.nbytes + late),
                    _hip.DeviceBuffer.from_array(state))
    try:
        _hip.check(L.va_memcpy_h2d(src.ptr + late, frames.ctypes.data, frames.nbytes, None))
        _hip.check(L.va_stream_sync(None))
        _hip.check(L.va_bg_update(_hip.BG_MODES["mean"], 0, src.ptr + late, dst.ptr + late if want_diff else None,
                                  st.ptr, int(n_seen), 0.0, frames.shape[0], int(np.prod(frames.shape[1:])), None))
        diff = None
        if want_diff:
            diff = np.empty_like(frames)
            _hip.check(L.va_memcpy_d2h(diff.ctypes.data, dst.ptr + late, diff.nbytes, None))
            _hip.check(L.va_stream_sync(None))
        return diff, st.download(state.shape, np.float64)
    finally:
        for b in (src, dst, st):
            b.free()


def _check_update(oracle, form, kind, n_seen, n):
    shape, late = FORMS[form]
    ref_diff, ref_state = _reference(oracle, shape, kind, n_seen, n)
    for want_diff in (True, False):
        diff, state = _update(_clip(shape)[:n], _state(shape, kind), n_seen, want_diff, late)
        where = (form, kind, n_seen, n, want_diff)
        if want_diff:
            assert np.array_equal(diff, ref_diff), where
        assert np.array_equal(state, ref_state), where


@pytest.mark.parametrize("form", sorted(FORMS))
def test_update_frame_counts(oracle, form):
    """any state (the saturating kernels), with and without a difference output, every frame count"""
    for n in FRAME_COUNTS:
        for n_seen in (0, 2 ** 24 - 3):
            for kind in ("u8", "wild"):
                _check_update(oracle, form, kind, n_seen, n)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_update_large_counts(oracle, form):
    for n_seen, n in LARGE_COUNTS:
        for kind in ("u8", "wild"):
            _check_update(oracle, form, kind, n_seen, n)


def _engine(shape):
    from video import _hip
    from video.engine import FrameEngine
    _hip.lib()
    return FrameEngine(size=(shape[1], shape[0]), max_batch=MAX_N, background="mean")


def _check_pipeline(eng, oracle, frames, state, n_seen, ref, where):
    eng.set_background(state, n_seen)
    diff = eng.run(frames, want=("filtered",))["filtered"]
    got, seen = eng.get_background()
    assert seen == n_seen + frames.shape[0], where
    assert np.array_equal(diff, ref[0]), where
    assert np.array_equal(got, ref[1]), where


@pytest.mark.parametrize("form", ["narrow", "scalar", "wide"])
def test_pipeline_vouched_range(oracle, form):
    """a pipeline whose state was set inside [0, 255] runs the kernels without the saturation; one set outside
    that range must not"""
    shape = FORMS[form][0]
    eng = _engine(shape)
    try:
        for n in FRAME_COUNTS:
            for n_seen in (0, 2 ** 24 - 3):
                _check_pipeline(eng, oracle, _clip(shape)[:n], _state(shape, "u8"), n_seen,
                                _reference(oracle, shape, "u8", n_seen, n), (form, n_seen, n))
        for n_seen, n in LARGE_COUNTS:
            for kind in ("u8", "wild"):
                _check_pipeline(eng, oracle, _clip(shape)[:n], _state(shape, kind), n_seen,
                                _reference(oracle, shape, kind, n_seen, n), (form, kind, n_seen, n))
    finally:
        eng.close()


def test_byte_lanes(oracle):
    """every packed byte at its maximum (frames of 255 against a zero state), and every byte lane of the
    extraction and of the pack with a value of its own (frames that count 0 .. 255 along x)"""
    shape = (4, 256)
    n = 17
    ramp = (np.arange(256)[None, None, :] + 3 * np.arange(shape[0])[None, :, None]
            + 5 * np.arange(n)[:, None, None]).astype(np.uint8)
    cases = (("full", np.full((n,) + shape, 255, np.uint8), np.zeros(shape)),
             ("ramp", ramp, np.zeros(shape)),
             ("ramp on a state", ramp, np.linspace(0.0, 255.0, shape[0] * shape[1]).reshape(shape)))
    eng = _engine(shape)
    try:
        for name, frames, state in cases:
            for n_seen in (0, 9):
                ref = oracle.bg_mean_u8(frames, mean=state, n_seen=n_seen)
                if name == "full" and n_seen == 0:
                    assert ref[0][0].min() == 255
                for late in (0, 8):
                    for want_diff in (True, False):
                        diff, got = _update(frames, state, n_seen, want_diff, late)
                        if want_diff:
                            assert np.array_equal(diff, ref[0]), (name, n_seen, late)
                        assert np.array_equal(got, ref[1]), (name, n_seen, late, want_diff)
                _check_pipeline(eng, oracle, frames, state, n_seen, ref, (name, n_seen))
    finally:
        eng.close()
