"""Running mean of 8-bit frames: the frame counts at which the division-free kernel changes its path.

The kernel works the first group of eight frames off ahead of its first loop (batches of 24 frames and more), walks
two groups per round there with the frames and the reciprocals of a group asked for one group ahead, takes full
groups that have another one behind them through a second loop and ends with the last group, full or not.  Batches
shorter than 24 frames skip the first two parts.  Every case compares the difference images and the final state of
`va_bg_update` with `oracle.bg_mean_u8`, bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# around the group of 8, the round of 16, the first loop's threshold of 24, its rounds (8 + 16 k, then 24 + 16 k
# frames leave one or two groups to the second loop) and the 256-entry argument table (257: reciprocals in memory)
FRAME_COUNTS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 39, 40, 41, 48, 257)
MAX_N = max(FRAME_COUNTS)
# 2^40 - 8: the two-operation second quotient is on for batches up to 7 frames and off from 8 on
HISTORIES = (0, 1000, 2 ** 40 - 8, 2 ** 53 - 300)
# name -> (frame shape, bytes by which the frame and difference buffers are entered late)
FORMS = {"wide": ((16, 64), 0),        # 64 x 16, 16-byte aligned: 16 px per thread, four waves
         "narrow": ((8, 24), 8),       # 24 x 8, 8-byte aligned only: 8 px per thread
         "plain": ((5, 7), 0)}         # a pixel count that is no multiple of 8: plain division, one px per thread
SPECIALS = [0.0, 255.0, 1e-300, 254.99999999999997, 1.0 / 3.0, 5e-324]

_cache = {}


def _clip(shape):
    key = ("clip", shape)
    if key not in _cache:
        rng = np.random.default_rng(11 + sum(shape))
        _cache[key] = rng.integers(0, 256, (MAX_N,) + shape, dtype=np.uint8)
    return _cache[key]


def _state(shape, kind):
    """'u8': values in [0, 255] with the special ones among them; 'wild': values outside that range as well"""
    key = ("state", shape, kind)
    if key not in _cache:
        rng = np.random.default_rng(5 + sum(shape))
        st = rng.random(shape) * 255
        st.reshape(-1)[:len(SPECIALS)] = SPECIALS
        if kind == "wild":
            st.reshape(-1)[len(SPECIALS):len(SPECIALS) + 5] = [-3.5, 300.25, 1e6, -1e-9, 255.5]
            st.reshape(-1)[-3:] = [-200.0, 256.0, 511.75]
        _cache[key] = st
    return _cache[key]


def _reference(oracle, shape, kind, n_seen, first, n):
    key = ("ref", shape, kind, n_seen, first, n)
    if key not in _cache:
        _cache[key] = oracle.bg_mean_u8(_clip(shape)[first:first + n], mean=_state(shape, kind), n_seen=n_seen)
    return _cache[key]


def _update(frames, state, n_seen, want_diff, late, batches=None):
    """va_bg_update on device copies of `frames` and `state`, in one launch or in the given batches back to back
    on the same state; the frame and difference buffers start `late` bytes into their allocations.  Returns
    (difference images or None, new state)."""
    from video import _hip
    L = _hip.lib()
    px = int(np.prod(frames.shape[1:]))
    src, dst, st = (_hip.DeviceBuffer(frames.nbytes + late), _hip.DeviceBuffer(frames.nbytes + late),
                    _hip.DeviceBuffer.from_array(state))
    try:
        _hip.check(L.va_memcpy_h2d(src.ptr + late, frames.ctypes.data, frames.nbytes, None))
        _hip.check(L.va_stream_sync(None))
        first = 0
        for n in batches or (frames.shape[0],):
            _hip.check(L.va_bg_update(_hip.BG_MODES["mean"], 0, src.ptr + late + first * px,
                                      dst.ptr + late + first * px if want_diff else None,
                                      st.ptr, int(n_seen) + first, 0.0, n, px, None))
            first += n
        assert first == frames.shape[0]
        diff = None
        if want_diff:
            diff = np.empty_like(frames)
            _hip.check(L.va_memcpy_d2h(diff.ctypes.data, dst.ptr + late, diff.nbytes, None))
            _hip.check(L.va_stream_sync(None))
        return diff, st.download(state.shape, np.float64)
    finally:
        for b in (src, dst, st):
            b.free()


@pytest.mark.parametrize("n_seen", HISTORIES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_frame_counts(oracle, form, n_seen):
    """every frame count, a state inside [0, 255] and one outside it, with and without a difference output"""
    shape, late = FORMS[form]
    for n in FRAME_COUNTS:
        for kind in ("u8", "wild"):
            ref_diff, ref_state = _reference(oracle, shape, kind, n_seen, 0, n)
            for want_diff in (True, False):
                diff, state = _update(_clip(shape)[:n], _state(shape, kind), n_seen, want_diff, late)
                where = (form, kind, n_seen, n, want_diff)
                if want_diff:
                    assert np.array_equal(diff, ref_diff), where
                assert np.array_equal(state, ref_state), where


@pytest.mark.parametrize("form", sorted(FORMS))
def test_two_launches_on_one_state(oracle, form):
    """the second launch starts from whatever the first left: the group ahead of the first loop and the short
    batch's entry of the second loop both meet a state that is not the caller's"""
    shape, late = FORMS[form]
    for batches in ((40, 41), (41, 17), (9, 48)):
        n = sum(batches)
        for n_seen in (0, 1000):
            ref_diff, ref_state = _reference(oracle, shape, "wild", n_seen, 0, n)
            for want_diff in (True, False):
                diff, state = _update(_clip(shape)[:n], _state(shape, "wild"), n_seen, want_diff, late, batches)
                where = (form, batches, n_seen, want_diff)
                if want_diff:
                    assert np.array_equal(diff, ref_diff), where
                assert np.array_equal(state, ref_state), where


def test_pipeline_vouched_range(oracle):
    """a pipeline whose state was set inside [0, 255] runs the kernel without the saturation of the difference
    (the flagship's form), over the same frame counts and histories"""
    from video import _hip
    from video.engine import FrameEngine
    _hip.lib()
    shape = FORMS["wide"][0]
    eng = FrameEngine(size=(shape[1], shape[0]), max_batch=MAX_N, background="mean")
    try:
        for n in FRAME_COUNTS:
            for n_seen in HISTORIES:
                ref_diff, ref_state = _reference(oracle, shape, "u8", n_seen, 0, n)
                eng.set_background(_state(shape, "u8"), n_seen)
                diff = eng.run(_clip(shape)[:n], want=("filtered",))["filtered"]
                got, seen = eng.get_background()
                assert seen == n_seen + n
                assert np.array_equal(diff, ref_diff), (n_seen, n)
                assert np.array_equal(got, ref_state), (n_seen, n)
    finally:
        eng.close()
