"""CPU: the sliding-window median of DESIGN.md §9, "Sliding median".  The two restatements agree with the fixture; the
entry points are declared, exported and bound with the pinned argument lists and refuse bad arguments before a device
is touched; the state-size formula; va_sliding_median_math.h, compiled with the host compiler under sanitizers into a
stand-alone program, gives the fixture's planes for every case, in one call and in chunks, from buffers of exactly the
sizes of what they hold, and leaves the same state bytes however the frames are split; the argument checks of
ops.SlidingMedian / ops.sliding_median; the plumbing of FilterSlidingMedianBackground on a NumPy stand-in of the model.
Comparisons are exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sliding_median_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -22


@pytest.fixture(scope="module")
def cases():
    return K.fixture()


def test_fixture_covers_the_windows_sizes_and_contents(cases):
    assert len(cases) == len(K.CASES)
    assert {w for w, _, _, _, _ in cases.values()} == set(K.WINDOWS)
    assert {f.shape[1] for _, f, _, _, _ in cases.values()} >= {1, 17, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 4}
    assert {name.split("_")[2] for name in cases} == set(K.CONTENTS)
    for name, (window, frames, lower, upper, diff) in cases.items():
        assert len(frames) == K.frames_of(window) and frames.dtype == np.uint8, name
        assert not lower[0].any() and not upper[0].any() and np.array_equal(diff[0], frames[0] >> 0), name
        assert (lower <= upper).all(), name
    w255 = cases["w255_px17_constant"]
    assert (w255[1][:, 0] == 200).all()                     # a uint8 counter reaches 255
    assert (cases["w256_px20_constant"][1][:, 0] == 200).all()


def test_restatements_agree_with_the_fixture(cases):
    for name, (window, frames, lower, upper, diff) in cases.items():
        first = K.restate_sorted(frames, window)
        second = K.restate_histogram(frames, window, ret_current=True)
        for got_a, got_b, want in zip(first, second, (lower, upper, diff)):
            assert got_a.dtype == np.uint8 and np.array_equal(got_a, want) and np.array_equal(got_b, want), name
        tail = np.sort(frames[-window:], axis=0)
        assert np.array_equal(second[3], tail[(window - 1) // 2]) and np.array_equal(second[4], tail[window // 2]), name
    window, frames, lower, upper, diff = cases["w64_px17_noise"]
    for k in (0, 1, 2, 63, 64, 65, 196):                    # and against np.median over explicit windows
        median = np.median(frames[max(0, k - window):k], axis=0) if k else np.zeros(17)
        assert np.array_equal((lower[k].astype(np.float64) + upper[k]) / 2, median), k
        assert np.array_equal(diff[k], np.minimum(np.trunc(np.abs(frames[k] - median)), 255).astype(np.uint8)), k


def test_entry_points_are_declared_exported_and_bound():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    pinned = {
        "va_sliding_median_state_bytes": ("size_t", ["size_t", "int"], (C.c_size_t, [C.c_size_t, C.c_int])),
        "va_sliding_median_u8": ("int", ["const uint8_t *", "int", "size_t", "size_t", "int", "int64_t", "void *",
                                         "uint8_t *", "uint8_t *", "uint8_t *", "void *"],
                                 (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int64] +
                                  [C.c_void_p] * 5)),
        "va_sliding_median_current": ("int", ["const void *", "size_t", "int", "int64_t", "uint8_t *", "uint8_t *",
                                              "void *"],
                                      (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int64] + [C.c_void_p] * 3)),
    }
    lib = _hip.load_library()
    for name, (result, args, bound) in pinned.items():
        found = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found and found.group(1) == result, name + " is not declared"
        types = [re.sub(r"\s*\w+$", "", " ".join(arg.split())) for arg in found.group(2).split(",")]
        assert types == args, name
        assert hasattr(lib, name) and _hip.SIGNATURES[name] == bound, name


def test_state_size_formula():
    from video import _hip
    lib = _hip.load_library()
    for px in (1, 17, 127, 128, 129, 260, 1920 * 1080, 3 * 3840 * 2160):
        for window in (1, 2, 64, 255, 256, 300, 65535):
            assert lib.va_sliding_median_state_bytes(px, window) == K.state_bytes(px, window), (px, window)
    assert K.state_bytes(128, 255) == 128 * (260 + 255) and K.state_bytes(128, 256) == 128 * (516 + 256)
    for px, window in ((0, 5), (5, 0), (5, -1), (5, 65536), (1 << 37, 5)):
        assert lib.va_sliding_median_state_bytes(px, window) == 0


def test_entry_points_refuse_bad_arguments_before_a_device():
    from video import _hip
    lib = _hip.load_library()
    P, S, Q = 4096, 8192, 16384               # made-up addresses; never dereferenced

    def refused(fn, *args):
        rc = getattr(lib, fn)(*args)
        return rc == INVALID and lib.va_last_error().decode().startswith(fn + ": ")

    run = "va_sliding_median_u8"
    assert refused(run, None, 4, 16, 16, 5, 0, S, Q, None, None, None)          # no frames
    assert refused(run, P, 4, 16, 16, 5, 0, None, Q, None, None, None)          # no state
    assert refused(run, P, 4, 16, 16, 5, 0, S + 4, Q, None, None, None)         # a state off its 16 bytes
    assert refused(run, P, 4, 16, 16, 0, 0, S, Q, None, None, None)
    assert refused(run, P, 4, 16, 16, 65536, 0, S, Q, None, None, None)
    assert refused(run, P, 4, 0, 16, 5, 0, S, Q, None, None, None)
    assert refused(run, P, -1, 16, 16, 5, 0, S, Q, None, None, None)
    assert refused(run, P, 4, 16, 15, 5, 0, S, Q, None, None, None)
    assert refused(run, P, 4, 16, 16, 5, -1, S, Q, None, None, None)
    assert lib.va_sliding_median_u8(P, 0, 16, 16, 5, 0, S, Q, Q, Q, None) == 0   # n = 0: nothing to do, no device
    assert lib.va_sliding_median_u8(None, 0, 16, 16, 5, 7, S, None, None, None, None) == 0
    now = "va_sliding_median_current"
    assert refused(now, None, 16, 5, 0, Q, Q, None) and refused(now, S, 0, 5, 0, Q, Q, None)
    assert refused(now, S, 16, 0, 0, Q, Q, None) and refused(now, S, 16, 65536, 0, Q, Q, None)
    assert refused(now, S, 16, 5, -1, Q, Q, None)


def test_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    exe = K.compile_shim(tmp_path)
    runs, names = [], []
    for name, (window, frames, _, _, _) in cases.items():
        n, px = frames.shape
        splits = [[n], [7, n - 7], [window - 1, 1, window + 1, n - 2 * window - 1] if window > 1 else [1] * n]
        if n <= 200 or px <= 2:
            splits.append([1] * n)
        splits.append([0, 2 * window + 3, 0, n - 2 * window - 3])       # frames enter and leave in one call
        for i, counts in enumerate(splits):
            runs.append((frames, window, px + (0, 3, 4, 0, 1)[i % 5], counts))
            names.append((name, counts if len(counts) < 6 else "singles"))
    got = K.run_shim(exe, runs)
    state_of = {}
    for (name, split), (lower, upper, diff, now_lower, now_upper, state) in zip(names, got):
        window, frames, want_lower, want_upper, want_diff = cases[name]
        assert np.array_equal(lower, want_lower) and np.array_equal(upper, want_upper), (name, split)
        assert np.array_equal(diff, want_diff), (name, split)
        tail = np.sort(frames[-window:], axis=0)
        assert np.array_equal(now_lower, tail[(window - 1) // 2]), (name, split)
        assert np.array_equal(now_upper, tail[window // 2]), (name, split)
        assert state_of.setdefault(name, state.tobytes()) == state.tobytes(), (name, split)
    # the state as documented: the ring holds the last `window` frames, frame k in slot k % window
    window, frames = cases["w64_px129_alternating"][:2]
    state = np.frombuffer(state_of["w64_px129_alternating"], np.uint8)
    ring = state[2 * (256 * K.TILE + 4 * K.TILE):].reshape(window, 2 * K.TILE)
    for k in range(len(frames) - window, len(frames)):
        assert np.array_equal(ring[k % window, :129], frames[k]) and not ring[k % window, 129:].any()


def test_argument_checks_raise_before_a_device_is_touched(monkeypatch):
    from video import _hip, ops
    from video.filters import FilterBackground, FilterSlidingMedianBackground
    from video.io.memory import VideoMemory

    def no_device(*a, **k):
        raise AssertionError("an argument check came after the device was asked for")
    monkeypatch.setattr(_hip, "lib", no_device)
    u8 = np.zeros((9, 4, 6), np.uint8)
    for bad in (u8.astype(np.int16), u8.astype(np.float32), u8.astype(np.float64), u8.astype(bool)):
        with pytest.raises(TypeError):
            ops.sliding_median(bad, 5)
    for bad_window in (0, -1, 65536, 2.5, True, None):
        with pytest.raises(ValueError):
            ops.sliding_median(u8, bad_window)
        with pytest.raises(ValueError):
            ops.SlidingMedian((4, 6), bad_window)
        with pytest.raises(ValueError):
            FilterSlidingMedianBackground(VideoMemory(u8), window=bad_window)
    for bad_shape in (np.zeros((4, 6), np.uint8), np.zeros((9, 4, 6, 2), np.uint8), np.zeros((9, 0, 6), np.uint8)):
        with pytest.raises(ValueError):
            ops.sliding_median(bad_shape, 5)
    for bad_frame_shape in ((4,), (4, 6, 2), (0, 6), (4, 6, 3, 1)):
        with pytest.raises(ValueError):
            ops.SlidingMedian(bad_frame_shape, 5)
    empty = ops.sliding_median(np.zeros((0, 4, 6), np.uint8), 5)
    assert empty.shape == (0, 4, 6) and empty.dtype == np.float64
    with pytest.raises(ValueError):
        FilterBackground(VideoMemory(u8), mode="median")
    FilterSlidingMedianBackground(VideoMemory(u8))            # construction alone needs no device


class NumpyModel(object):
    """ops.SlidingMedian's interface on the histogram restatement, for the plumbing test: it remembers the frames
    since its last reset, and counts the frames and calls it was given"""
    frames_in = calls = 0

    def __init__(self, frame_shape, window, stream=None):
        self.frame_shape, self.window = tuple(frame_shape), window
        self.reset()

    def reset(self):
        self.seen = np.zeros((0, int(np.prod(self.frame_shape))), np.uint8)

    def close(self):
        self.seen = None

    def process(self, frames, want=("diff",), keep=False):
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.shape[1:] == self.frame_shape and not keep
        NumpyModel.frames_in += len(frames)
        NumpyModel.calls += 1
        start = len(self.seen)
        self.seen = np.concatenate([self.seen, frames.reshape(len(frames), -1)])
        lower, upper, diff = K.restate_histogram(self.seen, self.window)
        planes = dict(lower=lower, upper=upper, diff=diff)
        return {name: planes[name][start:].reshape(frames.shape) for name in want}

    @property
    def median(self):
        if not len(self.seen):
            return np.zeros(self.frame_shape)
        return np.median(self.seen[-self.window:], axis=0).reshape(self.frame_shape)


def forward_only(data):
    from video.io.base import VideoBase

    class Forward(VideoBase):
        seekable = False

        def __init__(self):
            VideoBase.__init__(self, size=(data.shape[2], data.shape[1]), frame_count=len(data), is_color=False)
            self._at = 0

        def set_frame_pos(self, index):
            self._at = index

        def get_frame(self, index):
            return data[index]

        def get_next_frame(self):
            if self._at >= len(data):
                raise StopIteration
            self._at += 1
            return data[self._at - 1]

    return Forward()


def test_filter_plumbing_on_a_numpy_model(monkeypatch):
    from video import ops
    import video.filters as F
    from video.io.memory import VideoMemory
    monkeypatch.setattr(ops, "SlidingMedian", NumpyModel)
    rng = np.random.default_rng(5)
    window, count = 9, 100
    clip = rng.integers(0, 256, (count, 3, 5), dtype=np.uint8)
    lower, upper, diff = (a.reshape(clip.shape) for a in K.restate_histogram(clip.reshape(count, -1), window))
    median = (lower.astype(np.float64) + upper) / 2
    last = np.median(clip[-window:], axis=0)

    video = F.FilterSlidingMedianBackground(VideoMemory(clip), window=window)
    assert not isinstance(video, F._GpuStage) and video.frame_count == count
    assert np.array_equal(video.background, np.zeros((3, 5)))
    NumpyModel.frames_in = NumpyModel.calls = 0
    for k, frame in enumerate(video):                                   # sequential: batches of 32, no replay
        assert np.array_equal(frame, diff[k]), k
        want = median[k + 1] if k + 1 < count else last
        assert np.array_equal(video.background, want), k
    assert k == count - 1 and NumpyModel.frames_in == count and NumpyModel.calls == 4
    NumpyModel.frames_in = 0
    for k in (57, 58, 59, 3, 99, 0, 20):                                # random access
        assert np.array_equal(video.get_frame(k), diff[k]), k
        assert video.get_frame_pos() == k
        assert np.array_equal(video.background, median[k + 1] if k + 1 < count else last), k
    # a seek replays the `window` frames before its target (fewer near the start) and its batch reads up to 32:
    # 57: 9 + 32; 58, 59: from that batch; 3: 3 + 32; 99: 9 + 1; 0: 32; 20: from that batch
    assert NumpyModel.frames_in == 41 + 35 + 10 + 32
    NumpyModel.frames_in = 0
    video.set_frame_pos(40)                                             # iteration after a seek
    assert np.array_equal(video.background, median[40])
    for k in range(40, 50):
        assert np.array_equal(video.get_next_frame(), diff[k]), k
    assert NumpyModel.frames_in == window + 32
    video.close()

    plain = F.FilterSlidingMedianBackground(forward_only(clip), window=window)     # forward-only: frame by frame
    for k, frame in enumerate(plain):
        assert np.array_equal(frame, diff[k]), k
        if k in (0, 8, 9, 50):
            assert np.array_equal(plain.background, median[k + 1]), k
    assert k == count - 1
    with pytest.raises(TypeError):
        next(iter(F.FilterSlidingMedianBackground(VideoMemory(clip.astype(np.int16)), window=window)))


def test_good_arguments_fail_loudly_without_a_gpu():
    from video import _hip, ops
    from video.filters import FilterSlidingMedianBackground
    from video.io.memory import VideoMemory
    u8 = np.zeros((9, 4, 6), np.uint8)
    if not _hip.gpu_available():
        with pytest.raises(_hip.HipUnavailableError):
            ops.sliding_median(u8, 5)
        with pytest.raises(_hip.HipUnavailableError):
            ops.SlidingMedian((4, 6), 5)
        with pytest.raises(_hip.HipUnavailableError):
            next(iter(FilterSlidingMedianBackground(VideoMemory(u8), window=5)))
