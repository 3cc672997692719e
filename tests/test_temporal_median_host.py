"""CPU: the temporal rank planes of DESIGN.md §9, "Temporal median".  The entry point is declared, exported and bound with
the pinned argument list; va_median_math.h, compiled with the host compiler under sanitizers into a stand-alone program,
gives the fixture's planes for every case and rank set, from buffers of exactly the stacks' sizes; the q -> rank mapping
and the median from rank planes equal NumPy for every depth 1 .. 255; the index rule of measure_median; every argument
check raises before a device is touched.  Comparisons are exact."""
import os
import re

import numpy as np
import pytest

import temporal_median_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -22


@pytest.fixture(scope="module")
def cases():
    fix = K.fixture()
    assert len(fix) >= 100
    return fix


def test_fixture_covers_the_depths_sizes_and_contents(cases):
    depths = {len(frames) for frames, _ in cases.values()}
    assert depths >= {1, 2, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255} | {9, 16, 17}
    assert {frames.shape[1] for frames, _ in cases.values()} >= {1, 2, 3, 4, 5, 7, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1027}
    for t in depths:
        sizes = {frames.shape[1] for frames, _ in cases.values() if len(frames) == t}
        assert any(px % 4 == 0 for px in sizes) and any(px % 2 == 1 for px in sizes), t
    assert {name.split("_")[2] for name in cases} == {"noise", "zeros", "full", "ties", "middle", "ascending",
                                                      "descending", "outlier"}
    for name, (frames, sets) in cases.items():
        t = len(frames)
        listed = [ranks for ranks, _ in sets]
        assert sorted({(t - 1) // 2, t // 2}) in listed and [0] in listed and [t - 1] in listed and [0, t - 1] in listed
        assert any(len(r) == 8 and r == sorted(r, reverse=True) and len(set(r)) < 8 for r in listed), name
        assert t < 8 or any(len(set(r)) == 8 for r in listed), name
        for ranks, planes in sets:
            assert np.array_equal(planes, np.sort(frames, axis=0)[ranks]), name


def test_entry_point_is_declared_exported_and_bound():
    from video import _hip
    text = open(os.path.join(ROOT, "include", "videoanalysis_hip.h")).read()
    found = re.search(r"int\s+va_temporal_ranks_u8\s*\(([^)]*)\)\s*;", text)
    assert found, "va_temporal_ranks_u8 is not declared"
    types = [re.sub(r"\s*\w+$", "", " ".join(arg.split())) for arg in found.group(1).split(",")]
    assert types == ["const uint8_t *", "int", "size_t", "size_t", "const int32_t *", "int", "uint8_t *", "void *"]
    lib = _hip.load_library()
    assert hasattr(lib, "va_temporal_ranks_u8")
    import ctypes as C
    assert _hip.SIGNATURES["va_temporal_ranks_u8"] == (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p,
                                                                 C.c_int, C.c_void_p, C.c_void_p])


def test_entry_point_refuses_bad_arguments_before_a_device():
    from video import _hip
    lib = _hip.load_library()
    P, Q = 4096, 8192                 # made-up addresses; never dereferenced
    ranks = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int32)
    R = ranks.ctypes.data

    def refused(*args):
        rc = lib.va_temporal_ranks_u8(*args)
        return rc == INVALID and lib.va_last_error().decode().startswith("va_temporal_ranks_u8: ")

    assert refused(None, 9, 16, 16, R, 1, Q, None) and refused(P, 9, 16, 16, None, 1, Q, None)
    assert refused(P, 9, 16, 16, R, 1, None, None)
    assert refused(P, 0, 16, 16, R, 1, Q, None) and refused(P, 256, 16, 16, R, 1, Q, None)
    assert refused(P, 9, 0, 16, R, 1, Q, None) and refused(P, 9, 16, 15, R, 1, Q, None)
    assert refused(P, 9, 16, 16, R, 0, Q, None) and refused(P, 9, 16, 16, R, 9, Q, None)
    assert refused(P, 7, 16, 16, R, 8, Q, None)                     # a rank = t
    ranks[3] = -1
    assert refused(P, 9, 16, 16, R, 8, Q, None)


def test_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    exe = K.compile_shim(tmp_path)
    calls, want, names = [], [], []
    for name, (frames, sets) in cases.items():
        for ranks, planes in sets:
            calls.append((frames, ranks, frames.shape[1]))
            want.append(planes)
            names.append((name, ranks))
    # strides beyond px: an aligned plane size on an odd stride (byte path), an odd one on a stride of four (byte path
    # again: px decides), and an aligned one on an aligned stride with a gap (dword path)
    for name, stride in (("t64_px16_noise", 19), ("t65_px17_noise", 20), ("t17_px4_noise", 8), ("t255_px16_ties", 32)):
        frames, sets = cases[name]
        for ranks, planes in sets:
            calls.append((frames, ranks, stride))
            want.append(planes)
            names.append((name, ranks, stride))
    got = K.run_shim(exe, calls)
    for planes, expected, what in zip(got, want, names):
        assert np.array_equal(planes, expected), what


def test_percentile_ranks_equal_numpy_for_every_depth():
    from video import ops
    rng = np.random.default_rng(7)
    for t in range(1, 256):
        stack = rng.integers(0, 256, (t, 6), dtype=np.uint8)
        ordered = np.sort(stack, axis=0)
        for method in K.METHODS:
            for q in K.PERCENTILES:
                r = ops.percentile_rank(t, q, method)
                assert isinstance(r, int) and 0 <= r < t
                assert np.array_equal(ordered[r], np.percentile(stack, q, axis=0, method=method)), (t, q, method)
    for method in K.METHODS:                                            # and as the kernel would be asked
        ranks = [ops.percentile_rank(26, q, method) for q in (28, 56, 12.5)]
        stack = rng.integers(0, 256, (26, 6), dtype=np.uint8)
        assert np.array_equal(np.sort(stack, axis=0)[ranks], np.percentile(stack, (28, 56, 12.5), axis=0, method=method))
    for bad in (-1, 100.5, float("nan")):
        with pytest.raises(ValueError):
            ops.percentile_rank(9, bad)
    with pytest.raises(ValueError):
        ops.percentile_rank(9, 50, "linear")


def test_median_from_rank_planes_equals_numpy_for_every_depth():
    from video import ops
    rng = np.random.default_rng(8)
    for t in range(1, 256):
        stack = rng.integers(0, 256, (t, 9), dtype=np.uint8)
        stack[:, 0], stack[: (t + 1) // 2, 1], stack[(t + 1) // 2:, 1] = 255, 254, 255
        ordered = np.sort(stack, axis=0)
        lo, hi = ops.median_ranks(t)
        assert (lo, hi) == ((t - 1) // 2, t // 2)
        got, want = ops.median_of_ranks(ordered[lo], ordered[hi]), np.median(stack, axis=0)
        assert got.dtype == np.float64 and want.dtype == np.float64 and got.tobytes() == want.tobytes(), t


def test_index_rule():
    from video.analysis.video import sample_indices
    for count, most in ((1, 1), (5, 101), (101, 101), (102, 101), (1000, 255), (256, 255)):
        idx = sample_indices(count, most)
        assert len(idx) == min(count, most) and idx[0] == 0 and idx[-1] < count
        assert all(b > a for a, b in zip(idx, idx[1:])), (count, most)
        if count <= most:
            assert idx == list(range(count))
        else:
            assert idx == [(j * count) // most for j in range(most)]


def _forward_only(data):
    """a forward-only view of an array (what a pipe or a fork client is to measure_median) that counts its reads"""
    from video.io.base import VideoBase

    class Forward(VideoBase):
        seekable = False

        def __init__(self):
            VideoBase.__init__(self, size=(data.shape[2], data.shape[1]), frame_count=len(data), is_color=False)
            self.reads = 0

        def get_frame(self, index):
            if not 0 <= index < self.frame_count:
                raise IndexError(index)
            self.reads += 1
            return data[index]

    return Forward()


def test_sampled_frames_seekable_and_forward_only():
    from video.analysis import video as V
    from video.io.memory import VideoMemory
    data = np.arange(300, dtype=np.uint8).reshape(300, 1, 1) * np.ones((1, 2, 3), np.uint8)
    want = data[V.sample_indices(300, 101)]
    mem = VideoMemory(data)
    mem.set_frame_pos(17)
    assert np.array_equal(V._sampled_stack(mem, 101, "test"), want) and mem.get_frame_pos() == 17
    fwd = _forward_only(data)
    assert np.array_equal(V._sampled_stack(fwd, 101, "test"), want)
    assert fwd.reads == V.sample_indices(300, 101)[-1] + 1             # it stops at the last frame it needs
    assert np.array_equal(V._sampled_stack(VideoMemory(data[:7]), 101, "test"), data[:7])


def test_argument_checks_raise_before_a_device_is_touched(monkeypatch):
    from video import _hip, ops
    from video.analysis.video import measure_median, measure_percentiles
    from video.filters import FilterBackground, FilterMedianBackground
    from video.io.memory import VideoMemory

    def no_device(*a, **k):
        raise AssertionError("an argument check came after the device was asked for")
    monkeypatch.setattr(_hip, "lib", no_device)
    u8 = np.zeros((9, 4, 6), np.uint8)
    for bad in (u8.astype(np.int16), u8.astype(np.float32), u8.astype(np.float64), u8.astype(bool)):
        with pytest.raises(TypeError):
            ops.temporal_ranks(bad, [0])
    for bad_ranks in ([9], [-1], [0] * 9, [], [1.5], [0, 1, 2, 3, 4, 5, 6, 7, 8]):
        with pytest.raises(ValueError):
            ops.temporal_ranks(u8, bad_ranks)
    with pytest.raises(ValueError):
        ops.temporal_ranks(np.zeros((256, 2, 2), np.uint8), [0])
    with pytest.raises(ValueError):
        ops.temporal_ranks(np.zeros((511, 2, 2), np.uint8), [0], step=2)      # 256 planes in use
    with pytest.raises(ValueError):
        ops.temporal_ranks(u8, [5], step=2)                                   # 5 planes in use: ranks 0 .. 4
    for bad_step in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ops.temporal_ranks(u8, [0], step=bad_step)
    for bad_shape in (np.zeros((4, 6), np.uint8), np.zeros((9, 4, 6, 2), np.uint8), np.zeros((0, 4, 6), np.uint8),
                      np.zeros((9, 0, 6), np.uint8)):
        with pytest.raises(ValueError):
            ops.temporal_ranks(bad_shape, [0])
    with pytest.raises(TypeError):
        ops.temporal_median(u8.astype(np.float32))
    with pytest.raises(ValueError):
        ops.temporal_median(np.zeros((256, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        ops.temporal_percentiles(u8, 50, method="linear")
    with pytest.raises(ValueError):
        ops.temporal_percentiles(u8, 101)
    video = VideoMemory(u8)
    for bad in (0, 256, -3, 2.5):
        with pytest.raises(ValueError):
            measure_median(video, max_frames=bad)
        with pytest.raises(ValueError):
            measure_percentiles(video, 50, max_frames=bad)
        with pytest.raises(ValueError):
            FilterMedianBackground(video, frames=bad)
    with pytest.raises(ValueError):
        measure_percentiles(video, 50, method="midpoint")
    empty = VideoMemory(np.zeros((0, 4, 6), np.uint8))
    with pytest.raises(ValueError):
        measure_median(empty)
    with pytest.raises(ValueError):
        FilterMedianBackground(empty)
    for dtype in (np.int16, np.float32):
        with pytest.raises(TypeError):
            measure_median(VideoMemory(u8.astype(dtype)))
        with pytest.raises(TypeError):
            FilterMedianBackground(VideoMemory(u8.astype(dtype)))
    with pytest.raises(ValueError):
        FilterBackground(video, mode="median")


def test_good_arguments_fail_loudly_without_a_gpu():
    from video import _hip, ops
    from video.filters import FilterMedianBackground
    from video.io.memory import VideoMemory
    u8 = np.zeros((9, 4, 6), np.uint8)
    if not _hip.gpu_available():
        with pytest.raises(_hip.HipUnavailableError):
            ops.temporal_ranks(u8, [0, 8])
        with pytest.raises(_hip.HipUnavailableError):
            ops.temporal_median(u8)
        with pytest.raises(_hip.HipUnavailableError):
            FilterMedianBackground(VideoMemory(u8))
