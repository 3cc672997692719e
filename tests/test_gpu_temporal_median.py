"""GPU: va_temporal_ranks_u8, ops.temporal_ranks / temporal_median / temporal_percentiles, measure_median and
FilterMedianBackground ("Temporal median") against the fixture two restatements agreed on and against
NumPy.  Every comparison is of bytes.  The `hostile` fixture (the pattern of tests/test_gpu_hostile_memory.py, fill
bytes 0x00 and 0xFF) repeats the fixture on dirty pooled memory with guarded tails; the raw calls run on output buffers
that were filled with a pattern first, with a tail behind them."""
import numpy as np
import pytest

import temporal_median_checks as K

pytestmark = pytest.mark.gpu

TAIL = 256
FILLS = (0x00, 0xFF)
DEPTHS = (1, 2, 64, 65, 255)
# (case, step, the byte of the planes in between): both paths, dword and byte accesses, both K of the counting path
STEPPED = (("t64_px16_noise", 2, 255), ("t64_px17_noise", 3, 0), ("t65_px16_noise", 3, 255), ("t65_px17_noise", 2, 0),
           ("t5_px17_ties", 2, 255), ("t17_px4_noise", 3, 0), ("t33_px256_descending", 2, 0))


@pytest.fixture(scope="module")
def cases():
    return K.fixture()


@pytest.fixture(params=FILLS, ids=["fill_00", "fill_ff"])
def hostile(request):
    """the test fill mode, on around one test; no guarded buffer leaks into another module's tests and no unguarded
    one into these"""
    from video import _hip, ops
    _hip.lib()
    ops.pool_clear()
    _hip.set_fill_mode(request.param)
    try:
        yield request.param
        found = _hip.check_guards()
    finally:
        _hip.set_fill_mode(-1)
        ops.pool_clear()
        _hip.check_guards()             # (what pool_clear's free() may still have recorded is not a later test's)
    assert found == [], found


def check_fixture_through_ops(cases):
    from video import ops
    for name, (frames, sets) in cases.items():
        t, px = frames.shape
        for ranks, planes in sets:
            got = ops.temporal_ranks(frames.reshape(t, 1, px), ranks)
            assert got.dtype == np.uint8 and got.shape == (len(ranks), 1, px), name
            assert np.array_equal(got.reshape(len(ranks), px), planes), (name, ranks)
    for name, step, filler in STEPPED:
        frames, sets = cases[name]
        stack = K.stepped(frames, step, filler)
        for ranks, planes in sets:
            got = ops.temporal_ranks(stack.reshape(len(stack), 1, -1), ranks, step=step)
            assert np.array_equal(got.reshape(len(ranks), -1), planes), (name, step, ranks)


def test_fixture_cases(cases):
    check_fixture_through_ops(cases)


def test_fixture_cases_on_hostile_memory(cases, hostile):
    check_fixture_through_ops(cases)


def abi(frames, ranks, stride, pattern, **passed):
    """one va_temporal_ranks_u8 call on an output buffer filled with `pattern`, with a tail: (status, planes, clean).
    passed: t, frame_stride or nranks as the call gets them, where they differ from what the buffers were made for"""
    from video import _hip
    L = _hip.lib()
    t, px = frames.shape
    flat = np.full((t - 1) * stride + px, 0x5A, np.uint8)
    for i in range(t):
        flat[i * stride:i * stride + px] = frames[i]
    rk = np.array(ranks, np.int32)
    k = len(rk)
    src, out = _hip.DeviceBuffer.from_array(flat), _hip.DeviceBuffer(k * px + TAIL)
    try:
        _hip.check(L.va_memset(out.ptr, pattern, k * px + TAIL, None))
        rc = L.va_temporal_ranks_u8(src.ptr, passed.get("t", t), px, passed.get("frame_stride", stride), rk.ctypes.data,
                                    passed.get("nranks", k), out.ptr, None)
        _hip.check(L.va_stream_sync(None))
        raw = out.download((k * px + TAIL,), np.uint8)
    finally:
        src.free()
        out.free()
    return rc, raw[:k * px].reshape(k, px), bool((raw[k * px:] == pattern).all())


RAW_CASES = ("t1_px1_zeros", "t8_px17_ties", "t9_px64_middle", "t32_px1027_ascending", "t64_px16_noise",
             "t64_px1027_ties", "t65_px16_noise", "t65_px1027_noise", "t255_px17_noise", "t255_px16_outlier")


@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_call_writes_its_planes_and_nothing_else(cases, name):
    frames, sets = cases[name]
    px = frames.shape[1]
    for ranks, planes in sets:
        for stride in (px, px + 3, (px + 3) // 4 * 4 + 4):
            first = abi(frames, ranks, stride, 0x00)
            second = abi(frames, ranks, stride, 0xFF)
            for rc, got, clean in (first, second):
                assert rc == 0 and clean, (name, ranks, stride)
                assert np.array_equal(got, planes), (name, ranks, stride)
            assert first[1].tobytes() == second[1].tobytes()


def test_bad_arguments_leave_the_planes_untouched(cases):
    frames, _ = cases["t9_px64_middle"]
    px = frames.shape[1]
    rc, got, clean = abi(frames, [4, 0], px, 0xA5)
    assert rc == 0 and clean and np.array_equal(got, np.sort(frames, axis=0)[[4, 0]])
    for ranks, passed in (([4, 0], dict(t=0)), ([4, 0], dict(t=256)), ([9], {}), ([0, 1, 9, 3], {}), ([4, -1], {}),
                          ([0] * 9, {}), ([4, 0], dict(nranks=0)), ([4, 0], dict(frame_stride=px - 1))):
        rc, got, clean = abi(frames, ranks, px, 0xA5, **passed)
        assert rc == -22 and clean and (got == 0xA5).all(), (ranks, passed)          # VA_ERR_INVALID


def test_device_frames_input():
    from video import ops
    rng = np.random.default_rng(11)
    for shape in ((64, 9, 12), (65, 5, 7, 3)):
        stack = rng.integers(0, 256, shape, dtype=np.uint8)
        dev = ops.DeviceFrames.upload(stack)
        try:
            for step in (1, 3):
                t = len(range(0, shape[0], step))
                ranks = [t - 1, 0, t // 2]
                want = ops.temporal_ranks(stack, ranks, step=step)
                assert np.array_equal(want, np.sort(stack[::step], axis=0)[ranks])
                assert ops.temporal_ranks(dev, ranks, step=step).tobytes() == want.tobytes()
            assert ops.temporal_median(dev).tobytes() == np.median(stack, axis=0).tobytes()
            assert np.array_equal(dev.download(), stack) and dev.shape == shape
        finally:
            dev.release()


@pytest.fixture(scope="module")
def stacks():
    """{(t, colour): stack}: (t, 37, 53) -- an odd plane size, two workgroups -- and (t, 16, 64, 3)"""
    rng = np.random.default_rng(12)
    out = {}
    for t in DEPTHS:
        out[t, False] = rng.integers(0, 256, (t, 37, 53), dtype=np.uint8)
        quiet = (90 + rng.integers(0, 6, (t, 16, 64, 3))).astype(np.uint8)
        quiet[rng.random((t, 16, 64, 3)) < 0.2] = 250
        out[t, True] = quiet
    return out


@pytest.mark.parametrize("t", DEPTHS)
def test_median_and_percentiles_equal_numpy(stacks, t):
    from video import ops
    for colour in (False, True):
        stack = stacks[t, colour]
        got = ops.temporal_median(stack)
        assert got.dtype == np.float64 and got.tobytes() == np.median(stack, axis=0).tobytes()
        for method in K.METHODS:
            got = ops.temporal_percentiles(stack, K.PERCENTILES, method=method)
            want = np.percentile(stack, K.PERCENTILES, axis=0, method=method)
            assert got.dtype == np.uint8 and want.dtype == np.uint8 and got.tobytes() == want.tobytes(), (t, method)
        one = ops.temporal_percentiles(stack, 90, method="higher")
        assert one.shape == stack.shape[1:] and np.array_equal(one, np.percentile(stack, 90, axis=0, method="higher"))
        if t >= 3:
            half = ops.temporal_median(stack, step=2)
            assert half.tobytes() == np.median(stack[::2], axis=0).tobytes()
    many = list(range(0, 101, 4))                       # 26 percentiles: more than eight distinct ranks from t = 64 on
    got = ops.temporal_percentiles(stacks[t, False], many, method="nearest")
    assert np.array_equal(got, np.percentile(stacks[t, False], many, axis=0, method="nearest"))


def test_two_calls_write_identical_bytes(stacks, hostile):
    from video import ops
    for t in (64, 255):
        first = ops.temporal_ranks(stacks[t, False], [0, t // 2, t - 1])
        second = ops.temporal_ranks(stacks[t, False], [0, t // 2, t - 1])
        assert first.tobytes() == second.tobytes() == np.sort(stacks[t, False], axis=0)[[0, t // 2, t - 1]].tobytes()


@pytest.fixture(scope="module")
def clip():
    """300 frames of 24 x 40: a noisy ground and a bright block that crosses it, so that the mean keeps a ghost"""
    rng = np.random.default_rng(13)
    frames = (60 + rng.integers(0, 9, (300, 24, 40))).astype(np.uint8)
    for k in range(300):
        x = (k * 40) // 300
        frames[k, 8:16, max(x - 3, 0):x + 3] = 220
    return frames


def test_measure_median_and_percentiles(clip):
    from video.analysis.video import measure_median, measure_percentiles, sample_indices
    from video.io.memory import VideoMemory
    video = VideoMemory(clip)
    video.set_frame_pos(5)
    used = clip[sample_indices(300, 101)]
    got = measure_median(video, max_frames=101)
    assert got.dtype == np.float64 and got.tobytes() == np.median(used, axis=0).tobytes()
    assert video.get_frame_pos() == 5 and got.max() < 80                 # no ghost of the block
    assert measure_median(VideoMemory(clip[:40])).tobytes() == np.median(clip[:40], axis=0).tobytes()
    lo_hi = measure_percentiles(video, (0, 100), max_frames=255)
    used = clip[sample_indices(300, 255)]
    assert np.array_equal(lo_hi, np.stack([used.min(axis=0), used.max(axis=0)]))


def test_filter_median_background(clip):
    import video.filters as F
    from video.analysis.video import sample_indices
    from video.io.memory import VideoMemory
    frames = np.ascontiguousarray(clip[::6])                            # 50 frames: the block crosses the whole frame
    median = np.median(frames[sample_indices(50, 31)], axis=0)
    mine = F.FilterMedianBackground(VideoMemory(frames), frames=31)
    plain = F.FilterBackground(VideoMemory(frames), mode="static", background=median)
    assert isinstance(mine, F.FilterBackground) and mine.mode == "static"
    assert mine.background.dtype == np.float64 and mine.background.tobytes() == median.tobytes()
    for k in range(len(frames)):
        assert np.array_equal(mine.get_frame(k), plain.get_frame(k)), k
    was = F._GpuStage.contract
    try:
        for contract in (True, False):
            F._GpuStage.contract = contract
            a = F.FilterThreshold(F.FilterBlur(F.FilterMedianBackground(VideoMemory(frames), frames=31), 2), 20)
            b = F.FilterThreshold(F.FilterBlur(F.FilterBackground(VideoMemory(frames), mode="static",
                                                                  background=median), 2), 20)
            assert (a._runner() is not None) == contract and (b._runner() is not None) == contract
            seen = 0
            for fa, fb in zip(a, b):
                assert np.array_equal(fa, fb)
                seen += int(fa.any())
            assert seen >= 40                                           # the block shows in the masks
            a.close()
            b.close()
    finally:
        F._GpuStage.contract = was
