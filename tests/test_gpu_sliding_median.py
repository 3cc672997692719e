"""GPU: va_sliding_median_u8 / va_sliding_median_current, ops.SlidingMedian, ops.sliding_median and
FilterSlidingMedianBackground ("Sliding median") against the fixture two restatements agreed on, against
the restatements themselves and against np.median over explicit windows.  Every comparison is of bytes.  The raw calls
run on pattern-filled output buffers with a tail behind them and on a state with a tail behind it; the `hostile`
fixture (the pattern of tests/test_gpu_temporal_median.py, fill bytes 0x00 and 0xFF) repeats the fixture on dirty
pooled memory with guarded tails."""
import numpy as np
import pytest

import sliding_median_checks as K

pytestmark = pytest.mark.gpu

TAIL = 256
FILLS = (0x00, 0xFF)
PLANES = ("lower", "upper", "diff")


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
    for name, (window, frames, lower, upper, diff) in cases.items():
        n, px = frames.shape
        model = ops.SlidingMedian((1, px), window)
        try:
            assert model.state_bytes == K.state_bytes(px, window)
            assert not model.lower.any() and not model.median.any()
            cut = min(n, window + 2)
            got = model.process(frames[:cut].reshape(cut, 1, px), want=PLANES)
            rest = model.process(frames[cut:].reshape(n - cut, 1, px), want=PLANES + ("median",))
            assert model.n_seen == n
            for plane, want in zip(PLANES, (lower, upper, diff)):
                both = np.concatenate([got[plane], rest[plane]]).reshape(n, px)
                assert both.dtype == np.uint8 and np.array_equal(both, want), (name, plane)
            assert rest["median"].dtype == np.float64
            assert np.array_equal(rest["median"].reshape(-1, px), (lower[cut:].astype(np.float64) + upper[cut:]) / 2)
            tail = np.sort(frames[-window:], axis=0)
            assert np.array_equal(model.lower[0], tail[(window - 1) // 2]), name
            assert np.array_equal(model.upper[0], tail[window // 2]), name
            assert model.median.tobytes() == np.median(frames[-window:], axis=0)[None].tobytes(), name
        finally:
            model.close()


def test_fixture_cases(cases):
    check_fixture_through_ops(cases)


def test_fixture_cases_on_hostile_memory(cases, hostile):
    check_fixture_through_ops(cases)


def abi(frames, window, counts, stride=None, late=0, outs=PLANES, pattern=0xA5, passed=None):
    """the calls `counts` of va_sliding_median_u8 from a zero state, frames and outputs entered `late` bytes into
    their buffers, the outputs and the state's tail filled with `pattern` first.  Returns (statuses, {plane: (n, px)},
    (current lower, current upper), state bytes, clean): clean says that the tails behind the outputs and the state
    still hold the pattern.  passed: window, px, frame_stride or n_seen as the calls get them where they differ from
    what the buffers were made for"""
    from video import _hip
    L = _hip.lib()
    passed = passed or {}
    n, px = frames.shape
    stride = px if stride is None else stride
    flat = np.full(late + ((n - 1) * stride + px if n else 0) + 1, 0x5A, np.uint8)
    for i in range(n):
        flat[late + i * stride:late + i * stride + px] = frames[i]
    nstate = K.state_bytes(px, window)
    src, state = _hip.DeviceBuffer.from_array(flat), _hip.DeviceBuffer(nstate + TAIL)
    bufs = {plane: _hip.DeviceBuffer(late + n * px + TAIL) for plane in outs}
    now = _hip.DeviceBuffer(2 * px + TAIL)
    try:
        _hip.check(L.va_memset(state.ptr, 0, nstate, None))
        _hip.check(L.va_memset(state.ptr + nstate, pattern, TAIL, None))
        for buf in list(bufs.values()) + [now]:
            _hip.check(L.va_memset(buf.ptr, pattern, buf.nbytes, None))
        statuses, seen = [], 0
        for count in counts:
            ptrs = [bufs[plane].ptr + late + seen * px if plane in bufs else None for plane in PLANES]
            statuses.append(L.va_sliding_median_u8(src.ptr + late + seen * stride, count, passed.get("px", px),
                                                   passed.get("frame_stride", stride), passed.get("window", window),
                                                   passed.get("n_seen", seen), state.ptr, ptrs[0], ptrs[1], ptrs[2],
                                                   None))
            seen += count
        statuses.append(L.va_sliding_median_current(state.ptr, passed.get("px", px), passed.get("window", window),
                                                    passed.get("n_seen", seen), now.ptr, now.ptr + px, None))
        _hip.check(L.va_stream_sync(None))
        raw = {plane: buf.download((buf.nbytes,), np.uint8) for plane, buf in bufs.items()}
        raw_now, raw_state = now.download((now.nbytes,), np.uint8), state.download((state.nbytes,), np.uint8)
    finally:
        for buf in [src, state, now] + list(bufs.values()):
            buf.free()
    clean = bool((raw_state[nstate:] == pattern).all() and (raw_now[2 * px:] == pattern).all())
    planes = {}
    for plane, r in raw.items():
        clean = clean and bool((r[:late] == pattern).all() and (r[late + n * px:] == pattern).all())
        planes[plane] = r[late:late + n * px].reshape(n, px)
    return statuses, planes, (raw_now[:px], raw_now[px:2 * px]), raw_state[:nstate].tobytes(), clean


def splits_of(n, window):
    """one call; single frames; 7 + rest; calls of 0, 1, W - 1, W, W + 1 frames and the rest; 2 W + 3 (frames enter and
    leave in one call) and the rest"""
    out = [[n], [1] * n, [7, n - 7], [2 * window + 3, n - 2 * window - 3]]
    if window > 1:
        out.append([0, 1, window - 1, window, window + 1, n - 3 * window - 1])
    return out


RAW_CASES = ("w1_px1_noise", "w1_px129_ties", "w2_px17_noise", "w2_px128_alternating", "w3_px127_noise",
             "w3_px260_ascending", "w64_px17_noise", "w64_px128_ties", "w64_px129_alternating", "w64_px260_noise",
             "w64_px127_descending", "w255_px17_constant", "w255_px17_alternating", "w256_px20_constant",
             "w256_px16_alternating", "w300_px17_noise", "w300_px20_ties")


@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_calls_in_any_split_write_their_planes_and_the_same_state(cases, name):
    window, frames, lower, upper, diff = cases[name]
    n, px = frames.shape
    states = set()
    for i, counts in enumerate(splits_of(n, window)):
        # a stride of px (dwords where px allows), one with filler that is no multiple of four, one that is; every
        # other split enters its buffers one byte late
        stride, late = (px, px + 3, (px + 3) // 4 * 4 + 4)[i % 3], i % 2
        statuses, planes, now, state, clean = abi(frames, window, counts, stride, late, pattern=(0x00, 0xFF)[i % 2])
        assert statuses == [0] * (len(counts) + 1) and clean, (name, counts[:6])
        for plane, want in zip(PLANES, (lower, upper, diff)):
            assert np.array_equal(planes[plane], want), (name, plane, counts[:6])
        tail = np.sort(frames[-window:], axis=0)
        assert np.array_equal(now[0], tail[(window - 1) // 2]) and np.array_equal(now[1], tail[window // 2]), name
        states.add(state)
    assert len(states) == 1, name                           # chunk invariance, down to the state's bytes


@pytest.mark.parametrize("name", ("w3_px260_ascending", "w64_px260_noise", "w64_px128_ties", "w256_px17_noise"))
def test_each_output_alone_and_none(cases, name):
    window, frames, lower, upper, diff = cases[name]
    n = len(frames)
    whole = abi(frames, window, [n])
    for late in (0, 1):                                     # px = 260 one byte late: unaligned pointers
        for plane, want in zip(PLANES, (lower, upper, diff)):
            statuses, planes, _, state, clean = abi(frames, window, [5, n - 5], late=late, outs=(plane,))
            assert statuses == [0, 0, 0] and clean and list(planes) == [plane]
            assert np.array_equal(planes[plane], want), (name, plane)
            assert state == whole[3]
    statuses, planes, now, state, clean = abi(frames, window, [n], outs=())
    assert statuses == [0, 0] and clean and state == whole[3]
    assert np.array_equal(now[0], whole[2][0]) and np.array_equal(now[1], whole[2][1])


def test_bad_arguments_leave_everything_untouched(cases):
    window, frames = cases["w3_px16_scene"][:2]
    good = abi(frames, window, [len(frames)])
    assert good[0] == [0, 0] and good[4] and np.array_equal(good[1]["diff"], cases["w3_px16_scene"][4])
    empty = bytes(K.state_bytes(16, window))
    for passed in (dict(window=0), dict(window=65536), dict(px=0), dict(frame_stride=15), dict(n_seen=-1)):
        statuses, planes, now, state, clean = abi(frames, window, [4], passed=passed)
        expected = [-22, 0 if passed in (dict(frame_stride=15),) else -22]      # VA_ERR_INVALID; `current` takes no stride
        assert statuses == expected and clean and state == empty, passed
        assert all((plane == 0xA5).all() for plane in planes.values()), passed
        if statuses[1]:
            assert (now[0] == 0xA5).all() and (now[1] == 0xA5).all(), passed
    statuses, planes, _, state, clean = abi(frames, window, [-1])
    assert statuses[0] == -22 and clean and state == empty and all((p == 0xA5).all() for p in planes.values())
    statuses, planes, _, state, clean = abi(frames, window, [0, 0])
    assert statuses == [0, 0, 0] and clean and state == empty and all((p == 0xA5).all() for p in planes.values())


def test_window_of_65535_fills_a_uint16_counter():
    window, px, n = 65535, 8, 65540
    rng = np.random.default_rng(31)
    frames = np.full((n, px), 90, np.uint8)
    frames[rng.integers(0, n, 40), rng.integers(1, px, 40)] = 250       # a few outliers; column 0 stays constant
    frames[0, 1], frames[1, 1], frames[2, 2], frames[n - 3, 3] = 3, 200, 0, 255
    lower, upper, diff, now_lower, now_upper = K.restate_histogram(frames, window, ret_current=True)
    assert (lower[1:, 0] == 90).all() and lower[1, 1] == 3 and upper[2, 1] == 200
    statuses, planes, now, _, clean = abi(frames, window, [n])
    assert statuses == [0, 0] and clean
    for plane, want in zip(PLANES, (lower, upper, diff)):
        assert np.array_equal(planes[plane], want), plane
    assert np.array_equal(now[0], now_lower) and np.array_equal(now[1], now_upper)


@pytest.fixture(scope="module")
def clip():
    """150 frames of 12 x 20: a drifting noisy ground and a bright block that rests, then moves on"""
    rng = np.random.default_rng(13)
    frames = (60 + np.arange(150)[:, None, None] // 10 + rng.integers(0, 9, (150, 12, 20))).astype(np.uint8)
    frames[30:55, 4:8, 2:8] = 220
    frames[55:90, 4:8, 10:16] = 220
    return frames


def test_model_and_trailing_medians_equal_numpy(clip):
    from video import ops
    rng = np.random.default_rng(14)
    colour = rng.integers(0, 256, (40, 5, 7, 3), dtype=np.uint8)
    for stack, window in ((clip, 25), (clip[:30], 64), (colour, 6), (colour, 7), (clip[:9], 1)):
        got = ops.sliding_median(stack, window)
        want = K.trailing_medians(stack, window)
        assert got.dtype == np.float64 and got.shape == stack.shape and got.tobytes() == want.tobytes(), window
    model = ops.SlidingMedian(colour.shape[1:], 6)
    dev = ops.DeviceFrames.upload(colour)
    try:
        assert not model.process(colour[:0], want=("lower",))["lower"].size and model.n_seen == 0
        first = model.process(colour[:11], want="median")["median"]                # a host array ...
        rest = dev.gather(range(11, 40))
        kept = model.process(rest, want=("diff", "upper"), keep=True)              # ... then a kept stack
        rest.release()
        assert model.n_seen == 40 and isinstance(kept["diff"], ops.DeviceFrames) and kept["diff"].shape == (29, 5, 7, 3)
        for k in range(11):
            before = np.median(colour[max(0, k - 6):k], axis=0) if k else np.zeros(colour.shape[1:])
            assert np.array_equal(first[k], before), k
        diff, upper = kept["diff"].download(), kept["upper"].download()
        for k in range(11, 40):
            window = np.sort(colour[k - 6:k], axis=0)
            assert np.array_equal(upper[k - 11], window[3]), k
            assert np.array_equal(diff[k - 11], np.minimum(np.trunc(np.abs(colour[k] - np.median(window, axis=0))),
                                                           255).astype(np.uint8)), k
        assert model.median.tobytes() == np.median(colour[-6:], axis=0).tobytes()
        assert np.array_equal(dev.download(), colour)
        model.reset()
        assert model.n_seen == 0 and not model.upper.any()
        again = model.process(dev, want="median")["median"]
        assert np.array_equal(again[:11], first)
        with pytest.raises(ValueError):
            model.process(colour[:, :4], want="diff")
        with pytest.raises(ValueError):
            model.process(colour, want=("median",), keep=True)
        for stack in kept.values():
            stack.release()
    finally:
        dev.release()
        model.close()


def test_filter_sliding_median_background(clip):
    import video.filters as F
    from video.io.memory import VideoMemory
    window, count = 40, len(clip)
    lower, upper, diff = (a.reshape(clip.shape) for a in K.restate_histogram(clip.reshape(count, -1), window))
    median = (lower.astype(np.float64) + upper) / 2
    video = F.FilterSlidingMedianBackground(VideoMemory(clip), window=window)
    assert np.array_equal(video.background, np.zeros(clip.shape[1:]))
    for k, frame in enumerate(video):                                   # sequential iteration
        assert frame.dtype == np.uint8 and np.array_equal(frame, diff[k]), k
        if k + 1 < count:
            assert video.background.tobytes() == median[k + 1].tobytes(), k
    assert k == count - 1
    assert video.background.tobytes() == np.median(clip[-window:], axis=0).tobytes()
    assert diff[60:75, 4:8, 10:16].min() > 100              # a block that rests for under half the window stays out
    for k in np.random.default_rng(15).integers(0, count, 8).tolist() + [0, count - 1]:      # random positions
        assert np.array_equal(video.get_frame(k), diff[k]), k
    video.set_frame_pos(97)                                             # iteration after a seek
    assert video.background.tobytes() == median[97].tobytes()
    for k in range(97, 140):
        assert np.array_equal(video.get_next_frame(), diff[k]), k
        assert video.background.tobytes() == median[k + 1].tobytes(), k
    video.close()
    mean = F.FilterBackground(VideoMemory(clip), mode="mean")           # what the mean keeps of the block
    ghost = np.stack([np.array(f) for f in mean])[100:, 4:8, 10:16].mean()
    assert ghost > 3 * diff[140:, 4:8, 10:16].mean()
    mean.close()
