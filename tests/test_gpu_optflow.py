"""GPU: Farneback optical flow (va_optflow.hip) and FilterOpticalFlow bit-exact against the NumPy restatement
of tests/golden/make_golden_optflow.py and its committed fixture."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_optflow", os.path.join(ROOT, "tests", "golden", "make_golden_optflow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def fx():
    from video import _hip
    _hip.lib()
    return np.load(os.path.join(ROOT, "tests", "golden", "optflow_v1.npz"), allow_pickle=False)


def _gpu(frames, **params):
    from video import ops
    return ops.optical_flow_farneback(frames, ret_flow=True, **params)


def _same(got, want):
    flow, mag = got
    assert flow.dtype == np.float32 and mag.dtype == np.float32
    assert np.array_equal(flow, want[0]), "flow differs at %d values" % np.count_nonzero(flow != want[0])
    assert np.array_equal(mag, want[1]), "magnitude differs at %d values" % np.count_nonzero(mag != want[1])


def test_fixture(fx):
    for name, n, h, w, seed, step, dtype, extra, full in G.CASES:
        params = G.params_of(extra)
        if full:
            frames = fx[name + "_frames"]
            _same(_gpu(frames, **params), (fx[name + "_flow"], fx[name + "_mag"]))
        else:
            frames = G.case_frames(n, h, w, seed, step, dtype)
            assert np.array_equal(G.sha(frames), fx[name + "_frames_sha"])
            flow, mag = _gpu(frames, **params)
            idx = G.sample_index(mag.size, seed)
            assert np.array_equal(mag.reshape(-1)[idx], fx[name + "_mag_sample"])
            assert np.array_equal(flow.reshape(-1, 2)[idx], fx[name + "_flow_sample"])
            assert np.array_equal(G.sha(mag), fx[name + "_mag_sha"])
            assert np.array_equal(G.sha(flow), fx[name + "_flow_sha"])


# (n, h, w, params): the 32-pixel rule at several sizes, odd and tiny frames, both poly_n, every winsize
# branch, 1 and 4 iterations, two pyramid scales
RANDOM_CASES = [
    (2, 40, 50, {}),
    (2, 63, 64, dict(levels=5)),
    (3, 135, 241, {}),
    (2, 5, 7, {}),
    (2, 9, 11, dict(winsize=5)),
    (2, 70, 90, dict(poly_n=7, poly_sigma=1.5)),
    (2, 80, 96, dict(winsize=1)),
    (2, 96, 80, dict(winsize=5, iterations=4)),
    (2, 100, 130, dict(iterations=1, pyr_scale=0.6, levels=4)),
    (3, 150, 200, dict(pyr_scale=0.6, poly_n=7, poly_sigma=1.1, winsize=3)),
]


@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_random_cases(fx, case):
    n, h, w, extra = RANDOM_CASES[case]
    params = G.params_of(extra)
    frames = G.texture_frames(n, h, w, 100 + case, step=((case % 3) - 1, 1 + case % 2))
    _same(_gpu(frames, **params), G.optical_flow(frames, **params))


def test_one_1080p_pair(fx):
    frames = G.texture_frames(2, 1080, 1920, 77, step=(2, -1), cell=16)
    _same(_gpu(frames, **G.REFERENCE_PARAMS), G.optical_flow(frames, **G.REFERENCE_PARAMS))


def test_uint8_and_float32_inputs_agree(fx):
    from video import ops
    frames = G.texture_frames(3, 64, 72, 5, step=(1, 1))
    a = _gpu(frames)
    for dt in (np.float32, np.float64, np.int16):
        b = _gpu(frames.astype(dt))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), dt
    assert np.array_equal(ops.optical_flow_farneback(frames), a[1])


def test_stack_equals_pairs_and_any_chunking(fx, monkeypatch):
    from video import _hip, ops
    frames = G.texture_frames(7, 48, 80, 11, step=(1, 0))
    flow, mag = _gpu(frames)
    for k in range(6):
        f1, m1 = _gpu(frames[k:k + 2])
        assert np.array_equal(f1[0], flow[k]) and np.array_equal(m1[0], mag[k])
    L = _hip.lib()
    ws = lambda k: L.va_farneback_workspace_bytes(k, 48, 80, 0.5, 3, 2, 3, 5)
    for pairs in (1, 2, 4):
        monkeypatch.setattr(ops, "OPTFLOW_WORKSPACE_BUDGET", ws(pairs + 1))
        f2, m2 = _gpu(frames)
        assert np.array_equal(f2, flow) and np.array_equal(m2, mag), pairs


class _ForwardOnly(object):
    """a non-seekable source over an array"""

    def __new__(cls, frames):
        from video.io.base import VideoBase

        class ForwardOnly(VideoBase):
            seekable = False

            def __init__(self, frames):
                super(ForwardOnly, self).__init__(size=(frames.shape[2], frames.shape[1]),
                                                  frame_count=len(frames), is_color=False)
                self._frames = frames

            def get_next_frame(self):
                if self._frame_pos >= self.frame_count:
                    raise StopIteration
                self._frame_pos += 1
                return self._process_frame(self._frames[self._frame_pos - 1])

            def get_frame(self, index):
                raise NotImplementedError("forward only")

        return ForwardOnly(frames)


def test_filter_iteration_get_frame_and_listeners(fx):
    from video import ops
    from video.filters import FilterOpticalFlow
    from video.io.memory import VideoMemory
    frames = G.texture_frames(12, 40, 64, 21, step=(0, 1))
    want = ops.optical_flow_farneback(frames)
    flt = FilterOpticalFlow(VideoMemory(frames))
    flt.batch = 5
    assert flt.frame_count == 11
    seen = []
    flt.register_listener(lambda f: seen.append(np.array(f)))
    got = [np.array(f) for f in flt]
    assert len(got) == 11 and len(seen) == 11
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(seen, want))
    for k in (7, 0, 10, -1, 3):
        assert np.array_equal(flt.get_frame(k), want[k])
    assert len(seen) == 16
    flt.set_frame_pos(9)
    assert np.array_equal(flt.get_next_frame(), want[9])
    plain = FilterOpticalFlow(VideoMemory(frames))
    assert all(np.array_equal(a, b) for a, b in zip(plain, want))
    fwd = FilterOpticalFlow(_ForwardOnly(frames))
    assert fwd.frame_count == 11
    fseen = []
    fwd.register_listener(lambda f: fseen.append(1))
    got = [np.array(f) for f in fwd]
    assert len(got) == 11 and len(fseen) == 11
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        next(iter(FilterOpticalFlow(VideoMemory(np.zeros((3, 40, 48, 3), np.uint8)))))


def _abi_call(L, src, dtype, n, h, w, flow, mag, ws, wsb, stream=None, **kw):
    p = G.params_of(kw)
    return L.va_optical_flow_farneback(src, dtype, n, h, w, p["pyr_scale"], p["levels"], p["winsize"],
                                       p["iterations"], p["poly_n"], p["poly_sigma"], kw.get("flags", 0), flow, mag,
                                       ws, wsb, stream)


def test_flow_only_and_magnitude_only(fx):
    from video import _hip
    from video._hip import DeviceBuffer, check
    L = _hip.lib()
    n, h, w = 3, 60, 70
    frames = G.texture_frames(n, h, w, 31, step=(1, -1))
    want_flow, want_mag = G.optical_flow(frames, **G.REFERENCE_PARAMS)
    wsb = L.va_farneback_workspace_bytes(n, h, w, 0.5, 3, 2, 3, 5)
    src, ws = DeviceBuffer.from_array(frames), DeviceBuffer(wsb)
    fb, mb = DeviceBuffer((n - 1) * h * w * 8), DeviceBuffer((n - 1) * h * w * 4)
    check(_abi_call(L, src.ptr, _hip.VA_U8, n, h, w, fb.ptr, None, ws.ptr, wsb))
    assert np.array_equal(fb.download((n - 1, h, w, 2), np.float32), want_flow)
    check(_abi_call(L, src.ptr, _hip.VA_U8, n, h, w, None, mb.ptr, ws.ptr, wsb))
    assert np.array_equal(mb.download((n - 1, h, w), np.float32), want_mag)


def test_two_geometries_back_to_back_on_a_created_stream(fx):
    """both calls share one workspace and are not synchronised in between: the second call's resize tables
    must not overwrite the first's while its kernels still run"""
    from video import _hip
    from video._hip import DeviceBuffer, check
    L = _hip.lib()
    shapes = [(4, 270, 480), (3, 200, 150), (4, 270, 480)]
    wsb = max(L.va_farneback_workspace_bytes(n, h, w, 0.5, 3, 2, 3, 5) for n, h, w in shapes)
    ws = DeviceBuffer(wsb)
    stream = C.c_void_p()
    check(L.va_stream_create(C.byref(stream)))
    try:
        runs = []
        for i, (n, h, w) in enumerate(shapes):
            frames = G.texture_frames(n, h, w, 40 + i, step=(i - 1, 1))
            src, mb = DeviceBuffer.from_array(frames), DeviceBuffer((n - 1) * h * w * 4)
            check(_abi_call(L, src.ptr, _hip.VA_U8, n, h, w, None, mb.ptr, ws.ptr, wsb, stream))
            runs.append((frames, src, mb))
        check(L.va_stream_sync(stream))
        for frames, src, mb in runs:
            n, h, w = frames.shape
            want = G.optical_flow(frames, **G.REFERENCE_PARAMS)[1]
            assert np.array_equal(mb.download((n - 1, h, w), np.float32), want)
    finally:
        check(L.va_stream_destroy(stream))


def test_error_codes_and_texts(fx):
    from video import _hip, ops
    from video._hip import DeviceBuffer
    L = _hip.lib()
    frames = G.texture_frames(2, 40, 48, 3)
    src, ws = DeviceBuffer.from_array(frames), DeviceBuffer(1 << 20)
    out = DeviceBuffer(40 * 48 * 4)
    bad = [(dict(), 1, "at least 2 frames"),
           (dict(pyr_scale=1.0), 2, "pyr_scale"), (dict(pyr_scale=0.0), 2, "pyr_scale"),
           (dict(levels=-1), 2, "levels"), (dict(winsize=0), 2, "winsize"), (dict(iterations=0), 2, "iterations"),
           (dict(poly_n=6), 2, "poly_n"), (dict(flags=256), 2, "flags")]
    for kw, n, text in bad:
        rc = _abi_call(L, src.ptr, _hip.VA_U8, n, 40, 48, None, out.ptr, ws.ptr, 1 << 20, **kw)
        assert rc == -22, (kw, rc)
        assert text in L.va_last_error().decode(), kw
        with pytest.raises(_hip.HipError, match=text):
            ops.optical_flow_farneback(np.zeros((n, 40, 48), np.uint8), **kw)
    assert _abi_call(L, src.ptr, _hip.VA_U8, 2, 40, 48, None, None, ws.ptr, 1 << 20) == -22
    assert "both NULL" in L.va_last_error().decode()
    assert _abi_call(L, src.ptr, 7, 2, 40, 48, None, out.ptr, ws.ptr, 1 << 20) == -22
    assert _abi_call(L, src.ptr, _hip.VA_U8, 2, 40, 48, None, out.ptr, ws.ptr, 1000) == -34
    assert "workspace" in L.va_last_error().decode()
    with pytest.raises(ValueError):
        ops.optical_flow_farneback(np.zeros((2, 40, 48, 3), np.uint8))
