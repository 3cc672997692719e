"""video.ops, the per-call host layer, behind a counting proxy of the C ABI.

The proxy wraps a library bound with `video._hip.SIGNATURES` and counts va_malloc / va_free / va_memcpy_h2d /
va_memcpy_d2h / va_stream_sync (and whatever kernel entry points a test names).  On a box without a GPU the library
is the oracle's twin, oracle/libvideoanalysis_cpu.so (tests/test_abi_twin.py); the tests marked gpu put the product
behind the same proxy for the ops the twin lacks.  Three properties of the host path are pinned:

  conservation : a call the library refuses hands every pooled buffer back -- good, refused, good allocates what the
                 first good call allocated and frees nothing (a buffer left to the garbage collector is a hipFree,
                 which synchronises the device: what the pool exists to avoid)
  ABI calls    : a warm call makes exactly the ABI calls it made at commit 3b20f39, before the ops shared one
                 buffer lease, one ragged packer and one retry loop (and, for the ops whose results outlive the call,
                 at commit 6c0fbaa, before the lease owned those results); the host path's speed check, and an exact one
  retry        : the run-again step of the point-list ops, reached with DEFAULT_POINT_CAPACITY set to 4
  ownership    : who holds a DeviceFrames after each op, on success and after a refusal (the table in compose_layers',
                 draw's and jpeg_encode's docstrings), and that a refused upload hands its buffer back

The two pure helpers under the ops, the byte layout (_Layout) and the run-again step (_rerun), are tested at the end
of the twin's part.
"""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libvideoanalysis_cpu.so")
COUNTED = ("va_malloc", "va_free", "va_memcpy_h2d", "va_memcpy_d2h", "va_stream_sync")


class CountingLib(object):
    """a bound library with the calls of COUNTED (+ `extra`) counted; va_trim is answered with 0, and an entry point
    named in `refuse` with -22 by the proxy itself: the library is not called, nothing is launched"""

    def __init__(self, lib, extra=()):
        self._lib = lib
        self.calls = dict.fromkeys(COUNTED + tuple(extra), 0)
        self.refuse = set()

    def __getattr__(self, name):
        if name == "va_trim":
            return lambda nbytes: 0
        if name in self.refuse:
            return lambda *args: -22
        fn = getattr(self._lib, name)
        if name not in self.calls:
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted

    def reset(self):
        for k in self.calls:
            self.calls[k] = 0

    def counters(self):
        return tuple(self.calls[k] for k in COUNTED)


def _behind_proxy(monkeypatch, lib, extra=()):
    """video.ops runs on `lib` through a CountingLib until the test ends; the pool is empty before and after"""
    from video import _hip, ops
    ops.pool_clear()                              # whatever an earlier test pooled belongs to the real library
    proxy = CountingLib(lib, extra)
    monkeypatch.setattr(_hip, "lib", lambda device=None: proxy)
    monkeypatch.setattr(_hip, "load_library", lambda: proxy)
    return proxy, ops


@pytest.fixture
def twin(monkeypatch, oracle):
    from video import _hip
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libvideoanalysis_cpu.so"],
                          stdout=subprocess.DEVNULL)
    lib = C.CDLL(CPU_LIB)
    for name, (res, args) in _hip.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.va_init(0) == 0
    proxy, ops = _behind_proxy(monkeypatch, lib)
    yield proxy
    ops.pool_clear()                              # the twin's buffers go back through the twin


@pytest.fixture
def product(monkeypatch):
    from video import _hip
    proxy, ops = _behind_proxy(monkeypatch, _hip.lib(), ("va_largest_contour", "va_distance_map_path",
                                                         "va_farthest_points"))
    yield proxy
    ops.pool_clear()


def warm_counters(proxy, call):
    """COUNTED of the second of two identical calls on an empty pool"""
    from video import ops
    ops.pool_clear()
    call()
    proxy.reset()
    call()
    return proxy.counters()


def assert_conserved(proxy, good, refused, same_sizes=True):
    """good, refused, good on an empty pool: no va_free at all, and no va_malloc beyond the first good call's.
    Where the refused call needs other sizes than the good one (same_sizes=False) it allocates those once; refused a
    second time it must not allocate again, which is what shows that they went back to the pool."""
    from video import _hip, ops

    def refuse():
        with pytest.raises((RuntimeError, ValueError)) as err:           # (HipError is a RuntimeError)
            refused()
        assert getattr(err.value, "code", -22) == -22, err.value

    ops.pool_clear()
    proxy.reset()
    good()
    first = proxy.calls["va_malloc"]
    assert first > 0
    refuse()
    second = proxy.calls["va_malloc"]
    good()
    refuse()
    assert proxy.calls["va_free"] == 0 and proxy.calls["va_malloc"] == second
    if same_sizes:
        assert second == first


def _same(got, want):
    got, want = (x if isinstance(x, (tuple, list)) else (x,) for x in (got, want))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


# ------------------------------------------------------------------------------------- on the twin (no GPU)
_RNG = np.random.default_rng(7)
A = _RNG.integers(0, 256, (3, 20, 30), dtype=np.uint8)
B = _RNG.integers(0, 256, (3, 20, 30), dtype=np.uint8)
F = (_RNG.random((3, 20, 30)) * 255).astype(np.float32)
COL = _RNG.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
MASK = np.where(_RNG.random((3, 20, 30)) < 0.4, np.uint8(255), np.uint8(0))
SQUARE = np.array([[0, 0], [4, 0], [4, 4], [0, 4]], np.int32)


def _background(ops, want_diff=True):
    bg = ops.BackgroundModel((20, 30), "mean")
    try:
        return bg.process(A, want_diff), bg.state
    finally:
        bg._state.free()                          # the model owns its state: not pooled, not left to the collector


def _twin_cases(ops, O):
    """name -> (the call, the oracle's answer)"""
    lab, cnt = O.label_batch(MASK)
    norm = ((np.clip(A.astype(np.float64), 50, 200) - 50) * (255 / 150.0) + 0).astype(np.int64).astype(np.uint8)
    return {
        "label": (lambda: ops.label(MASK), lambda: (lab, cnt)),
        "region_stats": (lambda: ops.region_stats(lab[0], int(cnt[0]))[:, :14],
                         lambda: O.region_stats(lab[0], int(cnt[0]))[:, :14]),
        "threshold": (lambda: ops.threshold(A, 100), lambda: O.threshold_u8(A, 100)),
        "mono_mean": (lambda: ops.mono_mean(COL), lambda: O.mono_mean_u8(COL)),
        "normalize": (lambda: ops.normalize(A, 50, 200, 255 / 150.0, 0), lambda: norm),
        "time_difference": (lambda: ops.time_difference(A, B), lambda: O.time_difference_u8(A, B)),
        "welford": (lambda: ops.welford(A), lambda: O.welford_u8(A)),
        "morph": (lambda: ops.morph(MASK, "dilate", "rect", 5), lambda: O.morph_u8(MASK, O.DILATE, O.RECT, 5)),
        "resize": (lambda: ops.resize(A, (17, 13)), lambda: O.resize_u8(A, (17, 13))),
        "contour_moments": (lambda: ops.contour_moments(SQUARE),
                            lambda: np.array([O.contour_moments(SQUARE)[k] for k in O.MOMENT_KEYS[:10]])),
        "background": (lambda: _background(ops), lambda: O.bg_mean_u8(A)),
        "gaussian_f32": (lambda: ops.gaussian_blur(F, 2.0), lambda: O.gaussian_f32(F, 2.0)),
        "gaussian_cv3": (lambda: ops.gaussian_blur(A, 2.0, tap_rule="cv3"),
                         lambda: O.gaussian_u8(A, 2.0, tap_rule="cv3")),
        "gaussian_u8": (lambda: ops.gaussian_blur(A, 2.0), lambda: O.gaussian_u8(A, 2.0)),
    }


# (va_malloc, va_free, va_memcpy_h2d, va_memcpy_d2h, va_stream_sync) of one warm call at commit 3b20f39.  The model
# of "background" is built and dropped inside the call: its state is the one buffer allocated and freed.  Plain uint8
# gaussian_blur could not run on the twin at that commit (it looked up an entry point the twin lacks); its counters
# there were taken with the product behind the proxy, see WARM_AT_PARENT_GPU.
WARM_AT_PARENT = {
    "label": (0, 0, 1, 2, 3), "region_stats": (0, 0, 1, 1, 2), "threshold": (0, 0, 1, 1, 2),
    "mono_mean": (0, 0, 1, 1, 2), "normalize": (0, 0, 1, 1, 2), "time_difference": (0, 0, 2, 1, 3),
    "welford": (0, 0, 3, 2, 5), "morph": (0, 0, 1, 1, 2), "resize": (0, 0, 1, 1, 2),
    "contour_moments": (0, 0, 1, 1, 2), "background": (1, 1, 2, 2, 4), "gaussian_f32": (0, 0, 1, 1, 2),
    "gaussian_cv3": (0, 0, 1, 1, 2), "gaussian_u8": (0, 0, 1, 1, 2),
}


@pytest.mark.parametrize("name", sorted(WARM_AT_PARENT))
def test_result_and_abi_calls_of_a_warm_call(twin, oracle, name):
    from video import ops
    call, want = _twin_cases(ops, oracle)[name]
    _same(call(), want())
    counters = warm_counters(twin, call)
    print(name, dict(zip(COUNTED, counters)))
    assert counters == WARM_AT_PARENT[name]


def test_refused_calls_return_their_buffers(twin):
    from video import ops
    assert_conserved(twin, lambda: ops.label(MASK), lambda: ops.label(MASK, connectivity=5))
    assert_conserved(twin, lambda: ops.gaussian_blur(F, 2.0), lambda: ops.gaussian_blur(F, -1))
    assert_conserved(twin, lambda: ops.gaussian_blur(A, 2.0), lambda: ops.gaussian_blur(A, -1))
    assert_conserved(twin, lambda: ops.gaussian_blur(A, 2.0, tap_rule="cv3"),
                     lambda: ops.gaussian_blur(A, -1, tap_rule="cv3"))
    # _pointwise_u8, behind threshold / mono_mean / normalize / morph / detect_peaks: an operation code of no name
    assert_conserved(twin, lambda: ops.morph(MASK, "dilate"), lambda: ops.morph(MASK, 7))
    bg = ops.BackgroundModel((20, 30), "static", background=A[0])
    try:                                          # a static background has nothing to do without the difference
        assert_conserved(twin, lambda: bg.process(A), lambda: bg.process(A, want_diff=False))
    finally:
        bg._state.free()


def test_a_refused_upload_returns_its_buffer(twin):
    """DeviceFrames.upload behind a proxy whose va_memcpy_h2d answers -22: the buffer is back in the pool, so good,
    refused, good frees nothing and allocates nothing beyond the first upload"""
    from video import ops

    def good():
        stack = ops.DeviceFrames.upload(A)
        assert np.array_equal(stack.download(), A)
        stack.release()

    def refused():
        twin.refuse.add("va_memcpy_h2d")
        try:
            ops.DeviceFrames.upload(A)
        finally:
            twin.refuse.clear()
    assert_conserved(twin, good, refused)
    assert twin.calls["va_malloc"] == 1


def test_layout_names_the_fields_of_one_buffer():
    """int64, float64 and int32 fields, one of them empty: the offsets are the cumulative byte sizes, the packed bytes
    the fields' bytes in order, and the typed views of a download the fields"""
    from video import ops
    fields = {"off": np.arange(5, dtype=np.int64), "tol": np.zeros(0, np.float64),
              "pts": np.linspace(-1, 1, 6).reshape(3, 2), "cnt": np.array([7, -8, 9], np.int32)}
    lay = ops._Layout(**fields)
    sizes = [a.nbytes for a in fields.values()]
    assert sizes == [40, 0, 48, 12]
    assert [lay.at[name] for name in fields] == [0, 40, 40, 88] and lay.nbytes == 100
    packed = lay.packed()
    assert packed.dtype == np.uint8 and packed.shape == (100,)
    assert np.array_equal(packed, np.concatenate([a.reshape(-1).view(np.uint8) for a in fields.values()]))
    for name, a in fields.items():
        got = lay.view(packed, name)
        assert got.dtype == a.dtype and np.array_equal(got, a.reshape(-1))

    class Buffer(object):
        ptr = 4096
    assert [lay.ptr(Buffer, name) for name in fields] == [4096, 4136, 4136, 4184]
    # an output layout is given as (count, dtype) and lies the same way
    outs = ops._Layout(off=(5, np.int64), tol=(0, np.float64), pts=(6, np.float64), cnt=(3, np.int32))
    assert outs.at == lay.at and outs.nbytes == lay.nbytes
    assert np.array_equal(outs.view(packed, "cnt"), fields["cnt"]) and outs.view(packed, "cnt").dtype == np.int32


def test_rerun_runs_once_more_with_the_needs_and_never_a_third_time():
    from video import ops
    calls = []

    def run(*caps):
        calls.append(caps)
        return "payload %d" % len(calls), (np.int64(10), np.int64(300))
    assert ops._rerun(run, 10, 300) == ("payload 1", (10, 300)) and calls == [(10, 300)]      # the needs fit
    for caps in ((9, 300), (10, 299), (0, 0)):
        del calls[:]
        payload, needs = ops._rerun(run, *caps)
        assert calls == [caps, (10, 300)] and all(type(c) is int for c in calls[1])
        assert payload == "payload 2" and tuple(needs) == (10, 300)
    del calls[:]

    def grows(*caps):                             # needs that exceed the second caps too: still no third call
        calls.append(caps)
        return None, tuple(c + 1 for c in caps)
    assert ops._rerun(grows, 4) == (None, (6,)) and calls == [(4,), (5,)]


# ------------------------------------------------------------------------------------- on the product (GPU)
BOXES = [(2, 3, 5, 7), (0, 0, 0, 4), (-1, 1, 9, 3)]                          # (x, y, w, h)
POLYS = [np.array([[2, 3], [6, 4], [4, 9]]), np.array([[0, 0], [0, 3]]), np.array([[-1, 1], [7, 1], [7, 3], [0, 3]])]
RAGGED = [np.ones((h, w), np.uint8) for _, _, w, h in BOXES]
NOTCHED = np.zeros((16, 16), np.uint8)
NOTCHED[3:13, 3:13] = 1
NOTCHED[3:7, 7:9] = 0


MASKS = np.stack([NOTCHED, NOTCHED[::-1]])                                   # the masks of find_contours
TILES = np.ascontiguousarray(A[:2, :16, :16])                                # frames of the masks' size
HIGHLIGHT = np.where(A[0] > 128, np.uint8(1), np.uint8(0))
LAYERS = [[("highlight", HIGHLIGHT, None, 100), ("add", B[f], None)] for f in range(3)]
COMMANDS = [[("polyline", [[2, 3], [25, 4], [12, 17]], True, 200), ("circle", (10 + f, 9), 5, False, 90)]
            for f in range(3)]
CURVES = [np.cumsum(_RNG.random((k, 2)) + 0.25, axis=0) for k in (5, 12, 23, 40)]      # four open curves
SKELETON = np.zeros((16, 16), np.uint8)
SKELETON[8, 2:14] = SKELETON[3:13, 7] = 1
JPEG_FRAMES = _RNG.integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)
_JPEG_FILES = {}


def _jpeg_files(ops, sampling):
    """the files of JPEG_FRAMES, encoded once a test"""
    if sampling not in _JPEG_FILES:
        _JPEG_FILES[sampling] = ops.jpeg_encode(JPEG_FRAMES, sampling=sampling)
    return _JPEG_FILES[sampling]


def _released(stack):
    """the array of a DeviceFrames, which goes back to the pool"""
    out = stack.download()
    stack.release()
    return out


def _drawn_contours(ops, frames, **kw):
    found = ops.find_contours(MASKS, keep=True)
    try:
        return ops.draw_contours(frames, found, 255, **kw)
    finally:
        found.release()


def _gradients(ops):
    fx, fy, shape = ops.potential_gradients(A, 1.5)
    fx.free()
    fy.free()
    return shape


def _gpu_cases(ops):
    on_device = ops.DeviceFrames.upload
    return {
        "fill_polys": lambda: ops.fill_polys(POLYS, BOXES),
        "distance_transform": lambda: ops.distance_transform(RAGGED),
        "guo_hall_thinning": lambda: ops.guo_hall_thinning(RAGGED + [np.zeros((0, 0), np.uint8)]),
        "gaussian_u8": lambda: ops.gaussian_blur(A, 2.0),
        "find_contours": lambda: ops.find_contours(MASKS, ret_info=True, moments=True),
        "find_contours_keep": lambda: ops.find_contours(MASKS, keep=True).release(),
        "compose_array": lambda: ops.compose_layers(A, LAYERS),
        "compose_array_keep": lambda: _released(ops.compose_layers(A, LAYERS, keep=True)),
        "compose_array_color_keep": lambda: _released(ops.compose_layers(A, LAYERS, color=True, keep=True)),
        "compose_device": lambda: ops.compose_layers(on_device(A), LAYERS),
        "compose_device_keep": lambda: _released(ops.compose_layers(on_device(A), LAYERS, keep=True)),
        "compose_device_color": lambda: ops.compose_layers(on_device(A), LAYERS, color=True),
        "draw": lambda: ops.draw(A, COMMANDS),
        "draw_device_keep": lambda: _released(ops.draw(on_device(COL), [COMMANDS[0][:1], COMMANDS[1][1:]], keep=True)),
        "draw_contours": lambda: _drawn_contours(ops, TILES),
        "draw_contours_device_keep": lambda: _released(_drawn_contours(ops, on_device(TILES), keep=True)),
        "jpeg_encode": lambda: ops.jpeg_encode(JPEG_FRAMES),
        "jpeg_encode_420": lambda: ops.jpeg_encode(JPEG_FRAMES, sampling="4:2:0"),
        "jpeg_encode_device": lambda: _jpeg_from_device(ops),
        "jpeg_decode": lambda: ops.jpeg_decode(_jpeg_files(ops, "4:4:4")),
        "jpeg_decode_420_keep": lambda: _released(ops.jpeg_decode(_jpeg_files(ops, "4:2:0"), keep=True)),
        "curves_equidistant": lambda: ops.curves_equidistant(CURVES, spacing=0.75, ret_lengths=True),
        "simplify_rdp": lambda: ops.simplify_curves(CURVES, 0.2),
        "simplify_visvalingam": lambda: ops.simplify_curves(CURVES, 0.05, method="visvalingam"),
        "skeleton_graphs": lambda: [tuple(g[:2]) for g in ops.skeleton_graphs([SKELETON, SKELETON[:9, :12]])],
        "potential_gradients": lambda: _gradients(ops),
    }


def _jpeg_from_device(ops):
    stack = ops.DeviceFrames.upload(JPEG_FRAMES)
    try:
        return ops.jpeg_encode(stack)
    finally:
        stack.release()


# as WARM_AT_PARENT, with libvideoanalysis_hip.so behind the proxy; from "find_contours" on: at commit 6c0fbaa, before the
# lease owned the results that outlive a call, the exact-room rerun was one step and the packed buffers had a layout
WARM_AT_PARENT_GPU = {"fill_polys": (0, 0, 4, 2, 6), "distance_transform": (0, 0, 3, 2, 5),
                      "guo_hall_thinning": (0, 0, 3, 3, 6), "gaussian_u8": (0, 0, 1, 1, 2),
                      "find_contours": (0, 0, 1, 6, 7), "find_contours_keep": (0, 0, 1, 2, 3),
                      "compose_array": (0, 0, 5, 1, 6), "compose_array_keep": (0, 0, 5, 1, 7),
                      "compose_array_color_keep": (0, 0, 5, 1, 7), "compose_device": (0, 0, 5, 1, 6),
                      "compose_device_keep": (0, 0, 5, 1, 7), "compose_device_color": (0, 0, 5, 1, 6),
                      "draw": (0, 0, 4, 2, 6), "draw_device_keep": (0, 0, 4, 2, 6), "draw_contours": (0, 0, 2, 4, 6),
                      "draw_contours_device_keep": (0, 0, 2, 4, 6), "jpeg_encode": (0, 0, 2, 3, 5),
                      "jpeg_encode_420": (0, 0, 2, 3, 5), "jpeg_encode_device": (0, 0, 2, 3, 5),
                      "jpeg_decode": (0, 0, 3, 2, 5), "jpeg_decode_420_keep": (0, 0, 3, 2, 5),
                      "curves_equidistant": (0, 0, 1, 1, 2), "simplify_rdp": (0, 0, 1, 1, 2),
                      "simplify_visvalingam": (0, 0, 1, 1, 2), "skeleton_graphs": (0, 0, 3, 6, 9),
                      "potential_gradients": (2, 2, 1, 0, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WARM_AT_PARENT_GPU))
def test_abi_calls_of_a_warm_call_on_the_product(product, name):
    from video import ops
    counters = warm_counters(product, _gpu_cases(ops)[name])
    print(name, dict(zip(COUNTED, counters)))
    assert counters == WARM_AT_PARENT_GPU[name]


@pytest.mark.gpu
def test_refused_calls_return_their_buffers_on_the_product(product):
    """both refusals are argument checks: nothing is launched"""
    from video import ops
    ok = np.ones((2, 8, 8), np.uint8)
    wide = np.ones((2, 8, 8200), np.uint8)        # frames wider than 8192 columns are refused; other sizes than `ok`
    assert_conserved(product, lambda: ops.distance_map(ok, [[(1, 1)], [(2, 2)]], [[(5, 5)], [(6, 6)]]),
                     lambda: ops.distance_map(wide, [[(1, 1)], [(2, 2)]], [[(5, 5)], [(6, 6)]]), same_sizes=False)
    tall = np.zeros((65535 * 32 + 1, 1), np.uint8)                            # the scratch query answers 0
    assert_conserved(product, lambda: ops.guo_hall_thinning([NOTCHED], implementation="tiled"),
                     lambda: ops.guo_hall_thinning([tall], implementation="tiled"))


def _refusing(proxy, entry, call):
    """`call` with the entry point `entry` answered -22 by the proxy"""
    def refused():
        proxy.refuse.add(entry)
        try:
            return call()
        finally:
            proxy.refuse.clear()
    return refused


@pytest.mark.gpu
def test_refused_launches_return_the_results_too(product):
    """the ops whose results outlive the call, with their entry point answered -22 by the proxy (nothing is launched):
    the pooled results are back in the pool, and a DeviceFrames handed in is still the caller's and holds its frames"""
    from video import ops
    cases = (("va_find_contours", lambda: ops.find_contours(MASKS, keep=True).release()),
             ("va_compose_layers_u8", lambda: ops.compose_layers(A, LAYERS, color=True, keep=True).release()),
             ("va_draw_u8", lambda: ops.draw(A, COMMANDS)),
             ("va_draw_contours_u8", lambda: _drawn_contours(ops, TILES)),
             ("va_jpeg_decode_u8", lambda: ops.jpeg_decode(_jpeg_files(ops, "4:4:4"), keep=True).release()))
    _jpeg_files(ops, "4:4:4")
    for entry, call in cases:
        assert_conserved(product, call, _refusing(product, entry, call))
    stack, color = ops.DeviceFrames.upload(A), ops.DeviceFrames.upload(COL)
    tiles = ops.DeviceFrames.upload(TILES)
    for entry, held, call in (
            ("va_compose_layers_u8", stack, lambda: ops.compose_layers(stack, LAYERS, keep=True)),
            ("va_compose_layers_u8", stack, lambda: ops.compose_layers(stack, LAYERS, color=True)),
            ("va_draw_u8", stack, lambda: ops.draw(stack, COMMANDS)),
            ("va_draw_u8", color, lambda: ops.draw(color, COMMANDS[:2], keep=True)),
            ("va_draw_contours_u8", tiles, lambda: _drawn_contours(ops, tiles)),
            ("va_jpeg_encode_u8", color, lambda: ops.jpeg_encode(color)),
            ("va_find_contours", tiles, lambda: ops.find_contours(tiles))):
        with pytest.raises(RuntimeError):
            _refusing(product, entry, call)()
        assert held.buf is not None, entry
    for held, frames in ((stack, A), (color, COL), (tiles, TILES)):
        assert np.array_equal(_released(held), frames)


@pytest.mark.gpu
def test_refused_gradients_free_their_planes(product):
    """fx and fy are not pooled: a refused potential_gradients frees exactly the two, at once and not through the
    collector, and allocates nothing else anew; a good call hands them to the caller"""
    from video import ops
    refused = _refusing(product, "va_sobel5_f64", lambda: _gradients(ops))
    ops.pool_clear()
    _gradients(ops)
    for _ in range(2):
        product.reset()
        with pytest.raises(RuntimeError):
            refused()
        assert (product.calls["va_malloc"], product.calls["va_free"]) == (2, 2)
        gc.collect()
        assert product.calls["va_free"] == 2
        product.reset()
        assert _gradients(ops) == A.shape
        assert (product.calls["va_malloc"], product.calls["va_free"]) == (2, 2)


@pytest.mark.gpu
def test_who_holds_the_frames_after_each_op(product):
    """the ownership table of the ops that take a DeviceFrames: which objects are released (buf is None) after a call
    that succeeds and after one that is refused, and whether keep=True returns the object handed in"""
    from video import ops
    up = ops.DeviceFrames.upload
    mono = lambda: up(A)

    def check(make, call, entry, released, same=None):
        """call(stack) on a fresh stack: on success `released` says whether it is released, `same` whether the result
        is the stack itself (None: an array comes back); refused, it stays the caller's"""
        stack = make()
        out = call(stack)
        assert (stack.buf is None) == released
        if same is None:
            assert isinstance(out, np.ndarray)
        else:
            assert isinstance(out, ops.DeviceFrames) and (out is stack) == same and out.buf is not None
            out.release()
        stack = make()
        with pytest.raises(RuntimeError):
            _refusing(product, entry, lambda: call(stack))()
        assert stack.buf is not None
        assert np.array_equal(_released(stack), A)

    compose = "va_compose_layers_u8"
    check(mono, lambda s: ops.compose_layers(s, LAYERS, keep=True), compose, released=False, same=True)
    check(mono, lambda s: ops.compose_layers(s, LAYERS, color=True, keep=True), compose, released=True, same=False)
    check(mono, lambda s: ops.compose_layers(s, LAYERS, color=True), compose, released=True)
    check(mono, lambda s: ops.compose_layers(s, LAYERS), compose, released=True)
    check(mono, lambda s: ops.draw(s, COMMANDS, keep=True), "va_draw_u8", released=False, same=True)
    check(mono, lambda s: ops.draw(s, COMMANDS), "va_draw_u8", released=True)
    tiles = lambda: up(A[:, :16, :16])
    found = ops.find_contours(np.stack([NOTCHED] * 3), keep=True)
    try:
        for keep in (True, False):
            stack = tiles()
            out = ops.draw_contours(stack, found, 255, keep=keep)
            assert (out is stack) if keep else (isinstance(out, np.ndarray) and stack.buf is None)
            stack.release()
            stack = tiles()
            with pytest.raises(RuntimeError):
                _refusing(product, "va_draw_contours_u8", lambda: ops.draw_contours(stack, found, 255, keep=keep))()
            assert stack.buf is not None
            stack.release()
    finally:
        found.release()
    # no pixels: the stack handed in is released, zeros come back, on the device under keep
    for shape in ((0, 20, 30), (3, 0, 30), (3, 20, 0)):
        for keep in (False, True):
            stack = up(np.zeros(shape, np.uint8))
            out = ops.compose_layers(stack, [[]] * shape[0], keep=keep)
            assert stack.buf is None and isinstance(out, ops.DeviceFrames if keep else np.ndarray)
            assert (_released(out) if keep else out).shape == shape
    # jpeg_encode and find_contours read a DeviceFrames and leave it alone, refused or not
    color, masks = up(JPEG_FRAMES), up(MASKS)
    for stack, entry, call in ((color, "va_jpeg_encode_u8", lambda: ops.jpeg_encode(color)),
                               (masks, "va_find_contours", lambda: ops.find_contours(masks))):
        call()
        assert stack.buf is not None
        with pytest.raises(RuntimeError):
            _refusing(product, entry, call)()
        assert stack.buf is not None
    assert np.array_equal(_released(color), JPEG_FRAMES) and np.array_equal(_released(masks), MASKS)


@pytest.mark.gpu
def test_point_lists_longer_than_the_capacity_run_again_with_room(product, monkeypatch):
    from video import ops
    dmap = ops.distance_map(np.ones((12, 12), np.uint8), [(0, 0)])
    calls = {
        "va_largest_contour": lambda **kw: ops.largest_contour(NOTCHED, **kw)[::2],      # (points, components)
        "va_distance_map_path": lambda **kw: ops.distance_map_path(dmap, (11, 11), **kw),
        "va_farthest_points": lambda **kw: ops.farthest_points(NOTCHED, ret_path=True, **kw),
    }
    whole = {}
    for entry, call in calls.items():
        product.reset()
        whole[entry] = call()
        points = whole[entry][0] if entry == "va_largest_contour" else whole[entry]
        assert len(points) > 4 and product.calls[entry] == 1
    monkeypatch.setattr(ops, "DEFAULT_POINT_CAPACITY", 4)
    for entry, call in calls.items():
        product.reset()
        _same(call(), whole[entry])
        assert product.calls[entry] == 2, entry
        product.reset()
        first = call(max_points=4)                # an explicit capacity truncates: one launch, the first four points
        assert product.calls[entry] == 1, entry
        if entry == "va_largest_contour":
            _same(first, (whole[entry][0][:4], whole[entry][1]))
        else:
            _same(first, whole[entry][:4])
