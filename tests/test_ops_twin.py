"""video.ops, the per-call host layer, behind a counting proxy of the C ABI.

The proxy wraps a library bound with `video._hip.SIGNATURES` and counts va_malloc / va_free / va_memcpy_h2d /
va_memcpy_d2h / va_stream_sync (and whatever kernel entry points a test names).  On a box without a GPU the library
is the oracle's twin, oracle/libvideoanalysis_cpu.so (tests/test_abi_twin.py); the tests marked gpu put the product
behind the same proxy for the ops the twin lacks.  Three properties of the host path are pinned:

  conservation : a call the library refuses hands every pooled buffer back -- good, refused, good allocates what the
                 first good call allocated and frees nothing (a buffer left to the garbage collector is a hipFree,
                 which synchronises the device: what the pool exists to avoid)
  ABI calls    : a warm call makes exactly the ABI calls it made at commit 3b20f39, before the ops shared one
                 buffer lease, one ragged packer and one retry loop; the host path's speed check, and an exact one
  retry        : the grow-and-retry loop of the point-list ops, reached with DEFAULT_POINT_CAPACITY set to 4
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libvideoanalysis_cpu.so")
COUNTED = ("va_malloc", "va_free", "va_memcpy_h2d", "va_memcpy_d2h", "va_stream_sync")


class CountingLib(object):
    """a bound library with the calls of COUNTED (+ `extra`) counted; va_trim is answered with 0"""

    def __init__(self, lib, extra=()):
        self._lib = lib
        self.calls = dict.fromkeys(COUNTED + tuple(extra), 0)

    def __getattr__(self, name):
        if name == "va_trim":
            return lambda nbytes: 0
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
        with pytest.raises((_hip.HipError, ValueError)) as err:
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


# ------------------------------------------------------------------------------------- on the product (GPU)
BOXES = [(2, 3, 5, 7), (0, 0, 0, 4), (-1, 1, 9, 3)]                          # (x, y, w, h)
POLYS = [np.array([[2, 3], [6, 4], [4, 9]]), np.array([[0, 0], [0, 3]]), np.array([[-1, 1], [7, 1], [7, 3], [0, 3]])]
RAGGED = [np.ones((h, w), np.uint8) for _, _, w, h in BOXES]
NOTCHED = np.zeros((16, 16), np.uint8)
NOTCHED[3:13, 3:13] = 1
NOTCHED[3:7, 7:9] = 0


def _gpu_cases(ops):
    return {
        "fill_polys": lambda: ops.fill_polys(POLYS, BOXES),
        "distance_transform": lambda: ops.distance_transform(RAGGED),
        "guo_hall_thinning": lambda: ops.guo_hall_thinning(RAGGED + [np.zeros((0, 0), np.uint8)]),
        "gaussian_u8": lambda: ops.gaussian_blur(A, 2.0),
    }


# as WARM_AT_PARENT, with libvideoanalysis_hip.so behind the proxy
WARM_AT_PARENT_GPU = {"fill_polys": (0, 0, 4, 2, 6), "distance_transform": (0, 0, 3, 2, 5),
                      "guo_hall_thinning": (0, 0, 3, 3, 6), "gaussian_u8": (0, 0, 1, 1, 2)}


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
