"""NumPy-in / NumPy-out wrappers over the C ABI (one upload, kernels, one download).

These are the per-call building blocks behind ``video.filters`` and ``video.analysis``; the
batched, device-resident path is :class:`video.engine.FrameEngine`.  Everything here runs on
the GPU through ``libvideoanalysis_hip.so`` -- nothing is computed with NumPy.
"""
import collections
import ctypes as C
import math
import threading

import numpy as np

from . import _hip
from ._hip import DeviceBuffer, check

# ------------------------------------------------------------------------ device-buffer pool
# The per-call wrappers below run once per frame when filters are used one by one; a hipMalloc /
# hipFree pair per operand and call (both synchronise the device) used to dominate them.  Buffers
# are recycled by size class (powers of two) instead; the pool is bounded and trimmed on overflow.
_POOL = {}
_POOL_BYTES = 0
_POOL_LOCK = threading.Lock()       # VideoPreprocessor runs these ops from one worker thread per function
POOL_CAPACITY = 4 << 30


_FILL = _hip.fill_mode()            # the test fill mode's byte, -1 when off: _hip.set_fill_mode keeps it current


def _on_fill_mode(byte):
    global _FILL
    _FILL = byte


_hip._fill_watchers.append(_on_fill_mode)


def _take(nbytes):
    """a device buffer of at least `nbytes` bytes (recycled when one of its size class is free)"""
    global _POOL_BYTES
    size = max(256, 1 << max(int(nbytes) - 1, 1).bit_length())
    if _FILL >= 0:
        return _take_guarded(int(nbytes), size)
    with _POOL_LOCK:
        free = _POOL.get(size)
        if free:
            _POOL_BYTES -= size
            return free.pop()
    return DeviceBuffer(size)


def _take_guarded(nbytes, size):
    """_take in the test fill mode: the whole buffer holds the fill byte, a recycled one as much as a fresh one, and
    its guarded range starts at the size asked for: the slack of the size class, then the tail"""
    global _POOL_BYTES
    buf = None
    with _POOL_LOCK:
        free = _POOL.get(size)
        if free:
            _POOL_BYTES -= size
            buf = free.pop()
    if buf is not None and buf._fill != _FILL:      # pooled under another setting of the mode
        buf.free()
        buf = None
    if buf is None:
        buf = DeviceBuffer(size)
    else:
        buf.refill()
    buf._asked = nbytes
    return buf


def _upload(arr, stream=None):
    arr = np.ascontiguousarray(arr)
    buf = _take(arr.nbytes)
    buf.upload(arr, stream)
    return buf


def _give(*bufs):
    """hand buffers back (every call below has synchronised its stream by then)"""
    global _POOL_BYTES
    damage = _damage(bufs) if _FILL >= 0 else None
    for b in bufs:
        if b is None:
            continue
        with _POOL_LOCK:
            keep = _POOL_BYTES + b.nbytes <= POOL_CAPACITY
            if keep:
                _POOL.setdefault(b.nbytes, []).append(b)
                _POOL_BYTES += b.nbytes
        if not keep:
            b.free()
    if damage:
        raise _hip.GuardViolation(damage)


def _damage(bufs):
    """test fill mode: what the guarded ranges of a call's buffers show (this synchronises, which the mode may);
    None when they all still hold the fill byte"""
    found = [d for d in (b.check_guard() for b in bufs if b is not None) if d]
    if not found:
        return None
    return ("a call with buffers of %s bytes wrote behind the end of %s"
            % ([b._asked for b in bufs if b is not None], "; ".join(found)))


def pool_clear():
    """free every pooled buffer (tests; before handing the GPU to another library) and let the
    library's own scratch pool go back to the device (va_trim)"""
    global _POOL_BYTES
    with _POOL_LOCK:
        bufs = [b for free in _POOL.values() for b in free]
        _POOL.clear()
        _POOL_BYTES = 0
    for b in bufs:
        b.free()
    try:
        _hip.load_library().va_trim(0)
    except Exception:
        pass


class _Lease(list):
    """the pooled device buffers of one call (the list holds them).  Every buffer handed out goes back to the pool
    when the block ends: after the call's downloads, which synchronise its stream, or on an exception as it is,
    without a synchronisation of its own (none may be added to any path: the pool exists to keep them off the
    per-call ops).  The one exception is compose_layers(keep=True), which returns without a download: it
    synchronises its stream once before its tables go back to the pool, because the launch still reads them.
    A buffer that outlives the call is a result (result, adopt): the lease owns it until the block ends.  A clean end
    leaves it to the caller; an exception disposes of it with the rest: into the pool, or through its own `drop`."""
    stream = None                       # the call's stream, for the ops that have one: _Lease.on(stream)

    def __init__(self):
        list.__init__(self)
        self.results = []               # (buffer, drop)

    @classmethod
    def on(cls, stream):
        lease = cls()
        lease.stream = stream
        return lease

    def __enter__(self):
        return self

    def __exit__(self, failure, *exc):
        try:
            if failure is not None:
                self.recall()
        finally:
            _give(*self)

    def take(self, nbytes):
        """a buffer of at least `nbytes` bytes for an output or a workspace"""
        buf = _take(nbytes)
        self.append(buf)
        return buf

    def adopt(self, buf, drop=None):
        """`buf` becomes a result of this call; drop: how a buffer that is not the pool's is disposed of"""
        self.results.append((buf, drop))
        return buf

    def result(self, nbytes):
        """a pooled buffer of at least `nbytes` bytes that is a result of this call"""
        return self.adopt(_take(nbytes))

    def absorb(self, buf):
        """the pooled buffer `buf`, a result or the caller's, is the lease's from now on: it goes back with the rest"""
        self.results = [(b, drop) for b, drop in self.results if b is not buf]
        self.append(buf)

    def recall(self):
        """the results so far are disposed of now: after a failure, or before a second attempt takes its own"""
        lost, self.results = self.results, []
        for buf, drop in lost:
            (drop or _give)(buf)

    def upload(self, arr):
        """a buffer holding `arr`, copied on the call's stream; None (an optional operand left out) stays None"""
        if arr is None:
            return None
        buf = self.take(arr.nbytes)
        buf.upload(arr, self.stream)
        return buf


def _ptr(buf):
    return None if buf is None else buf.ptr


def _rerun(run, *caps):
    """run(*caps) launches with room for caps and returns (payload, needs), what the input needs of each.  A need beyond
    its cap runs exactly once more, with the needs as caps; the last answer is returned, and the buffers are run's."""
    payload, needs = run(*caps)
    if any(int(need) > cap for need, cap in zip(needs, caps)):
        payload, needs = run(*(int(need) for need in needs))
    return payload, needs


class _Layout(object):
    """named fields back to back in one buffer of `nbytes`, in the order given and unpadded (the orders in use are
    naturally aligned), field `name` at byte at[name].  A field is an array (an upload) or (count, dtype) (an output)."""

    def __init__(self, **fields):
        self.fields, self.at, self.nbytes = fields, {}, 0
        for name, field in fields.items():
            self.at[name] = self.nbytes
            self.nbytes += field[0] * np.dtype(field[1]).itemsize if type(field) is tuple else field.nbytes

    def packed(self):
        """the uint8 array of an upload: the bytes of every field"""
        return np.concatenate([np.frombuffer(arr, np.uint8) for arr in self.fields.values()])     # (C-contiguous arrays)

    def ptr(self, buf, name):
        """the device address of field `name` in the buffer `buf`"""
        return buf.ptr + self.at[name]

    def view(self, raw, name):
        """field `name` of the downloaded uint8 array `raw`, in its dtype"""
        field = self.fields[name]
        count, dtype = field if type(field) is tuple else (field.size, field.dtype)
        return np.frombuffer(raw, dtype, count, self.at[name])


# the one dtype -> VA_* table (TEMPORAL_DTYPES: what the temporal statistics take, which is all of it)
_DTYPE_CODES = {np.dtype(np.uint8): _hip.VA_U8, np.dtype(np.int16): _hip.VA_I16,
                np.dtype(np.float32): _hip.VA_F32, np.dtype(np.float64): _hip.VA_F64}
TEMPORAL_DTYPES = _DTYPE_CODES
_TARGET_DTYPES = (np.uint8, np.float32, np.float64)       # what normalize_any and gaussian_noise write


def _as_mask(a, keep_uint8=False):
    """contiguous uint8 mask, 1 where `a` is non-zero; keep_uint8: a uint8 array goes through with its own values"""
    a = np.asarray(a)
    if keep_uint8 and a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a != 0, np.uint8)


def _as_batch(arr, frame_ndim):
    """returns (contiguous array, n, frame_shape, was_single)"""
    arr = np.ascontiguousarray(arr)
    if arr.ndim == frame_ndim:
        return arr, 1, arr.shape, True
    if arr.ndim == frame_ndim + 1:
        return arr, arr.shape[0], arr.shape[1:], False
    raise ValueError("expected %d or %d dimensions, got shape %r"
                     % (frame_ndim, frame_ndim + 1, arr.shape))


def _hwc(frame_shape):
    if len(frame_shape) == 2:
        return frame_shape[0], frame_shape[1], 1
    if len(frame_shape) == 3:
        return frame_shape
    raise ValueError("frames must be (H,W) or (H,W,C), got %r" % (frame_shape,))


def _map(fn, arr, out_shape, out_dtype, *args):
    """fn(src, dst, *args) from the uploaded `arr` into a buffer that comes back as an out_shape / out_dtype array"""
    with _Lease() as d:
        src, dst = d.upload(arr), d.take(math.prod(out_shape) * np.dtype(out_dtype).itemsize)
        check(fn(src.ptr, dst.ptr, *args))
        return dst.download(out_shape, out_dtype)


def _pointwise_u8(fn, arr, out_shape, *args):
    return _map(fn, arr, out_shape, np.uint8, *args)


def gaussian_blur(frames, sigma, color=False, implementation=None, tap_rule="cv4"):
    """cv2.GaussianBlur(frame, (0,0), sigma) on uint8 or float32 frames
    (FilterBlur._process_frame, video/filters.py:388-392).

    frames: (H,W), (N,H,W); with color=True (H,W,C), (N,H,W,C).
    implementation: None (library's choice) or 'generic' (uint8 only, for cross-checks).
    tap_rule (uint8 only): 'cv4' | 'cv3', see FilterBlur.
    """
    frames = np.asarray(frames)
    if frames.dtype not in (np.uint8, np.float32):
        raise TypeError("gaussian_blur supports uint8 and float32, got %s" % frames.dtype)
    arr, n, fshape, single = _as_batch(frames, 3 if color else 2)
    h, w, c = _hwc(fshape)
    L = _hip.lib()
    if arr.dtype != np.uint8:
        fn = L.va_gaussian_f32
    elif tap_rule != "cv4":
        if implementation is not None:
            raise ValueError("the implementation hooks run the default tap rule only")
        fn = lambda *a: L.va_gaussian_u8_rule(*(a[:7] + (_hip.TAP_RULES[tap_rule],) + a[7:]))
    else:
        fn = getattr(L, {None: "va_gaussian_u8", "generic": "va_gaussian_u8_generic",
                         "valu": "va_gaussian_u8_valu"}[implementation])
    with _Lease() as d:                 # not through _map: the op that runs once per frame pays for no extra call
        src, dst = d.upload(arr), d.take(arr.nbytes)
        check(fn(src.ptr, dst.ptr, n, h, w, c, float(sigma), None))
        return dst.download(arr.shape, arr.dtype)


class BackgroundModel(object):
    """device-resident background state (BUILD-DEFINED FilterBackground; cumulative mean =
    measure_mean's arithmetic, video/analysis/video.py:33)."""

    def __init__(self, frame_shape, mode="mean", rate=0.02, dtype=np.uint8, background=None):
        self.mode = _hip.BG_MODES[mode]
        if self.mode == _hip.BG_NONE:
            raise ValueError("mode must be 'mean', 'ema' or 'static'")
        self.frame_shape = tuple(frame_shape)
        self.px = int(np.prod(self.frame_shape))
        self.rate = float(rate)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.uint8, np.float32):
            raise TypeError("background model supports uint8 and float32 frames")
        if self.dtype == np.float32 and self.mode != _hip.BG_EMA:
            raise ValueError("float32 frames support mode='ema' only")
        self.state_dtype = np.float32 if self.mode == _hip.BG_EMA else np.float64
        self.n_seen = 0
        init = np.zeros(self.frame_shape, self.state_dtype)
        if background is not None:
            init = np.ascontiguousarray(background, self.state_dtype).reshape(self.frame_shape)
        elif self.mode == _hip.BG_STATIC:
            raise ValueError("mode='static' needs a background image")
        self._state = _upload(init)

    def process(self, frames, want_diff=True):
        """fold `frames` (N, *frame_shape) in, return |frame - bg_prev| per frame"""
        arr = np.ascontiguousarray(frames, self.dtype)
        if arr.shape[1:] != self.frame_shape:
            raise ValueError("frames of shape %r do not match %r" % (arr.shape[1:], self.frame_shape))
        n = arr.shape[0]
        with _Lease() as d:
            src = d.upload(arr)
            dst = d.take(arr.nbytes) if want_diff else None
            check(_hip.lib().va_bg_update(self.mode, _DTYPE_CODES[self.dtype], src.ptr, _ptr(dst), self._state.ptr,
                                          self.n_seen, self.rate, n, self.px, None))
            if self.mode != _hip.BG_STATIC:
                self.n_seen += n
            return dst.download(arr.shape, arr.dtype) if dst else None

    @property
    def state(self):
        return self._state.download(self.frame_shape, self.state_dtype)

    def set_state(self, state, n_seen):
        self._state.upload(np.ascontiguousarray(state, self.state_dtype).reshape(self.frame_shape))
        self.n_seen = int(n_seen)


def _temporal_frames(frames):
    arr = np.ascontiguousarray(frames)
    if arr.dtype not in TEMPORAL_DTYPES:
        raise TypeError("temporal statistics take uint8, int16, float32 or float64 frames on the GPU path, got %s"
                        % arr.dtype)
    return arr


def welford(frames, mean=None, m2=None, n_seen=0):
    """Welford update of measure_mean_std (video/analysis/video.py:48-50); returns (mean, M2).
    uint8, int16 (FilterTimeDifference), float32 or float64 (FilterNormalize's float64 target) frames."""
    arr = _temporal_frames(frames)
    fshape = arr.shape[1:]
    px = int(np.prod(fshape))
    mean = np.zeros(fshape) if mean is None else np.ascontiguousarray(mean, np.float64)
    m2 = np.zeros(fshape) if m2 is None else np.ascontiguousarray(m2, np.float64)
    with _Lease() as d:
        src, dm, dq = d.upload(arr), d.upload(mean), d.upload(m2)
        if arr.dtype == np.uint8:
            check(_hip.lib().va_welford_u8(src.ptr, dm.ptr, dq.ptr, int(n_seen), arr.shape[0], px, None))
        else:
            check(_hip.lib().va_welford_any(src.ptr, _DTYPE_CODES[arr.dtype], dm.ptr, dq.ptr, int(n_seen),
                                            arr.shape[0], px, None))
        return dm.download(fshape, np.float64), dq.download(fshape, np.float64)


def running_mean(frames, mean=None, n_seen=0):
    """measure_mean's update `mean*n/(n+1) + frame/(n+1)` (video/analysis/video.py:33) over a batch of
    uint8 / int16 / float32 / float64 frames, NumPy's promotions included; returns the float64 mean"""
    arr = _temporal_frames(frames)
    fshape = arr.shape[1:]
    px = int(np.prod(fshape))
    mean = np.zeros(fshape) if mean is None else np.ascontiguousarray(mean, np.float64)
    with _Lease() as d:
        src, dm = d.upload(arr), d.upload(mean)
        check(_hip.lib().va_mean_any(src.ptr, _DTYPE_CODES[arr.dtype], dm.ptr, int(n_seen), arr.shape[0], px, None))
        return dm.download(fshape, np.float64)


# ------------------------------------------------------------------------ temporal median and rank planes
TEMPORAL_MAX_PLANES = 255        # kMaxPlanes and kMaxRanks of va_median_math.h: the planes and ranks of one call
TEMPORAL_MAX_RANKS = 8
PERCENTILE_METHODS = ("lower", "higher", "nearest")


def _temporal_planes(frames, step, what):
    """(DeviceFrames or contiguous uint8 array, planes in use, frame shape) of a stack read every `step` frames;
    every check of the stack is here, and none of them needs a device"""
    src, n, h, w, c, _ = _frames_in(frames, what)
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or step < 1:
        raise ValueError("%s: step is an integer >= 1, got %r" % (what, step))
    t = (n + int(step) - 1) // int(step)
    if t < 1 or h * w * c == 0:
        raise ValueError("%s: the stack %r holds no pixels" % (what, (n, h, w, c)))
    if t > TEMPORAL_MAX_PLANES:
        raise ValueError("%s: at most %d planes a call, got %d (every %d of %d frames)"
                         % (what, TEMPORAL_MAX_PLANES, t, step, n))
    return src, t, (h, w) + ((3,) if c == 3 else ())


def _check_ranks(ranks, t, what):
    ranks = [ranks] if isinstance(ranks, (int, np.integer)) else list(ranks)
    if not 1 <= len(ranks) <= TEMPORAL_MAX_RANKS:
        raise ValueError("%s: 1 .. %d ranks a call, got %d" % (what, TEMPORAL_MAX_RANKS, len(ranks)))
    for r in ranks:
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r < t:
            raise ValueError("%s: ranks of %d planes are integers 0 .. %d, got %r" % (what, t, t - 1, r))
    return np.array(ranks, np.int32)


def temporal_ranks(frames, ranks, step=1, stream=None):
    """out[j] = np.sort(frames[::step], axis=0)[ranks[j]]: the rank planes of a uint8 stack over time (DESIGN.md §9,
    "Temporal median"; va_temporal_ranks_u8), exact.  frames: a uint8 array (t, h, w) or (t, h, w, 3), or a
    DeviceFrames, which is not changed; step > 1 reads the planes 0, step, 2 step, ... where they lie (a frame stride,
    no gather).  At most 255 planes in use and 8 ranks, each 0 .. planes - 1, in any order, repeats allowed.
    Returns (len(ranks), h, w[, 3]) uint8."""
    src, t, fshape = _temporal_planes(frames, step, "temporal_ranks")
    rk = _check_ranks(ranks, t, "temporal_ranks")
    px = math.prod(fshape)
    L = _hip.lib()
    with _Lease.on(stream) as d:
        ptr = src.buf.ptr if isinstance(src, DeviceFrames) else d.upload(src).ptr
        out = d.take(len(rk) * px)
        check(L.va_temporal_ranks_u8(ptr, t, px, int(step) * px, rk.ctypes.data, len(rk), out.ptr, stream))
        return out.download((len(rk),) + fshape, np.uint8, stream)


def median_ranks(t):
    """the two ranks whose mean is the median of t values (equal for odd t)"""
    return (t - 1) // 2, t // 2


def median_of_ranks(lower, upper):
    """np.median from the planes of median_ranks: float64, bit for bit"""
    return (lower.astype(np.float64) + upper) / 2


def temporal_median(frames, step=1):
    """np.median(frames[::step], axis=0) of a uint8 stack (or DeviceFrames), float64, bit for bit"""
    src, t, _ = _temporal_planes(frames, step, "temporal_median")
    lo, hi = median_ranks(t)
    planes = temporal_ranks(src, [lo] if lo == hi else [lo, hi], step)
    return median_of_ranks(planes[0], planes[-1])


def percentile_rank(t, q, method="lower"):
    """the index into t sorted values that np.percentile(..., q, method=method) takes, for the methods that take one
    value.  The ends are integers.  In between NumPy computes (t - 1) * (q / 100) in float64 and rounds that; the
    exact quotient (t - 1) * q // 100 differs from it for some (t, q) -- t = 26, q = 28, 'higher' gives 8, not 7 --
    so NumPy's own expression is used."""
    if method not in PERCENTILE_METHODS:
        raise ValueError("percentile method is one of %r (the interpolating ones are not built), got %r"
                         % (PERCENTILE_METHODS, method))
    if not 0 <= q <= 100:                                   # (a NaN fails this too)
        raise ValueError("percentiles lie in 0 .. 100, got %r" % (q,))
    if q == 0 or q == 100:
        return 0 if q == 0 else t - 1
    virtual = (t - 1) * np.true_divide(q, 100)
    return int({"lower": np.floor, "higher": np.ceil, "nearest": np.around}[method](virtual))


def temporal_percentiles(frames, q, method="lower", step=1):
    """np.percentile(frames[::step], q, axis=0, method=method) of a uint8 stack (or DeviceFrames) for method 'lower',
    'higher' or 'nearest': one uint8 plane for a scalar q, a stack of one plane per entry for a sequence.  The
    distinct ranks go to the device eight a call."""
    src, t, fshape = _temporal_planes(frames, step, "temporal_percentiles")
    scalar = np.ndim(q) == 0
    want = [percentile_rank(t, float(v), method) for v in np.atleast_1d(np.asarray(q, np.float64)).ravel()]
    distinct = sorted(set(want))
    planes, uploaded = {}, None
    if len(distinct) > TEMPORAL_MAX_RANKS and not isinstance(src, DeviceFrames):
        src = uploaded = DeviceFrames.upload(src)           # several calls: one upload
    try:
        for a in range(0, len(distinct), TEMPORAL_MAX_RANKS):
            part = distinct[a:a + TEMPORAL_MAX_RANKS]
            planes.update(zip(part, temporal_ranks(src, part, step)))
    finally:
        if uploaded is not None:
            uploaded.release()
    out = np.stack([planes[r] for r in want]) if want else np.zeros((0,) + fshape, np.uint8)
    return out[0] if scalar else out


# ------------------------------------------------------------------------ sliding-window median
SLIDING_MAX_WINDOW = 65535       # kMaxWindow of va_sliding_median_math.h: a uint16 counter holds the whole window
SLIDING_WANTS = ("diff", "lower", "upper", "median")


def _check_window(window, what):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= SLIDING_MAX_WINDOW:
        raise ValueError("%s: window is an integer 1 .. %d, got %r" % (what, SLIDING_MAX_WINDOW, window))
    return int(window)


class SlidingMedian(object):
    """the exact median of the `window` frames before each frame of a uint8 stream, streaming ("Sliding
    median"; va_sliding_median_u8).  The object holds the device state -- per-pixel histograms, the rank tracker and a
    ring of the last `window` frames, allocated once -- and n_seen, the frames folded in so far.

    For frame k: lower[k] / upper[k] are the sorted window max(0, k - window) .. k - 1 at ranks (cnt - 1) // 2 and
    cnt // 2 (cnt = min(k, window); both 0 for the empty window), median = (lower + upper) / 2 in float64 = np.median
    of the window, diff = sat_u8(trunc(|frame - median|)), FilterBackground's rule.  Then frame k enters the window.
    frame_shape: (h, w) or (h, w, 3); 1 <= window <= 65535."""

    def __init__(self, frame_shape, window, stream=None):
        shape = tuple(int(v) for v in frame_shape)
        if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3) or min(shape) < 1:
            raise ValueError("SlidingMedian: frames are (h, w) or (h, w, 3) with at least one pixel, got %r"
                             % (frame_shape,))
        self.window = _check_window(window, "SlidingMedian")
        self.frame_shape, self.px, self.stream = shape, math.prod(shape), stream
        self.n_seen = 0
        L = _hip.lib()
        self.state_bytes = int(L.va_sliding_median_state_bytes(self.px, self.window))
        if self.state_bytes < 1:
            raise ValueError("SlidingMedian: no state for %d pixels and a window of %d" % (self.px, self.window))
        self._state = _take(self.state_bytes)
        self.reset()

    def reset(self):
        """back to the empty window"""
        check(_hip.lib().va_memset(self._state.ptr, 0, self.state_bytes, self.stream))
        self.n_seen = 0

    def close(self):
        """hands the state back to the pool (after a synchronisation: a launch may still use it)"""
        state, self._state = getattr(self, "_state", None), None
        if state is not None:
            check(_hip.lib().va_stream_sync(self.stream))
            _give(state)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, frames, want=("diff",), keep=False):
        """folds `frames` -- a uint8 array (n, *frame_shape) or a DeviceFrames of that shape, which is not changed --
        into the window and returns {name: planes} for the names in `want`, any of 'diff', 'lower', 'upper' (uint8,
        (n, *frame_shape)) and 'median' (float64); want=() updates the state only.  keep=True returns the uint8 planes
        as DeviceFrames, the caller's to release ('median' is computed on the host and cannot be kept)."""
        want = (want,) if isinstance(want, str) else tuple(want)
        for name in want:
            if name not in SLIDING_WANTS:
                raise ValueError("SlidingMedian.process: want holds any of %r, got %r" % (SLIDING_WANTS, name))
        if keep and "median" in want:
            raise ValueError("SlidingMedian.process: 'median' is float64 from the host and cannot be kept")
        src, n, h, w, c, _ = _frames_in(frames, "SlidingMedian.process")
        if (h, w) + ((3,) if c == 3 else ()) != self.frame_shape:
            raise ValueError("SlidingMedian.process: frames of shape %r do not match %r"
                             % ((h, w) + ((3,) if c == 3 else ()), self.frame_shape))
        if self._state is None:
            raise ValueError("SlidingMedian.process: the model is closed")
        planes = [name for name in ("lower", "upper", "diff")
                  if name in want or (name != "diff" and "median" in want)]
        if n == 0:                                           # nothing enters the window
            if keep:
                return {name: DeviceFrames(_take(1), 0, h, w, c) for name in want}
            return {name: np.zeros((0,) + self.frame_shape, np.float64 if name == "median" else np.uint8)
                    for name in want}
        L, nbytes = _hip.lib(), n * self.px
        with _Lease.on(self.stream) as d:
            ptr = src.buf.ptr if isinstance(src, DeviceFrames) else d.upload(src).ptr
            bufs = {name: (d.result(nbytes) if keep else d.take(nbytes)) for name in planes}
            check(L.va_sliding_median_u8(ptr, n, self.px, self.px, self.window, self.n_seen, self._state.ptr,
                                         _ptr(bufs.get("lower")), _ptr(bufs.get("upper")), _ptr(bufs.get("diff")),
                                         self.stream))
            self.n_seen += n
            if keep:
                check(L.va_stream_sync(self.stream))        # the uploaded frames go back to the pool with the lease
                return {name: DeviceFrames(bufs[name], n, h, w, c) for name in want}
            host = {name: buf.download((n,) + self.frame_shape, np.uint8, self.stream) for name, buf in bufs.items()}
            if not host:
                check(L.va_stream_sync(self.stream))
        out = {name: host[name] for name in want if name != "median"}
        if "median" in want:
            out["median"] = median_of_ranks(host["lower"], host["upper"])
        return out

    def _current(self):
        L = _hip.lib()
        with _Lease.on(self.stream) as d:
            lo, up = d.take(self.px), d.take(self.px)
            check(L.va_sliding_median_current(self._state.ptr, self.px, self.window, self.n_seen, lo.ptr, up.ptr,
                                              self.stream))
            return (lo.download(self.frame_shape, np.uint8, self.stream),
                    up.download(self.frame_shape, np.uint8, self.stream))

    @property
    def lower(self):
        """the window as it stands at rank (cnt - 1) // 2: what the next frame would get as `lower`"""
        return self._current()[0]

    @property
    def upper(self):
        return self._current()[1]

    @property
    def median(self):
        """np.median of the frames in the window now, float64 (zeros for the empty window)"""
        return median_of_ranks(*self._current())


def sliding_median(frames, window, stream=None):
    """out[k] = np.median(frames[max(0, k - window + 1):k + 1], axis=0): the trailing medians of a uint8 stack (or a
    DeviceFrames), frame k included, float64 (n, h, w[, 3]), bit for bit.  One SlidingMedian pass: the planes before
    frame k + 1 are those of the window that ends with frame k, and the last ones are the state's current planes."""
    src, n, h, w, c, _ = _frames_in(frames, "sliding_median")
    window = _check_window(window, "sliding_median")
    fshape = (h, w) + ((3,) if c == 3 else ())
    if h * w == 0:
        raise ValueError("sliding_median: the stack %r holds no pixels" % ((n, h, w, c),))
    if n == 0:
        return np.zeros((0,) + fshape, np.float64)
    model = SlidingMedian(fshape, window, stream)
    try:
        before = model.process(src, want=("lower", "upper"))
        now = model._current()
        lower = np.concatenate([before["lower"][1:], now[0][None]])
        upper = np.concatenate([before["upper"][1:], now[1][None]])
    finally:
        model.close()
    return median_of_ranks(lower, upper)


def time_difference(this_frame, prev_frame):
    """this.astype(int16) - prev  (FilterTimeDifference, video/filters.py:564-568)"""
    a = np.ascontiguousarray(this_frame, np.uint8)
    b = np.ascontiguousarray(prev_frame, np.uint8)
    if a.shape != b.shape:
        raise ValueError("frame shapes differ")
    with _Lease() as d:
        da, db, do = d.upload(a), d.upload(b), d.take(a.size * 2)
        check(_hip.lib().va_time_difference_u8(da.ptr, db.ptr, do.ptr, a.size, None))
        return do.download(a.shape, np.int16)


def threshold(frames, thresh, maxval=255):
    """BUILD-DEFINED FilterThreshold: frames > thresh ? maxval : 0"""
    a = np.ascontiguousarray(frames, np.uint8)
    return _pointwise_u8(_hip.lib().va_threshold_u8, a, a.shape, a.size, int(thresh), int(maxval), None)


def mono_mean(frames):
    """np.mean(frame, axis=2).astype(uint8)  (FilterMonochrome, video/filters.py:365-366)"""
    a = np.ascontiguousarray(frames, np.uint8)
    if a.shape[-1] != 3:
        raise ValueError("last dimension must be 3")
    return _pointwise_u8(_hip.lib().va_mono_mean_u8, a, a.shape[:-1], a.size // 3, None)


def rot90(frames, k=1, color=False):
    """np.rot90(frame, k) per frame (FilterRotate, video/filters.py:339-344).
    frames: (H,W) / (N,H,W), with color=True (H,W,C) / (N,H,W,C); any dtype whose pixel
    (channels x itemsize) is 1, 2, 3, 4, 6, 8 or 12 bytes."""
    arr, n, fshape, single = _as_batch(np.ascontiguousarray(frames), 3 if color else 2)
    h, w, c = _hwc(fshape)
    k = int(k) % 4
    out_shape = ((w, h) if k & 1 else (h, w)) + ((c,) if color else ())
    out = _map(_hip.lib().va_rot90, arr, (n,) + out_shape, arr.dtype, n, h, w, c * arr.dtype.itemsize, k, None)
    return out[0] if single else out


def normalize(frames, fmin, fmax, alpha, tmin):
    """clip + affine + astype(uint8)  (FilterNormalize, video/filters.py:126-132)"""
    a = np.ascontiguousarray(frames, np.uint8)
    return _pointwise_u8(_hip.lib().va_normalize_u8, a, a.shape, a.size, float(fmin), float(fmax),
                         float(alpha), float(tmin), None)


INTERPOLATIONS = {"nearest": 0, "linear": 1, "cubic": 2, "area": 3, "lanczos": 4}


def resize(frames, size, interpolation="linear", color=False):
    """cv2.resize(frame, size, interpolation=...) per frame (FilterResize, video/filters.py:310-314);
    size = (width, height); uint8 or float32 frames (H,W) / (N,H,W), with color=True (H,W,C) / (N,H,W,C)"""
    frames = np.asarray(frames)
    if frames.dtype not in (np.uint8, np.float32):
        raise TypeError("resize supports uint8 and float32 frames on the GPU path, got %s" % frames.dtype)
    if interpolation not in INTERPOLATIONS:
        raise ValueError("Unknown interpolation method: %s" % (interpolation,))
    arr, n, fshape, single = _as_batch(frames, 3 if color else 2)
    h, w, c = _hwc(fshape)
    dw, dh = int(size[0]), int(size[1])
    if dw < 1 or dh < 1:
        raise ValueError("target size must be positive, got %r" % (size,))
    out_shape = (n, dh, dw) + ((c,) if color else ())
    fn = _hip.lib().va_resize_u8 if arr.dtype == np.uint8 else _hip.lib().va_resize_f32
    out = _map(fn, arr, out_shape, arr.dtype, n, h, w, c, dh, dw, INTERPOLATIONS[interpolation], None)
    return out[0] if single else out


def normalize_any(frames, fmin, fmax, alpha, tmin, dtype):
    """FilterNormalize for uint8 / float32 frames and uint8 / float32 / float64 targets
    (video/filters.py:126-132): clip, (f - fmin)*alpha + tmin, astype(dtype), with NumPy's types: in float64 for uint8
    frames, in float32 throughout for float32 frames"""
    a = np.ascontiguousarray(frames)
    dtype = np.dtype(dtype)
    if a.dtype not in (np.uint8, np.float32) or dtype not in _TARGET_DTYPES:
        raise TypeError("normalize: %s -> %s is not supported on the GPU path" % (a.dtype, dtype))
    with _Lease() as d:
        src, dst = d.upload(a), d.take(a.size * dtype.itemsize)
        check(_hip.lib().va_normalize(src.ptr, _DTYPE_CODES[a.dtype], dst.ptr, _DTYPE_CODES[dtype], a.size,
                                      float(fmin), float(fmax), float(alpha), float(tmin), None))
        return dst.download(a.shape, dtype)


def gaussian_noise(shape, dtype=np.float64, mean=0.0, std=1.0, seed=0, first_index=0):
    """`mean + std*randn(*shape)` produced on the GPU (VideoGaussianNoise, video/io/computed.py:36-41):
    sample i of the seeded stream is a function of (seed, first_index + i) only"""
    dtype = np.dtype(dtype)
    if dtype not in _TARGET_DTYPES:
        raise TypeError("gaussian_noise: dtype %s is not supported on the GPU path" % dtype)
    count = int(np.prod(shape))
    with _Lease() as d:
        dst = d.take(max(count, 1) * dtype.itemsize)
        check(_hip.lib().va_gaussian_noise(dst.ptr, _DTYPE_CODES[dtype], count, float(mean), float(std),
                                           int(seed) & (2 ** 64 - 1), int(first_index), None))
        return dst.download(tuple(shape), dtype)


def morph(frames, op, shape="rect", ksize=3, implementation=None):
    """cv2.erode / cv2.dilate (video/analysis/image.py:248-251) on (H,W) or (N,H,W) uint8.
    implementation='bits' runs the bit-packed kernel of the pipeline (binary masks only)."""
    arr, n, fshape, _ = _as_batch(np.asarray(frames, np.uint8), 2)
    h, w = fshape
    L = _hip.lib()
    fn = L.va_morph_bits_u8 if implementation == "bits" else L.va_morph_u8
    return _pointwise_u8(fn, arr, arr.shape, n, h, w, _hip.MORPH_OPS.get(op, op),
                         _hip.SHAPES.get(shape, shape), int(ksize), None)


def _label(d, arr, n, h, w, connectivity):
    """label the (n, h, w) uint8 masks `arr` in buffers of the lease `d`; returns the (labels, counts) buffers"""
    L = _hip.lib()
    src, lab, cnt = d.upload(arr), d.take(arr.size * 4), d.take(max(n, 1) * 4)
    ws_bytes = L.va_label_workspace_bytes(n, h, w)
    ws = d.take(ws_bytes)
    check(L.va_label_i32(src.ptr, lab.ptr, cnt.ptr, n, h, w, int(connectivity), ws.ptr, ws_bytes, None))
    return lab, cnt


def label(masks, connectivity=4):
    """ndimage.measurements.label (video/analysis/regions.py:162) for (H,W) or (N,H,W) masks.
    returns (labels int32, counts): counts is an int for a single mask, else an int32 array"""
    arr, n, fshape, single = _as_batch(_as_mask(masks, keep_uint8=True), 2)
    h, w = fshape
    with _Lease() as d:
        lab, cnt = _label(d, arr, n, h, w, connectivity)
        labels = lab.download(arr.shape, np.int32)
        counts = cnt.download((n,), np.int32)
    if single:
        return labels, int(counts[0])
    return labels, counts


def region_stats(labels, max_labels):
    """per-label area / raw moments / bbox: (N?, max_labels, 16) int64, see _hip.STAT_NAMES"""
    arr, n, fshape, single = _as_batch(np.asarray(labels, np.int32), 2)
    h, w = fshape
    max_labels = max(int(max_labels), 1)
    with _Lease() as d:
        src, st = d.upload(arr), d.take(n * max_labels * _hip.STATS_STRIDE * 8)
        check(_hip.lib().va_moments_i64(src.ptr, n, h, w, max_labels, st.ptr, None))
        out = st.download((n, max_labels, _hip.STATS_STRIDE), np.int64)
    return out[0] if single else out


def largest_region(mask, connectivity=4):
    """label + areas + first-max argmax + select, all on the GPU.
    returns (mask of the largest region as bool, its area, number of regions)"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be 2-d")
    m = _as_mask(m, keep_uint8=True)
    h, w = m.shape
    L = _hip.lib()
    with _Lease() as d:
        lab, cnt = _label(d, m, 1, h, w, connectivity)
        count = int(cnt.download((1,), np.int32)[0])
        if count == 0:
            return np.zeros(m.shape, bool), 0, 0
        st, big, area, sel = d.take(count * _hip.STATS_STRIDE * 8), d.take(4), d.take(8), d.take(m.size)
        check(L.va_moments_i64(lab.ptr, 1, h, w, count, st.ptr, None))
        check(L.va_largest_region(lab.ptr, cnt.ptr, st.ptr, 1, h, w, count, big.ptr, area.ptr,
                                  sel.ptr, None))
        out = sel.download(m.shape, np.uint8).astype(bool)
        return out, int(area.download((1,), np.int64)[0]), count


DEFAULT_POINT_CAPACITY = 4096     # room for the points of a contour or a path when the caller names none


def _with_room(max_points, run):
    """run(capacity) launches with room for `capacity` points per item and returns (points buffer, counts found).
    An explicit max_points truncates; otherwise a count beyond DEFAULT_POINT_CAPACITY (rare: a very long contour or
    path) runs once more with room for the largest.  Returns (points buffer, counts kept, capacity)."""
    def once(cap):
        pts, counts = run(cap)
        return (pts, counts, cap), (counts.max(initial=0),)
    (pts, counts, cap), _ = once(int(max_points)) if max_points else _rerun(once, DEFAULT_POINT_CAPACITY)
    return pts, np.minimum(counts, cap), cap


def largest_contour(mask, max_points=None, moments=False):
    """outer contour (cv2 RETR_EXTERNAL / CHAIN_APPROX_SIMPLE) of the component with the largest
    contour area.  returns (points (N,2) int32, area float, number of components); with
    moments=True also the ten spatial cv2.moments(contour) values, computed from the points while
    they are still on the device"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be 2-d")
    m = _as_mask(m, keep_uint8=True)
    h, w = m.shape
    L = _hip.lib()
    with _Lease() as d:
        src = d.upload(m)
        ws_bytes = L.va_contour_workspace_bytes(1, h, w)
        ws = d.take(ws_bytes)
        npts, area, ncomp = d.take(4), d.take(8), d.take(4)

        def run(cap):
            pts = d.take(cap * 8)
            check(L.va_largest_contour(src.ptr, 1, h, w, pts.ptr, cap, npts.ptr, area.ptr, ncomp.ptr,
                                       ws.ptr, ws_bytes, None))
            return pts, npts.download((1,), np.int32)
        pts, n, cap = _with_room(max_points, run)
        count = int(ncomp.download((1,), np.int32)[0])
        points = pts.download((int(n[0]), 2), np.int32)
        res = (points, float(area.download((1,), np.float64)[0]), count)
        if moments:
            mom = d.take(10 * 8)
            check(L.va_contour_moments(pts.ptr, npts.ptr, 1, cap, 0, mom.ptr, None))
            res += (mom.download((10,), np.float64),)
        return res


DEFAULT_CONTOUR_CAPACITY = 4096          # contours / points of a find_contours batch the first launch has room for
DEFAULT_CONTOUR_POINT_CAPACITY = 1 << 17
# va_contour_info, include/videoanalysis_hip.h
CONTOUR_INFO_DTYPE = np.dtype([("frame", np.int32), ("npoints", np.int32), ("start", np.int32, 2),
                               ("rect", np.int32, 4), ("area", np.float64), ("perimeter", np.float64)])
CONTOUR_RECORD_DTYPE = np.dtype([("area", np.float64), ("perimeter", np.float64), ("rect", np.int32, 4)])


class DeviceContours(object):
    """one va_find_contours result that stays on the device: the records (`info`, CONTOUR_INFO_DTYPE), the offsets
    (`point_off`, ncontours + 1 int64) and the points (`points`, int32 (x, y)) in leased buffers, with what the host
    knows of them: the stack's n, h, w, the contours per frame (`counts`, int32) and the totals `ncontours` and
    `npoints`.  ops.draw_contours draws it; download() gives what find_contours returns for a stack; release()
    hands the buffers back to the pool (the caller has synchronised by then: find_contours and download() do)."""

    def __init__(self, info, point_off, points, n, h, w, counts, ncontours, npoints):
        self.info, self.point_off, self.points = info, point_off, points
        self.n, self.h, self.w = n, h, w
        self.counts, self.ncontours, self.npoints = counts, int(ncontours), int(npoints)

    def download(self, ret_info=False, moments=False, stream=None):
        """the per-frame lists of (N, 1, 2) int32 contours; ret_info and moments append what find_contours appends"""
        n, k, npts = self.n, self.ncontours, self.npoints
        extras = bool(ret_info) + bool(moments)
        if n == 0:
            return ([],) * (1 + extras) if extras else []
        offsets = self.point_off.download((k + 1,), np.int64, stream)
        points = self.points.download((npts, 2), np.int32, stream)
        first = np.concatenate([[0], np.cumsum(self.counts, dtype=np.int64)])
        res = ([[points[offsets[s]:offsets[s + 1]].reshape(-1, 1, 2) for s in range(first[f], first[f + 1])]
                for f in range(n)],)
        if ret_info:
            rec = self.info.download((k,), CONTOUR_INFO_DTYPE, stream)
            out = np.empty(k, CONTOUR_RECORD_DTYPE)
            for name in CONTOUR_RECORD_DTYPE.names:
                out[name] = rec[name]
            res += ([out[first[f]:first[f + 1]] for f in range(n)],)
        if moments:
            with _Lease.on(stream) as d:
                mom = d.take(max(k, 1) * 80)
                check(_hip.lib().va_contour_moments_ragged(self.points.ptr, self.point_off.ptr, k, 0, mom.ptr, stream))
                allm = mom.download((k, 10), np.float64, stream)
            res += ([allm[first[f]:first[f + 1]] for f in range(n)],)
        return res if len(res) > 1 else res[0]

    def release(self):
        bufs = (self.info, self.point_off, self.points)
        self.info = self.point_off = self.points = None
        _give(*bufs)


def find_contours(masks, ret_info=False, moments=False, stream=None, keep=False):
    """cv2.findContours(mask, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)[1] for one mask (h, w) or a stack
    (n, h, w), foreground = non-zero (video/analysis/regions.py:180-182, :229-231, :575-576;
    video/io/composer.py:228): the list of (N, 1, 2) int32 contours in OpenCV's order, one list per frame for a
    stack.  ret_info appends, per frame, a structured array (CONTOUR_RECORD_DTYPE) of cv2.contourArea,
    cv2.arcLength(c, True) and cv2.boundingRect (x, y, w, h) of its contours; moments appends the (k, 10) spatial
    cv2.moments(contour) values per frame, computed from the points on the device.  The first launch has room for
    DEFAULT_CONTOUR_CAPACITY contours and DEFAULT_CONTOUR_POINT_CAPACITY points in the batch; a batch that holds
    more runs exactly once more, with exact room.
    masks may be a monochrome DeviceFrames (a stack: it is not uploaded and stays the caller's).  keep=True returns a
    DeviceContours instead (ret_info and moments are then its download()'s): 16 bytes of totals and the counts per
    frame cross to the host, and no points."""
    if isinstance(masks, DeviceFrames):
        if masks.c != 1:
            raise ValueError("find_contours: masks on the device are a monochrome stack, got %d channels" % masks.c)
        arr, n, fshape, single = None, masks.n, (masks.h, masks.w), False
    else:
        arr, n, fshape, single = _as_batch(np.asarray(masks), 2)
    h, w = fshape
    if n == 0:
        found = DeviceContours(None, None, None, 0, h, w, np.zeros(0, np.int32), 0, 0)
    else:
        if h == 0 or w == 0:
            raise ValueError("find_contours: frames of shape %r have no pixels" % (tuple(fshape),))
        if arr is not None:
            arr = _as_mask(arr, keep_uint8=True)
        L = _hip.lib()
        with _Lease.on(stream) as d:
            ws_bytes = L.va_find_contours_workspace_bytes(n, h, w)
            src = masks.buf if arr is None else d.upload(arr)
            ws, ncb, tot = d.take(ws_bytes), d.take(n * 4), d.take(16)

            def run(capc, capp):
                d.recall()                  # the result's buffers outlive the lease; a first attempt's do not
                held = [d.result(nbytes) for nbytes in (max(capc, 1) * CONTOUR_INFO_DTYPE.itemsize, (capc + 1) * 8,
                                                        max(capp, 1) * 8)]
                check(L.va_find_contours(src.ptr, n, h, w, ncb.ptr, tot.ptr, held[0].ptr, held[1].ptr, capc,
                                         held[2].ptr, capp, ws.ptr, ws_bytes, stream))
                return held, tot.download((2,), np.int64, stream)
            held, (k, npts) = _rerun(run, DEFAULT_CONTOUR_CAPACITY, DEFAULT_CONTOUR_POINT_CAPACITY)
            found = DeviceContours(held[0], held[1], held[2], n, h, w, ncb.download((n,), np.int32, stream), k, npts)
    if keep:
        return found
    with _Lease.on(stream) as d:            # the result's buffers are this lease's: they go back behind the download
        d.extend((found.info, found.point_off, found.points))
        res = found.download(ret_info, moments, stream)
    if single:
        res = tuple(r[0] for r in res) if isinstance(res, tuple) else res[0]
    return res


# ------------------------------------------------------------------------ region links between consecutive frames
DEFAULT_LINK_CAPACITY = 1 << 16          # links of a region_links batch the first launch has room for
LINK_WORKSPACE_ROOM = 256 << 20          # ... and the workspace it may get beyond what that capacity needs
RegionLinks = collections.namedtuple("RegionLinks", "offsets a b count")


class DeviceLabels(object):
    """an int32 label stack (n, h, w) at the device address `ptr`, which stays its owner's (the engine's label
    buffer, a torch tensor's data_ptr()): what region_links takes in place of an array, and does not upload"""

    def __init__(self, ptr, n, h, w):
        self.ptr, self.n, self.h, self.w = int(ptr), int(n), int(h), int(w)


def region_links(labels, prev=None, stream=None, cap=None):
    """the overlap tables between consecutive label planes ("Region links"; va_region_links): pair t is
    (labels[t - 1], labels[t]), pair 0 is (prev, labels[0]) and has no links without prev.  A link is (a, b, count):
    count > 0 pixels hold the label a >= 1 in the earlier plane and b >= 1 in the later one (values <= 0 are
    background); the links of a pair come in the order of their first pixel.  Returns RegionLinks(offsets, a, b,
    count): pair t owns offsets[t] : offsets[t + 1] (int64, n + 1 entries) of the int32 arrays a, b and count.
    labels: an (n, h, w) array, or a DeviceLabels; prev: an (h, w) array, or the device address of such a plane.
    The first launch has room for `cap` links (DEFAULT_LINK_CAPACITY); a batch that may hold more runs exactly once
    more, with the room the first run asked for.  Only the tables cross to the host."""
    L = _hip.lib()
    if isinstance(labels, DeviceLabels):
        arr, n, h, w = None, labels.n, labels.h, labels.w
    else:
        arr = np.ascontiguousarray(np.asarray(labels), np.int32)
        if arr.ndim != 3:
            raise ValueError("region_links: labels are an (n, h, w) stack, got shape %r" % (arr.shape,))
        n, h, w = arr.shape
    prev_arr = None
    if prev is not None and not isinstance(prev, (int, np.integer)):
        prev_arr = np.ascontiguousarray(np.asarray(prev), np.int32)
        if prev_arr.shape != (h, w):
            raise ValueError("region_links: prev of shape %r does not match frames of %r" % (prev_arr.shape, (h, w)))
    if h <= 0 or w <= 0:
        raise ValueError("region_links: frames of shape %r have no pixels" % ((h, w),))
    cap = DEFAULT_LINK_CAPACITY if cap is None else int(cap)
    if cap < 0:
        raise ValueError("region_links: negative capacity %d" % cap)
    if n == 0:
        return RegionLinks(np.zeros(1, np.int64), *(np.zeros(0, np.int32) for _ in range(3)))
    with _Lease.on(stream) as d:
        src = labels.ptr if arr is None else d.upload(arr).ptr
        first = _ptr(d.upload(prev_arr)) if prev_arr is not None else (int(prev or 0) or None)
        nl, tot = d.take(n * 4), d.take(16)

        def run(room):
            # a launch whose capacity is short still counts the links; with room for the tables of a candidate every
            # fourth pixel (up to LINK_WORKSPACE_ROOM) it counts all pairs side by side on all but the busiest stacks
            ws_bytes = max(L.va_region_links_workspace_bytes(n, h, w, room),
                           min(L.va_region_links_workspace_bytes(n, h, w, n * h * w // 4), LINK_WORKSPACE_ROOM))
            ws, rec = d.take(ws_bytes), d.take(max(room, 1) * 16)
            check(L.va_region_links(first, src, n, h, w, nl.ptr, tot.ptr, rec.ptr, room, ws.ptr, ws_bytes, stream))
            total, need = tot.download((2,), np.int64, stream)
            return (rec, int(total)), (need,)
        (rec, total), _ = _rerun(run, cap)
        counts = nl.download((n,), np.int32, stream)
        table = rec.download((total, 4), np.int32, stream)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    return RegionLinks(offsets, *(np.ascontiguousarray(table[:, k]) for k in (1, 2, 3)))


# ------------------------------------------------------------------------ region intensity
INTENSITY_STRIDE = 8                     # int64 per (frame, label, channel) of an intensity table
INTENSITY_NAMES = ("sum", "sumsq", "sumx", "sumy", "min", "max", "count")        # its slots 0 .. 6; slot 7 is zero
_SLOT = {name: k for k, name in enumerate(INTENSITY_NAMES)}


class RegionIntensity(object):
    """an intensity table as DESIGN.md §9, "Region intensity", pins it, and its float64 completion on the host (NumPy
    on the small table; the device call that fills such a table is not part of the library yet, see there).
    raw: (..., labels, c, 8) int64 -- sum v, sum v^2, sum v x, sum v y, min, max, pixels, 0 -- label l at [l - 1];
    hist: (..., labels, c, 256) uint32 or None.  The leading axes are the call's (n,), or none for one frame
    (frame(t)).  An empty region gives NaN, or -1 where the result is an integer."""

    def __init__(self, raw, hist=None):
        self.raw, self.hist = raw, hist

    def frame(self, t, count=None):
        """frame t of a stack alone, cut to its first `count` labels"""
        cut = slice(None) if count is None else slice(0, max(int(count), 0))
        return RegionIntensity(self.raw[t][cut], None if self.hist is None else self.hist[t][cut])

    def _slot(self, k):
        return self.raw[..., k].astype(np.float64)

    @property
    def count(self):
        """(..., labels) int64: the pixels of each region"""
        return self.raw[..., 0, _SLOT["count"]]

    @property
    def mean(self):
        """(..., labels, c): S0 / N"""
        n = self._slot(_SLOT["count"])
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, self._slot(_SLOT["sum"]) / n, np.nan)

    @property
    def var(self):
        """(..., labels, c): the population variance S1 / N - mean^2, clipped at 0"""
        n, mean = self._slot(_SLOT["count"]), self.mean
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, np.maximum(self._slot(_SLOT["sumsq"]) / n - mean * mean, 0.0), np.nan)

    @property
    def std(self):
        return np.sqrt(self.var)

    @property
    def min(self):
        """(..., labels, c) int64, -1 for an empty region"""
        return np.where(self.raw[..., _SLOT["count"]] > 0, self.raw[..., _SLOT["min"]], -1)

    @property
    def max(self):
        return np.where(self.raw[..., _SLOT["count"]] > 0, self.raw[..., _SLOT["max"]], -1)

    @property
    def weighted_centroid(self):
        """(..., labels, c, 2): (S2 / S0, S3 / S0), the centroid (x, y) weighted by brightness; NaN where S0 = 0"""
        s0 = self._slot(_SLOT["sum"])
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((s0 > 0)[..., None],
                            np.stack([self._slot(_SLOT["sumx"]), self._slot(_SLOT["sumy"])], -1) / s0[..., None], np.nan)

    def percentile(self, q):
        """(..., labels, c) int64: the smallest v whose cumulative count is >= max(1, ceil(q / 100 N)) (nearest rank),
        -1 for an empty region; needs the histograms"""
        if self.hist is None:
            raise ValueError("percentile needs the histograms (this table was made without them)")
        q = float(q)
        if not 0.0 <= q <= 100.0:
            raise ValueError("percentile: q is 0 .. 100, got %r" % (q,))
        n = self.raw[..., _SLOT["count"]]
        rank = np.maximum(1, np.ceil(q / 100.0 * n.astype(np.float64))).astype(np.int64)
        below = (np.cumsum(self.hist, axis=-1, dtype=np.int64) < rank[..., None]).sum(-1)
        return np.where(n > 0, below, -1).astype(np.int64)

    @property
    def median(self):
        return self.percentile(50)


# ------------------------------------------------------------------------ geodesic distance maps
_I32_MAX = 2 ** 31 - 1


def _point_table(per_frame, n):
    """(n, m, 2) int32 table + (n,) counts from one list of (x, y) points per frame; coordinates
    beyond int32 become -1 (outside every frame, as they are)"""
    lists = [[] if p is None else [tuple(q) for q in p] for p in per_frame]
    if len(lists) != n:
        raise ValueError("need one point list per frame (%d frames, %d lists)" % (n, len(lists)))
    m = max([1] + [len(l) for l in lists])
    tab = np.full((n, m, 2), -1, np.int32)
    cnt = np.zeros(n, np.int32)
    for f, l in enumerate(lists):
        for i, q in enumerate(l):
            for k in (0, 1):
                v = int(q[k])
                tab[f, i, k] = v if -1 <= v <= _I32_MAX else -1
        cnt[f] = len(l)
    return tab, cnt


def distance_map(fillable, start_points, end_points=None):
    """geodesic distance maps (8-neighbours, straight 1, diagonal sqrt2) -- make_distance_map,
    video/analysis/regions.py:455-509.  fillable: (h, w) or (N, h, w), non-zero where the map may be
    filled; start_points: (x, y) points, one list per frame when batched; end_points likewise or
    None.  Returns int32 maps: 0 not fillable, 1 not reached, 2 + floor(distance) filled."""
    arr, n, fshape, single = _as_batch(np.asarray(fillable), 2)
    arr = _as_mask(arr)
    h, w = fshape
    if single:
        start_points = [start_points]
        end_points = None if end_points is None else [end_points]
    st, nst = _point_table(start_points, n)
    L = _hip.lib()
    ws_bytes = L.va_geodesic_workspace_bytes(n, h, w)
    with _Lease() as d:
        src, sb, nsb, out, ws = d.upload(arr), d.upload(st), d.upload(nst), d.take(arr.size * 4), d.take(ws_bytes)
        et, net = (None, None) if end_points is None else _point_table(end_points, n)
        eb, neb = d.upload(et), d.upload(net)
        check(L.va_distance_map_i32(src.ptr, n, h, w, sb.ptr, nsb.ptr, st.shape[1], _ptr(eb), _ptr(neb),
                                    0 if et is None else et.shape[1], out.ptr, ws.ptr, ws_bytes, None))
        return out.download(arr.shape, np.int32)


def _download_paths(pts, npath, cap, n):
    allp = pts.download((n, cap, 2), np.int32)
    return [allp[f, :npath[f]].astype(np.int64) for f in range(n)]


def distance_map_path(dmap, end_point, max_points=None):
    """the reference's walk from `end_point` down a distance map to its minimum --
    shortest_path_in_distance_map, video/analysis/regions.py:513-565.  dmap: (h, w) or (N, h, w)
    integers below 2^31; end_point: (x, y), or (N, 2) when batched.  Returns the (K, 2) int64 path of
    (x, y) points (a list of them when batched); K = 0 where the end point lies outside the map or
    its value is <= 1."""
    a = np.asarray(dmap)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError("distance maps are integer arrays")
    if a.size and a.max() > _I32_MAX:
        raise ValueError("distance map values must stay below 2^31")
    arr, n, fshape, single = _as_batch(a, 2)
    arr = np.ascontiguousarray(np.maximum(arr, 0), np.int32)
    h, w = fshape
    ends, _ = _point_table([[end_point]] if single else [[e] for e in end_point], n)
    L = _hip.lib()
    ws_bytes = L.va_geodesic_workspace_bytes(n, h, w)
    with _Lease() as d:
        src, eb, npb, ws = d.upload(arr), d.upload(ends[:, 0].copy()), d.take(n * 4), d.take(ws_bytes)

        def run(cap):
            pts = d.take(n * cap * 8)
            check(L.va_distance_map_path(src.ptr, n, h, w, eb.ptr, pts.ptr, cap, npb.ptr, ws.ptr, ws_bytes, None))
            return pts, npb.download((n,), np.int32)
        paths = _download_paths(*_with_room(max_points, run), n=n)
        return paths[0] if single else paths


def farthest_points(masks, p1=None, ret_path=False, max_points=None, ret_stats=False):
    """get_farthest_points, video/analysis/regions.py:568-611, for one mask (h, w) or a batch
    (N, h, w), foreground = non-zero.  p1: (x, y), or (N, 2) when batched; None: the first point of
    the longest external contour.  The whole iteration runs on the GPU.  Returns (p1, p2) as (N, 2)
    int64 arrays ((2,) for one mask), (-1, -1) for a frame without a component when p1 is None (a
    given p1 is only a start: one outside the frame or off the mask is ignored by the first map, and
    comes back as given when the loop ends there, an empty mask); with
    ret_path the (K, 2) int64 paths from p2 instead (a list when batched).  ret_stats appends
    (distance value at p2 (N,), [maps built, sweeps] (N, 2)) as int32 arrays."""
    arr, n, fshape, single = _as_batch(np.asarray(masks), 2)
    arr = _as_mask(arr)
    h, w = fshape
    L = _hip.lib()
    ws_bytes = L.va_geodesic_workspace_bytes(n, h, w)
    with _Lease() as d:
        src, p1o, p2o, dist, rounds, npb, ws = (d.upload(arr), d.take(n * 8), d.take(n * 8), d.take(n * 4),
                                                d.take(n * 8), d.take(n * 4), d.take(ws_bytes))
        p1b = None
        if p1 is not None:
            given = [p1] if single else list(p1)
            tab, _ = _point_table([[q] for q in given], n)
            p1b = d.upload(tab[:, 0].copy())

        def run(cap):                 # without ret_path there is no list to outgrow the capacity: no counts are read
            pts = d.take(n * cap * 8) if ret_path else None
            check(L.va_farthest_points(src.ptr, n, h, w, _ptr(p1b), p1o.ptr, p2o.ptr, dist.ptr, rounds.ptr, _ptr(pts),
                                       cap, npb.ptr, ws.ptr, ws_bytes, None))
            return pts, npb.download((n,), np.int32) if ret_path else np.zeros(0, np.int32)
        pts, npath, cap = _with_room(max_points, run)
        if ret_path:
            res = _download_paths(pts, npath, cap, n)
            res = (res[0] if single else res,)
        else:
            a, b = p1o.download((n, 2), np.int32).astype(np.int64), p2o.download((n, 2), np.int32).astype(np.int64)
            if p1 is not None:        # a start never replaced is returned as given, not as the kernel read it
                kept = rounds.download((n, 2), np.int32)[:, 0] == 1
                for f in np.nonzero(kept)[0]:
                    q = [int(v) for v in given[f]]
                    if all(-2 ** 63 <= v < 2 ** 63 for v in q):
                        a[f] = q
            res = (a[0], b[0]) if single else (a, b)
        if ret_stats:
            dv, rv = dist.download((n,), np.int32), rounds.download((n, 2), np.int32)
            res += (dv[0], rv[0]) if single else (dv, rv)
        return res if len(res) > 1 else res[0]


def contour_moments(contour):
    """the ten spatial moments of cv2.moments(contour) as a float64 array (m00 m10 m01 m20 m11 m02
    m30 m21 m12 m03) -- regionprops(contour=...), video/analysis/image.py:355; Polygon.moments,
    video/analysis/shapes.py:533.  Integer arrays are int32 points, everything else float32
    points (the two forms cv2.moments accepts; other dtypes it would read as an image)."""
    c = np.asarray(contour)
    if c.size == 0 or c.size % 2:
        raise ValueError("contour must hold (x, y) points")
    is_float = 0 if np.issubdtype(c.dtype, np.integer) else 1
    c = np.ascontiguousarray(c.reshape(-1, 2), np.float32 if is_float else np.int32)
    with _Lease() as d:
        pts, out = d.upload(c), d.take(10 * 8)
        check(_hip.lib().va_contour_moments(pts.ptr, None, 1, len(c), is_float, out.ptr, None))
        return out.download((10,), np.float64)


def detect_peaks(img, include_plateaus=True):
    """boolean mask of the local maxima (video/analysis/image.py:267-306), uint8 or float32 images"""
    a = np.ascontiguousarray(img)
    if a.dtype not in (np.uint8, np.float32) or a.ndim != 2:
        raise TypeError("detect_peaks expects a 2-d uint8 or float32 image on the GPU path")
    fn = _hip.lib().va_detect_peaks_u8 if a.dtype == np.uint8 else _hip.lib().va_detect_peaks_f32
    return _pointwise_u8(fn, a, a.shape, 1, a.shape[0], a.shape[1], 1 if include_plateaus else 0, None).astype(bool)


def mask_thinning(img):
    """skeleton by iterated 3x3-cross erosion/dilation (python method of mask_thinning,
    video/analysis/image.py:243-258); returns (skeleton uint8, iterations)"""
    a = np.ascontiguousarray(img, np.uint8)
    if a.ndim != 2:
        raise ValueError("mask must be 2-d")
    h, w = a.shape
    it = C.c_int()
    with _Lease() as d:
        cur, tmp, skel = d.upload(a), d.take(a.size), d.take(a.size)
        check(_hip.lib().va_mask_thinning_u8(cur.ptr, tmp.ptr, skel.ptr, h, w, C.byref(it), None))
        return skel.download(a.shape, np.uint8), it.value


def image_statistics(img, kernel="box", ksize=5, prior=0.0, exclude_center=False, ret_var=True):
    """local mean (and variance) in a window around every pixel
    (get_image_statistics, video/analysis/image.py:131-201), uint8 or float32 images (float values are
    truncated to integers first, as the reference's `img.astype(np.int)` does)"""
    a = np.ascontiguousarray(img)
    if a.dtype not in (np.uint8, np.float32) or a.ndim != 2:
        raise TypeError("image_statistics expects a 2-d uint8 or float32 image on the GPU path")
    h, w = a.shape
    fn = _hip.lib().va_image_statistics_u8 if a.dtype == np.uint8 else _hip.lib().va_image_statistics_f32
    with _Lease() as d:
        src, dm, dv = d.upload(a), d.take(a.size * 8), (d.take(a.size * 8) if ret_var else None)
        check(fn(src.ptr, dm.ptr, _ptr(dv), 1, h, w, {"box": 0, "ellipse": 1, "circle": 1}[kernel], int(ksize),
                 float(prior), 1 if exclude_center else 0, None))
        mean = dm.download(a.shape, np.float64)
        return (mean, dv.download(a.shape, np.float64)) if ret_var else mean


# ------------------------------------------------------------------------ dense optical flow
OPTFLOW_WORKSPACE_BUDGET = 2 << 30      # device workspace of one call; longer stacks go in overlapping chunks


def optical_flow_farneback(frames, pyr_scale=0.5, levels=3, winsize=2, iterations=3, poly_n=5, poly_sigma=1.2,
                           flags=0, ret_flow=False):
    """cv2.calcOpticalFlowFarneback(frames[k], frames[k + 1], None, ...) for every consecutive pair of an
    (n, h, w) stack (n >= 2), and the magnitude of cv2.cartToPolar -- FilterOpticalFlow,
    video/filters.py:572-589.  uint8 and float32 frames go to the GPU as they are; other real dtypes are
    converted with astype(float32), as convertTo does.  Returns the magnitudes, (n - 1, h, w) float32, or
    (flow (n - 1, h, w, 2), magnitudes) with ret_flow=True.  Stacks whose workspace would exceed
    OPTFLOW_WORKSPACE_BUDGET run in chunks that share one frame; the result does not depend on it."""
    arr = np.asarray(frames)
    if arr.ndim != 3:
        raise ValueError("expected an (n, h, w) stack of single-channel frames, got shape %r" % (arr.shape,))
    if arr.dtype not in (np.uint8, np.float32):
        if arr.dtype.kind not in "biuf":
            raise TypeError("optical flow: frames of dtype %s are not supported" % arr.dtype)
        arr = arr.astype(np.float32)
    arr, dtype = np.ascontiguousarray(arr), _DTYPE_CODES[arr.dtype]
    n, h, w = arr.shape
    args = (float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n))
    L = _hip.lib()
    ws_of = lambda k: L.va_farneback_workspace_bytes(k, h, w, *args)
    if n < 2 or ws_of(2) == 0 or int(flags) != 0:       # let the library name the bad argument
        check(L.va_optical_flow_farneback(None, dtype, n, h, w, *args, float(poly_sigma), int(flags), None, None,
                                          None, 0, None))
    per_pair = ws_of(3) - ws_of(2)
    pairs = max(1, min(n - 1, (OPTFLOW_WORKSPACE_BUDGET - ws_of(2)) // per_pair + 1))
    mag = np.empty((n - 1, h, w), np.float32)
    flow = np.empty((n - 1, h, w, 2), np.float32) if ret_flow else None
    for a in range(0, n - 1, pairs):
        k = min(pairs, n - 1 - a)
        ws_bytes = ws_of(k + 1)
        with _Lease() as d:
            src, mb, fb, ws = (d.upload(arr[a:a + k + 1]), d.take(k * h * w * 4),
                               d.take(k * h * w * 8) if ret_flow else None, d.take(ws_bytes))
            check(L.va_optical_flow_farneback(src.ptr, dtype, k + 1, h, w, *args, float(poly_sigma), 0, _ptr(fb),
                                              mb.ptr, ws.ptr, ws_bytes, None))
            mag[a:a + k] = mb.download((k, h, w), np.float32)
            if ret_flow:
                flow[a:a + k] = fb.download((k, h, w, 2), np.float32)
    return (flow, mag) if ret_flow else mag


# ------------------------------------------------------------------------------- active contours
SNAKE_MAX_POINTS = 1024          # kSnakeMaxN: the longest contour va_active_contour takes


def _potential_stack(frames):
    """(contiguous (n, h, w) uint8 / float32 array, VA dtype) for the Sobel pass"""
    arr = np.asarray(frames)
    if arr.dtype not in (np.uint8, np.float32):
        raise TypeError("active contour potentials must be uint8 or float32, got %s" % arr.dtype)
    if arr.ndim == 2:
        arr = arr[None]
    if arr.ndim != 3:
        raise ValueError("expected an (h, w) potential or an (n, h, w) stack, got shape %r" % (arr.shape,))
    return np.ascontiguousarray(arr), _DTYPE_CODES[arr.dtype]


def potential_gradients(frames, sigma=0.0, stream=None):
    """ActiveContour.set_potential's dense part on the device (video/analysis/active_contour.py:104-110):
    cv2.GaussianBlur(p, (0, 0), sigma) when sigma > 0 (va_gaussian_u8 / va_gaussian_f32, the taps FilterBlur
    uses), then cv2.Sobel(p, CV_64F, 1, 0, ksize=5) and (0, 1).  frames: (h, w) or (n, h, w), uint8 or float32.
    Returns (fx, fy, (n, h, w)) with fx and fy float64 DeviceBuffers that the caller owns."""
    arr, dtype = _potential_stack(frames)
    n, h, w = arr.shape
    L = _hip.lib()
    with _Lease.on(stream) as d:
        # fx and fy are the caller's to free, not pooled: a call that fails frees them, the caller never sees them
        fx, fy = (d.adopt(DeviceBuffer(arr.nbytes * (8 // arr.itemsize)), DeviceBuffer.free) for _ in range(2))
        src, blur = d.upload(arr), None
        if sigma > 0 and n:
            blur = d.take(arr.nbytes)
            fn = L.va_gaussian_u8 if dtype == _hip.VA_U8 else L.va_gaussian_f32
            check(fn(src.ptr, blur.ptr, n, h, w, 1, float(sigma), stream))
        check(L.va_sobel5_f64((blur or src).ptr, dtype, fx.ptr, fy.ptr, n, h, w, stream))
        check(L.va_stream_sync(stream))
    return fx, fy, (n, h, w)


def sobel5_f64(frames, dx=True, dy=True):
    """cv2.Sobel(frame, cv2.CV_64F, 1, 0, ksize=5) and cv2.Sobel(frame, cv2.CV_64F, 0, 1, ksize=5) of uint8 or
    float32 frames, (h, w) or (n, h, w); returns (fx, fy), float64 arrays of the input's shape (None for a
    plane not asked for)"""
    frames = np.asarray(frames)
    arr, dtype = _potential_stack(frames)
    n, h, w = arr.shape
    L = _hip.lib()
    with _Lease() as d:
        src, bx, by = d.upload(arr), (d.take(arr.size * 8) if dx else None), (d.take(arr.size * 8) if dy else None)
        check(L.va_sobel5_f64(src.ptr, dtype, _ptr(bx), _ptr(by), n, h, w, None))
        return tuple(b.download(arr.shape, np.float64).reshape(frames.shape) if b else None for b in (bx, by))


def active_contour(fx, fy, shape, points, npoints, frames, mats, mat_offsets, anchor_flags, anchor_vals, gamma,
                   tol_gamma, max_iterations, stream=None):
    """every iteration of m snakes in one launch (ActiveContour.find_contour's loop, active_contour.py:160-191).
    fx, fy: float64 DeviceBuffers of `shape` = (n, h, w) (potential_gradients).  points: (m, max_points, 2)
    float64 equidistant curves, npoints (m,) their lengths, frames (m,) their frames; mats: the flat float64
    table of TRANSPOSED inverse evolution matrices, mat_offsets (m,) the element offset of each contour's;
    anchor_flags (m, max_points) uint8 (bit 0: x fixed, bit 1: y fixed) or None, anchor_vals (m, max_points, 2).
    Returns (points, iterations, total_variation).  Every upload waits for `stream`'s earlier work
    (va_memcpy_h2d), so back-to-back calls on one stream cannot overwrite inputs still in use."""
    n, h, w = shape
    pts = np.ascontiguousarray(points, np.float64)
    m, max_points = pts.shape[:2]
    L = _hip.lib()
    mats = np.ascontiguousarray(mats, np.float64)
    anchored = anchor_flags is not None
    with _Lease.on(stream) as d:
        pb, nb, fb, mb, ob, ab, vb = (
            d.upload(pts), d.upload(np.ascontiguousarray(npoints, np.int32)),
            d.upload(np.ascontiguousarray(frames, np.int32)), d.upload(mats),
            d.upload(np.ascontiguousarray(mat_offsets, np.int64)),
            d.upload(np.ascontiguousarray(anchor_flags, np.uint8) if anchored else None),
            d.upload(np.ascontiguousarray(anchor_vals, np.float64) if anchored else None))
        it_buf, tv_buf = d.take(max(m, 1) * 4), d.take(max(m, 1) * 8)
        check(L.va_active_contour(fx.ptr, fy.ptr, n, h, w, m, max_points, nb.ptr, fb.ptr, mb.ptr, ob.ptr, mats.size,
                                  _ptr(ab), _ptr(vb), float(gamma), float(tol_gamma), int(max_iterations), pb.ptr,
                                  it_buf.ptr, tv_buf.ptr, stream))
        return (pb.download(pts.shape, np.float64, stream), it_buf.download((m,), np.int32, stream),
                tv_buf.download((m,), np.float64, stream))


# ------------------------------------------------------------------------------------------ polygons
FILL_MAX_VERTS = 1024            # VA_FILL_MAX_VERTS .. VA_DT_MAX_HEIGHT, include/videoanalysis_hip.h
FILL_MAX_SIDE = 16384
FILL_MAX_COORD = 1 << 20
DT_MAX_WIDTH = 4096
DT_MAX_HEIGHT = 16384


def _pack_ragged(items):
    """one flat buffer for m items of different sizes.  items: 2-d arrays, or their (h, w) shapes alone for
    a call that has no input pixels.  Returns (flat, shapes int32 (m, 2), offsets int64 (m,), sizes int64 (m,),
    total): item i is sizes[i] elements at offsets[i] of `total`; flat is the concatenated pixels (one placeholder
    byte when there are none at all), None for shapes"""
    m = len(items)
    arrays = np.ndim(items[0]) == 2
    shapes = np.array([a.shape for a in items] if arrays else items, np.int32).reshape(m, 2)
    sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
    offsets = np.zeros(m, np.int64)
    offsets[1:] = np.cumsum(sizes)[:-1]
    total = int(sizes.sum())
    flat = None
    if arrays:
        flat = np.concatenate([a.reshape(-1) for a in items]) if total else np.zeros(1, np.uint8)
    return flat, shapes, offsets, sizes, total


def _split_ragged(flat, shapes, offsets, sizes):
    """the per-item (h, w) arrays of a flat result laid out by _pack_ragged"""
    return [flat[o:o + s].reshape(hw) for o, s, hw in zip(offsets.tolist(), sizes.tolist(), shapes.tolist())]


def _check_status(status, what):
    bad = np.flatnonzero(status != 0)
    if len(bad):
        raise ValueError("%s: item %d is beyond the kernel's limits (status %d)" % (what, bad[0], status[bad[0]]))


def _fill_tables(contours, boxes, what):
    """the checked operands of va_fill_poly for m > 0 polygons: (verts int32 (k, 2), vert_off int64 (m + 1,), boxes
    int64 (m, 4)); raises as fill_polys documents"""
    m = len(contours)
    bx = np.asarray(boxes, np.int64).reshape(-1, 4)
    if len(bx) != m:
        raise ValueError("%s: need one box per contour (%d contours, %d boxes)" % (what, m, len(bx)))
    polys = []
    for k, c in enumerate(contours):
        c = np.asarray(c)
        if not np.issubdtype(c.dtype, np.integer):
            raise TypeError("%s: contour %d must hold integer vertices, got %s" % (what, k, c.dtype))
        c = c.reshape(-1, 2).astype(np.int64)
        if not 1 <= len(c) <= FILL_MAX_VERTS:
            raise ValueError("%s: contour %d has %d vertices (1 .. %d are supported)"
                             % (what, k, len(c), FILL_MAX_VERTS))
        if np.any(np.abs(c - bx[k, :2]) > FILL_MAX_COORD) or np.any(np.abs(c) >= 2 ** 31):
            raise ValueError("%s: contour %d has a vertex more than %d px from its box" % (what, k, FILL_MAX_COORD))
        polys.append(c)
    if np.any(bx[:, 2:] < 0):
        raise ValueError("negative dimensions are not allowed")
    if np.any(bx[:, 2:] > FILL_MAX_SIDE) or np.any(np.abs(bx[:, :2]) >= 2 ** 31):
        raise ValueError("%s: boxes are limited to %d x %d px with int32 origins"
                         % (what, FILL_MAX_SIDE, FILL_MAX_SIDE))
    verts = np.ascontiguousarray(np.concatenate(polys), np.int32)
    vert_off = np.zeros(m + 1, np.int64)
    vert_off[1:] = np.cumsum([len(c) for c in polys])
    return verts, vert_off, bx


def fill_polys(contours, boxes, dtype=np.uint8, stream=None):
    """cv2.fillPoly(np.zeros((h, w), dtype), [contour], color=1, offset=(-x, -y)) for every polygon of a list, in
    one launch (Polygon.get_mask, video/analysis/shapes.py:586-592; lineType LINE_8, shift 0).  contours: (k, 2)
    integer (x, y) vertices per polygon; boxes: one (x, y, w, h) per polygon, the box's origin in vertex
    coordinates and its size; dtype uint8 or int32.  Returns the list of (h, w) masks (0 / 1)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.uint8, np.int32):
        raise TypeError("fill_polys: masks are uint8 or int32, got %s" % dtype)
    m = len(contours)
    if m == 0:
        return []
    verts, vert_off, bx = _fill_tables(contours, boxes, "fill_polys")
    _, shapes, out_off, sizes, total = _pack_ragged(bx[:, [3, 2]])
    with _Lease.on(stream) as d:
        vb, ob, bb, oob, out, st = (d.upload(verts), d.upload(vert_off), d.upload(bx.astype(np.int32)),
                                    d.upload(out_off), d.take(max(total, 1) * dtype.itemsize), d.take(m * 4))
        check(_hip.lib().va_fill_poly(vb.ptr, ob.ptr, len(verts), bb.ptr, oob.ptr, total, m, dtype.itemsize, out.ptr,
                                      st.ptr, stream))
        _check_status(st.download((m,), np.int32, stream), "fill_polys")
        flat = out.download((total,), dtype, stream)
    return _split_ragged(flat, shapes, out_off, sizes)


def distance_transform(masks, stream=None):
    """cv2.distanceTransform(mask, cv2.DIST_L2, 5) (float32) of every mask of a list, in one launch
    (Polygon.get_centerline_optimized, video/analysis/shapes.py:742).  masks: 2-d arrays, non-zero = foreground,
    at most DT_MAX_WIDTH columns and DT_MAX_HEIGHT rows.  Returns the list of float32 distance maps."""
    arrs = []
    for k, a in enumerate(masks):
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("distance_transform: mask %d is not 2-d (shape %r)" % (k, a.shape))
        if a.shape[1] > DT_MAX_WIDTH or a.shape[0] > DT_MAX_HEIGHT:
            raise ValueError("distance_transform: mask %d of shape %r exceeds %d rows x %d columns"
                             % (k, a.shape, DT_MAX_HEIGHT, DT_MAX_WIDTH))
        arrs.append(a)
    m = len(arrs)
    if m == 0:
        return []
    flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
    with _Lease.on(stream) as d:
        src, sb, ob, out, st = (d.upload(_as_mask(flat)), d.upload(shapes), d.upload(offsets), d.take(max(total, 1) * 4),
                                d.take(m * 4))
        check(_hip.lib().va_distance_transform_l2_5(src.ptr, sb.ptr, ob.ptr, total, m, int(shapes[:, 1].max()),
                                                    out.ptr, st.ptr, stream))
        _check_status(st.download((m,), np.int32, stream), "distance_transform")
        res = out.download((max(total, 1),), np.float32, stream)
    return _split_ragged(res, shapes, offsets, sizes)


# ------------------------------------------------------------------------------- batched centre lines
GRAD_RESIDENT_MAX_PIXELS = 8192  # VA_GRAD_RESIDENT_MAX_PIXELS: h * w of an item the resident blur + Sobel kernel takes
GRAD_CLASSES = (2048, 4096, GRAD_RESIDENT_MAX_PIXELS)   # one launch per class: 16, 32 and 64 KiB of LDS a workgroup


def _plan_ragged_gradients(d, shapes, offsets, sizes, resident):
    """uploads the tables of the resident launches, one per size class of `resident` (the LDS of a launch is that
    of its largest item, so one large item must not cost the small ones their occupancy): the items' shapes and
    offsets in class order.  Returns (shapes buffer, offsets buffer, [(first entry, entries, largest item)])."""
    classes = {}
    for k in resident:
        classes.setdefault(next(c for c in GRAD_CLASSES if sizes[k] <= c), []).append(k)
    order = [k for cap in sorted(classes) for k in classes[cap]]
    launches, first = [], 0
    for cap in sorted(classes):
        idx = classes[cap]
        launches.append((first, len(idx), int(sizes[idx].max())))
        first += len(idx)
    if not order:
        return None, None, launches
    return d.upload(np.ascontiguousarray(shapes[order])), d.upload(np.ascontiguousarray(offsets[order])), launches


def _enqueue_ragged_gradients(d, plan, src, code, shapes, offsets, sizes, total, sigma, resident, fx, fy, st_ptr,
                              stream):
    """blur + Sobel of the items of the ragged device buffer `src` (VA dtype `code`) into the float64 planes fx, fy;
    everything is enqueued on `stream` and nothing is copied: the items of `resident` through
    va_potential_gradients_ragged as `plan` (_plan_ragged_gradients) groups them, every other item on its own
    through va_gaussian_* + va_sobel5_f64 at its offset of the same planes.  st_ptr: device address of an int32
    status vector with room for len(resident) entries, written in the plan's order."""
    L = _hip.lib()
    itemsize = 1 if code == _hip.VA_U8 else 4
    sb, ob, launches = plan
    for first, count, max_pixels in launches:
        check(L.va_potential_gradients_ragged(src.ptr, code, sb.ptr + 8 * first, ob.ptr + 8 * first, total, count,
                                              max_pixels, float(sigma), fx.ptr, fy.ptr, st_ptr + 4 * first, stream))
    blur = None
    for k in sorted(set(range(len(sizes))) - set(resident)):
        (h, w), o = (int(v) for v in shapes[k]), int(offsets[k])
        if h * w == 0:
            continue
        item = src.ptr + o * itemsize
        if sigma > 0:
            blur = blur or d.take(int(sizes.max()) * itemsize)
            fn = L.va_gaussian_u8 if code == _hip.VA_U8 else L.va_gaussian_f32
            check(fn(item, blur.ptr, 1, h, w, 1, float(sigma), stream))
            item = blur.ptr
        check(L.va_sobel5_f64(item, code, fx.ptr + 8 * o, fy.ptr + 8 * o, 1, h, w, stream))


def _grad_resident_items(sizes, code, sigma, implementation, what):
    """indices of the items the resident kernel takes; implementation='resident' raises for the others"""
    if implementation not in (None, "resident"):
        raise ValueError("%s: unknown implementation %r" % (what, implementation))
    if code == _hip.VA_U8 and sigma > 0:
        ok = np.zeros(len(sizes), bool)
    else:
        ok = sizes <= GRAD_RESIDENT_MAX_PIXELS
    if implementation == "resident" and not ok.all():
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError("%s: the resident kernel does not take item %d (%d pixels; at most %d, and uint8 items "
                         "only without a blur)" % (what, k, sizes[k], GRAD_RESIDENT_MAX_PIXELS))
    return [int(k) for k in np.flatnonzero(ok)]


def potential_gradients_ragged(potentials, sigma=0.0, implementation=None, stream=None):
    """potential_gradients for a list of 2-d potentials of different shapes, all float32 or all uint8: each item is
    blurred (sigma > 0) and differentiated as an image of its own, with BORDER_REFLECT_101 at its own edges, so
    every item gets the bits potential_gradients gives it alone.  Items of up to GRAD_RESIDENT_MAX_PIXELS pixels
    run in va_potential_gradients_ragged (one workgroup per item, the item in LDS); larger ones, and uint8 items
    with sigma > 0 (a fixed-point blur), go one by one through va_gaussian_* + va_sobel5_f64.
    implementation='resident' forces the kernel and raises ValueError for an item it cannot take.
    Returns (fx, fy, shapes int32 (m, 2), offsets int64 (m,)): fx and fy are float64 DeviceBuffers that the caller
    owns, item i's planes are shapes[i] at element offset offsets[i]."""
    arrs = [np.asarray(a) for a in potentials]
    for k, a in enumerate(arrs):
        if a.dtype not in (np.uint8, np.float32):
            raise TypeError("potential_gradients_ragged: potentials must be uint8 or float32, item %d is %s"
                            % (k, a.dtype))
        if a.dtype != arrs[0].dtype:
            raise TypeError("potential_gradients_ragged: one dtype per call (item 0 is %s, item %d is %s)"
                            % (arrs[0].dtype, k, a.dtype))
        if a.ndim != 2:
            raise ValueError("potential_gradients_ragged: item %d is not 2-d (shape %r)" % (k, a.shape))
    if not sigma >= 0:
        raise ValueError("potential_gradients_ragged: sigma must be >= 0, got %r" % (sigma,))
    m = len(arrs)
    if m == 0:
        _hip.lib()
        return DeviceBuffer(0), DeviceBuffer(0), np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
    flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
    code = _DTYPE_CODES[arrs[0].dtype]
    resident = _grad_resident_items(sizes, code, sigma, implementation, "potential_gradients_ragged")
    L = _hip.lib()
    with _Lease.on(stream) as d:
        fx, fy = (d.adopt(DeviceBuffer(total * 8), DeviceBuffer.free) for _ in range(2))
        src, st = d.upload(flat), d.take(m * 4)
        plan = _plan_ragged_gradients(d, shapes, offsets, sizes, resident)
        _enqueue_ragged_gradients(d, plan, src, code, shapes, offsets, sizes, total, sigma, resident, fx, fy,
                                  st.ptr, stream)
        if resident:
            _check_status(st.download((len(resident),), np.int32, stream), "potential_gradients_ragged")
        else:
            check(L.va_stream_sync(stream))
    return fx, fy, shapes, offsets


def active_contour_ragged(fx, fy, shapes, offsets, points, npoints, items, mats, mat_offsets, anchor_flags, anchor_vals,
                          gamma, tol_gamma, max_iterations, stream=None):
    """active_contour on the ragged planes of potential_gradients_ragged / centerline_gradients: fx, fy, shapes,
    offsets as they return them, items (m,) the item each contour runs on; everything else as active_contour takes
    and returns it.  A contour whose item is out of range comes back untouched with -1 iterations."""
    pts = np.ascontiguousarray(points, np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2:
        raise ValueError("active_contour_ragged: points must be (m, max_points, 2), got shape %r" % (pts.shape,))
    m, max_points = pts.shape[:2]
    shapes = np.ascontiguousarray(shapes, np.int32).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    npoints = np.ascontiguousarray(npoints, np.int32).reshape(-1)
    items = np.ascontiguousarray(items, np.int32).reshape(-1)
    mat_offsets = np.ascontiguousarray(mat_offsets, np.int64).reshape(-1)
    if len(shapes) != len(offsets):
        raise ValueError("active_contour_ragged: %d shapes and %d offsets" % (len(shapes), len(offsets)))
    if not len(npoints) == len(items) == len(mat_offsets) == m:
        raise ValueError("active_contour_ragged: npoints, items and mat_offsets need one entry per contour (%d)" % m)
    total = int((shapes[:, 0].astype(np.int64) * shapes[:, 1]).sum())
    L = _hip.lib()
    if m == 0:
        return pts.copy(), np.zeros(0, np.int32), np.zeros(0, np.float64)
    mats = np.ascontiguousarray(mats, np.float64)
    anchored = anchor_flags is not None
    with _Lease.on(stream) as d:
        pb, nb, fb, mb, ob, ab, vb, sb, gb = (
            d.upload(pts), d.upload(npoints), d.upload(items), d.upload(mats), d.upload(mat_offsets),
            d.upload(np.ascontiguousarray(anchor_flags, np.uint8) if anchored else None),
            d.upload(np.ascontiguousarray(anchor_vals, np.float64) if anchored else None),
            d.upload(shapes if len(shapes) else np.zeros((1, 2), np.int32)),
            d.upload(offsets if len(offsets) else np.zeros(1, np.int64)))
        it_buf, tv_buf = d.take(m * 4), d.take(m * 8)
        check(L.va_active_contour_ragged(fx.ptr, fy.ptr, sb.ptr, gb.ptr, total, len(shapes), m, max_points, nb.ptr,
                                         fb.ptr, mb.ptr, ob.ptr, mats.size, _ptr(ab), _ptr(vb), float(gamma),
                                         float(tol_gamma), int(max_iterations), pb.ptr, it_buf.ptr, tv_buf.ptr, stream))
        return (pb.download(pts.shape, np.float64, stream), it_buf.download((m,), np.int32, stream),
                tv_buf.download((m,), np.float64, stream))


def centerline_gradients(contours, boxes, sigma=1.0, stream=None):
    """the dense part of Polygon.get_centerline_optimized (video/analysis/shapes.py:735-743) for m polygons: the
    uint8 masks of fill_polys(contours, boxes), their distance transforms and the blurred distance maps' Sobel
    planes, every table uploaded first and the kernels then back to back on one stream -- va_fill_poly,
    va_distance_transform_l2_5, va_potential_gradients_ragged
    (items above GRAD_RESIDENT_MAX_PIXELS one by one, as in potential_gradients_ragged).  Masks and distance maps
    stay in leased device buffers, no pixel plane crosses to the host, and the status vectors are read once,
    after the last launch.  contours, boxes as fill_polys takes them.  Returns (fx, fy, shapes, offsets) as
    potential_gradients_ragged does."""
    m = len(contours)
    if not sigma >= 0:
        raise ValueError("centerline_gradients: sigma must be >= 0, got %r" % (sigma,))
    if m == 0:
        _hip.lib()
        return DeviceBuffer(0), DeviceBuffer(0), np.zeros((0, 2), np.int32), np.zeros(0, np.int64)
    verts, vert_off, bx = _fill_tables(contours, boxes, "centerline_gradients")
    _, shapes, offsets, sizes, total = _pack_ragged(bx[:, [3, 2]])
    if shapes[:, 1].max() > DT_MAX_WIDTH or shapes[:, 0].max() > DT_MAX_HEIGHT:
        raise ValueError("centerline_gradients: boxes are limited to %d rows x %d columns"
                         % (DT_MAX_HEIGHT, DT_MAX_WIDTH))
    resident = _grad_resident_items(sizes, _hip.VA_F32, sigma, None, "centerline_gradients")
    L = _hip.lib()
    with _Lease.on(stream) as d:
        fx, fy = (d.adopt(DeviceBuffer(total * 8), DeviceBuffer.free) for _ in range(2))
        vb, vob, bb, sb, ob = (d.upload(verts), d.upload(vert_off), d.upload(bx.astype(np.int32)), d.upload(shapes),
                               d.upload(offsets))
        mask, dist, st = d.take(max(total, 1)), d.take(max(total, 1) * 4), d.take(3 * m * 4)
        plan = _plan_ragged_gradients(d, shapes, offsets, sizes, resident)
        check(L.va_fill_poly(vb.ptr, vob.ptr, len(verts), bb.ptr, ob.ptr, total, m, 1, mask.ptr, st.ptr, stream))
        check(L.va_distance_transform_l2_5(mask.ptr, sb.ptr, ob.ptr, total, m, int(shapes[:, 1].max()), dist.ptr,
                                           st.ptr + 4 * m, stream))
        # a mask or a map a status refuses is not written: what the later kernels make of it is discarded below
        _enqueue_ragged_gradients(d, plan, dist, _hip.VA_F32, shapes, offsets, sizes, total, sigma, resident, fx, fy,
                                  st.ptr + 8 * m, stream)
        status = st.download((2 * m + len(resident),), np.int32, stream)
        _check_status(status[:m], "centerline_gradients (fill)")
        _check_status(status[m:2 * m], "centerline_gradients (distance transform)")
        _check_status(status[2 * m:], "centerline_gradients (gradients)")
    return fx, fy, shapes, offsets


# ------------------------------------------------------------------------------------ Guo-Hall thinning
THIN_RESIDENT_MAX_WORDS = 15360  # VA_THIN_RESIDENT_MAX_WORDS: h * ceil(w / 32) of a mask the resident kernel takes
THIN_RESIDENT_DEFAULT_WORDS = 4096  # larger masks take the tiled path by default: at 15360 words it measured 3.1x faster
THIN_TILED_SUB_ITERATIONS = 0    # sub-iterations per launch of the tiled path (0: the library's default, 16)
THIN_TILED_POLL = 0              # launches between two host reads of the changed flags (0: the default, 2)


def _thin_words(shape):
    return int(shape[0]) * ((int(shape[1]) + 31) // 32)


def _thin_resident(arrs, stream):
    """one va_guo_hall_thinning_batch call over 2-d uint8 arrays; (skeletons, int32 iterations)"""
    m = len(arrs)
    flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
    with _Lease.on(stream) as d:
        src, sb, ob, out, it, st = (d.upload(flat), d.upload(shapes), d.upload(offsets), d.take(max(total, 1)),
                                    d.take(m * 4), d.take(m * 4))
        check(_hip.lib().va_guo_hall_thinning_batch(src.ptr, sb.ptr, ob.ptr, total, m,
                                                    max(_thin_words(a.shape) for a in arrs), out.ptr, it.ptr, st.ptr,
                                                    stream))
        _check_status(st.download((m,), np.int32, stream), "guo_hall_thinning")
        iters = it.download((m,), np.int32, stream)
        res = out.download((max(total, 1),), np.uint8, stream)
    return _split_ragged(res, shapes, offsets, sizes), iters


def _thin_tiled(stack, stream):
    """va_guo_hall_thinning_u8 on an (n, h, w) uint8 stack with n, h, w >= 1; (skeletons, int32 iterations)"""
    n, h, w = stack.shape
    L = _hip.lib()
    need = L.va_guo_hall_thinning_scratch_bytes(n, h, w)
    if need == 0:
        raise ValueError("guo_hall_thinning: a stack of shape %r is beyond the tiled path's limits" % (stack.shape,))
    iters = np.zeros(n, np.int32)
    with _Lease.on(stream) as d:
        src, scratch, dst = d.upload(stack), d.take(need), d.take(stack.size)
        check(L.va_guo_hall_thinning_u8(src.ptr, scratch.ptr, need, dst.ptr, n, h, w, int(THIN_TILED_SUB_ITERATIONS),
                                        int(THIN_TILED_POLL), iters.ctypes.data, None, stream))
        return dst.download(stack.shape, np.uint8, stream), iters


def guo_hall_thinning(masks, implementation=None, ret_iterations=False, stream=None):
    """thinning.guo_hall_thinning(mask) -- the `guo-hall` method of mask_thinning, video/analysis/image.py:236-241 --
    of every mask of a list of 2-d arrays (ragged) or of one (n, h, w) stack; uint8 or bool, non-zero = foreground.
    The definition is pinned in DESIGN.md §9: parallel sub-iterations until an iteration deletes nothing, the first
    and last row and column never tested.  Returns uint8 skeletons in the same form (the input's own values where a
    pixel survives; the inputs are left alone), and with ret_iterations also the int32 iteration counts.
    implementation: None (masks of up to THIN_RESIDENT_DEFAULT_WORDS packed words run to their fixed point in LDS, one
    launch per size class of the kernel, at most three; larger ones go through bit planes in HBM, equal shapes stacked), 'resident' or 'tiled'."""
    if implementation not in (None, "resident", "tiled"):
        raise ValueError("guo_hall_thinning: unknown implementation %r" % (implementation,))
    is_stack = isinstance(masks, np.ndarray)
    if is_stack and masks.ndim != 3:
        raise ValueError("guo_hall_thinning: expected a list of 2-d masks or an (n, h, w) stack, got shape %r"
                         % (masks.shape,))
    arrs = []
    for k, a in enumerate(masks):
        a = np.asarray(a)
        if a.dtype != np.uint8 and a.dtype != np.bool_:
            raise TypeError("guo_hall_thinning: mask %d has dtype %s (uint8 or bool are supported)" % (k, a.dtype))
        if a.ndim != 2:
            raise ValueError("guo_hall_thinning: mask %d is not 2-d (shape %r)" % (k, a.shape))
        if implementation == "resident" and _thin_words(a.shape) > THIN_RESIDENT_MAX_WORDS:
            raise ValueError("guo_hall_thinning: mask %d of shape %r needs %d packed words, the resident kernel "
                             "takes %d" % (k, a.shape, _thin_words(a.shape), THIN_RESIDENT_MAX_WORDS))
        arrs.append(np.ascontiguousarray(a).view(np.uint8))
    m = len(arrs)
    out, iters = [None] * m, np.ones(m, np.int32)
    resident, tiled = [], {}
    for k, a in enumerate(arrs):
        if a.size == 0:                                      # nothing to test: unchanged after one iteration
            out[k] = a.copy()
        elif implementation != "tiled" and _thin_words(a.shape) <= (
                THIN_RESIDENT_MAX_WORDS if implementation == "resident" else THIN_RESIDENT_DEFAULT_WORDS):
            resident.append(k)
        else:
            tiled.setdefault(a.shape, []).append(k)
    # one launch per size class of the kernel (4 / 16 / 60 words per thread): the LDS and the registers of a launch
    # are those of its largest mask, so one large mask must not cost the small ones their occupancy
    classes = {}
    for k in resident:
        words = _thin_words(arrs[k].shape)
        classes.setdefault(0 if words <= 1024 else 1 if words <= 4096 else 2, []).append(k)
    for idx in classes.values():
        res, it = _thin_resident([arrs[k] for k in idx], stream)
        for k, r, i in zip(idx, res, it):
            out[k], iters[k] = r, i
    for shape, idx in tiled.items():
        for a in range(0, len(idx), 65535):
            part = idx[a:a + 65535]
            res, it = _thin_tiled(np.stack([arrs[k] for k in part]), stream)
            for k, r, i in zip(part, res, it):
                out[k], iters[k] = r, i
    if is_stack:
        out = np.stack(out) if m else np.zeros(masks.shape, np.uint8)
    return (out, iters) if ret_iterations else out


# ------------------------------------------------------------------------- affine warps and line scans
WARP_MAX_SIDE = 32767            # VA_WARP_MAX_SIDE .. VA_WARP_INVERSE_MAP, include/videoanalysis_hip.h
WARP_CHUNK = 64
WARP_TILE_W, WARP_TILE_H = 64, 16
WARP_INVERSE_MAP = 1


def affine_transforms(src_pts, dst_pts):
    """cv2.getAffineTransform(src, dst) for a batch of point triples: (m, 3, 2) each (or one (3, 2) pair), cast to
    float32 as cv2 takes them; returns (m, 2, 3) float64.  The 6x6 systems (rows i and i + 3 = (x_i, y_i, 1, 0, 0, 0
    | X_i) and (0, 0, 0, x_i, y_i, 1 | Y_i)) are solved as cv::solve(DECOMP_LU) solves them, operation by operation
    (DESIGN.md §9): the order is part of the definition, a closed form changes pixels.  Host arithmetic, vectorised
    over the batch.  A pivot below 100 eps (collinear source points) raises ValueError."""
    src = np.asarray(src_pts, np.float32).astype(np.float64).reshape(-1, 3, 2)
    dst = np.asarray(dst_pts, np.float32).astype(np.float64).reshape(-1, 3, 2)
    if len(src) != len(dst):
        raise ValueError("affine_transforms: %d source and %d destination triples" % (len(src), len(dst)))
    m = len(src)
    a, b = np.zeros((m, 6, 6)), np.zeros((m, 6))
    a[:, :3, 0:2], a[:, :3, 2] = src, 1.0
    a[:, 3:, 3:5], a[:, 3:, 5] = src, 1.0
    b[:, :3], b[:, 3:] = dst[:, :, 0], dst[:, :, 1]
    idx = np.arange(m)
    for i in range(6):
        k = i + np.argmax(np.abs(a[:, i:, i]), axis=1)       # the first of the largest, as the scan with `>` finds it
        bad = np.flatnonzero(~(np.abs(a[idx, k, i]) >= 100 * np.finfo(np.float64).eps))
        if len(bad):
            raise ValueError("affine_transforms: the source points of item %d are collinear" % bad[0])
        row, rhs = a[idx, i].copy(), b[idx, i].copy()
        a[idx, i], b[idx, i] = a[idx, k], b[idx, k]
        a[idx, k], b[idx, k] = row, rhs
        d = -1 / a[:, i, i]
        for j in range(i + 1, 6):
            alpha = a[:, j, i] * d
            a[:, j, i + 1:] += alpha[:, None] * a[:, i, i + 1:]
            b[:, j] += alpha * b[:, i]
    for i in range(5, -1, -1):
        s = b[:, i].copy()
        for c in range(i + 1, 6):
            s -= a[:, i, c] * b[:, c]
        b[:, i] = s / a[:, i, i]
    return b.reshape(m, 2, 3)


def _warp_frames(frames, m, frame_index, what):
    """(contiguous (n, h, w) uint8 stack, int32 frame index per item)"""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        raise TypeError("%s: single-channel uint8 frames only, got %s" % (what, frames.dtype))
    arr, n, fshape, _ = _as_batch(frames, 2)
    arr = arr.reshape((n,) + tuple(fshape))
    if fshape[0] < 1 or fshape[1] < 1:
        raise ValueError("%s: empty frames of shape %r" % (what, tuple(fshape)))
    if frame_index is None:
        if n != 1:
            raise ValueError("%s: a stack of %d frames needs a frame_index per item" % (what, n))
        fidx = np.zeros(m, np.int32)
    else:
        fidx = np.asarray(frame_index, np.int64).reshape(-1)
        if len(fidx) != m or np.any(fidx < 0) or np.any(fidx >= n):
            raise ValueError("%s: frame_index must hold %d entries in 0 .. %d" % (what, m, n - 1))
        fidx = fidx.astype(np.int32)
    return arr, fidx


def _work_prefix(counts, what):
    """(int32 exclusive prefix of the per-item work-item counts, their total)"""
    total = int(counts.sum())
    if total >= 2 ** 31:
        raise ValueError("%s: %d work items in one call (fewer than 2^31 are supported)" % (what, total))
    prefix = np.zeros(len(counts), np.int64)
    prefix[1:] = np.cumsum(counts)[:-1]
    return prefix.astype(np.int32), total


def line_scan_tables(p1, p2, half_width=5):
    """the host side of line_scan (video/analysis/image.py:95-103) for m scans: (matrices (m, 2, 3) float64, rows,
    cols int64 (m,)).  length = hypot, angle = arctan2 in float64, p0 = (p1x + hw sin, p1y - hw cos); the triple
    (p0, p1, p2) maps onto ((0, 0), (0, hw), (length, hw)); the strip has int(2 hw) rows and int(length) columns.
    An empty strip or one beyond WARP_MAX_SIDE raises ValueError."""
    p1 = np.asarray(p1, np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    m = len(p1)
    if len(p2) != m:
        raise ValueError("line_scans: %d start and %d end points" % (m, len(p2)))
    hw = np.broadcast_to(np.asarray(half_width, np.float64), (m,)) if np.ndim(half_width) == 0 else \
        np.asarray(half_width, np.float64).reshape(-1)
    if len(hw) != m:
        raise ValueError("line_scans: %d half widths for %d scans" % (len(hw), m))
    dx, dy = p2[:, 0] - p1[:, 0], p2[:, 1] - p1[:, 1]
    length, angle = np.hypot(dx, dy), np.arctan2(dy, dx)
    if not (np.all(np.isfinite(length)) and np.all(np.isfinite(hw))):
        raise ValueError("line_scans: points and half widths must be finite")
    bad = np.flatnonzero((length < 1) | (2 * hw < 1))
    if len(bad):
        raise ValueError("line_scans: scan %d is empty (length %g, half width %g)" % (bad[0], length[bad[0]], hw[bad[0]]))
    bad = np.flatnonzero((length >= WARP_MAX_SIDE + 1) | (2 * hw >= WARP_MAX_SIDE + 1))
    if len(bad):
        raise ValueError("line_scans: scan %d exceeds %d pixels a side" % (bad[0], WARP_MAX_SIDE))
    src = np.stack([np.stack([p1[:, 0] + hw * np.sin(angle), p1[:, 1] - hw * np.cos(angle)], 1), p1, p2], 1)
    dst = np.zeros((m, 3, 2))
    dst[:, 1, 1], dst[:, 2, 0], dst[:, 2, 1] = hw, length, hw
    return affine_transforms(src, dst), (2 * hw).astype(np.int64), length.astype(np.int64)


def line_scans(frames, p1, p2, half_width=5, frame_index=None, stream=None, ret_sums=False):
    """line_scan(img, p1, p2, half_width) (video/analysis/image.py:89-106) for m scans in one launch: the mean over
    the width of the strip from p1 to p2 that cv2.warpAffine cuts out of the frame ("Affine warps and
    line scans").  frames: one (h, w) uint8 frame or an (n, h, w) stack with frame_index (m,) naming each scan's
    frame; p1, p2: (m, 2) (x, y) points; half_width: a number or (m,).  Returns the list of float64 profiles, each
    the GPU's exact int32 column sums divided by the strip's rows; with ret_sums also the list of those sums."""
    mats, rows, cols = line_scan_tables(p1, p2, half_width)
    m = len(rows)
    arr, fidx = _warp_frames(frames, m, frame_index, "line_scans")
    if m == 0:
        return ([], []) if ret_sums else []
    n, h, w = arr.shape
    _, shapes, offsets, sizes, total = _pack_ragged(np.stack([np.ones(m, np.int64), cols], 1))
    prefix, chunks = _work_prefix(np.maximum(1, -(-cols // WARP_CHUNK)), "line_scans")
    with _Lease.on(stream) as d:
        fb, ib, mb, sb, ob, pb = (d.upload(arr), d.upload(fidx), d.upload(mats),
                                  d.upload(np.stack([rows, cols], 1).astype(np.int32)), d.upload(offsets),
                                  d.upload(prefix))
        out, st = d.take(total * 4), d.take(m * 4)
        check(_hip.lib().va_line_scan_u8(fb.ptr, n, h, w, m, ib.ptr, mb.ptr, sb.ptr, ob.ptr, pb.ptr, chunks, total,
                                         out.ptr, st.ptr, stream))
        _check_status(st.download((m,), np.int32, stream), "line_scans")
        flat = out.download((total,), np.int32, stream)
    sums = [s[0] for s in _split_ragged(flat, shapes, offsets, sizes)]
    profiles = [s.astype(np.float64) / r for s, r in zip(sums, rows.tolist())]
    return (profiles, sums) if ret_sums else profiles


def warp_affine(frames, matrices, sizes, frame_index=None, inverse=False, stream=None):
    """cv2.warpAffine(frame, matrix, (dw, dh)) with INTER_LINEAR and BORDER_CONSTANT 0 for m items in one launch
    (get_subimage, video/analysis/image.py:81-82).  frames: one (h, w) uint8 frame or an (n, h, w)
    stack with frame_index (m,); matrices: (m, 2, 3) float64 forward maps (or one (2, 3)); sizes: (m, 2) NumPy shapes
    (dh, dw) of the destinations; inverse: True, or (m,) booleans, for matrices that map destination to source
    (cv2.WARP_INVERSE_MAP).  Returns the list of (dh, dw) uint8 arrays.  An empty destination raises ValueError
    (OpenCV would warp to the source's size)."""
    mats = np.ascontiguousarray(matrices, np.float64).reshape(-1, 2, 3)
    m = len(mats)
    sz = np.asarray(sizes, np.int64).reshape(-1, 2)
    if len(sz) != m:
        raise ValueError("warp_affine: %d matrices and %d sizes" % (m, len(sz)))
    bad = np.flatnonzero(np.any(sz < 1, axis=1))
    if len(bad):
        raise ValueError("warp_affine: destination %d is empty (%d x %d)" % (bad[0], sz[bad[0], 0], sz[bad[0], 1]))
    if np.any(sz > WARP_MAX_SIDE):
        raise ValueError("warp_affine: destinations are limited to %d pixels a side" % WARP_MAX_SIDE)
    flags = np.broadcast_to(np.asarray(inverse, bool), (m,)).astype(np.int32) * WARP_INVERSE_MAP
    arr, fidx = _warp_frames(frames, m, frame_index, "warp_affine")
    if m == 0:
        return []
    n, h, w = arr.shape
    _, shapes, offsets, sizes_, total = _pack_ragged(sz)
    prefix, tiles = _work_prefix(np.maximum(1, (-(-sz[:, 0] // WARP_TILE_H)) * (-(-sz[:, 1] // WARP_TILE_W))),
                                 "warp_affine")
    with _Lease.on(stream) as d:
        fb, ib, mb, sb, gb, ob, pb = (d.upload(arr), d.upload(fidx), d.upload(mats), d.upload(shapes),
                                      d.upload(flags), d.upload(offsets), d.upload(prefix))
        out, st = d.take(total), d.take(m * 4)
        check(_hip.lib().va_warp_affine_u8(fb.ptr, n, h, w, m, ib.ptr, mb.ptr, sb.ptr, gb.ptr, ob.ptr, pb.ptr, tiles,
                                           total, out.ptr, st.ptr, stream))
        _check_status(st.download((m,), np.int32, stream), "warp_affine")
        flat = out.download((total,), np.uint8, stream)
    return _split_ragged(flat, shapes, offsets, sizes_)


# ------------------------------------------------------------------------------------ skeleton graphs
DEFAULT_SKELETON_NODE_CAPACITY = 1 << 16     # nodes / edges / points of a skeleton_graphs batch the first launch
DEFAULT_SKELETON_EDGE_CAPACITY = 1 << 16     # has room for (4096 worm skeletons: 8192, 4096 and some 400 000)
DEFAULT_SKELETON_POINT_CAPACITY = 1 << 20
# va_skeleton_node, va_skeleton_edge, include/videoanalysis_hip.h
SKELETON_NODE_DTYPE = np.dtype([("item", np.int32), ("x", np.int32), ("y", np.int32), ("degree", np.int32),
                                ("pixels", np.int32)])
SKELETON_EDGE_DTYPE = np.dtype([("item", np.int32), ("node_a", np.int32), ("node_b", np.int32),
                                ("npoints", np.int32), ("length", np.float64)])


class SkeletonGraph(tuple):
    """the graph of one item: (nodes, edges, curves) -- SKELETON_NODE_DTYPE and SKELETON_EDGE_DTYPE records in the
    definition's order, and one (npoints, 2) int32 array of (x, y) points per edge"""
    __slots__ = ()
    nodes = property(lambda self: self[0])
    edges = property(lambda self: self[1])
    curves = property(lambda self: self[2])


def _skeleton_graph_run(d, src, sb, ob, total, m, stream):
    """va_skeleton_graph on packed items that are on the device already (lease d): the first launch with the default
    capacities and, if a total exceeds one, exactly one more with exact room; the m SkeletonGraphs"""
    L = _hip.lib()
    ws_bytes = L.va_skeleton_graph_workspace_bytes(total, m)
    ws, cnt, tot = d.take(ws_bytes), d.take(m * 8), d.take(24)

    def run(capn, cape, capp):
        nodes, edges, off, pts = (d.take(max(capn, 1) * SKELETON_NODE_DTYPE.itemsize),
                                  d.take(max(cape, 1) * SKELETON_EDGE_DTYPE.itemsize), d.take((cape + 1) * 8),
                                  d.take(max(capp, 1) * 8))
        check(L.va_skeleton_graph(src.ptr, sb.ptr, ob.ptr, total, m, cnt.ptr, tot.ptr, nodes.ptr, capn, edges.ptr,
                                  off.ptr, cape, pts.ptr, capp, ws.ptr, ws_bytes, stream))
        return (nodes, edges, off, pts), tot.download((3,), np.int64, stream)
    (nodes, edges, off, pts), totals = _rerun(run, DEFAULT_SKELETON_NODE_CAPACITY, DEFAULT_SKELETON_EDGE_CAPACITY,
                                              DEFAULT_SKELETON_POINT_CAPACITY)
    nn, ne, npts = (int(t) for t in totals)
    counts = cnt.download((m, 2), np.int32, stream).astype(np.int64)
    node_rec = nodes.download((nn,), SKELETON_NODE_DTYPE, stream)
    edge_rec = edges.download((ne,), SKELETON_EDGE_DTYPE, stream)
    offsets = off.download((ne + 1,), np.int64, stream)
    points = pts.download((npts, 2), np.int32, stream)
    fn = np.concatenate([[0], np.cumsum(counts[:, 0])])
    fe = np.concatenate([[0], np.cumsum(counts[:, 1])])
    return [SkeletonGraph((node_rec[fn[i]:fn[i + 1]], edge_rec[fe[i]:fe[i + 1]],
                           [points[offsets[s]:offsets[s + 1]] for s in range(fe[i], fe[i + 1])])) for i in range(m)]


def skeleton_graphs(skeletons, stream=None):
    """the skeleton graph of every image of a list of 2-d arrays of any shapes, of one 2-d array or of an (n, h, w)
    stack (uint8 or bool, non-zero = foreground), in one va_skeleton_graph call: nodes, edges and branch curves by
    the definition pinned in DESIGN.md §9, "Skeleton graphs" (m-adjacency; node pixels have degree != 2; an edge is
    a chain of degree-2 pixels between two node pixels) -- what MorphologicalGraph.from_skeleton
    (video/analysis/morphological_graph.py:287-378) walks on the host, without its dependence on a pop order.
    Returns one SkeletonGraph per image (a single one for a 2-d array).  The first launch has room for
    DEFAULT_SKELETON_NODE_CAPACITY nodes, DEFAULT_SKELETON_EDGE_CAPACITY edges and DEFAULT_SKELETON_POINT_CAPACITY
    points in the batch; a batch that holds more runs exactly once more, with exact room."""
    single = isinstance(skeletons, np.ndarray) and skeletons.ndim == 2
    if isinstance(skeletons, np.ndarray) and skeletons.ndim not in (2, 3):
        raise ValueError("skeleton_graphs: expected a list of 2-d images, one image or an (n, h, w) stack, got "
                         "shape %r" % (skeletons.shape,))
    arrs = []
    for k, a in enumerate([skeletons] if single else skeletons):
        a = np.asarray(a)
        if a.dtype != np.uint8 and a.dtype != np.bool_:
            raise TypeError("skeleton_graphs: image %d has dtype %s (uint8 or bool are supported)" % (k, a.dtype))
        if a.ndim != 2:
            raise ValueError("skeleton_graphs: image %d is not 2-d (shape %r)" % (k, a.shape))
        if a.size >= 2 ** 29:
            raise ValueError("skeleton_graphs: image %d has %d pixels (fewer than 2^29 are supported)" % (k, a.size))
        arrs.append(np.ascontiguousarray(a).view(np.uint8))
    m = len(arrs)
    if m == 0:
        return []
    flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
    if total >= 2 ** 31 - 2:
        raise ValueError("skeleton_graphs: %d pixels in one call (fewer than 2^31 - 2 are supported)" % total)
    with _Lease.on(stream) as d:
        src, sb, ob = d.upload(flat), d.upload(shapes), d.upload(offsets)
        res = _skeleton_graph_run(d, src, sb, ob, total, m, stream)
    return res[0] if single else res


def polygon_skeleton_graphs(contours, boxes, stream=None):
    """the skeleton graphs of m polygons (Polygon.get_morphological_graph's pixel work, video/analysis/shapes.py:
    631-637): the uint8 masks of fill_polys(contours, boxes), their Guo-Hall skeletons and the graphs of those,
    every table uploaded first and the kernels then back to back on one stream -- va_fill_poly,
    va_guo_hall_thinning_batch (one launch per size class, as guo_hall_thinning), va_skeleton_graph.  Masks and
    skeletons stay in leased device buffers, no pixel plane crosses to the host.  Only a box above
    THIN_RESIDENT_MAX_WORDS packed words takes the per-item path: fill_polys and guo_hall_thinning (its tiled
    form) for that box alone, its skeleton copied into the batch's skeleton buffer before the graph kernel.
    contours, boxes as fill_polys takes them.  Returns one SkeletonGraph per polygon, in box coordinates."""
    m = len(contours)
    if m == 0:
        return []
    verts, vert_off, bx = _fill_tables(contours, boxes, "polygon_skeleton_graphs")
    _, shapes, offsets, sizes, total = _pack_ragged(bx[:, [3, 2]])
    words = [_thin_words(s) for s in shapes]
    large = [k for k, wd in enumerate(words) if wd > THIN_RESIDENT_MAX_WORDS]
    large_skel = [np.ascontiguousarray(sk) for sk in guo_hall_thinning(
        fill_polys([contours[k] for k in large], bx[large], stream=stream), stream=stream)] if large else []
    if total >= 2 ** 31 - 2:
        raise ValueError("polygon_skeleton_graphs: %d pixels in one call (fewer than 2^31 - 2 are supported)" % total)
    classes = {}
    for k, wd in enumerate(words):
        if 0 < wd <= THIN_RESIDENT_MAX_WORDS:
            classes.setdefault(0 if wd <= 1024 else 1 if wd <= 4096 else 2, []).append(k)
    L = _hip.lib()
    with _Lease.on(stream) as d:
        vb, vob, bb, sb, ob = (d.upload(verts), d.upload(vert_off), d.upload(bx.astype(np.int32)), d.upload(shapes),
                               d.upload(offsets))
        tables = [(idx, d.upload(shapes[idx]), d.upload(offsets[idx])) for idx in classes.values()]
        mask, skel, st, it = d.take(max(total, 1)), d.take(max(total, 1)), d.take(2 * m * 4), d.take(m * 4)
        check(L.va_fill_poly(vb.ptr, vob.ptr, len(verts), bb.ptr, ob.ptr, total, m, 1, mask.ptr, st.ptr, stream))
        at = m
        for idx, csb, cob in tables:
            check(L.va_guo_hall_thinning_batch(mask.ptr, csb.ptr, cob.ptr, total, len(idx),
                                               max(words[k] for k in idx), skel.ptr, it.ptr + 4 * (at - m),
                                               st.ptr + 4 * at, stream))
            at += len(idx)
        for k, sk in zip(large, large_skel):
            check(L.va_memcpy_h2d(skel.ptr + int(offsets[k]), sk.ctypes.data, sk.nbytes, stream))   # (contiguous)
        if large:
            check(L.va_stream_sync(stream))    # pageable sources: the copies are complete before they go away
        # an empty box has no pixels in either buffer; a mask a status refuses is not written, and what the later
        # kernels make of it is discarded below: the statuses are read once, after the last launch
        res = _skeleton_graph_run(d, skel, sb, ob, total, m, stream)
        status = st.download((at,), np.int32, stream)
        _check_status(status[:m], "polygon_skeleton_graphs (fill)")
        _check_status(status[m:], "polygon_skeleton_graphs (thinning)")
        return res


# ------------------------------------------------------------------------------------ outline queries
OUTLINE_LANES = {None: 0, "lanes8": 8, "lanes64": 64}
# implementation=None: 64 lanes a query when the queries of the batch look at this many edges or more on average,
# else 8 ("Outline queries": between 256 and 512 edges the 64-lane kernel overtakes the 8-lane one)
OUTLINE_WIDE_MIN_EDGES = 384
OUTLINE_MAX_POINTS = 2 ** 31 - 2


def _pack_outlines(outlines, what):
    """(points float64 flat, point offsets int64 (m + 1,), points per outline int64 (m,)) of m outlines, each an
    (n, 2) array-like of any length; one without points may have any empty shape"""
    arrs = []
    for k, o in enumerate(outlines):
        a = np.asarray(o, np.float64)
        if a.size == 0 and a.ndim <= 2:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("%s: outline %d has shape %r, not (n, 2)" % (what, k, a.shape))
        if len(a) > OUTLINE_MAX_POINTS:
            raise ValueError("%s: outline %d has %d points (at most 2^31 - 2 are supported)" % (what, k, len(a)))
        arrs.append(a)
    if not arrs:
        return np.zeros(1, np.float64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
    return flat, np.append(offsets, total) // 2, shapes[:, 0].astype(np.int64)


def _outline_index(index, m, q, what):
    """the int32 outline index of q queries over m outlines, checked"""
    if index is None:
        if m == 1:
            return np.zeros(q, np.int32)
        if q != m:
            raise ValueError("%s: without an index, %d outlines need %d queries, one each in order (got %d)"
                             % (what, m, m, q))
        return np.arange(m, dtype=np.int32)
    idx = np.asarray(index, np.int64).reshape(-1)
    if len(idx) != q:
        raise ValueError("%s: %d index entries for %d queries" % (what, len(idx), q))
    if np.any(idx < 0) or np.any(idx >= m):
        raise ValueError("%s: index must lie in 0 .. %d" % (what, m - 1))
    return idx.astype(np.int32)


def _outline_lanes(edges, implementation, what):
    """the lanes a query gets in the batch's one launch: those of a named implementation, or for None the rule over
    the edge counts the batch's queries look at: 64 from a mean of OUTLINE_WIDE_MIN_EDGES on, else 8"""
    if implementation not in OUTLINE_LANES:
        raise ValueError("%s: implementation is None, 'lanes8' or 'lanes64', got %r" % (what, implementation))
    if implementation is not None:
        return OUTLINE_LANES[implementation]
    return 64 if len(edges) and edges.mean() >= OUTLINE_WIDE_MIN_EDGES else 8


def _query_points(points, what, name):
    p = np.asarray(points, np.float64)
    if p.size == 0 and p.ndim <= 2:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("%s: %s has shape %r, not (q, 2)" % (what, name, p.shape))
    return p


def ray_hits(outlines, closed, anchors, fars, index=None, implementation=None, stream=None):
    """where q rays first hit their outlines (get_ray_hitpoint, video/analysis/regions.py:353-391, for every ray of
    a batch; DESIGN.md §9, "Outline queries").  outlines: a list of m (n, 2) array-likes of (x, y) points of any
    lengths, 0 and 1 included, converted to float64; closed: m flags, a true one adds the edge from the last point
    to the first; anchors, fars: (q, 2), ray k runs from anchors[k] to fars[k]; index: (q,) the outline of each
    ray.  index=None means the one outline for every ray when m == 1, else ray k onto outline k, which needs
    q == m.  implementation: None (by the mean edge count of the batch's queries, OUTLINE_WIDE_MIN_EDGES),
    'lanes8' or 'lanes64'; one launch, and all give the same bytes.  Returns (t (q,) float64, hits (q, 2) float64, edge (q,)
    int32, count (q,) int32): the hitting edge with the smallest (t, edge), the hit point anchor + t (far - anchor)
    and the number of hitting edges; without a hit t and the point are NaN, edge is -1 and count 0.  A bad index or
    outline raises ValueError before anything is launched; a query the device refuses raises RuntimeError."""
    what = "ray_hits"
    flat, point_off, npts = _pack_outlines(outlines, what)
    m = len(npts)
    flags = np.asarray(closed, bool).reshape(-1)
    if len(flags) != m:
        raise ValueError("%s: %d closed flags for %d outlines" % (what, len(flags), m))
    a, f = _query_points(anchors, what, "anchors"), _query_points(fars, what, "fars")
    q = len(a)
    if len(f) != q:
        raise ValueError("%s: %d anchors and %d far points" % (what, q, len(f)))
    idx = _outline_index(index, m, q, what)
    edges = np.where(npts == 0, 0, np.where(flags, npts, npts - 1))[idx] if q else np.zeros(0, np.int64)
    lanes = _outline_lanes(edges, implementation, what)
    if q == 0:
        return np.zeros(0), np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32)
    L = _hip.lib()
    with _Lease.on(stream) as d:
        pb, ob, cb, ab, fb, ib = (d.upload(flat), d.upload(point_off), d.upload(flags.astype(np.uint8)), d.upload(a),
                                  d.upload(f), d.upload(idx))
        out = d.take(32 * q)                   # t | hits | edge | count: one download
        check(L.va_ray_hits(pb.ptr, ob.ptr, cb.ptr, int(point_off[-1]), m, ab.ptr, fb.ptr, ib.ptr, q, lanes, out.ptr,
                            out.ptr + 8 * q, out.ptr + 24 * q, out.ptr + 28 * q, stream))
        raw = out.download((32 * q,), np.uint8, stream)
    t, hits = raw[:8 * q].view(np.float64), raw[8 * q:24 * q].view(np.float64).reshape(q, 2)
    edge, count = raw[24 * q:28 * q].view(np.int32), raw[28 * q:].view(np.int32)
    bad = np.flatnonzero(count < 0)
    if len(bad):
        raise RuntimeError("%s: the device refused ray %d" % (what, bad[0]))
    return t.copy(), hits.copy(), edge.copy(), count.copy()


def points_in_outlines(outlines, points, index=None, implementation=None, stream=None):
    """whether q points lie inside their rings (Polygon.contains, video/analysis/shapes.py:552-554, for a batch;
    DESIGN.md §9, "Outline queries").  outlines: a list of m (n, 2) array-likes of any lengths, converted to
    float64, each closed with the edge from its last point to its first; points: (q, 2); index: (q,) the ring of
    each point.  index=None means the one ring for every point when m == 1, else point k in ring k, which needs
    q == m.  implementation as ray_hits takes it.  Returns (q,) bool: True strictly inside; the boundary, a ring of
    fewer than three points and a non-finite point give False.  A bad index or outline raises ValueError before
    anything is launched; a query the device refuses raises RuntimeError."""
    what = "points_in_outlines"
    flat, point_off, npts = _pack_outlines(outlines, what)
    m = len(npts)
    p = _query_points(points, what, "points")
    q = len(p)
    idx = _outline_index(index, m, q, what)
    lanes = _outline_lanes(npts[idx] if q else np.zeros(0, np.int64), implementation, what)
    if q == 0:
        return np.zeros(0, bool)
    L = _hip.lib()
    with _Lease.on(stream) as d:
        pb, ob, xb, ib = d.upload(flat), d.upload(point_off), d.upload(p), d.upload(idx)
        out = d.take(q)
        check(L.va_points_in_outlines(pb.ptr, ob.ptr, int(point_off[-1]), m, xb.ptr, ib.ptr, q, lanes, out.ptr, stream))
        inside = out.download((q,), np.uint8, stream)
    bad = np.flatnonzero(inside > 1)
    if len(bad):
        raise RuntimeError("%s: the device refused point %d" % (what, bad[0]))
    return inside != 0


# ------------------------------------------------------------------------------------ equidistant curves
CURVES_MAX_POINTS = 1 << 24      # VA_CURVES_MAX_POINTS, VA_CURVES_MAX_STEPS, include/videoanalysis_hip.h
CURVES_MAX_STEPS = 1 << 20
CURVES_MAX_COORD = 1e100         # a curve with a larger coordinate (or a non-finite one) is resampled on the host
# the batched callers (video.analysis.curves.resample_many) go to the device from this many curves on; below it the
# per-curve Python loop is quicker than a device round trip ("Equidistant curves": the crossover)
CURVES_DEVICE_MIN_BATCH = 8
CURVES_ROOM_SLACK = 3            # points a walked curve gets beyond the estimate of its result in the first launch

# (dx, dy, sqrt(fma(dy, dy, dx * dx)), sqrt(dx * dx + dy * dy)): vectors on which the two forms differ
_NORM_PROBES = (
    ("0x1.33ef6c3c6472fp-2", "-0x1.b4bf2ef288857p-1", "0x1.cf177153ae392p-1", "0x1.cf177153ae391p-1"),
    ("-0x1.24dfc42b81355p+1", "-0x1.1fdbb9ed7b8f3p+1", "0x1.9aa7b68af0f63p+1", "0x1.9aa7b68af0f64p+1"),
    ("-0x1.880492c3cc3d2p+2", "0x1.3a5260ab86f1ap+1", "0x1.a65900c38e989p+2", "0x1.a65900c38e988p+2"),
    ("0x1.e7d8a19827d10p+1", "-0x1.715a919dda321p+2", "0x1.baa11a0e9e82ep+2", "0x1.baa11a0e9e82dp+2"),
    ("-0x1.f90c310f4b3b1p-1", "0x1.504291301551cp+2", "0x1.56228c0aa6030p+2", "0x1.56228c0aa602fp+2"),
    ("0x1.a1fa05313cde3p+1", "-0x1.78034bce8cb5ap+2", "0x1.ae3027468bb1bp+2", "0x1.ae3027468bb1cp+2"),
)
_norm_pinned = None


def host_norm_is_pinned():
    """whether this host's np.linalg.norm of a 2-vector is sqrt(fma(dy, dy, dx * dx)), the form the device walk is
    pinned to (NumPy's dot on a BLAS with FMA); checked once on _NORM_PROBES.  Where it is not, the batched
    callers keep resampling on the host, so that they still equal the per-curve function on this host."""
    global _norm_pinned
    if _norm_pinned is None:
        _norm_pinned = all(float(np.linalg.norm(np.array([float.fromhex(x), float.fromhex(y)]))) == float.fromhex(fused)
                           for x, y, fused, _ in _NORM_PROBES)
    return _norm_pinned


def _per_curve(value, m, what, name):
    """None, one value for every curve, or one per curve: a list of m entries"""
    if value is None or np.ndim(value) == 0:
        return [value] * m
    value = list(value)
    if len(value) != m:
        raise ValueError("%s: %d %s entries for %d curves" % (what, len(value), name, m))
    return value


def _curve_on_host(curve, spacing, count, offset):
    """one curve through the host function, translated: ((K, 2) float64, its float32-rule length)"""
    from .analysis import curves as _curves
    res = _curves.make_curve_equidistant(curve, spacing=spacing, count=count)
    res = np.asarray(res, np.float64)
    if offset is not None:
        res = _curves.translate_points(res, offset[0], offset[1])
    return res, float(_curves.curve_length(res))


def curves_equidistant(curves, spacing=None, count=None, offsets=None, ret_lengths=False, stream=None):
    """curves.make_curve_equidistant (video/analysis/curves.py:103-148) for every curve of a list in one
    va_curves_equidistant call, bit for bit the per-curve function ("Equidistant curves").  curves: m
    (n, 2) array-likes of any lengths, converted to float64.  spacing: None, one spacing or one per curve (None
    entries allowed); a curve with a spacing is walked and a point dropped every L / rint(L / spacing).  A curve
    without one gets `count` points at equal arc length: count is None (as many as the curve has), one integer or
    one per curve.  offsets: None or one (xoff, yoff) per curve, added to every coordinate of the result
    (curves.translate_points).  One packed upload, three launches, one download; the first launch has room for an
    estimate of the result, a batch that holds more runs exactly once more, with exact room.
    Curves of fewer than 2 points, with a non-finite coordinate or one beyond CURVES_MAX_COORD, with a count below
    1, of another shape than (n, 2), and curves the device refuses (VA_CURVES_MAX_STEPS) go through the host
    function one by one, in order.  A spacing that is not a positive finite number is a ValueError.
    Returns the list of (K, 2) float64 arrays; ret_lengths appends the (m,) float64 curves.curve_length of each
    result."""
    what = "curves_equidistant"
    curves = list(curves)
    m = len(curves)
    spacings, counts = _per_curve(spacing, m, what, "spacing"), _per_curve(count, m, what, "count")
    for s in spacings:
        if s is not None and not (s > 0 and math.isfinite(s)):
            raise ValueError("%s: a spacing must be a positive finite number, got %r" % (what, s))
    shifts = None
    if offsets is not None:
        shifts = np.asarray(offsets, np.float64).reshape(-1, 2)
        if len(shifts) != m:
            raise ValueError("%s: %d offsets for %d curves" % (what, len(shifts), m))
    results, lengths = [None] * m, np.zeros(m, np.float64)

    def on_host(k):
        results[k], lengths[k] = _curve_on_host(curves[k], spacings[k], counts[k],
                                                None if shifts is None else shifts[k])

    # what the device takes -- (n, 2) with 2 <= n, finite coordinates within CURVES_MAX_COORD, a count it can hold --
    # is kept; the rest goes through the host function now, in order
    dev, arrs = [], []
    for k in range(m):
        a = np.asarray(curves[k], np.float64)
        ct = counts[k]
        if (a.ndim == 2 and a.shape[1] == 2 and 2 <= len(a) <= CURVES_MAX_POINTS
                and (spacings[k] is not None or ct is None or 1 <= ct < 2 ** 31)
                and bool((np.abs(a) <= CURVES_MAX_COORD).all())):                 # (a NaN fails the comparison)
            dev.append(k)
            arrs.append(a)
        else:
            on_host(k)
    if dev:
        md = len(dev)
        flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
        npts, first = shapes[:, 0].astype(np.int64), np.append(offsets, total) // 2
        sp = np.array([0.0 if spacings[k] is None else float(spacings[k]) for k in dev])
        ct = np.array([n if counts[k] is None else int(counts[k]) for k, n in zip(dev, npts)], np.int64)
        walked = sp > 0
        # room of the first launch: the counts, and for a walked curve an estimate of its result from the float64
        # polyline length (the sizes themselves come from the count pass; what the walk may not exceed bounds it)
        xy = flat.reshape(-1, 2)
        seg = np.append(np.hypot(*(xy[1:] - xy[:-1]).T), 0.0)
        seg[first[1:] - 1] = 0.0
        steps = np.minimum(np.add.reduceat(seg, first[:-1]) * (1 + 1e-5) / np.where(walked, sp, 1.0),
                           2.0 * CURVES_MAX_STEPS)
        room = int(np.where(walked, np.maximum(np.floor(steps).astype(np.int64) + CURVES_ROOM_SLACK, npts), ct).sum())
        # one packed upload: [point offsets | spacings | translations | points | counts]
        ins = _Layout(off=first.astype(np.int64), sp=sp,
                      tr=np.ascontiguousarray(shifts[dev]) if shifts is not None else np.zeros(0),
                      pts=flat, ct=np.where(walked, 0, ct).astype(np.int32))
        L = _hip.lib()
        with _Lease.on(stream) as d:
            src = d.upload(ins.packed())

            def run(cap):
                # one output buffer: [total | out offsets | in lengths | out lengths | counts | status | points]
                outs = _Layout(total=(1, np.int64), off=(md + 1, np.int64), lin=(md, np.float64),
                               lout=(md, np.float64), cnt=(md, np.int32), st=(md, np.int32),
                               pts=(2 * max(cap, 1), np.float64))
                out = d.take(outs.nbytes)
                check(L.va_curves_equidistant(ins.ptr(src, "pts"), ins.ptr(src, "off"), total // 2, md,
                                              ins.ptr(src, "sp"), ins.ptr(src, "ct"),
                                              ins.ptr(src, "tr") if shifts is not None else None,
                                              outs.ptr(out, "cnt"), outs.ptr(out, "off"), outs.ptr(out, "lin"),
                                              outs.ptr(out, "st"), outs.ptr(out, "total"), outs.ptr(out, "pts"), cap,
                                              outs.ptr(out, "lout"), stream))
                raw = out.download((outs.nbytes,), np.uint8, stream)
                return (outs, raw), outs.view(raw, "total")
            (outs, raw), needs = _rerun(run, room)         # a need beyond the room: nothing was written
        found = int(needs[0])
        out_off, out_len, status = (outs.view(raw, name) for name in ("off", "lout", "st"))
        pts = outs.view(raw, "pts")[:2 * found].reshape(found, 2).copy()
        for j, k in enumerate(dev):
            if status[j] != 0:                 # (VA_CURVES_MAX_STEPS: the reference's own walk, as slow as it is)
                on_host(k)
            else:
                results[k], lengths[k] = pts[out_off[j]:out_off[j + 1]], out_len[j]
    return (results, lengths) if ret_lengths else results


# ------------------------------------------------------------------------------------------ simplification
SIMPLIFY_MAX_POINTS = 1 << 24    # VA_SIMPLIFY_MAX_POINTS, include/videoanalysis_hip.h
SIMPLIFY_METHODS = ("rdp", "visvalingam")
# simplify_curves goes to the device from this many curves on; below it the pinned definition in Python is quicker
# than a device round trip ("Simplification": the crossover)
SIMPLIFY_DEVICE_MIN_BATCH = 4


def _rdp_keep_host(P, eps):
    """the pinned Ramer-Douglas-Peucker ("Simplification") on one (n, 2) float64 curve, a span at a
    time in NumPy: every product, difference, root and quotient is rounded on its own, as on the device.  Returns
    the kept flags (bool, one per point)"""
    n = len(P)
    keep = np.zeros(n, bool)
    if n < 3:
        keep[:] = True
        return keep
    keep[0] = keep[-1] = True
    tol = eps if eps > 0 else 0.0
    x, y = P[:, 0], P[:, 1]
    todo = [(0, n - 1)]
    with np.errstate(all="ignore"):
        while todo:
            i0, i1 = todo.pop()
            if i1 - i0 < 2:
                continue
            if x[i0] == x[i1]:
                d = np.abs(x[i0 + 1:i1] - x[i0])
            else:
                ax, ay = x[i1] - x[i0], y[i1] - y[i0]
                bx, by = x[i0] - x[i0 + 1:i1], y[i0] - y[i0 + 1:i1]
                d = np.abs(ax * by - ay * bx) / np.sqrt(ax * ax + ay * ay)
            d = np.where(d > 0, d, 0.0)                # (a NaN distance is never the largest)
            k = int(np.argmax(d))                      # the first of the largest
            if d[k] > tol:
                keep[i0 + 1 + k] = True
                todo.append((i0, i0 + 1 + k))
                todo.append((i0 + 1 + k, i1))
    return keep


def _visvalingam_keep_host(P, thr, closed):
    """the pinned Visvalingam procedure ("Simplification") on one (n, 2) float64 ring (closed, no
    closing duplicate) or open line, with Python floats: a heap of point indices, prev / next links and heapq's two
    sift procedures, the areas measured afresh at every comparison.  Returns the kept flags (bool); a ring of fewer
    than 3 points, or left with fewer than 3, keeps none"""
    n = len(P)
    keep = np.zeros(n, bool)
    if n < 3:
        keep[:] = not closed
        return keep
    xs, ys = P[:, 0].tolist(), P[:, 1].tolist()
    prev = [i - 1 if i > 0 else (n - 1 if closed else 0) for i in range(n)]
    nxt = [i + 1 if i + 1 < n else (0 if closed else n - 1) for i in range(n)]
    heap = list(range(n)) if closed else list(range(1, n - 1))

    def area(i):
        b, a = prev[i], nxt[i]
        return abs(xs[i] * (ys[b] - ys[a]) + xs[b] * (ys[a] - ys[i]) + xs[a] * (ys[i] - ys[b])) / 2.0

    def siftdown(startpos, pos):
        item = heap[pos]
        while pos > startpos:
            parentpos = (pos - 1) >> 1
            parent = heap[parentpos]
            if not area(item) < area(parent):
                break
            heap[pos] = parent
            pos = parentpos
        heap[pos] = item

    def siftup(pos):
        end, startpos, item = len(heap), pos, heap[pos]
        childpos = 2 * pos + 1
        while childpos < end:
            rightpos = childpos + 1
            if rightpos < end and not area(heap[childpos]) < area(heap[rightpos]):
                childpos = rightpos
            heap[pos] = heap[childpos]
            pos = childpos
            childpos = 2 * pos + 1
        heap[pos] = item
        siftdown(startpos, pos)

    for i in reversed(range(len(heap) // 2)):
        siftup(i)
    floor = 2 if closed else 0
    while len(heap) > floor:
        top = heap[0]
        if area(top) >= thr:
            break
        b, a = prev[top], nxt[top]
        nxt[b] = a
        prev[a] = b
        last = heap.pop()
        if heap:
            heap[0] = last
            siftup(0)
    if closed and len(heap) < 3:
        return keep
    keep[heap] = True
    if not closed:
        keep[0] = keep[-1] = True
    return keep


def _simplify_on_host(points, tolerance, method, closed):
    """the kept flags of one curve by the pinned definition in Python"""
    P = np.asarray(points, np.float64).reshape(-1, 2)
    if method == "rdp":
        return _rdp_keep_host(P, float(tolerance))
    return _visvalingam_keep_host(P, float(tolerance), closed)


def simplify_curves(curves, tolerance, method="rdp", closed=False, stream=None):
    """Simplifies every curve of a list in one device call ("Simplification").  method "rdp":
    Ramer-Douglas-Peucker on open curves (curves.simplify_curve's algorithm with the pinned distance,
    va_simplify_rdp), tolerance the largest distance a dropped point may have from its chord.  method
    "visvalingam": the reference's heap procedure (regions.simplify_contour, va_simplify_visvalingam), tolerance the
    triangle area below which a point goes; closed=True takes every curve as a ring without a closing duplicate,
    closed=False as an open line with fixed ends.  curves: m (n, 2) array-likes of any lengths; tolerance: one number
    or one per curve.  One packed upload, one call, one download of the flags and counts.
    Returns a list with, per curve, the kept rows of the array as it was given, so its dtype survives; a ring that
    vanishes (fewer than 3 points are left, or were given) is None.
    Curves with a non-finite coordinate or an integer of 2^53 and beyond, of a dtype that is neither integer nor
    float, curves the device refuses (a NaN tolerance, more than SIMPLIFY_MAX_POINTS points), empty curves and every
    curve of a batch below SIMPLIFY_DEVICE_MIN_BATCH go through the same definition in Python
    (_simplify_on_host, not curves.simplify_curve), which gives the same flags.  A curve of
    another shape than (n, 2), an unknown method and closed=True with "rdp" are a ValueError."""
    what = "simplify_curves"
    if method not in SIMPLIFY_METHODS:
        raise ValueError("%s: method is one of %s, got %r" % (what, SIMPLIFY_METHODS, method))
    if closed and method == "rdp":
        raise ValueError("%s: Ramer-Douglas-Peucker takes open curves (closed=False)" % what)
    curves = list(curves)
    m = len(curves)
    tolerances = _per_curve(tolerance, m, what, "tolerance")
    if any(t is None for t in tolerances):
        raise ValueError("%s: a tolerance is a number, got None" % what)
    given, flags = [], [None] * m
    dev, arrs = [], []
    for k in range(m):
        a = np.asarray(curves[k])
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("%s: curve %d has shape %r, expected (n, 2)" % (what, k, a.shape))
        given.append(a)
        kind = a.dtype.kind
        if not 0 < len(a) <= SIMPLIFY_MAX_POINTS or tolerances[k] != tolerances[k] or kind not in "iuf":
            continue
        if kind != "f" and a.dtype.itemsize > 4 and int(np.abs(a).max()) >= 2 ** 53:
            continue
        if kind == "f" and not np.isfinite(a).all():
            continue
        dev.append(k)
        arrs.append(a)
    if len(dev) >= max(SIMPLIFY_DEVICE_MIN_BATCH, 1):
        md = len(dev)
        if len({a.dtype for a in arrs}) > 1:           # (each converted on its own: no promotion among them)
            arrs = [a.astype(np.float64) for a in arrs]
        flat, shapes, offsets, sizes, total = _pack_ragged(arrs)
        flat = flat.astype(np.float64, copy=False)
        npoints = total // 2
        first = np.append(offsets, total) // 2
        tol = np.array([float(tolerances[k]) for k in dev], np.float64)
        # one packed upload: [point offsets | tolerances | points]; one output buffer: [counts | status | flags]
        ins = _Layout(off=first.astype(np.int64), tol=tol, pts=flat)
        outs = _Layout(cnt=(md, np.int32), st=(md, np.int32), keep=(npoints, np.uint8))
        L = _hip.lib()
        with _Lease.on(stream) as d:
            src = d.upload(ins.packed())
            out = d.take(outs.nbytes)
            operands = (ins.ptr(src, "pts"), ins.ptr(src, "off"), npoints, md, ins.ptr(src, "tol"))
            results = (outs.ptr(out, "keep"), outs.ptr(out, "cnt"), outs.ptr(out, "st"))
            if method == "rdp":
                check(L.va_simplify_rdp(*operands, *results, stream))
            else:
                need = L.va_simplify_visvalingam_workspace_bytes(npoints)
                ws = d.take(need)
                check(L.va_simplify_visvalingam(*operands, 1 if closed else 0, *results, ws.ptr, need, stream))
            raw = out.download((outs.nbytes,), np.uint8, stream)
        status = outs.view(raw, "st")
        keep = outs.view(raw, "keep") != 0
        run, bounds = (status == 0).tolist(), first.tolist()
        for j, k in enumerate(dev):
            if run[j]:
                flags[k] = keep[bounds[j]:bounds[j + 1]]
    results = []
    for k in range(m):
        kept = flags[k] if flags[k] is not None else _simplify_on_host(given[k], tolerances[k], method, closed)
        results.append(None if closed and not kept.any() else given[k][kept])
    return results


# ------------------------------------------------------------------------------------------------ composer
COMPOSE_CHANNELS = {0: 0, "r": 0, "red": 0, 1: 1, "g": 1, "green": 1, 2: 2, "b": 2, "blue": 2}   # composer.py:43-45
COMPOSE_LAYER_DTYPE = np.dtype([("kind", np.int32), ("image_channels", np.int32), ("channel", np.int32),
                                ("reserved", np.int32), ("image_off", np.int64), ("mask_off", np.int64),
                                ("factor", np.float64), ("alpha", np.float32), ("beta", np.float32)])   # va_compose_layer
DRAW_CMD_DTYPE = np.dtype([("kind", np.int32), ("flags", np.int32), ("color", np.uint32), ("radius", np.int32),
                           ("cx", np.int32), ("cy", np.int32), ("count", np.int32), ("reserved", np.int32),
                           ("first", np.int64)])                                                        # va_draw_cmd
_COMPOSE_KINDS = {"highlight": 1, "add": 2, "blend": 3}      # VA_COMPOSE_*, VA_DRAW_*, include/videoanalysis_hip.h
_DRAW_POLYLINE, _DRAW_CIRCLE = 1, 2
DRAW_MAX_COORD = FILL_MAX_COORD


class DeviceFrames(object):
    """a uint8 frame stack (n, h, w) or (n, h, w, 3) that stays on the device between compose_layers and draw calls
    (keep=True); download() copies it to the host, release() hands its buffer back to the pool (the caller has
    synchronised by then: download() does)"""

    def __init__(self, buf, n, h, w, c):
        self.buf, self.n, self.h, self.w, self.c = buf, n, h, w, c

    @property
    def shape(self):
        return (self.n, self.h, self.w) + ((3,) if self.c == 3 else ())

    @property
    def nbytes(self):
        return self.n * self.h * self.w * self.c

    @classmethod
    def upload(cls, frames, stream=None):
        arr, n, h, w, c = _frame_stack(frames, "DeviceFrames.upload")
        with _Lease.on(stream) as d:
            buf = d.result(max(arr.nbytes, 1))
            buf.upload(arr, stream)
            return cls(buf, n, h, w, c)

    def download(self, stream=None):
        return self.buf.download(self.shape, np.uint8, stream)

    def gather(self, indices, stream=None):
        """a new DeviceFrames of the frames `indices` of this one, in that order (the caller's, like an upload):
        device-to-device copies, one per run of consecutive frames; synchronises the stream"""
        idx = [int(i) for i in indices]
        if any(not 0 <= i < self.n for i in idx):
            raise IndexError("DeviceFrames.gather: frames are 0 .. %d, got %r" % (self.n - 1, idx))
        frame = self.h * self.w * self.c
        with _Lease.on(stream) as d:
            out = DeviceFrames(d.result(max(len(idx) * frame, 1)), len(idx), self.h, self.w, self.c)
            L, k = _hip.lib(), 0
            while k < len(idx) and frame:
                run = 1
                while k + run < len(idx) and idx[k + run] == idx[k] + run:
                    run += 1
                check(L.va_memcpy_d2d(out.buf.ptr + k * frame, self.buf.ptr + idx[k] * frame, run * frame, stream))
                k += run
            check(L.va_stream_sync(stream))
            return out

    def release(self, into=None):
        buf, self.buf = self.buf, None
        if buf is not None:
            (_give if into is None else into.absorb)(buf)      # into: a lease, which gives it back with its own


def _frame_stack(frames, what):
    """(contiguous uint8 array, n, h, w, c) of a stack (n, h, w) or (n, h, w, 3)"""
    arr = np.asarray(frames)
    if arr.dtype != np.uint8:
        raise TypeError("%s: frames are uint8, got %s" % (what, arr.dtype))
    if not (arr.ndim == 3 or (arr.ndim == 4 and arr.shape[3] == 3)):
        raise ValueError("%s: frames are a stack (n, h, w) or (n, h, w, 3), got shape %r" % (what, arr.shape))
    return (np.ascontiguousarray(arr),) + tuple(arr.shape[:3]) + (1 if arr.ndim == 3 else 3,)


def _frames_in(frames, what):
    """(src, n, h, w, c, owned): the caller's DeviceFrames, or the _frame_stack array the call uploads itself (owned)"""
    if isinstance(frames, DeviceFrames):
        return frames, frames.n, frames.h, frames.w, frames.c, False
    return _frame_stack(frames, what) + (True,)


def _frames_on_device(d, src, owned):
    """the DeviceFrames of `src` (_frames_in); one the call uploads itself is a result of the lease `d`"""
    if owned:
        src = DeviceFrames.upload(src, d.stream)
        d.adopt(src.buf)
    return src


def _frames_out(d, stack, keep):
    """the tail of the ops that return frames, in their lease `d`: the stack under keep, else its download and release"""
    if keep:
        return stack
    out = stack.download(d.stream)
    stack.release(into=d)
    return out


class _BytePacker(object):
    """byte planes of one call in one buffer, each at a 16-byte boundary; the same array object is stored once"""

    def __init__(self):
        self.parts, self.nbytes, self.seen = [], 0, {}

    def add(self, arr, origin=None):
        origin = arr if origin is None else origin           # what the caller handed in, of which arr is the bytes
        key = id(origin)
        if key not in self.seen:
            flat = np.ascontiguousarray(arr, np.uint8).reshape(-1)
            pad = -len(flat) % 16
            self.seen[key] = (self.nbytes, origin)           # (the reference keeps the id alive)
            self.parts += [flat, np.zeros(pad, np.uint8)] if pad else [flat]
            self.nbytes += len(flat) + pad
        return self.seen[key][0]

    def packed(self):
        return np.concatenate(self.parts) if self.parts else None


def _compose_tables(layers, n, h, w, c, what):
    """the checked operands of va_compose_layers_u8: (records, layer_off, images, masks), the last two packed byte
    arrays or None, or the DeviceFrames whose planes the layers name as (DeviceFrames, index); raises as
    compose_layers documents"""
    if len(layers) != n:
        raise ValueError("%s: need one layer list per frame (%d frames, %d lists)" % (what, n, len(layers)))
    images, masks, recs = _BytePacker(), _BytePacker(), []
    off = np.zeros(n + 1, np.int64)

    device = {"mask": None, "image": None}       # the one DeviceFrames the call's device planes of a role come from

    def device_plane(operand, role):
        """(byte offset, channels) of the plane (DeviceFrames, index)"""
        stack, index = operand
        if isinstance(index, (bool, np.bool_)) or int(index) != index or not 0 <= index < stack.n:
            raise ValueError("%s: a device %s is plane 0 .. %d of its stack, got %r" % (what, role, stack.n - 1, index))
        if device[role] is None:
            device[role] = stack
        elif device[role] is not stack:
            raise ValueError("%s: all device %ss of one call must come from one DeviceFrames" % (what, role))
        return int(index) * h * w * stack.c, stack.c

    def is_device(operand):
        return isinstance(operand, tuple) and len(operand) == 2 and isinstance(operand[0], DeviceFrames)

    def mask_of(mask):
        if mask is None:
            return -1
        if is_device(mask):
            if (mask[0].h, mask[0].w, mask[0].c) != (h, w, 1):
                raise ValueError("%s: a mask of shape %r on frames of %r" % (what, mask[0].shape[1:], (h, w)))
            return device_plane(mask, "mask")[0]
        m = np.asarray(mask)
        if m.shape != (h, w):
            raise ValueError("%s: a mask of shape %r on frames of %r" % (what, m.shape, (h, w)))
        origin = mask if isinstance(mask, np.ndarray) else m
        if m.dtype != np.uint8:                  # non-zero is what counts; uint8 masks go as they are
            m = (m != 0).view(np.uint8)
        return masks.add(m, origin)

    def image_of(image):
        if is_device(image):
            if (image[0].h, image[0].w) != (h, w):
                raise ValueError("The two images to be added must have the same size")
            if image[0].c == 3 and c == 1:
                raise ValueError("Cannot add a color image to a monochrome one")
            return device_plane(image, "image")
        im = np.asarray(image)
        if im.dtype != np.uint8:
            raise TypeError("%s: images are uint8, got %s" % (what, im.dtype))
        if im.shape[:2] != (h, w) or not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
            raise ValueError("The two images to be added must have the same size")
        if im.ndim == 3 and c == 1:
            raise ValueError("Cannot add a color image to a monochrome one")
        return images.add(im, image if isinstance(image, np.ndarray) else im), (3 if im.ndim == 3 else 1)

    for f, frame_layers in enumerate(layers):
        for layer in frame_layers:
            kind = layer[0]
            rec = np.zeros((), COMPOSE_LAYER_DTYPE)
            rec["mask_off"] = -1
            if kind == "highlight":
                _, mask, channel, strength = layer
                if channel is None or (isinstance(channel, str) and channel == "all"):
                    channel = -1
                elif c == 1:
                    raise ValueError("Highlighting a specific channel is only supported for color videos.")
                else:
                    try:
                        channel = COMPOSE_CHANNELS[channel]
                    except (KeyError, TypeError):
                        raise ValueError("Unknown value `%s` for channel." % (channel,))
                if isinstance(strength, (bool, np.bool_)) or int(strength) != strength or not 0 <= strength <= 255:
                    raise ValueError("%s: the strength is an integer in 0 .. 255, got %r" % (what, strength))
                if mask is None:
                    raise ValueError("%s: a highlight needs a mask" % what)
                rec["channel"], rec["alpha"] = channel, float(int(strength))
                rec["factor"] = (255 - int(strength)) / 255
                rec["mask_off"] = mask_of(mask)
            elif kind == "add":
                _, image, mask = layer
                rec["image_off"], rec["image_channels"] = image_of(image)
                rec["mask_off"] = mask_of(mask)
            elif kind == "blend":
                _, image, weight, mask = layer
                weight = float(weight)
                if not math.isfinite(weight):
                    raise ValueError("%s: the weight must be finite, got %r" % (what, weight))
                rec["image_off"], rec["image_channels"] = image_of(image)
                rec["alpha"], rec["beta"] = np.float32(1 - weight), np.float32(weight)
                rec["mask_off"] = mask_of(mask)
            else:
                raise ValueError("%s: unknown layer %r" % (what, kind))
            rec["kind"] = _COMPOSE_KINDS[kind]
            recs.append(rec)
        off[f + 1] = len(recs)
    table = np.array(recs, COMPOSE_LAYER_DTYPE) if recs else np.zeros(0, COMPOSE_LAYER_DTYPE)
    for role, packer in (("mask", masks), ("image", images)):
        if device[role] is not None and packer.parts:
            raise ValueError("%s: device and host %ss in one call (the entry point takes one %ss buffer)"
                             % (what, role, role))
    return (table, off, device["image"] if device["image"] is not None else images.packed(),
            device["mask"] if device["mask"] is not None else masks.packed())


def compose_layers(frames, layers, color=None, keep=False, stream=None):
    """the pixel layers of VideoComposer (video/io/composer.py:103-105, :131-210) on a whole stack in one
    va_compose_layers_u8 launch ("Composer").  frames: uint8 (n, h, w) or (n, h, w, 3), or a
    DeviceFrames of an earlier call.  layers: one list per frame of
        ('highlight', mask, channel, strength)   channel None / 'all' or one of COMPOSE_CHANNELS; strength 0 .. 255
        ('add', image, mask)                     saturating add; mask None: everywhere
        ('blend', image, weight, mask)           cv2.addWeighted(frame, 1 - weight, image, weight, 0)
    applied in order; masks (h, w), taken as non-zero; images uint8 (h, w) or (h, w, 3).  color: None keeps the
    channels of the frames, True writes a colour stack (a monochrome frame is copied into the three channels first),
    False asks for a monochrome one.  An array that appears in several layers is uploaded once.  A mask or an image
    may be the pair (DeviceFrames, index): plane `index` of a stack that is already on the device (masks monochrome,
    taken as non-zero) and stays the caller's.  All device masks of one call come from one DeviceFrames, and so do all
    device images; device and host planes of the same role in one call are a ValueError.
    ValueError, before anything is launched: a size mismatch, a colour image or colour frames on a monochrome
    result, a channel on a monochrome stack, an unknown channel or layer, a strength outside 0 .. 255.
    Returns the composed stack; keep=True returns a DeviceFrames instead (a DeviceFrames handed in with the same
    channels is composed in place and returned; otherwise it is released)."""
    what = "compose_layers"
    frames, n, h, w, c_src, owned = _frames_in(frames, what)
    c = c_src if color is None else (3 if color else 1)
    if c_src == 3 and c == 1:
        raise ValueError("Cannot copy a color image into a monochrome video.")
    table, off, images, masks = _compose_tables(list(layers), n, h, w, c, what)
    if n == 0 or h == 0 or w == 0:
        out = np.zeros((n, h, w) + ((3,) if c == 3 else ()), np.uint8)
        if not owned:
            frames.release()
        return DeviceFrames.upload(out, stream) if keep else out
    L = _hip.lib()
    with _Lease.on(stream) as d:
        src = _frames_on_device(d, frames, owned)
        dst = src if c == c_src else DeviceFrames(d.result(n * h * w * c), n, h, w, c)
        tb, ob = d.upload(table) if len(table) else None, d.upload(off)
        (ib, ibytes), (mb, mbytes) = ((x.buf, x.nbytes) if isinstance(x, DeviceFrames) else
                                      (d.upload(x), 0 if x is None else len(x)) for x in (images, masks))
        check(L.va_compose_layers_u8(src.buf.ptr, c_src, dst.buf.ptr, n, h, w, c, _ptr(tb), ob.ptr, len(table),
                                     _ptr(ib), ibytes, _ptr(mb), mbytes, stream))
        if keep:                           # the tables go back to the pool: the launch must have read them
            check(L.va_stream_sync(stream))
        out = _frames_out(d, dst, keep)
        if dst is not src:
            src.release(into=d)
        return out


def _draw_color(color, c, what):
    """the uint32 of a command's colour: one byte on a monochrome stack, R | G << 8 | B << 16 on a colour one"""
    vals = [int(v) for v in np.atleast_1d(np.asarray(color)).reshape(-1)]
    if len(vals) == 1 and c == 3:
        vals = vals * 3
    if len(vals) != c:
        raise ValueError("%s: a colour of %d values on frames of %d channel(s)" % (what, len(vals), c))
    if any(not 0 <= v <= 255 for v in vals):
        raise ValueError("%s: colour values are 0 .. 255, got %r" % (what, color))
    return sum(v << (8 * i) for i, v in enumerate(vals))


def _draw_tables(commands, n, c, what):
    """the checked operands of va_draw_u8: (records, cmd_off, points int32 (k, 2))"""
    if len(commands) != n:
        raise ValueError("%s: need one command list per frame (%d frames, %d lists)" % (what, n, len(commands)))
    recs, pts, npts = [], [], 0
    off = np.zeros(n + 1, np.int64)
    for f, frame_cmds in enumerate(commands):
        for cmd in frame_cmds:
            rec = np.zeros((), DRAW_CMD_DTYPE)
            if cmd[0] == "polyline":
                _, points, closed, color = cmd
                p = np.asarray(points)
                if p.size and not np.issubdtype(p.dtype, np.integer):
                    raise TypeError("%s: polylines hold integer points, got %s" % (what, p.dtype))
                if p.size % 2:
                    raise ValueError("%s: a polyline is (k, 2) or (k, 1, 2) points, got shape %r" % (what, p.shape))
                p = p.reshape(-1, 2).astype(np.int64)
                if p.size and np.abs(p).max() > DRAW_MAX_COORD:
                    raise ValueError("%s: a coordinate is beyond +-%d" % (what, DRAW_MAX_COORD))
                rec["kind"], rec["flags"], rec["first"], rec["count"] = _DRAW_POLYLINE, bool(closed), npts, len(p)
                pts.append(p.astype(np.int32))
                npts += len(p)
            elif cmd[0] == "circle":
                _, center, radius, filled, color = cmd
                cx, cy, radius = int(center[0]), int(center[1]), int(radius)
                if max(abs(cx), abs(cy), abs(radius)) > DRAW_MAX_COORD:
                    raise ValueError("%s: a coordinate is beyond +-%d" % (what, DRAW_MAX_COORD))
                rec["kind"], rec["flags"], rec["cx"], rec["cy"], rec["radius"] = _DRAW_CIRCLE, bool(filled), cx, cy, radius
            else:
                raise ValueError("%s: unknown command %r" % (what, cmd[0]))
            rec["color"] = _draw_color(color, c, what)
            recs.append(rec)
        off[f + 1] = len(recs)
    table = np.array(recs, DRAW_CMD_DTYPE) if recs else np.zeros(0, DRAW_CMD_DTYPE)
    points = np.concatenate(pts) if npts else np.zeros((0, 2), np.int32)
    return table, off, np.ascontiguousarray(points, np.int32)


def _drawn(frames, owned, launch, keep, stream):
    """the body draw and draw_contours share, for frames as _frames_in gives them: launch(lease, DeviceFrames) draws
    in place (None: there is nothing to draw), and the stack comes back as _frames_out returns it"""
    if launch is None and owned and not keep:
        return frames.copy()
    with _Lease.on(stream) as d:
        dst = _frames_on_device(d, frames, owned)
        if launch is not None:
            launch(d, dst)
        return _frames_out(d, dst, keep)


def draw(frames, commands, keep=False, stream=None):
    """the thickness-1 drawing of VideoComposer (cv2.drawContours, polylines, rectangle, circle;
    video/io/composer.py:236, :257, :284, :298) on a whole stack in one va_draw_u8 launch, one workgroup per frame
    ("Composer").  frames: uint8 (n, h, w) or (n, h, w, 3), or a DeviceFrames.  commands: one list per
    frame of
        ('polyline', points, closed, color)           points (k, 2) or (k, 1, 2) integers, as find_contours returns
        ('circle', center, radius, filled, color)     OpenCV's integer circle; a negative radius draws nothing
    drawn in list order: the last command that covers a pixel decides it.  color: one value on a monochrome stack,
    (r, g, b) on a colour one (one value counts for all three).
    ValueError, before anything is launched: a coordinate or radius beyond +-DRAW_MAX_COORD, a colour outside
    0 .. 255 or of the wrong length, an unknown command; RuntimeError: a frame the device refused.
    Returns the stack; keep=True returns a DeviceFrames (the one handed in, drawn in place).  A DeviceFrames handed
    in without keep is downloaded and released."""
    what = "draw"
    frames, n, h, w, c, owned = _frames_in(frames, what)
    table, off, points = _draw_tables(list(commands), n, c, what)

    def launch(d, dst):
        tb, ob, pb, st = d.upload(table), d.upload(off), d.upload(points) if len(points) else None, d.take(n * 4)
        check(_hip.lib().va_draw_u8(dst.buf.ptr, n, h, w, c, tb.ptr, ob.ptr, len(table), _ptr(pb), len(points),
                                    st.ptr, stream))
        status = st.download((n,), np.int32, stream)
        bad = np.flatnonzero(status != 0)
        if len(bad):
            raise RuntimeError("%s: the device refused frame %d (status %d)" % (what, bad[0], status[bad[0]]))
    return _drawn(frames, owned, launch if len(table) else None, keep, stream)


def _frame_map(frame_map, n_src, n_out, what):
    """the checked int32 map of draw_contours, or None"""
    if frame_map is None:
        if n_src != n_out:
            raise ValueError("%s: contours of %d frames on %d frames need a frame_map" % (what, n_src, n_out))
        return None
    fm = np.asarray(frame_map)
    if fm.ndim != 1 or len(fm) != n_src:
        raise ValueError("%s: frame_map holds one entry per source frame (%d), got shape %r" % (what, n_src, fm.shape))
    if fm.size and not np.issubdtype(fm.dtype, np.integer):
        raise ValueError("%s: frame_map holds integers, got %s" % (what, fm.dtype))
    if fm.size and (fm.min() < -1 or fm.max() >= n_out):
        raise ValueError("%s: frame_map values are -1 .. %d" % (what, n_out - 1))
    return np.ascontiguousarray(fm, np.int32)


def draw_contours(frames, contours, color, frame_map=None, keep=False, stream=None):
    """every contour of a DeviceContours (find_contours(..., keep=True)) as a closed polyline of thickness 1 in one
    colour, in one chip-wide va_draw_contours_u8 launch (video/io/composer.py:228-237; DESIGN.md §9, "Annotating on
    the device"): the bytes of ops.draw with one closed polyline per contour, without the host lists.  frames: uint8
    (n, h, w) or (n, h, w, 3), or a DeviceFrames; color as for ops.draw.  frame_map: None (source frame f is drawn
    into frame f) or one integer per source frame, the frame it is drawn into or -1 for "not drawn".
    ValueError, before anything is launched: frames of another size than the contours', a frame_map of the wrong
    length or with a value outside -1 .. n - 1, a bad colour; RuntimeError: a non-zero device status.
    Returns the stack; keep=True returns a DeviceFrames (the one handed in, drawn in place).  A DeviceFrames handed
    in without keep is downloaded and released."""
    what = "draw_contours"
    frames, n, h, w, c, owned = _frames_in(frames, what)
    if not isinstance(contours, DeviceContours):
        raise TypeError("%s: contours are a DeviceContours, got %s" % (what, type(contours).__name__))
    if (contours.h, contours.w) != (h, w):
        raise ValueError("%s: contours of frames of %r on frames of %r" % (what, (contours.h, contours.w), (h, w)))
    packed = _draw_color(color, c, what)
    fm = _frame_map(frame_map, contours.n, n, what)

    def launch(d, dst):
        mb, st = d.upload(fm), d.take(4)
        check(_hip.lib().va_draw_contours_u8(dst.buf.ptr, n, h, w, c, contours.info.ptr, contours.point_off.ptr,
                                             contours.ncontours, contours.points.ptr, contours.npoints,
                                             _ptr(mb), contours.n, packed, st.ptr, stream))
        status = int(st.download((1,), np.int32, stream)[0])
        if status:
            raise RuntimeError("%s: the device refused a contour (status %d)" % (what, status))
    return _drawn(frames, owned, launch if contours.ncontours else None, keep, stream)


# ------------------------------------------------------------------------------------------------ Motion-JPEG
# ITU T.81 Annex K.1 / K.2 (natural order) and K.3 - K.6 as (BITS, HUFFVAL), keyed by the DHT byte Tc << 4 | Th
_JPEG_BASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_AC_COMMON = (
    0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a,
    0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a)
_JPEG_AC_HIGH = (
    0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda)
JPEG_DHT = {
    0x00: ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    0x10: ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
           (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
            0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
            0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a) + _JPEG_AC_COMMON + _JPEG_AC_HIGH
           + (0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
              0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    0x01: ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    0x11: ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
           (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
            0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
            0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a) + _JPEG_AC_COMMON[18:] + (0x82,)
           + _JPEG_AC_HIGH + (0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
                              0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
}
JPEG_MAX_SIDE = 65535            # SOF0 holds 16-bit sizes
JPEG_ROOM_DIVISOR = 4            # the first launch has room for the headers and a quarter of the raw bytes


def jpeg_tables(quality):
    """the (luma, chroma) quantisation tables of `quality` 1 .. 100 in natural order, uint8 (64,) each: the Annex K
    base tables under the IJG scaling, clip((base * scale + 50) // 100, 1, 255) with scale = 5000 // q below 50 and
    200 - 2 q from 50 on (host only)"""
    if isinstance(quality, (bool, np.bool_)) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError("jpeg_tables: the quality is an integer in 1 .. 100, got %r" % (quality,))
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint8)
                 for base in _JPEG_BASE)


def _jpeg_segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


JPEG_SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}      # the luma sampling (H, V) of a layout


def jpeg_sampling(sampling, c=3, what="jpeg_sampling"):
    """the luma sampling (H, V) of `sampling`: (1, 1), (2, 1), (2, 2) or "4:4:4", "4:2:2", "4:2:0"; a ValueError for
    anything else and for a subsampled layout of c = 1 component (host only)"""
    hv = JPEG_SAMPLINGS.get(sampling) if isinstance(sampling, str) else None
    if hv is None and isinstance(sampling, (tuple, list)) and len(sampling) == 2:
        if all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in sampling):
            hv = (int(sampling[0]), int(sampling[1]))
    if hv not in JPEG_SAMPLINGS.values():
        raise ValueError("%s: the sampling is (1, 1), (2, 1), (2, 2), '4:4:4', '4:2:2' or '4:2:0', got %r"
                         % (what, sampling))
    if c == 1 and hv != (1, 1):
        raise ValueError("%s: monochrome frames have no chroma to subsample (sampling %r)" % (what, sampling))
    return hv


def jpeg_header(h, w, c, quality, sampling=(1, 1)):
    """the bytes SOI .. SOS every frame's file starts with ("Motion-JPEG"): APP0 JFIF 1.01, one DQT per
    table, SOF0 with luma sampling `sampling` (Cb and Cr 1 x 1), one DHT per Annex K table (DC0, AC0 and, in colour,
    DC1, AC1), DRI = the MCUs of a row, ceil(w / 8 H), SOS (host only)"""
    h, w, c = int(h), int(w), int(c)
    hh, vv = jpeg_sampling(sampling, what="jpeg_header")
    if not (1 <= h <= JPEG_MAX_SIDE and 1 <= w <= JPEG_MAX_SIDE):
        raise ValueError("jpeg_header: sides are 1 .. %d, got %d x %d" % (JPEG_MAX_SIDE, w, h))
    if c not in (1, 3):
        raise ValueError("jpeg_header: 1 or 3 components, got %d" % c)
    jpeg_sampling(sampling, c, "jpeg_header")
    tables = jpeg_tables(quality)
    zz = list(_JPEG_ZIGZAG)
    comps = [(1, 0)] if c == 1 else [(1, 0), (2, 1), (3, 1)]
    out = b"\xff\xd8" + _jpeg_segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(1 if c == 1 else 2):
        out += _jpeg_segment(0xDB, bytes([t]) + tables[t][zz].tobytes())
    out += _jpeg_segment(0xC0, bytes([8, h >> 8, h & 255, w >> 8, w & 255, len(comps)])
                         + b"".join(bytes([i, hh << 4 | vv if i == 1 else 0x11, t]) for i, t in comps))
    for key in (0x00, 0x10) + ((0x01, 0x11) if c == 3 else ()):
        bits, vals = JPEG_DHT[key]
        out += _jpeg_segment(0xC4, bytes((key,) + bits + vals))
    ri = -(-w // (8 * hh))
    out += _jpeg_segment(0xDD, bytes([ri >> 8, ri & 255]))
    out += _jpeg_segment(0xDA, bytes([len(comps)]) + b"".join(bytes([i, 0x11 * t]) for i, t in comps)
                         + bytes([0, 63, 0]))
    return out


def jpeg_optimize_flag(optimize, what="jpeg_optimize_flag"):
    """`optimize` as a bool; a TypeError for anything but True and False (host only)"""
    if not isinstance(optimize, (bool, np.bool_)):
        raise TypeError("%s: optimize is True or False, got %r" % (what, optimize))
    return bool(optimize)


def jpeg_header_pieces(head):
    """(the bytes in front of the DHT segments, the bytes behind them) of a header that jpeg_header built (host only)"""
    head = bytes(head)
    at, first, last = 2, None, None
    while at < len(head):
        end = at + 2 + ((head[at + 2] << 8) | head[at + 3])
        if head[at + 1] == 0xC4:
            first, last = at if first is None else first, end
        at = end
    return head[:first], head[last:]


JPEG_TABLE_BYTES = 16 + 256      # one Huffman table at the ABI: BITS, then HUFFVAL with the unused entries 0
JPEG_COUNT_SUM_MAX = 2 ** 63 - 1 # of the 256 counts of one table


def jpeg_optimal_tables(freq, stream=None):
    """the optimised Huffman table of each row of symbol counts in one va_jpeg_optimal_tables call (DESIGN.md §9,
    "Optimised Huffman tables"): libjpeg's jpeg_gen_optimal_table without its limits on a count and on a size before
    the limit to 16 bits.  freq: non-negative integers (t, 256) or (256,), each row's sum at most JPEG_COUNT_SUM_MAX
    (the merges add counts in 64 bits).  Returns uint8 (t, JPEG_TABLE_BYTES) or
    (JPEG_TABLE_BYTES,): BITS (16), then HUFFVAL with the unused entries 0; a row of zeros gives an empty table."""
    what = "jpeg_optimal_tables"
    freq = np.asarray(freq)
    if freq.dtype.kind not in "iu" or freq.ndim not in (1, 2) or freq.shape[-1] != 256:
        raise ValueError("%s: the counts are integers (t, 256) or (256,), got %s %r" % (what, freq.dtype, freq.shape))
    if freq.size and freq.min() < 0:
        raise ValueError("%s: the counts are not negative" % what)
    if freq.size and max(int(np.sum(row, dtype=object)) for row in freq.reshape(-1, 256)) > JPEG_COUNT_SUM_MAX:
        raise ValueError("%s: the sum of a table's counts is at most 2^63 - 1 (the device adds them in 64 bits)" % what)
    rows = np.ascontiguousarray(freq.reshape(-1, 256), np.int64)
    t = len(rows)
    if t == 0:
        return np.zeros((0, JPEG_TABLE_BYTES), np.uint8)
    with _Lease.on(stream) as d:
        src = d.upload(rows)
        out = d.take(t * JPEG_TABLE_BYTES)
        check(_hip.lib().va_jpeg_optimal_tables(src.ptr, t, out.ptr, stream))
        tables = out.download((t, JPEG_TABLE_BYTES), np.uint8, stream)
    return tables[0] if freq.ndim == 1 else tables


def jpeg_encode(frames, quality=90, color=None, stream=None, ret_packed=False, sampling=(1, 1), optimize=False,
                ret_tables=False):
    """one baseline JFIF file per frame of a stack in one va_jpeg_encode_u8 call ("Motion-JPEG"): 4:4:4
    or monochrome, the Annex K Huffman tables, one restart interval per MCU row; the bytes are pinned and equal the
    restatement's.  sampling: (2, 1) / "4:2:2" or (2, 2) / "4:2:0" write colour frames with box-averaged chroma in
    one va_jpeg_encode_sampled_u8 call ("Subsampled Motion-JPEG encoding"), as pinned.  frames: uint8 (n, h, w) or (n, h, w, 3) RGB, or a DeviceFrames (it stays the caller's; nothing
    is uploaded then).  color: None takes the channels from the shape; True / False say what a 3-dimensional array
    is, one colour frame (h, w, 3) or a monochrome stack, and must agree with a 4-dimensional one.
    One upload of the frames and one of [tables | header], one call, and the downloads of the sizes and of the used
    bytes.  The first launch has room for the headers and 1 / JPEG_ROOM_DIVISOR of the raw bytes; a batch that
    needs more runs exactly once more, with exact room.
    optimize: the files are written with Huffman tables made for this call, one set shared by its frames, in one
    va_jpeg_encode_optimized_u8 call ("Optimised Huffman tables"): counts, tables and header are made on
    the device, and the same uploads, downloads and room apply (the plain header is never shorter than the optimised
    one).  ret_tables (with optimize): the tables follow as uint8 (2 or 4, JPEG_TABLE_BYTES), DC0, AC0[, DC1, AC1].
    Returns the list of n `bytes`; ret_packed: (uint8 blob, int64 offsets of n + 1 entries), frame k being
    blob[offsets[k]:offsets[k + 1]]."""
    what = "jpeg_encode"
    optimize = jpeg_optimize_flag(optimize, what)
    if ret_tables and not optimize:
        raise ValueError("%s: ret_tables needs optimize=True (the plain files hold the Annex K tables, JPEG_DHT)" % what)
    hh, vv = jpeg_sampling(sampling, what=what)
    if not isinstance(frames, DeviceFrames):
        frames = np.asarray(frames)                 # (_frames_in checks the dtype and the shape)
        if color is not None and frames.ndim == (3 if color else 2):
            frames = frames[None]
    frames, n, h, w, c, owned = _frames_in(frames, what)
    if color is not None and (c == 3) != bool(color):
        raise ValueError("%s: color=%r with frames of %d channel(s)" % (what, color, c))
    jpeg_sampling(sampling, c, what)
    if n and not (1 <= h <= JPEG_MAX_SIDE and 1 <= w <= JPEG_MAX_SIDE):
        raise ValueError("%s: sides are 1 .. %d, got %d x %d" % (what, JPEG_MAX_SIDE, w, h))
    tables = jpeg_tables(quality)
    ntab = 2 if c == 1 else 4
    if n == 0:
        out = (np.zeros(0, np.uint8), np.zeros(1, np.int64)) if ret_packed else []
        return (out, np.zeros((ntab, JPEG_TABLE_BYTES), np.uint8)) if ret_tables else out
    head = np.frombuffer(jpeg_header(h, w, c, quality, (hh, vv)), np.uint8)
    if optimize:
        pre, post = (np.frombuffer(piece, np.uint8) for piece in jpeg_header_pieces(head.tobytes()))
        consts = _Layout(luma=tables[0], chroma=tables[1], pre=pre, post=post)
        sizes = _Layout(total=(1, np.int64), offsets=(n + 1, np.int64), sizes=(n, np.int64),
                        tables=(ntab * JPEG_TABLE_BYTES, np.uint8))
    else:
        consts = _Layout(luma=tables[0], chroma=tables[1], head=head)
        sizes = _Layout(total=(1, np.int64), offsets=(n + 1, np.int64), sizes=(n, np.int64))
    nseg = -(-h // (8 * vv))
    room = n * (len(head) + 2 * nseg) + (n * h * w * c) // JPEG_ROOM_DIVISOR
    L = _hip.lib()
    with _Lease.on(stream) as d:
        src = d.upload(frames) if owned else frames.buf
        cb = d.upload(consts.packed())
        info = d.take(sizes.nbytes)

        def run(cap):
            out = d.take(max(cap, 1))
            tail = (sizes.ptr(info, "sizes"), sizes.ptr(info, "offsets"), sizes.ptr(info, "total"), out.ptr, cap, stream)
            if optimize:
                check(L.va_jpeg_encode_optimized_u8(src.ptr, n, h, w, c, hh, vv, consts.ptr(cb, "luma"),
                                                    consts.ptr(cb, "pre"), len(pre), consts.ptr(cb, "post"), len(post),
                                                    sizes.ptr(info, "tables"), *tail))
            elif (hh, vv) == (1, 1):
                check(L.va_jpeg_encode_u8(src.ptr, n, h, w, c, consts.ptr(cb, "luma"), consts.ptr(cb, "head"), len(head),
                                          *tail))
            else:
                check(L.va_jpeg_encode_sampled_u8(src.ptr, n, h, w, c, hh, vv, consts.ptr(cb, "luma"),
                                                  consts.ptr(cb, "head"), len(head), *tail))
            meta = info.download((sizes.nbytes,), np.uint8, stream)
            return (out, meta), sizes.view(meta, "total")
        (out, meta), (total,) = _rerun(run, room)   # a total beyond the room: nothing was written
        blob = out.download((int(total),), np.uint8, stream)
    offsets = sizes.view(meta, "offsets").copy()
    if ret_packed:
        files = (blob, offsets)
    else:
        raw = blob.tobytes()
        files = [raw[offsets[k]:offsets[k + 1]] for k in range(n)]
    return (files, sizes.view(meta, "tables").reshape(ntab, JPEG_TABLE_BYTES).copy()) if ret_tables else files


# ------------------------------------------------------------------------------------------------ Motion-JPEG decoding
JPEG_STATUS_BAD_CODE, JPEG_STATUS_OVERRUN, JPEG_STATUS_TRUNCATED, JPEG_STATUS_MARKER = 1, 2, 4, 8    # VA_JPEG_STATUS_*
_JPEG_STATUS_NAMES = ((JPEG_STATUS_BAD_CODE, "bad code"), (JPEG_STATUS_OVERRUN, "overrun"),
                      (JPEG_STATUS_TRUNCATED, "truncated"), (JPEG_STATUS_MARKER, "marker sequence"))
JPEG_HUFF_DECODE_BYTES = 1416                  # VA_JPEG_HUFF_DECODE_BYTES
JPEG_DECODE_WORKSPACE_MAX = 1 << 30            # a batch whose coefficients need more is decoded in chunks of frames
_JPEG_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
                   0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic sequential",
                   0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential",
                   0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}


def jpeg_parse_header(data, sampling="1x1"):
    """what the header of one stored JPEG file says, or a ValueError that names what the decoder does not take
    ("Motion-JPEG decoding": baseline SOF0 with 8-bit samples, 1 component or 3 of 1 x 1 sampling,
    8-bit DQT, any valid DHT, any DRI, one scan).  sampling="any" also takes the 3-component layouts of "Subsampled
    Motion-JPEG decoding": luma 2 x 1 (4:2:2) or 2 x 2 (4:2:0) with Cb and Cr 1 x 1.  Returns a dict: h, w, c,
    sampling (H, V) of the luma component ((1, 1) for one component), ri (the restart interval in MCUs of 8H x 8V
    pixels; the MCUs of the frame where DRI is absent or 0), nseg, scan_begin (the byte behind the SOS header),
    qtables (c, 64) uint8 in natural order, huff: per component ((BITS, HUFFVAL) of its DC table, of its AC table)
    (host only)"""
    what = "jpeg_parse_header"
    if sampling not in ("1x1", "any"):
        raise ValueError("%s: sampling is '1x1' or 'any', got %r" % (what, sampling))
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("%s: no SOI at the start of the file" % what)
    i, qt, huff, sof, ri = 2, {}, {}, None, 0
    while True:
        if i + 4 > len(data):
            raise ValueError("%s: the file ends before SOS" % what)
        if data[i] != 0xFF:
            raise ValueError("%s: a marker is expected at byte %d, found %02x" % (what, i, data[i]))
        m = data[i + 1]
        if m == 0xFF:                               # a fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:          # markers without a segment
            i += 2
            continue
        if m in (0xD8, 0xD9):
            raise ValueError("%s: marker %02x before SOS" % (what, m))
        length = (data[i + 2] << 8) | data[i + 3]
        if length < 2 or i + 2 + length > len(data):
            raise ValueError("%s: the segment of marker %02x at byte %d leaves the file" % (what, m, i))
        p = data[i + 4:i + 2 + length]
        if m == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError("%s: a 16-bit quantisation table; 8-bit tables are decoded" % what)
                if len(p) < 65 or (p[0] & 15) > 3:
                    raise ValueError("%s: a damaged DQT segment" % what)
                table = np.zeros(64, np.uint8)
                table[list(_JPEG_ZIGZAG)] = np.frombuffer(p[1:65], np.uint8)
                qt[p[0] & 15], p = table, p[65:]
        elif m == 0xC4:
            while p:
                if len(p) < 17:
                    raise ValueError("%s: a damaged DHT segment" % what)
                bits = tuple(p[1:17])
                n = sum(bits)
                if (p[0] >> 4) > 1 or (p[0] & 15) > 3 or n > 256 or len(p) < 17 + n:
                    raise ValueError("%s: a damaged DHT segment" % what)
                code = 0
                for k in range(16):
                    code += bits[k]
                    if code > (1 << (k + 1)):
                        raise ValueError("%s: a DHT segment with more codes of %d bits than there are" % (what, k + 1))
                    code <<= 1
                huff[p[0]], p = (bits, tuple(p[17:17 + n])), p[17 + n:]
        elif m == 0xC0 or m in _JPEG_SOF_NAMES:
            if len(p) < 6:
                raise ValueError("%s: a damaged frame header" % what)
            precision, h, w, nc = p[0], (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if precision != 8:
                raise ValueError("%s: sample precision %d; only 8-bit precision is decoded" % (what, precision))
            if m != 0xC0:
                raise ValueError("%s: %s mode (SOF%d); only baseline sequential is decoded"
                                 % (what, _JPEG_SOF_NAMES[m], m - 0xC0))
            if sof is not None:
                raise ValueError("%s: two frame headers" % what)
            if nc not in (1, 3) or len(p) < 6 + 3 * nc:
                raise ValueError("%s: %d components; 1 or 3 are decoded" % (what, nc))
            comps = [(p[6 + 3 * k], p[7 + 3 * k], p[8 + 3 * k]) for k in range(nc)]
            luma = (1, 1)
            for k, (_, hv, _) in enumerate(comps):
                if hv != 0x11 and nc > 1:
                    if sampling == "any" and k == 0 and hv in (0x21, 0x22):
                        luma = (hv >> 4, hv & 15)
                        continue
                    if sampling == "any":
                        raise ValueError("%s: sampling factors %d x %d of %s; luma 1 x 1, 2 x 1 (4:2:2) or 2 x 2 "
                                         "(4:2:0) with 1 x 1 chroma sampling is decoded"
                                         % (what, hv >> 4, hv & 15, "a chroma component" if k else "the luma component"))
                    raise ValueError("%s: sampling factors %d x %d (chroma subsampling such as 4:2:0 or 4:2:2); only "
                                     "1 x 1 sampling is decoded" % (what, hv >> 4, hv & 15))
            if h == 0:
                raise ValueError("%s: a frame height of 0 (DNL) is not decoded" % what)
            if w == 0:
                raise ValueError("%s: a frame width of 0" % what)
            sof = (h, w, comps, luma)
        elif m == 0xCC:
            raise ValueError("%s: arithmetic coding (DAC) is not decoded" % what)
        elif m == 0xDC:
            raise ValueError("%s: DNL is not decoded" % what)
        elif m == 0xDD:
            if len(p) < 2:
                raise ValueError("%s: a damaged DRI segment" % what)
            ri = (p[0] << 8) | p[1]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("%s: SOS before the frame header" % what)
            h, w, comps, luma = sof
            ns = p[0] if p else 0
            if len(p) < 1 + 2 * ns + 3:
                raise ValueError("%s: a damaged scan header" % what)
            if ns != len(comps) or [p[1 + 2 * k] for k in range(ns)] != [cid for cid, _, _ in comps]:
                raise ValueError("%s: more than one scan: this scan holds %d of the %d components"
                                 % (what, ns, len(comps)))
            if (p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]) != (0, 63, 0):
                raise ValueError("%s: a scan with Ss %d, Se %d, Ah/Al %02x is not baseline sequential"
                                 % (what, p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]))
            tables = []
            for k, (_, _, tq) in enumerate(comps):
                td, ta = p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15
                if tq not in qt:
                    raise ValueError("%s: quantisation table %d is not defined" % (what, tq))
                if td not in huff or (0x10 | ta) not in huff:
                    raise ValueError("%s: Huffman table %d / %d is not defined" % (what, td, ta))
                tables.append((huff[td], huff[0x10 | ta]))
            mcus = -(-h // (8 * luma[1])) * -(-w // (8 * luma[0]))
            ri = ri if ri else mcus
            return dict(h=h, w=w, c=len(comps), sampling=luma, ri=ri, nseg=(mcus + ri - 1) // ri,
                        scan_begin=i + 2 + length, qtables=np.stack([qt[tq] for _, _, tq in comps]), huff=tables)
        i += 2 + length


def _jpeg_decode_table(bits, vals):
    """one Huffman table as the device reads it (va_jpeg_decode_math.h, HuffDecode): look[9 bits] = length << 8 |
    symbol of the codes of at most 9 bits, maxcode[l] and valoff[l] of T.81 F.2.2.3 for the longer ones, the
    symbols"""
    look, maxcode = np.zeros(512, np.uint16), np.full(17, -1, np.int32)
    valoff, symbols = np.zeros(17, np.int32), np.zeros(256, np.uint8)
    symbols[:len(vals)] = vals
    code = k = 0
    for length in range(1, 17):
        count = bits[length - 1]
        if count:
            valoff[length] = k - code
            maxcode[length] = code + count - 1
            if length <= 9:
                for j in range(count):
                    look[(code + j) << (9 - length):(code + j + 1) << (9 - length)] = (length << 8) | vals[k + j]
            k, code = k + count, code + count
        code <<= 1
    out = look.tobytes() + maxcode.tobytes() + valoff.tobytes() + symbols.tobytes()
    assert len(out) == JPEG_HUFF_DECODE_BYTES
    return out


def _jpeg_header_key(head):
    return (head["h"], head["w"], head["c"], head["ri"], head["qtables"].tobytes(), tuple(head["huff"]),
            tuple(head["sampling"]))


def jpeg_decode_groups(heads):
    """[(first, stop)] of the runs of consecutive frames whose headers agree in size, components, sampling, restart
    interval and tables: each run is one va_jpeg_decode_u8 or va_jpeg_decode_sampled_u8 call (host only)"""
    groups, first = [], 0
    keys = [_jpeg_header_key(head) for head in heads]
    for k in range(1, len(keys) + 1):
        if k == len(keys) or keys[k] != keys[first]:
            groups.append((first, k))
            first = k
    return groups if keys else []


def jpeg_status_text(status):
    return " | ".join(name for bit, name in _JPEG_STATUS_NAMES if status & bit) or "ok"


# the split decoder ("Split Motion-JPEG decoding", with the measurements behind these three)
JPEG_SPLIT_SUB_BYTES = 256                     # raw bytes of a lane: 128 .. 512 measure within 10 % of each other
JPEG_SPLIT_MAX_ROUNDS = 16                     # rounds of the scan: an unused round costs 5 us, a frame that needs more
                                               # takes the one-lane path, 40 times the time
JPEG_SPLIT_MIN_BYTES = 2048                    # split=None: the mean entropy bytes a frame from which a group is split
                                               # (32 frames: one lane wins at 1.1 KB a frame, the split at 3.2 KB)


def jpeg_decode(streams, color=None, stream=None, keep=False, ret_status=False, split=None, ret_rounds=False):
    """the frames of a batch of stored baseline JPEG files ("Motion-JPEG decoding" and "Subsampled
    Motion-JPEG decoding"); the pixels are pinned and equal the restatement's.  Decoded are monochrome files, 4:4:4
    files, and 4:2:2 and 4:2:0 files (luma 2 x 1 or 2 x 2, Cb and Cr 1 x 1: what cameras, libjpeg and Pillow write by
    default), whose chroma is upsampled with libjpeg's triangle filter.  streams: a list of `bytes`, or the (blob,
    offsets) pair that jpeg_encode(ret_packed=True) returns.  Every header is parsed on the host (jpeg_parse_header
    with sampling="any", with its refusals); consecutive frames with identical headers go into one va_jpeg_decode_u8
    call each (va_jpeg_decode_sampled_u8 for the subsampled layouts), whose bytes are uploaded once; all frames must
    have one shape (ValueError otherwise).  color: None takes the components from the files; True / False must agree
    with them.
    Returns the uint8 array (n, h, w) or (n, h, w, 3) RGB; keep=True: a DeviceFrames that is the caller's (nothing but
    the status words is downloaded).  A frame whose status word is not 0 raises a ValueError that names the first
    such frame and its bits; ret_status=True returns (frames, int32 status (n,)) in place of raising: blocks at and
    behind an error in their segment decode as sample 128.
    split: how a group of frames without restart markers (one entropy segment a frame, one lane a frame on the path
    above) is decoded.  True, or the bytes of a subsequence (a multiple of 16 in 16 .. 65536): by
    va_jpeg_decode_split_u8, one lane per subsequence ("Split Motion-JPEG decoding"); False: as above;
    None: split where the group's mean entropy bytes a frame reach JPEG_SPLIT_MIN_BYTES.  Groups with restart markers
    always take the path above; pixels and status words are the same on both.  ret_rounds=True appends the int32
    array (n,) of the rounds the split decoder's scan took: 0 for a frame of the path above, -1 for one that did not
    converge in JPEG_SPLIT_MAX_ROUNDS and was decoded by one lane."""
    what = "jpeg_decode"
    if not (split is None or isinstance(split, (bool, np.bool_))):
        if int(split) != split or not 16 <= split <= 65536 or split % 16:
            raise ValueError("%s: split is None, a bool or a multiple of 16 in 16 .. 65536, got %r" % (what, split))
    sub_bytes = JPEG_SPLIT_SUB_BYTES if split is None or isinstance(split, (bool, np.bool_)) else int(split)
    if (isinstance(streams, tuple) and len(streams) == 2 and isinstance(streams[0], np.ndarray)
            and streams[0].dtype == np.uint8):
        blob = np.ascontiguousarray(streams[0]).ravel()
        offsets = np.asarray(streams[1], np.int64).ravel()
        if len(offsets) < 1 or offsets[0] < 0 or (np.diff(offsets) < 0).any() or offsets[-1] > len(blob):
            raise ValueError("%s: the offsets do not lie in the blob in ascending order" % what)
    else:
        files = [bytes(s) for s in streams]
        blob = np.frombuffer(b"".join(files), np.uint8)
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in files])]).astype(np.int64)
    n = len(offsets) - 1
    heads, last = [], (None, None)                   # last: a header's bytes up to the scan, and what they say
    for k in range(n):
        data = blob[offsets[k]:offsets[k + 1]].tobytes()
        if last[0] is not None and data.startswith(last[0]):     # the frames of a file mostly repeat one header
            heads.append(last[1])
            continue
        try:
            heads.append(jpeg_parse_header(data, sampling="any"))
        except ValueError as err:
            raise ValueError("%s: frame %d: %s" % (what, k, err))
        last = (data[:heads[-1]["scan_begin"]], heads[-1])
    if n == 0:
        frames = np.zeros((0, 0, 0), np.uint8)
        if keep:
            frames = DeviceFrames(_take(1), 0, 0, 0, 1)
        extra = ((np.zeros(0, np.int32),) if ret_status else ()) + ((np.zeros(0, np.int32),) if ret_rounds else ())
        return (frames,) + extra if extra else frames
    h, w, c = heads[0]["h"], heads[0]["w"], heads[0]["c"]
    for k, head in enumerate(heads):
        if (head["h"], head["w"], head["c"]) != (h, w, c):
            raise ValueError("%s: mixed shapes: frame %d is %d x %d x %d, frame 0 is %d x %d x %d"
                             % (what, k, head["w"], head["h"], head["c"], w, h, c))
    if color is not None and (c == 3) != bool(color):
        raise ValueError("%s: color=%r with files of %d component(s)" % (what, color, c))
    frame_bytes = h * w * c
    L = _hip.lib()
    with _Lease.on(stream) as d:
        out = (d.result if keep else d.take)(max(n * frame_bytes, 1))       # under keep it leaves with the caller
        status_buf = d.take(4 * n)
        rounds_buf, split_groups = d.take(4 * n), []
        for first, stop in jpeg_decode_groups(heads):
            k, head = stop - first, heads[first]
            base = int(offsets[first])
            src = d.upload(blob[base:max(int(offsets[stop]), base + 1)])
            scan_begin = np.array([hd["scan_begin"] for hd in heads[first:stop]], np.int64)
            meta = _Layout(offsets=offsets[first:stop + 1] - base, scan_begin=scan_begin)
            mb = d.upload(meta.packed())
            tables = b"".join(_jpeg_decode_table(*dc) + _jpeg_decode_table(*ac) for dc, ac in head["huff"])
            consts = _Layout(qtables=head["qtables"], huff=np.frombuffer(tables, np.uint8))
            cb = d.upload(consts.packed())
            files = (src.ptr, meta.ptr(mb, "offsets"), meta.ptr(mb, "scan_begin"), k, h, w, c)
            coding = (consts.ptr(cb, "qtables"), consts.ptr(cb, "huff"), len(tables), out.ptr + first * frame_bytes,
                      status_buf.ptr + 4 * first)
            luma = tuple(head["sampling"])
            scan_bytes = (np.diff(offsets[first:stop + 1]) - scan_begin).clip(0)
            if head["nseg"] == 1 and split is not False and (
                    split is not None or scan_bytes.mean() >= JPEG_SPLIT_MIN_BYTES):
                # one segment a frame: one lane per sub_bytes of it
                size, most = L.va_jpeg_decode_split_workspace_bytes, int(scan_bytes.max())
                one, need = (int(size(frames, h, w, c, luma[0], luma[1], sub_bytes, most)) for frames in (1, k))
                room = min(need, max(one, JPEG_DECODE_WORKSPACE_MAX))
                ws = d.take(room)
                check(L.va_jpeg_decode_split_u8(*files, luma[0], luma[1], *coding, ws.ptr, room, sub_bytes,
                                                JPEG_SPLIT_MAX_ROUNDS, most, rounds_buf.ptr + 4 * first, stream))
                split_groups.append((first, stop))
                continue
            # the plain entry for monochrome and 1 x 1 files, the _sampled one with (luma_h, luma_v) for the rest
            if luma == (1, 1):
                decode, size, luma = L.va_jpeg_decode_u8, L.va_jpeg_decode_workspace_bytes, ()
            else:
                decode, size = L.va_jpeg_decode_sampled_u8, L.va_jpeg_decode_sampled_workspace_bytes
            one, need = (int(size(frames, h, w, c, head["ri"], *luma)) for frames in (1, k))
            room = min(need, max(one, JPEG_DECODE_WORKSPACE_MAX))
            ws = d.take(room)
            check(decode(*files, head["ri"], *luma, *coding, ws.ptr, room, stream))
        status = status_buf.download((n,), np.int32, stream)
        rounds = np.zeros(n, np.int32)
        if ret_rounds and split_groups:
            got = rounds_buf.download((n,), np.int32, stream)
            for first, stop in split_groups:
                rounds[first:stop] = got[first:stop]
        if status.any() and not ret_status:
            bad = int(np.flatnonzero(status)[0])
            raise ValueError("%s: frame %d does not decode: %s (status %d); %d of %d frames have errors"
                             % (what, bad, jpeg_status_text(int(status[bad])), status[bad],
                                int(np.count_nonzero(status)), n))
        frames = DeviceFrames(out, n, h, w, c) if keep else out.download(
            (n, h, w) + ((3,) if c == 3 else ()), np.uint8, stream)
    extra = ((status,) if ret_status else ()) + ((rounds,) if ret_rounds else ())
    return (frames,) + extra if extra else frames


# ------------------------------------------------------------------------ template matching
MATCH_METHODS = _hip.MATCH_METHODS
MATCH_MAX_TEMPLATE_PIXELS = _hip.MATCH_MAX_TEMPLATE_PIXELS
MATCH_RESULT_DTYPE = np.dtype([("score", np.float64), ("x", np.int32), ("y", np.int32), ("status", np.int32)])
MATCH_STATUS_FRAME, MATCH_STATUS_TEMPLATE, MATCH_STATUS_EMPTY, MATCH_STATUS_OUTSIDE = 1, 2, 4, 8      # VA_MATCH_STATUS_*


def match_query_table(queries, what="match_templates"):
    """the (q, 6) int32 table (frame, templ, x0, y0, nx, ny) of queries given as such rows or as MATCH_QUERY_DTYPE
    records"""
    arr = np.asarray(queries)
    if arr.dtype == _hip.MATCH_QUERY_DTYPE:
        arr = arr.view(np.int32).reshape(-1, 6)
    if arr.size == 0:
        return np.zeros((0, 6), np.int32)
    if not np.issubdtype(arr.dtype, np.integer) or arr.ndim != 2 or arr.shape[1] != 6:
        raise ValueError("%s: queries are integer rows (frame, templ, x0, y0, nx, ny), got %s of shape %r"
                         % (what, arr.dtype, arr.shape))
    if np.any(np.abs(arr.astype(np.int64)) >= 2 ** 31):
        raise ValueError("%s: a query field does not fit int32" % what)
    return np.ascontiguousarray(arr, np.int32)


def match_query_status(table, n, h, w, shapes):
    """the status bits the device gives each query of `table` (match_query_table) on n frames (h, w) and templates of
    `shapes` (m, 2): host arithmetic, which sizes the buffers of match_templates"""
    q = table.astype(np.int64)
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    frame, templ, x0, y0, nx, ny = q.T
    status = np.zeros(len(q), np.int32)
    status[(frame < 0) | (frame >= n)] |= MATCH_STATUS_FRAME
    empty = (nx < 1) | (ny < 1)
    status[empty] |= MATCH_STATUS_EMPTY
    known = (templ >= 0) & (templ < len(shapes))
    status[~known] |= MATCH_STATUS_TEMPLATE
    th, tw = (shapes[np.where(known, templ, 0), k] if len(shapes) else np.zeros(len(q), np.int64) for k in (0, 1))
    outside = known & ~empty & ((x0 < 0) | (y0 < 0) | (x0 + nx - 1 + tw > w) | (y0 + ny - 1 + th > h))
    status[outside] |= MATCH_STATUS_OUTSIDE
    return status


def _match_templates_in(templates, what):
    arrs = []
    for k, t in enumerate(templates):
        t = np.asarray(t)
        if t.dtype != np.uint8:
            raise TypeError("%s: template %d must be uint8, got %s" % (what, k, t.dtype))
        if t.ndim != 2 or t.size < 1 or t.size > MATCH_MAX_TEMPLATE_PIXELS:
            raise ValueError("%s: template %d of shape %r: templates are 2-d with 1 .. %d pixels"
                             % (what, k, t.shape, MATCH_MAX_TEMPLATE_PIXELS))
        arrs.append(np.ascontiguousarray(t))
    return arrs


def match_templates(frames, templates, queries, method="ccoeff_normed", maps=False, keep=False, stream=None):
    """cv2.matchTemplate + cv2.minMaxLoc for a batch of queries in one launch chain ("Template matching";
    va_template_match_u8).  frames: a monochrome uint8 stack (n, h, w), or a DeviceFrames, which is not uploaded and
    stays the caller's.  templates: a list of 2-d uint8 arrays of 1 .. 65536 pixels each.  queries: rows (frame,
    templ, x0, y0, nx, ny): the template's top-left corner at (x0 + i, y0 + j) for 0 <= i < nx, 0 <= j < ny, all of
    which must hold the template inside the frame.  method: one of MATCH_METHODS (cv2.TM_* in lower case).
    Returns `best`, a MATCH_RESULT_DTYPE array: the minimum (sqdiff methods) or maximum score of each query and its
    position, the first in raster order among equals; a query with status != 0 (MATCH_STATUS_*) has score nan and
    position (-1, -1).  maps=True appends the list of (ny, nx) float64 score maps, (0, 0) for a flagged query.
    keep=True appends the DeviceFrames the call ran on (the caller's own, or the upload of a host stack, which is
    then the caller's to release).  TypeError / ValueError for arguments of the wrong type or shape, before a device
    is touched."""
    what = "match_templates"
    if method not in MATCH_METHODS:
        raise ValueError("%s: method %r is not one of %s" % (what, method, sorted(MATCH_METHODS)))
    src, n, h, w, c, owned = _frames_in(frames, what)
    if c != 1:
        raise ValueError("%s: frames are a monochrome stack (n, h, w); convert colour frames first" % what)
    if n and (h < 1 or w < 1):
        raise ValueError("%s: frames of shape %r have no pixels" % (what, (h, w)))
    arrs = _match_templates_in(templates, what)
    table = match_query_table(queries, what)
    nq, m = len(table), len(arrs)
    shapes = np.array([t.shape for t in arrs], np.int32).reshape(m, 2)
    status = match_query_status(table, n, h, w, shapes)
    sizes = np.where(status == 0, table[:, 4].astype(np.int64) * table[:, 5], 0)
    map_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(map_off[-1])
    best = np.zeros(nq, MATCH_RESULT_DTYPE)
    if nq == 0 or n == 0 or m == 0:
        best["score"], best["x"], best["y"], best["status"] = np.nan, -1, -1, status
        out = (best,) + (([np.zeros((0, 0))] * nq,) if maps else ())
        if keep:
            out += (DeviceFrames.upload(src, stream) if owned else src,)
        return out if len(out) > 1 else best
    L = _hip.lib()
    flat, _, toff, tsizes, _ = _pack_ragged(arrs)
    toff = np.concatenate([toff, [int(tsizes.sum())]]).astype(np.int64)
    with _Lease.on(stream) as d:
        dev = _frames_on_device(d, src, owned)
        ws_bytes = L.va_template_match_workspace_bytes(nq, total, m)
        if ws_bytes == 0:
            raise ValueError("%s: %d queries of %d positions are beyond what one call takes" % (what, nq, total))
        tb, sb, ob, qb = d.upload(flat), d.upload(shapes), d.upload(toff), d.upload(table)
        bb, ws = d.take(nq * 24), d.take(ws_bytes)
        mb, mo = (d.take(max(total, 1) * 8), d.upload(map_off)) if maps else (None, None)
        args = _hip.va_match_args(C.sizeof(_hip.va_match_args), MATCH_METHODS[method], dev.buf.ptr, n, h, w, 0, h * w,
                                  tb.ptr, sb.ptr, ob.ptr, m, qb.ptr, nq, total, bb.ptr, _ptr(mb), _ptr(mo), ws.ptr,
                                  ws_bytes, stream)
        check(L.va_template_match_u8(C.byref(args)))
        raw = bb.download((nq,), _hip.MATCH_BEST_DTYPE, stream)
        scores = mb.download((total,), np.float64, stream) if maps else None
        if not keep and owned:
            dev.release(into=d)
    good = raw["status"] == 0
    if not np.array_equal(good, status == 0):
        raise _hip.HipError(-5, "%s: the device and the host disagree on the status of the queries" % what)
    best["status"] = raw["status"]
    best["score"] = np.where(good, raw["score"], np.nan)
    best["x"], best["y"] = np.where(good, raw["x"], -1), np.where(good, raw["y"], -1)
    out = (best,)
    if maps:
        out += ([scores[map_off[k]:map_off[k + 1]].reshape((table[k, 5], table[k, 4]) if good[k] else (0, 0))
                 for k in range(nq)],)
    if keep:
        out += (dev,)
    return out if len(out) > 1 else best
