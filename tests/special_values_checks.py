"""Shared by tests/test_special_values_host.py and tests/test_gpu_special_values.py: the value classes that a float
input or state may hold, the builders that write them into the benign random images of the other tests, the
comparison `same_floats`, the cases both tests walk, and the stand-alone sanitized program around oracle/va_oracle.c
("Special values")."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------ the value classes
_F = np.float32
FLT_MIN, FLT_MAX = float(np.finfo(_F).tiny), float(np.finfo(_F).max)
FLT_SUB_MIN = float(_F(2.0 ** -149))
FLT_SUB_MAX = FLT_MIN - FLT_SUB_MIN
PAIR = 3e38                                  # two of them overflow in a + b, none of them in a * tap
# name -> the float32 values of the class ("pair" is placed by its own rule, see plant())
F32_CLASSES = {
    "nan": [float("nan")],
    "inf": [float("inf"), -float("inf")],
    "zero": [0.0, -0.0],
    "subnormal": [FLT_SUB_MIN, -FLT_SUB_MIN, FLT_SUB_MAX, -FLT_SUB_MAX],
    "flt_min": [FLT_MIN],
    "flt_max": [FLT_MAX, -FLT_MAX],
    "pair": [PAIR],
}
NONFINITE = ("nan", "inf")
F32_STATES = [v for name in ("nan", "inf", "zero", "subnormal", "flt_min", "flt_max") for v in F32_CLASSES[name]]

DBL_MIN, DBL_MAX = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)
F64_STATES = ([float("nan"), float("inf"), -float("inf"), 0.0, -0.0] + [k * 2.0 ** -1074 for k in range(1, 65)]
              + [DBL_MIN, 2.0 ** -1000, 1e300, -1e300, 1e308, DBL_MAX])
# the edges of the domain in which the running mean's kernels divide without a division (va_point.hip, kFastMeanMin
# and kFastMeanMax): the last values inside and the first outside.  mean_u8_case() gives every value a thread of its
# own, so the inside ones do go through the division-free arithmetic and each outside one trips the guard alone
FAST_MEAN_MIN, FAST_MEAN_MAX = 2.0 ** -900, 2.0 ** 960
DOMAIN_EDGES = [2.0 ** -900, float(np.nextafter(2.0 ** -900, 0)), 2.0 ** 960, float(np.nextafter(2.0 ** 960, np.inf)),
                -2.0 ** -900, -float(np.nextafter(2.0 ** 960, np.inf))]
MEAN_STATES = F64_STATES + DOMAIN_EDGES


def in_fast_domain(state):
    """bg_mean_u8_fast_kernel's test of one state value (false for NaN)"""
    a = np.abs(np.asarray(state, np.float64))
    with np.errstate(invalid="ignore"):
        return (a == 0) | ((a >= FAST_MEAN_MIN) & (a <= FAST_MEAN_MAX))


def fast_threads(state, v):
    """per thread of v consecutive pixels: whether the kernel keeps it on the division-free path (every value of the
    thread inside the domain)"""
    return in_fast_domain(state).reshape(-1, v).all(axis=1)


def finite_only(values):
    return [v for v in values if np.isfinite(v)]


def without_nan(values):
    return [v for v in values if not np.isnan(v)]


# ------------------------------------------------------------------------------------------------ comparison
def same_floats(got, want, where=None):
    """same dtype and shape, the same NaN mask, and the same BITS everywhere else: -0.0 is not 0.0, infinities and
    subnormals count.  The sign and payload of a NaN are not compared (a NaN that an invalid operation generates has
    the sign bit set on x86 and clear on the GPU)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, want.dtype, got.shape, want.shape)
    assert want.dtype in (np.float32, np.float64), (where, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    g, w = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    bad = (gn != wn) | (~wn & (g != w))
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%r: %d of %d elements differ, the first at %r: got %r (0x%x), want %r (0x%x)"
                             % (where, int(bad.sum()), bad.size, at, got[at], int(g[at]), want[at], int(w[at])))


def differs(a, b):
    try:
        same_floats(a, b)
    except AssertionError:
        return True
    return False


# -------------------------------------------------------------------------------------------- input builders
def benign(shape, seed):
    """the float32 image of the existing GPU tests (test_gpu_configs.py, test_gpu_parity.py)"""
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * 3 - 1).astype(np.float32)


class _Sites(object):
    """positions of one (h, w) plane handed out once each: an interior pixel, the first and last row and column (the
    reflected border), a pixel inside a group of four and the last pixel of one"""

    def __init__(self, h, w, start=0):
        self.h, self.w, self.used, self.count = h, w, set(), start

    def _free(self, y, x, dy, dx):
        """(y, x), or the next free pixel along its line; on a small plane, whose border line may be full, any free
        pixel, and (y, x) again once the plane is full (the later value stays)"""
        for _ in range(self.h if dy else self.w):
            if (y, x) not in self.used:
                break
            y, x = (y + dy) % self.h, (x + dx) % self.w
        else:
            free = [(j, i) for j in range(self.h) for i in range(self.w) if (j, i) not in self.used]
            if free:
                y, x = free[len(free) // 2]
        self.used.add((y, x))
        return y, x

    def seven(self):
        h, w, v = self.h, self.w, self.count
        self.count += 1
        groups = max(w // 4, 1)
        return [self._free(min(2, h - 1) + (4 * v) % max(h - 4, 1), min(2, w - 1) + (9 * v + 3) % max(w - 4, 1), 0, 1),
                self._free(0, (5 + 7 * v) % w, 0, 1), self._free(h - 1, (2 + 7 * v) % w, 0, 1),
                self._free((3 + 5 * v) % h, 0, 1, 0), self._free((1 + 5 * v) % h, w - 1, 1, 0),
                self._free((6 + 3 * v) % h, min(4 * ((2 * v + 1) % groups) + 1, w - 1), 1, 0),
                self._free((7 + 3 * v) % h, min(4 * ((2 * v + 2) % groups) + 3, w - 1), 1, 0)]


def plant(plane, classes, turn=0):
    """write the values of `classes` into the (h, w) float32 view `plane`, each at the seven positions of _Sites
    (`turn` moves them, so that the frames of a stack differ where a temporal filter looks); the
    "pair" class is two horizontal runs of nine 3e38 pixels one row above and one below a centre row (after a row pass
    both are still above FLT_MAX / 2, so the column pass's a + b overflows where tap-by-tap sums would not) and two
    single pixels left and right of a centre column"""
    h, w = plane.shape
    sites = _Sites(h, w, 3 * turn)
    if "pair" in classes and h >= 6 and w >= 13:
        yc, x0 = h // 2 + turn % 2, 1 + turn % 3
        plane[yc - 1, x0:x0 + 9] = PAIR
        plane[yc + 1, x0:x0 + 9] = PAIR
        plane[1, w // 2 - 1] = plane[1, w // 2 + 1] = PAIR
        sites.used |= {(y, x) for y in (yc - 1, yc + 1) for x in range(x0, x0 + 9)} | {(1, w // 2 - 1), (1, w // 2 + 1)}
    for name in classes:
        if name == "pair":
            continue
        for value in F32_CLASSES[name]:
            for y, x in sites.seven():
                plane[y, x] = value


FINITE_CLASSES = ("zero", "subnormal", "flt_min", "flt_max")


def _planes(a, color):
    """the (h, w) views a spatial filter treats independently: frames, and the channels of colour frames"""
    if color:
        a4 = a if a.ndim == 4 else a[None]
        return [a4[f, :, :, c] for f in range(a4.shape[0]) for c in range(a4.shape[3])]
    return [a] if a.ndim == 2 else list(a)


def special_frames(shape, seed, color=False, only=None, turns=None):
    """the benign image of `shape` with every class written in.  The planes take turns, so that the non-finite values
    do not flood the frame: plane 0 holds the finite classes, plane 1 the non-finite ones, plane 2 (where there is
    one) the overflowing pair; a single plane holds them all.  only=<class>: that class alone, where it would be."""
    a = benign(shape, seed)
    planes = _planes(a, color)
    if turns is not None:
        pass
    elif len(planes) == 1:
        turns = [FINITE_CLASSES + NONFINITE + ("pair",)]
    elif len(planes) == 2:
        turns = [FINITE_CLASSES + ("pair",), NONFINITE]
    else:
        turns = [FINITE_CLASSES, NONFINITE, ("pair",)]
    for k, plane in enumerate(planes):
        classes = turns[k % len(turns)]
        plant(plane, [c for c in classes if only is None or c == only], k // len(turns))
    return a


def special_slots(nvalues, copies, group):
    """flat pixel index of value i in copy c of special_state(): [c][i].  Each value has a slot of `group` pixels of
    its own, slot after slot and copy after copy, and sits at a lane inside it that changes from value to value"""
    return [[(c * nvalues + i) * group + (5 * i + 3 * c) % group for i in range(nvalues)] for c in range(copies)]


def special_state(shape, values, seed, scale=255.0, dtype=np.float64, copies=3, group=1):
    """a benign state (random in [0, scale)) whose first pixels hold `copies` copies of every value.  group = 1: value
    after value.  group = 16: every value alone among 15 benign ones in an aligned group of 16 pixels, so that in a
    kernel whose threads own 8 or 16 consecutive pixels no two special values share a thread"""
    st = (np.random.default_rng(seed).random(shape) * scale).astype(dtype)
    flat = st.reshape(-1)
    assert copies * len(values) * group <= flat.size, (shape, len(values), group)
    for slots in special_slots(len(values), copies, group):
        flat[slots] = values
    return st


def frames_under_state(n, shape, nvalues, seed, group=1):
    """uint8 frames for special_state(copies=3): the pixels under the first copy (its whole slots) are 0 in every
    frame, those under the second 255, those under the third alternate 0, 255, ...; random elsewhere"""
    fr = np.random.default_rng(seed).integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
    flat = fr.reshape(n, -1)
    span = nvalues * group
    flat[:, :span] = 0
    flat[:, span:2 * span] = 255
    flat[:, 2 * span:3 * span] = (255 * (np.arange(n) % 2))[:, None]
    return fr


# ------------------------------------------------------------------------------------ the cases of both tests
GAUSS_SHAPES = (((2, 37, 53), False), ((2, 24, 64), False), ((1, 33, 40, 3), True))
GAUSS_SIGMAS = (1.0, 2.0, 3.3)               # compile-time radii 4 and 8, runtime radius 13


def gaussian_input(shape, color, only=None):
    return special_frames(shape, 100 + shape[-2], color, only)


RESIZE_MODES = ("nearest", "linear", "cubic", "area", "lanczos")


def resize_stack(only=None):
    """(2, 30, 40): the sizes (1, 1) and (7, 5) average a whole frame or a thirtieth of it, so the values that overflow
    a sum share the frame of the non-finite ones, and the other frame's averages stay finite"""
    return special_frames((2, 30, 40), 41, only=only,
                          turns=[("zero", "subnormal", "flt_min"), ("flt_max", "pair") + NONFINITE])


def resize_inputs():
    """name -> (frames, color, [(width, height), ...])"""
    return {"stack": (resize_stack(), False,
                      [(60, 45), (40, 30), (7, 5), (1, 1), (120, 90), (80, 60)]),
            "colour": (special_frames((20, 30, 3), 42, color=True), True, [(90, 60), (60, 40)])}


EMA_RATE = 0.05
MEAN_N_SEEN = (0, 1, 5, 11, 1000, 2 ** 24 - 3)
MEAN_N = (1, 9, 24, 40)                       # last group only, second loop, first loop


def mean_states(n_seen, want_diff):
    """the float64 states of a running-mean case: a NaN state makes the uint8 difference a conversion that C leaves
    undefined, so it is there in the state-only runs alone; so are the infinities at n_seen = 0, where Inf * 0 is NaN
    from the second frame on"""
    if not want_diff:
        return MEAN_STATES
    return without_nan(MEAN_STATES) if n_seen > 0 else finite_only(MEAN_STATES)


MEAN_GROUP = 16                               # pixels per slot of a running-mean state: the widest thread's


def form_shape(base_shape, nvalues):
    """the frame shape of a kernel form of test_gpu_bg_mean_paths.FORMS with room for three copies of nvalues states
    in slots of MEAN_GROUP pixels: the rows times an odd number, which leaves what selects the form -- whether 16 and
    whether 8 divide px -- as it is"""
    h, w = base_shape
    k = 1
    while h * k * w < 3 * MEAN_GROUP * nvalues:
        k += 2
    assert [(h * k * w) % d == 0 for d in (8, 16)] == [(h * w) % d == 0 for d in (8, 16)]
    return (h * k, w)


def ema_states(want_diff, n):
    """float32 EMA states of the uint8 model: as mean_states; an infinite state is NaN after one frame"""
    if not want_diff:
        return F32_STATES
    return without_nan(F32_STATES) if n == 1 else finite_only(F32_STATES)


def temporal_frames(dtype, seed=17):
    """(5, 9, 13) frames of the temporal statistics: float frames with every class (one plane holds them all), int16
    frames with the extremes"""
    shape = (5, 9, 13)
    if np.dtype(dtype) == np.int16:
        fr = np.random.default_rng(seed).integers(-255, 256, shape).astype(np.int16)
        fr[0, 0, :3] = fr[3, 4, 4:7] = fr[4, 8, -3:] = [32767, -32767, -32768]
        fr[1:, 0, 1] = -32768
        return fr
    fr = benign(shape, seed)
    for k, plane in enumerate(fr):
        plant(plane, [c for j, c in enumerate(FINITE_CLASSES + NONFINITE) if (j + k) % 2 == 0], k)
    return fr.astype(dtype)


def mean_numpy(frames, mean, n_seen):
    """oracle.measure_mean_numpy's loop body (video/analysis/video.py:33) from a given state"""
    mean = np.array(mean, np.float64)
    with np.errstate(all="ignore"):
        for k, frame in enumerate(frames):
            n = n_seen + k
            mean = mean * n / (n + 1) + frame / (n + 1)
    return mean


def welford_numpy(frames, mean, m2, n_seen):
    """oracle.measure_mean_std_numpy's loop body (video/analysis/video.py:48-50) from a given state"""
    mean, m2 = np.array(mean, np.float64), np.array(m2, np.float64)
    with np.errstate(all="ignore"):
        for k, frame in enumerate(frames):
            delta = frame - mean
            mean = mean + delta / (n_seen + k + 1)
            m2 = m2 + delta * (frame - mean)
    return mean, m2


def temporal_states(shape, seed=3):
    """(mean, m2) float64 states with every special value, one copy each, at different pixels of the two planes"""
    mean = special_state(shape, F64_STATES, seed, scale=2.0, copies=1)
    m2 = np.roll(special_state(shape, F64_STATES, seed + 1, scale=2.0, copies=1).reshape(-1), 7).reshape(shape)
    return mean, m2


NORMALIZE_BOUNDS = ((-0.5, 1.5, 1.0 / 2.0, 0.0),                    # clips the infinities and +-FLT_MAX
                    (-float("inf"), float("inf"), 2.0, 1.0),         # Inf - Inf at both ends
                    (FLT_SUB_MIN, FLT_MIN, 3.0, -0.0),               # the bounds are subnormal / FLT_MIN themselves
                    (-FLT_MAX, FLT_MAX, 2.0, 0.0))                   # f - fmin and * alpha overflow


def normalize_numpy(frames, fmin, fmax, alpha, tmin, dtype):
    """FilterNormalize._process_frame (video/filters.py:126-132) as NumPy evaluates it on float32 frames: the bounds,
    alpha and tmin join as float32, and only astype changes the type"""
    f = np.asarray(frames, np.float32)
    with np.errstate(all="ignore"):
        v = (np.clip(f, _F(fmin), _F(fmax)) - _F(fmin)) * _F(alpha) + _F(tmin)
        assert v.dtype == np.float32
        if np.dtype(dtype) == np.uint8:
            return v.astype(np.int64).astype(np.uint8)
        return v.astype(dtype)


def normalize_u8_input():
    """in-range float32 values for a uint8 target (out-of-range and NaN conversions are undefined in C): [0, 1) with
    -0.0, 0.0, subnormals of both signs and FLT_MIN"""
    f = np.random.default_rng(9).random((2, 9, 13), dtype=np.float32)
    f.reshape(-1)[:7] = [0.0, -0.0, FLT_SUB_MIN, -FLT_SUB_MIN, FLT_SUB_MAX, -FLT_SUB_MAX, FLT_MIN]
    return f


def statistics_input():
    """float32 image for image_statistics: -0.5, -0.0 and subnormals, which truncate to 0, and large values.  float32
    has steps of 256 at 2^31, so +-(2^31 + 0.5) are stored as +-2^31: the positive one is the first value past int32,
    the negative one the last inside it.  +-(2^31 + 256) and 2^40 are representable and past int32 on both sides, well
    inside int64"""
    img = (np.random.default_rng(78).random((33, 70)) * 200 - 50).astype(np.float32)
    vals = [-0.5, -0.0, 0.5, FLT_SUB_MIN, -FLT_SUB_MAX, FLT_MIN, 2.0 ** 31 + 0.5, -(2.0 ** 31 + 0.5), 2.0 ** 31 + 256,
            -(2.0 ** 31) - 256, 2.0 ** 40]
    sites = _Sites(*img.shape)
    for v in vals:
        for y, x in sites.seven()[:3]:
            img[y, x] = v
    return img


# -------------------------------------------------------------- the stand-alone sanitized program of the oracle
OPS = {"gaussian_f32": 1, "bg_ema_f32": 2, "bg_ema_u8": 3, "bg_mean_u8": 4, "welford_u8": 5, "welford_any": 6,
       "mean_any": 7, "bg_static_u8": 8, "resize_f32": 9, "div_model": 10}
ANY_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.int16): 3}


def record(op, ints=(), reals=(), arrays=()):
    """one call of the program: int64 op, seven int64 and two float64 parameters, then the input arrays"""
    ints, reals = list(ints) + [0] * (7 - len(ints)), list(reals) + [0.0] * (2 - len(reals))
    return struct.pack("<8q2d", OPS[op], *ints, *reals) + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def host_c_compiler():
    return shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")


def compile_driver(directory):
    """tests/special_values_driver.c + oracle/va_oracle.c, a program of its own, with UBSan and its float-cast
    check; the oracle's flags otherwise (no contraction)"""
    cc = host_c_compiler()
    assert cc is not None, "no host C compiler"
    exe = os.path.join(str(directory), "special_values_driver")
    subprocess.check_call([cc, "-O1", "-g", "-std=c11", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "special_values_driver.c"),
                           os.path.join(ROOT, "oracle", "va_oracle.c"), "-o", exe, "-lm"])
    return exe


def run_driver(exe, directory, records, name="calls"):
    """(exit code, stderr, bytes the program wrote) of the program on `records`"""
    src, dst = os.path.join(str(directory), name + ".in"), os.path.join(str(directory), name + ".out")
    with open(src, "wb") as f:
        f.write(b"".join(records))
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = b""
    if os.path.exists(dst):
        with open(dst, "rb") as f:
            out = f.read()
    return p.returncode, p.stderr.decode(errors="replace"), out


# ------------------------------------------------- the background and temporal cases, walked by both tests
def colour_state(frame_shape, seed):
    """float32 EMA state for (h, w, 3) frames: the non-finite values in channel 1 alone (the channel whose frames
    hold them too), the finite ones in channels 0 and 2"""
    st = benign(frame_shape, seed)
    fin = finite_only(F32_STATES)
    st[..., 1].reshape(-1)[3:3 + 3 * 5:5] = [v for v in F32_STATES if not np.isfinite(v)]
    for c in (0, 2):
        plane = st[..., c]
        idx = 7 + 11 * np.arange(len(fin)) + c
        plane.reshape(-1)[idx] = fin
    return st


ENGINE_SHAPE = (4, 33, 70, 3)                 # test_gpu_hostile_memory.test_engine_float32_chain's frames
ENGINE_SIGMA, ENGINE_RATE = 9.0, 0.02


def engine_cases():
    """[(n_seen, state or None)]: the engine's own start, and a set state with the special values"""
    return [(0, None), (3, colour_state(ENGINE_SHAPE[1:], 6))]


def engine_clip():
    return special_frames(ENGINE_SHAPE, 5, color=True)


EMA_SHAPES = ((8, 16), (9, 13))               # whole vectors of 4 floats / 8 bytes per thread; one pixel per thread


def ema_f32_cases():
    """[(frames, state, n_seen)]"""
    out = []
    for shape in EMA_SHAPES:
        fr = special_frames((4,) + shape, 50 + shape[1])
        st = special_state(shape, F32_STATES, 60 + shape[1], scale=2.0, dtype=np.float32)
        out += [(fr, st, 0), (fr, st, 3)]
    return out


def ema_u8_cases():
    """[(frames, state, n_seen, want_diff)]"""
    out = []
    for shape in EMA_SHAPES:
        for n in (1, 4):
            for want_diff in (True, False):
                values = ema_states(want_diff, n)
                fr = frames_under_state(n, shape, len(values), 70 + n)
                st = special_state(shape, values, 71, dtype=np.float32)
                out += [(fr, st, n_seen, want_diff) for n_seen in (0, 3)]
    return out


STATIC_SHAPES = ((16, 16), (15, 15))


def static_cases():
    """[(frames, background)]: a NaN background has no defined uint8 difference"""
    values = without_nan(F64_STATES)
    return [(frames_under_state(3, shape, len(values), 80), special_state(shape, values, 81))
            for shape in STATIC_SHAPES]


def bounded_mean_case(base_shape, n):
    """(frames, state): the special states that lie in [0, 255], which a pipeline runs through the kernels without
    the saturation -- zeros, subnormals, DBL_MIN, 2^-1000 and the lower edge of the division-free domain"""
    values = [v for v in MEAN_STATES if 0 <= v <= 255]
    shape = form_shape(base_shape, len(MEAN_STATES))
    return (frames_under_state(n, shape, len(values), 95, MEAN_GROUP),
            special_state(shape, values, 96, group=MEAN_GROUP))


ENGINE_MEAN_N_SEEN, ENGINE_MEAN_N = (1, 5, 2 ** 24 - 3), 9


GRADIENT_SHAPES = ((3, 3), (2, 13), (10, 2), (1, 7), (6, 9), (27, 82), (37, 53))
GRADIENT_CLASSES = (("zero", "subnormal"), ("nan",), ("inf",), ("flt_min", "flt_max"), ("pair", "zero"), NONFINITE,
                    FINITE_CLASSES)


def gradient_items():
    """potentials of the ragged gradients: the shapes of test_gpu_hostile_memory.GRAD_SHAPES, one group of classes
    each"""
    return [special_frames(s, 20 + k, turns=[GRADIENT_CLASSES[k % len(GRADIENT_CLASSES)]])
            for k, s in enumerate(GRADIENT_SHAPES)]


_MEAN_CACHE = {}


def mean_u8_case(base_shape, n_seen, n, want_diff):
    """(frames, state) of one running-mean case on the form whose FORMS shape is base_shape"""
    values = mean_states(n_seen, want_diff)
    key = (base_shape, len(values), n)
    if key not in _MEAN_CACHE:
        shape = form_shape(base_shape, len(MEAN_STATES))
        _MEAN_CACHE[key] = (frames_under_state(n, shape, len(values), 90 + n, MEAN_GROUP),
                            special_state(shape, values, 91, group=MEAN_GROUP))
    return _MEAN_CACHE[key]


def mean_u8_cases(base_shape):
    return [(n_seen, n, want_diff) + mean_u8_case(base_shape, n_seen, n, want_diff)
            for n_seen in MEAN_N_SEEN for n in MEAN_N for want_diff in (True, False)]


ROUNDING_N_SEEN = 2 ** 24 + 1                 # float32(n + 1) rounds from the second frame on


def temporal_cases():
    """[(frames, mean, m2, n_seen)] for running_mean and welford; mean / m2 None: the op's own zero state"""
    out = []
    shape = (9, 13)
    mean, m2 = temporal_states(shape)
    for dtype in (np.float32, np.float64, np.int16):
        fr = temporal_frames(dtype)
        out += [(fr, None, None, 0), (fr, mean, m2, 4)]
    out.append((temporal_frames(np.float32), None, None, ROUNDING_N_SEEN))
    return out


def oracle_calls(oracle, mean_base_shapes):
    """[(name, record of the sanitized program, [the oracle's outputs in the program's order])] for every input whose
    output the GPU test compares with oracle/va_oracle.c"""
    calls = []
    for shape, color in GAUSS_SHAPES:
        im = gaussian_input(shape, color)
        n, h, w, c = (shape if color else shape + (1,))
        for sigma in GAUSS_SIGMAS:
            calls.append((("gaussian", shape, sigma), record("gaussian_f32", (n, h, w, c), (sigma,), (im,)),
                          [oracle.gaussian_f32(im, sigma)]))
    for name, (im, color, sizes) in resize_inputs().items():
        a4 = im.reshape((-1,) + im.shape[-3:]) if color else im.reshape((-1,) + im.shape[-2:] + (1,))
        n, h, w, c = a4.shape
        for size in sizes:
            for mode in RESIZE_MODES:
                want = oracle.resize_f32(im, size, mode, layout="hwc" if color and im.ndim == 3 else None)
                calls.append((("resize", name, size, mode),
                              record("resize_f32", (n, h, w, c, size[1], size[0], oracle.RESIZE_MODES[mode]), (),
                                     (im,)), [want]))
    clip = engine_clip()
    for n_seen, st in engine_cases():
        d, bg = oracle.bg_ema_f32(clip, bg=st, n_seen=n_seen, rate=ENGINE_RATE)
        zero = np.zeros(clip.shape[1:], np.float32)
        calls.append((("engine ema", n_seen), record("bg_ema_f32", (len(clip), zero.size, n_seen, 1), (ENGINE_RATE,),
                                                     (clip, zero if st is None else st)), [d, bg]))
        calls.append((("engine gaussian", n_seen), record("gaussian_f32", clip.shape, (ENGINE_SIGMA,), (d,)),
                      [oracle.gaussian_f32(d, ENGINE_SIGMA)]))
    for fr, st, n_seen in ema_f32_cases():
        d, bg = oracle.bg_ema_f32(fr, bg=st, n_seen=n_seen, rate=EMA_RATE)
        calls.append((("ema f32", fr.shape, n_seen), record("bg_ema_f32", (len(fr), st.size, n_seen, 1), (EMA_RATE,),
                                                            (fr, st)), [d, bg]))
    for fr, st, n_seen, want_diff in ema_u8_cases():
        d, bg = oracle.bg_ema_u8(fr, bg=st, n_seen=n_seen, rate=EMA_RATE) if want_diff else (
            None, ema_u8_state_only(oracle, fr, st, n_seen))
        calls.append((("ema u8", fr.shape, n_seen, want_diff),
                      record("bg_ema_u8", (len(fr), st.size, n_seen, int(want_diff)), (EMA_RATE,), (fr, st)),
                      ([d] if want_diff else []) + [bg]))
    for fr, st in static_cases():
        calls.append((("static", fr.shape), record("bg_static_u8", (len(fr), st.size), (), (fr, st)),
                      [oracle.bg_static_u8(fr, st)]))
    for base in mean_base_shapes:
        for n_seen, n, want_diff, fr, st in mean_u8_cases(base):
            d, mean = oracle.bg_mean_u8(fr, mean=st, n_seen=n_seen, want_diff=want_diff)
            calls.append((("mean u8", base, n_seen, n, want_diff),
                          record("bg_mean_u8", (n, st.size, n_seen, int(want_diff)), (), (fr, st)),
                          ([d] if want_diff else []) + [mean]))
    for base in mean_base_shapes:               # (test_mean_u8_through_engine_model_and_running_mean)
        for n_seen in ENGINE_MEAN_N_SEEN:
            fr, st = bounded_mean_case(base, ENGINE_MEAN_N)
            calls.append((("mean u8 bounded", base, n_seen),
                          record("bg_mean_u8", (len(fr), st.size, n_seen, 1), (), (fr, st)),
                          list(oracle.bg_mean_u8(fr, mean=st, n_seen=n_seen))))
            fr, st = mean_u8_case(base, n_seen, ENGINE_MEAN_N, False)
            calls.append((("mean_any u8", base, n_seen),
                          record("mean_any", (len(fr), st.size, n_seen, 0), (), (fr, st)),
                          [oracle.mean_any(fr, st, n_seen)]))
    for fr, mean, m2, n_seen in temporal_cases():
        if fr.dtype == np.float64:
            continue                            # (the oracle's C has no float64 frames: NumPy's restatement)
        px = fr[0].size
        m0 = np.zeros(fr.shape[1:]) if mean is None else mean
        q0 = np.zeros(fr.shape[1:]) if m2 is None else m2
        code = ANY_DTYPES[fr.dtype]
        calls.append((("mean_any", fr.dtype, n_seen), record("mean_any", (len(fr), px, n_seen, code), (), (fr, m0)),
                      [oracle.mean_any(fr, mean, n_seen)]))
        calls.append((("welford_any", fr.dtype, n_seen),
                      record("welford_any", (len(fr), px, n_seen, code), (), (fr, m0, q0)),
                      list(oracle.welford_any(fr, mean, m2, n_seen))))
    fr, st = mean_u8_case(mean_base_shapes[0], 5, 9, False)
    calls.append((("welford_u8",), record("welford_u8", (len(fr), st.size, 5), (), (fr, st, st[::-1].copy())),
                  list(oracle.welford_u8(fr, st, st[::-1].copy(), 5))))
    return calls


def ema_u8_state_only(oracle, frames, state, n_seen):
    """the uint8 EMA's new state without its difference image (oracle.bg_ema_u8 always asks for one, and a NaN state
    has none that C defines): vao_bg_ema_u8 with diff_out = NULL"""
    import ctypes as C
    a = np.ascontiguousarray(frames, np.uint8)
    bg = np.array(state, np.float32)
    oracle.lib().vao_bg_ema_u8(a.ctypes.data_as(C.c_void_p), None, bg.ctypes.data_as(C.c_void_p), int(n_seen),
                               float(EMA_RATE), a.shape[0], int(np.prod(a.shape[1:])))
    return bg
