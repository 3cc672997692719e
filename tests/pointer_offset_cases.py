"""Device buffers entered at unaligned offsets: the late-buffer helper, the case table and its runner (DESIGN.md,
"Pointer offsets").

About twenty launchers choose their kernel from the address of a buffer as well as from the shape.  A case here names
one entry point, its buffers and a reference; the runner calls the entry point through the C ABI with every buffer
entered `late` bytes into a sentinel-filled allocation, for the offset combinations of `offset_combos`, under two
sentinel bytes, and compares every output with the reference bit for bit, every input with what was uploaded, and the
bytes in front of and behind every payload with the sentinel.  The same table runs against the oracle's twin of the
ABI (tests/test_pointer_offsets_host.py: no GPU; it checks the references and the bookkeeping) and against the
product (tests/test_gpu_pointer_offsets.py).

Each case carries, in `gate`, the file and condition of the pointer gate it crosses (or "none": a control case for an
entry point that has no gate today).  Shapes are the smallest at which aligned pointers take the vector kernel, so
that the offset alone changes the path, plus one that takes the byte kernel anyway.

The stream-order suite (tests/stream_order_cases.py; DESIGN.md, "Stream order") runs the same table on a created
stream: every call passes `ON.stream`, which is None here, and every data plane has a decoy (`Arg.decoy`).
"""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_LIB = os.path.join(ROOT, "oracle", "libvideoanalysis_cpu.so")

SENTINELS = (0xA5, 0x5A)        # a write of the sentinel value itself is invisible under one of them only
PAD = 64                        # sentinel bytes behind every payload
# bytes by which a buffer is entered late, by element size: the least offsets that break every gate, keep the 4-byte
# one, and keep the 8-byte one.  Element-type alignment is the caller's duty and is never broken.
OFFSETS = {1: (0, 1, 4, 8), 2: (0, 2, 8), 4: (0, 4, 8), 8: (0, 8)}
U8_LATE, F32_LATE = (0, 1), (0, 4)      # the offsets of a control case: an entry point without a gate today
VA_ERR_INVALID = -22
VA_U8, VA_F32, VA_F64, VA_I16 = 0, 1, 2, 3
BG_MEAN, BG_EMA, BG_STATIC = 1, 2, 3


class _On(object):
    """the stream every case's call is enqueued on: None (the null stream) unless a runner sets another for the time
    of its run (tests/stream_order_cases.py)"""
    stream = None


ON = _On()


def generator(name):
    """a module of tests/golden/make_golden_*.py: the restatements the families' own GPU tests compare with"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ backends
class Backend(object):
    """one implementation of include/videoanalysis_hip.h: the product ("hip") or the oracle's twin ("cpu")"""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def check(self, code):
        assert code == 0, (code, self.lib.va_last_error().decode("utf-8", "replace"))


def cpu_backend():
    import subprocess
    from video import _hip
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libvideoanalysis_cpu.so"],
                          stdout=subprocess.DEVNULL)
    lib = C.CDLL(CPU_LIB)
    for name, (res, args) in _hip.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.va_init(0) == 0
    return Backend(lib, "cpu")


def hip_backend():
    from video import _hip
    return Backend(_hip.lib(), "hip")


# ------------------------------------------------------------------------------------------- a late buffer
class LateBuffer(object):
    """an allocation of max_late + nbytes + PAD bytes whose payload starts `late` bytes in.  arm() fills the whole
    allocation with the sentinel and uploads the payload; collect() downloads the whole allocation, asserts that
    the bytes in [0, late) and behind late + nbytes still hold the sentinel, and returns the payload's bytes."""

    def __init__(self, be, nbytes, max_late):
        self.be, self.nbytes = be, int(nbytes)
        self.size = int(max_late) + self.nbytes + PAD
        self.base = C.c_void_p()
        be.check(be.lib.va_malloc(C.byref(self.base), self.size))
        # the allocator's own alignment, so that `late` alone decides what a gate sees
        assert self.base.value % (256 if be.name == "hip" else 16) == 0, hex(self.base.value)
        self.late = self.sentinel = None

    def arm(self, late, sentinel, payload=None):
        L = self.be.lib
        assert 0 <= late <= self.size - self.nbytes - PAD
        self.late, self.sentinel = int(late), int(sentinel)
        self.be.check(L.va_memset(self.base, self.sentinel, self.size, None))
        if payload is not None:
            payload = np.ascontiguousarray(payload)
            assert payload.nbytes == self.nbytes, (payload.nbytes, self.nbytes)
            self.be.check(L.va_memcpy_h2d(self.base.value + self.late, payload.ctypes.data, payload.nbytes, None))
        self.be.check(L.va_stream_sync(None))
        return self.base.value + self.late

    def collect(self, where):
        L = self.be.lib
        whole = np.empty(self.size, np.uint8)
        self.be.check(L.va_memcpy_d2h(whole.ctypes.data, self.base, whole.nbytes, None))
        self.be.check(L.va_stream_sync(None))
        head, tail = whole[:self.late], whole[self.late + self.nbytes:]
        bad = np.flatnonzero(head != self.sentinel)
        assert not bad.size, "%r: %d byte(s) written in front of the buffer, first at %d (the buffer starts at %d)" % (
            where, bad.size, int(bad[0]), self.late)
        bad = np.flatnonzero(tail != self.sentinel)
        assert not bad.size, "%r: %d byte(s) written behind the buffer, first %d byte(s) past its end" % (
            where, bad.size, int(bad[0]))
        return whole[self.late:self.late + self.nbytes]

    def free(self):
        if self.base.value:
            self.be.lib.va_free(self.base)
            self.base = C.c_void_p()


# -------------------------------------------------------------------------------------------------- cases
class Arg(object):
    """one device buffer of a case.  role: "in" (uploaded, must come back unchanged), "out" (compared with the
    reference), "inout" (uploaded and compared), "work" (entered late and guarded, contents unspecified afterwards:
    consumed inputs and caller scratch), "scratch" (never late: int64 tables and workspaces, whose alignment the
    header asks for).  array: the payload ("in", "inout", optionally "work"), or a function of the oracle that makes
    it on first use (then nbytes and itemsize are given); nbytes may be a function of the library (workspace sizes).
    decoy: a second valid payload of the same shape and dtype for the stream-order runner: None = the payload in
    reverse element order for the data planes ("in", "inout", "work" with a payload; reversal keeps the value domain),
    False = none, or an array.  Tables ("scratch") never have one: a kernel that ran ahead of its inputs must find
    nothing it could use as an address or a trip count but what the case itself passes."""

    def __init__(self, name, role, array=None, nbytes=None, itemsize=None, offsets=None, decoy=None):
        self.name, self.role = name, role
        assert decoy is None or decoy is False or role != "scratch", name
        self._decoy = decoy
        self.array = array if array is None or callable(array) else np.ascontiguousarray(array)
        self._nbytes = self.array.nbytes if nbytes is None else nbytes
        itemsize = itemsize or (self.array.itemsize if isinstance(self.array, np.ndarray) else 1)
        self.offsets = (0,) if role == "scratch" else tuple(offsets or OFFSETS[itemsize])

    def nbytes(self, lib):
        return int(self._nbytes(lib)) if callable(self._nbytes) else int(self._nbytes)

    def resolve(self, oracle):
        if callable(self.array):
            self.array = np.ascontiguousarray(self.array(oracle))
            self.array.setflags(write=False)

    def decoy(self):
        """the decoy payload (after resolve()), or None"""
        if self._decoy is False or self.role in ("out", "scratch") or not isinstance(self.array, np.ndarray):
            return None
        if self._decoy is None:
            return np.ascontiguousarray(self.array.reshape(-1)[::-1]).reshape(self.array.shape)
        decoy = np.ascontiguousarray(self._decoy)
        assert decoy.shape == self.array.shape and decoy.dtype == self.array.dtype, self.name
        return decoy


def out(name, shape, dtype, offsets=None):
    return Arg(name, "out", nbytes=int(np.prod(shape)) * np.dtype(dtype).itemsize, itemsize=np.dtype(dtype).itemsize,
               offsets=offsets)


class Case(object):
    """name; entries: the entry points (hooks included) the case calls; gate: file and condition of the pointer gate
    it crosses; args: its buffers; call(lib, ptr, ctx) -> the first non-zero return code, or 0; ref(oracle) -> {name:
    array} for every "out" / "inout" buffer; setup(lib) -> ctx and teardown(lib, ctx): hooks and handles around the
    offsets of the case; rejects(late) -> True: the call must return VA_ERR_INVALID, name the alignment and leave
    every buffer as it was; False (the default): it must succeed; None: either, never a wrong result; project: {name:
    function(array, refs)} applied to both sides before they are compared (the defined part of an output);
    prepare(lib, ctx): host-side state put back before every call, outside the call itself (it may synchronise);
    rejoin(lib, ctx, stream): makes `stream` wait for whatever the call enqueued elsewhere (a pipeline's side stream)."""

    def __init__(self, name, entries, gate, args, call, ref, setup=None, teardown=None, rejects=None, project=None,
                 prepare=None, rejoin=None):
        self.name, self.gate, self.args, self.call, self.ref = name, gate, list(args), call, ref
        self.entries = (entries,) if isinstance(entries, str) else tuple(entries)
        self.setup, self.teardown, self.rejects, self.project = setup, teardown, rejects, project or {}
        self.prepare, self.rejoin = prepare, rejoin

    def runs_on(self, lib):
        return all(hasattr(lib, e) for e in self.entries)

    def __repr__(self):
        return self.name


def offset_combos(args):
    """the all-zero control; every buffer alone at each of its offsets, the others aligned; and all of them late at
    once by amounts that differ between neighbours (rotations of their offset lists): gates are conjunctions"""
    lists = [a.offsets for a in args]
    combos = [tuple(0 for _ in args)]
    for i, offs in enumerate(lists):
        for o in offs[1:]:
            combos.append(tuple(o if j == i else 0 for j in range(len(args))))
    movable = [i for i, offs in enumerate(lists) if len(offs) > 1]
    if len(movable) > 1:
        for k in range(max(len(lists[i]) - 1 for i in movable)):
            combo = [0] * len(args)
            for pos, i in enumerate(movable):
                nz = lists[i][1:]
                combo[i] = nz[(pos + k) % len(nz)]
            combos.append(tuple(combo))
    seen, unique = set(), []
    for c in combos:
        if c not in seen:
            seen.add(c)
            unique.append(c)
    return unique


_REFS = {}


def reference(case, oracle):
    """computed once per case, for every offset, sentinel and backend, and left unchanged"""
    if case.name not in _REFS:
        refs = {k: np.ascontiguousarray(v) for k, v in case.ref(oracle).items()}
        for r in refs.values():
            r.setflags(write=False)
        _REFS[case.name] = refs
    return _REFS[case.name]


def run_case(be, case, oracle, sentinels=SENTINELS):
    """every offset combination of the case under every sentinel; returns the number of calls made"""
    L = be.lib
    assert case.runs_on(L), case
    refs = reference(case, oracle)
    assert set(refs) == {a.name for a in case.args if a.role in ("out", "inout")}, (case, sorted(refs))
    bufs, ctx, calls = {}, None, 0
    try:
        for a in case.args:
            a.resolve(oracle)
            bufs[a.name] = LateBuffer(be, a.nbytes(L), max(a.offsets))
        ctx = case.setup(L) if case.setup else None
        for sentinel in sentinels:
            for combo in offset_combos(case.args):
                late = {a.name: o for a, o in zip(case.args, combo)}
                where = (case.name, be.name, "0x%02X" % sentinel, late)
                ptr = {a.name: bufs[a.name].arm(late[a.name], sentinel,
                                                a.array if a.role != "out" else None)
                       for a in case.args}
                if case.prepare:
                    case.prepare(L, ctx)
                rc = case.call(L, ptr, ctx)
                calls += 1
                message = L.va_last_error().decode("utf-8", "replace") if rc else ""
                got = {a.name: bufs[a.name].collect(where + (a.name,)) for a in case.args}
                expected = case.rejects(late) if case.rejects else False
                if not any(combo):
                    assert rc == 0, ("the aligned control failed: a broken test, not a kernel bug", where, rc, message)
                if rc != 0:
                    assert expected is not False, (where, rc, message)
                    assert rc == VA_ERR_INVALID and "align" in message, (where, rc, message)
                    for a in case.args:                  # nothing was enqueued
                        if a.role != "out" and a.array is not None:
                            assert got[a.name].tobytes() == a.array.tobytes(), where + (a.name, "after a rejection")
                        else:
                            assert np.all(got[a.name] == sentinel), where + (a.name, "after a rejection")
                    continue
                assert expected is not True, (where, "ran, but the header promises VA_ERR_INVALID")
                for a in case.args:
                    if a.role == "in" or (a.role == "scratch" and a.array is not None):      # (tables are inputs too)
                        assert got[a.name].tobytes() == a.array.tobytes(), where + (a.name, "input changed")
                    elif a.role in ("out", "inout"):
                        want = refs[a.name]
                        g = got[a.name].view(want.dtype).reshape(want.shape)
                        if a.name in case.project:
                            g, want = case.project[a.name](g, refs), case.project[a.name](want, refs)
                        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(want).tobytes(), \
                            where + (a.name, "differs in %d element(s)" % int(np.count_nonzero(g != want)))
    finally:
        if case.teardown:
            case.teardown(L, ctx)
        for b in bufs.values():
            b.free()
    return calls


# ------------------------------------------------------------------------------------------------- inputs
def _u8(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def blob_masks(n, h, w, seed):
    """0/1 masks with a few discs and bars per frame and a little salt: several regions in every frame"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((n, h, w), np.uint8)
    for f in range(n):
        for _ in range(4):
            cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.5, min(h, w) / 4.0)
            m[f][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 1
        m[f, rng.integers(0, h), :] = 1
        m[f].reshape(-1)[rng.choice(h * w, 12, replace=False)] = 1
        m[f, ::5, ::7] = 0
    return m


def _first(*codes):
    for c in codes:
        if c:
            return c
    return 0


CASES = []


def _add(*a, **kw):
    case = Case(*a, **kw)
    assert case.name not in {c.name for c in CASES}, case.name
    CASES.append(case)
    return case


# ---------------------------------------------------------------------------------------------- pointwise
# counts: a full block of 256 threads x 16 px, and the same plus a vector tail and a byte tail
for _count in (4096, 4096 + 16 + 3):
    def _pointwise(count=_count):
        a, b, col = _u8(count, count), _u8(count + 1, count), _u8(count + 2, count, 3)
        alpha = 255 / 170.0

        # gate: va_point.hip launch_threshold_u8, `aligned(src, 16) && aligned(dst, 16)` (slow side: the kernel's
        # byte loop, vec == 0)
        _add("threshold_u8[%d]" % count, "va_threshold_u8",
             "va_point.hip launch_threshold_u8: aligned(src, 16) && aligned(dst, 16)",
             [Arg("src", "in", a), out("dst", a.shape, np.uint8)],
             lambda L, p, _: L.va_threshold_u8(p["src"], p["dst"], count, 100, 255, ON.stream),
             lambda O: {"dst": O.threshold_u8(a, 100)})
        # gate: va_point.hip launch_time_difference, `aligned(a, 8) && aligned(b, 8) && aligned(out, 16)`
        _add("time_difference_u8[%d]" % count, "va_time_difference_u8",
             "va_point.hip launch_time_difference: aligned(a, 8) && aligned(b, 8) && aligned(out, 16)",
             [Arg("a", "in", a), Arg("b", "in", b), out("out", a.shape, np.int16)],
             lambda L, p, _: L.va_time_difference_u8(p["a"], p["b"], p["out"], count, ON.stream),
             lambda O: {"out": O.time_difference_u8(a, b)})
        # gate: va_synth.hip:271 launch_pointwise_u8_x4 (dst % 4), and :107, the kernel's per-row `row_aligned` test of src;
        # slow side: normalize_u8_kernel, one byte per thread
        _add("normalize_u8[%d]" % count, "va_normalize_u8",
             "va_synth.hip:271 launch_pointwise_u8_x4: dst % 4; :107 row_aligned(src) in prepare_u8_x4_kernel",
             [Arg("src", "in", a), out("dst", a.shape, np.uint8)],
             lambda L, p, _: L.va_normalize_u8(p["src"], p["dst"], count, 30.0, 200.0, alpha, 0.0, ON.stream),
             lambda O: {"dst": ((np.clip(a.astype(np.float64), 30, 200) - 30) * alpha + 0).astype(np.int64)
                        .astype(np.uint8)})
        # gate: the same launcher with three channels; slow side: mono_mean_kernel
        _add("mono_mean_u8[%d]" % count, "va_mono_mean_u8",
             "va_synth.hip:271 launch_pointwise_u8_x4 (3 channels): dst % 4; :107 row_aligned(src)",
             [Arg("src", "in", col), out("dst", (count,), np.uint8)],
             lambda L, p, _: L.va_mono_mean_u8(p["src"], p["dst"], count, ON.stream),
             lambda O: {"dst": O.mono_mean_u8(col)})
    _pointwise()


# va_prepare_u8: crop 60 x 10 at (left, 1) of source rows 70 and 64 bytes-per-channel wide: with left = 0 and 4 on the
# 64-wide source every row of the crop starts 4-byte aligned, everywhere else the kernel's per-row test decides
def _prepare_cases():
    alpha = 255 / 170.0
    for sw in (70, 64):
        src = _u8(700 + sw, 2, 12, sw, 3)
        for left in (0, 1, 4):
            for mono, mname in ((-1, "keep"), (3, "mean")):
                for norm in (0, 1):
                    def ref(O, left=left, mono=mono, norm=norm, src=src):
                        crop = src[:, 1:11, left:left + 60].astype(np.float64)
                        v = crop if mono == -1 else (crop.sum(-1) / 3.0).astype(np.uint8).astype(np.float64)
                        if norm:
                            v = ((np.clip(v, 30, 200) - 30) * alpha + 0).astype(np.int64)
                        return {"dst": v.astype(np.uint8)}
                    shape = (2, 10, 60, 3) if mono == -1 else (2, 10, 60)
                    _add("prepare_u8[w%d,left%d,%s,norm%d]" % (sw, left, mname, norm), "va_prepare_u8",
                         "va_synth.hip:250 launch_prepare_u8: (width * out_c) % 4 == 0 && dst % 4 == 0; :107 the per-row row_aligned test",
                         [Arg("src", "in", src), out("dst", shape, np.uint8)],
                         lambda L, p, _, sw=sw, left=left, mono=mono, norm=norm: L.va_prepare_u8(
                             p["src"], p["dst"], 2, 12, sw, 3, left, 1, 60, 10, mono, norm, 30.0, 200.0, alpha, 0.0,
                             ON.stream),
                         ref)


_prepare_cases()


# ------------------------------------------------------------------- background models, temporal statistics
# three frames over two calls (two, then one).  px = 16 * 24: aligned pointers take the vector kernels; 5 * 7: the
# scalar kernels anyway, and the second call's frame pointer is odd by itself.  (The running mean has files of its
# own: test_gpu_bg_mean_paths.py, test_gpu_bg_mean_waits.py.)
def _temporal_cases():
    for shape in ((16, 24), (5, 7)):
        px = shape[0] * shape[1]
        tag = "%dx%d" % shape
        fr8 = _u8(px, 3, *shape)
        fr32 = np.random.default_rng(px + 1).random((3,) + shape, dtype=np.float32)
        fr16 = np.random.default_rng(px + 2).integers(-255, 256, (3,) + shape).astype(np.int16)
        static = np.random.default_rng(px + 3).random(shape) * 255

        def two_calls(fn, itemsize, px=px):
            """fn(frames pointer, difference pointer, n_seen, n) for frames [0, 2) and [2, 3)"""
            def call(L, p, _):
                step = 2 * px * itemsize
                return _first(fn(L, p, p["frames"], p["diff"] if "diff" in p else None, 0, 2),
                              fn(L, p, p["frames"] + step, p["diff"] + step if "diff" in p else None, 2, 1))
            return call

        # gate: va_point.hip launch_bg, EMA u8 and static: `px % kVec == 0 && aligned(fr, 8/16) && aligned(df, 8/16)`
        _add("bg_update[ema,u8,%s]" % tag, "va_bg_update",
             "va_point.hip launch_bg (EMA u8): px % 16 == 0 && aligned(fr, 16) && aligned(df, 16)",
             [Arg("frames", "in", fr8), out("diff", fr8.shape, np.uint8), Arg("state", "inout", np.zeros(shape, np.float32))],
             two_calls(lambda L, p, f, d, seen, n, px=px: L.va_bg_update(BG_EMA, VA_U8, f, d, p["state"], seen, 0.05, n,
                                                                         px, ON.stream), 1),
             lambda O, fr8=fr8: dict(zip(("diff", "state"), O.bg_ema_u8(fr8, rate=0.05))))
        _add("bg_update[ema,f32,%s]" % tag, "va_bg_update",
             "va_point.hip:747 launch_bg (EMA f32): px % 4 == 0 && aligned(fr, 16) && aligned(df, 16)",
             [Arg("frames", "in", fr32), out("diff", fr32.shape, np.float32),
              Arg("state", "inout", np.zeros(shape, np.float32))],
             two_calls(lambda L, p, f, d, seen, n, px=px: L.va_bg_update(BG_EMA, VA_F32, f, d, p["state"], seen, 0.05, n,
                                                                         px, ON.stream), 4),
             lambda O, fr32=fr32: dict(zip(("diff", "state"), O.bg_ema_f32(fr32, rate=0.05))))
        _add("bg_update[static,%s]" % tag, "va_bg_update",
             "va_point.hip launch_bg (static): px % 8 == 0 && aligned(fr, 8) && aligned(df, 8)",
             [Arg("frames", "in", fr8), out("diff", fr8.shape, np.uint8), Arg("state", "in", static)],
             two_calls(lambda L, p, f, d, seen, n, px=px: L.va_bg_update(BG_STATIC, VA_U8, f, d, p["state"], seen, 0.0,
                                                                         n, px, ON.stream), 1),
             lambda O, fr8=fr8, static=static: {"diff": O.bg_static_u8(fr8, static)})
        # gate: va_point.hip:768 launch_welford, `px % 8 == 0 && aligned(frames, 8)`
        _add("welford_u8[%s]" % tag, "va_welford_u8", "va_point.hip:768 launch_welford: px % 8 == 0 && aligned(frames, 8)",
             [Arg("frames", "in", fr8), Arg("mean", "inout", np.zeros(shape)), Arg("m2", "inout", np.zeros(shape))],
             two_calls(lambda L, p, f, d, seen, n, px=px: L.va_welford_u8(f, p["mean"], p["m2"], seen, n, px, ON.stream), 1),
             lambda O, fr8=fr8: dict(zip(("mean", "m2"), O.welford_u8(fr8))))
        for code, fr, name in ((VA_U8, fr8, "u8"), (VA_I16, fr16, "i16"), (VA_F32, fr32, "f32")):
            # no gate: one element per thread (control)
            _add("mean_any[%s,%s]" % (name, tag), "va_mean_any", "none (va_point.hip temporal_stats_kernel: control)",
                 [Arg("frames", "in", fr), Arg("mean", "inout", np.zeros(shape))],
                 two_calls(lambda L, p, f, d, seen, n, px=px, code=code: L.va_mean_any(f, code, p["mean"], seen, n, px,
                                                                                       ON.stream), fr.itemsize),
                 lambda O, fr=fr: {"mean": O.mean_any(fr)})
            _add("welford_any[%s,%s]" % (name, tag), "va_welford_any", "none (va_point.hip temporal_stats_kernel: control)",
                 [Arg("frames", "in", fr), Arg("mean", "inout", np.zeros(shape)), Arg("m2", "inout", np.zeros(shape))],
                 two_calls(lambda L, p, f, d, seen, n, px=px, code=code: L.va_welford_any(f, code, p["mean"], p["m2"],
                                                                                          seen, n, px, ON.stream), fr.itemsize),
                 lambda O, fr=fr: dict(zip(("mean", "m2"), O.welford_any(fr))))


_temporal_cases()


# va_temporal_ranks_u8.  gate: va_median.hip:100, `aligned(frames, 4) && aligned(out, 4) && frame_stride % 4 == 0 &&
# px % 4 == 0` (slow side: byte loads and stores); t = 9: one pass, t = 70: eight passes
def _rank_cases():
    for t in (9, 70):
        for px in (1024, 1023):
            fr = (_u8(t + px, t, px) // 3 * 3)          # (ties)
            ranks = np.array([t // 2, 0, t - 1], np.int32)
            _add("temporal_ranks_u8[t%d,px%d]" % (t, px), "va_temporal_ranks_u8",
                 "va_median.hip:100: aligned(frames, 4) && aligned(out, 4) && frame_stride % 4 == 0 && px % 4 == 0",
                 [Arg("frames", "in", fr), out("out", (3, px), np.uint8)],
                 lambda L, p, _, t=t, px=px, ranks=ranks: L.va_temporal_ranks_u8(p["frames"], t, px, px, ranks.ctypes.data,
                                                                                 3, p["out"], ON.stream),
                 lambda O, fr=fr, ranks=ranks: {"out": np.sort(fr, axis=0)[ranks]})


_rank_cases()


# ----------------------------------------------------------------------------------------------- Gaussian
def _gaussian_cases():
    def u8(name, entry, gate, shape, sigma, dst_offsets=None, rejects=None):
        im = _u8(sum(shape), *shape)
        n, h, w = shape[:3]
        c = shape[3] if len(shape) == 4 else 1
        _add(name, entry, gate, [Arg("src", "in", im), out("dst", shape, np.uint8, dst_offsets)],
             lambda L, p, _: getattr(L, entry)(p["src"], p["dst"], n, h, w, c, sigma, ON.stream),
             lambda O: {"dst": O.gaussian_u8(im, sigma)}, rejects=rejects)

    plan = "va_gauss.hip:370 gaussian_call: src % 16 == 0 && dst % 4 == 0 picks the single-pass families"
    # matrix-core family at aligned pointers (w >= 64, h >= 32, w % 16 == 0); dst late by 4, 8 and 12 keeps it and puts
    # its 16-byte buffer stores (va_gauss_mfma.hip:408) at addresses that are 4-byte aligned only; dst late by 1 or src
    # late by anything: the planes or generic kernels
    for sigma in (1.0, 5.0):
        u8("gaussian_u8[2x32x64,s%g]" % sigma, "va_gaussian_u8",
           plan + "; va_gauss_mfma.hip:437 launch_gauss_mfma_u8: src % 16, dst % 4", (2, 32, 64), sigma, (0, 1, 4, 8, 12))
    # dot4/dot2 family (w < 64): the library's choice, and the forced hook, which must reject or fall back
    u8("gaussian_u8[2x32x32,s1]", "va_gaussian_u8", plan + "; va_gauss_fused.hip:391 launch_gauss_fused_u8: src % 16",
       (2, 32, 32), 1.0)
    u8("gaussian_u8_valu[2x32x32,s1]", "va_gaussian_u8_valu",
       "va_gauss_fused.hip:391 launch_gauss_fused_u8: src % 16 (the forced family rejects, never mis-runs)",
       (2, 32, 32), 1.0, rejects=lambda late: None if late["src"] else False)
    # planes: the interleaved side of channel_planes_kernel crosses `inter_any & 3` (va_point.hip:870) on the way in
    # (src) and on the way out (dst); (w * 3) % 4 != 0 at w = 70 takes the byte side anyway, w = 64 the dword side
    for shape in ((2, 33, 70, 3), (2, 32, 64, 3)):
        u8("gaussian_u8[%s,s1]" % "x".join(map(str, shape)), "va_gaussian_u8",
           "va_point.hip:870 channel_planes_kernel: (w * C) & 3 == 0 && inter_any & 3 == 0", shape, 1.0)
    # frames too small for any single-pass family: the generic two-pass kernels at every offset
    u8("gaussian_u8[2x10x30,s1]", "va_gaussian_u8", "none at this shape (generic kernels: control)", (2, 10, 30), 1.0)

    # float32: vec4 / vec4s / vec4c of va_gauss_f32.hip (src % 16, w % 4; the column pass with dst % 8), and the
    # fused row pass (plan: src % 16); hook 0: the unrolled radius-8 kernels, hook 3: the runtime-radius ones
    for w in (64, 62):
        for hook in (0, 3):
            f = np.random.default_rng(w).random((2, 40, w), dtype=np.float32) * 2 - 0.5

            def setup(L, hook=hook):
                assert L.va_test_hook_gaussian_f32(hook) == 0

            _add("gaussian_f32[2x40x%d,s2,hook%d]" % (w, hook), ("va_gaussian_f32",) + (("va_test_hook_gaussian_f32",)
                                                                                        if hook else ()),
                 "va_gauss.hip:370 gaussian_call (f32): src % 16; va_gauss_f32.hip:466 vec4, :471 vec4s, :479 vec4c (dst % 8)",
                 [Arg("src", "in", f), out("dst", f.shape, np.float32)],
                 lambda L, p, _, w=w: L.va_gaussian_f32(p["src"], p["dst"], 2, 40, w, 1, 2.0, ON.stream),
                 lambda O, f=f: {"dst": O.gaussian_f32(f, 2.0)},
                 setup=setup if hook else None,
                 teardown=(lambda L, _: L.va_test_hook_gaussian_f32(0)) if hook else None)


_gaussian_cases()


# --------------------------------------------------------------------------------------------- morphology
def _morph_cases():
    for w in (64, 62):
        g = _u8(w, 2, 24, w)
        for op, oname in ((0, "erode"), (1, "dilate")):
            for shape, sname, k in ((0, "rect", 5), (1, "cross", 3)):
                # gate: va_morph.hip:770, `w % 4 == 0 && src % 4 == 0 && dst % 4 == 0 && scratch % 4 == 0`
                _add("morph_u8[%s,%s%d,w%d]" % (oname, sname, k, w), "va_morph_u8",
                     "va_morph.hip:770 grey morphology: w % 4 == 0 && src % 4 == 0 && dst % 4 == 0",
                     [Arg("src", "in", g), out("dst", g.shape, np.uint8)],
                     lambda L, p, _, w=w, op=op, shape=shape, k=k: L.va_morph_u8(p["src"], p["dst"], 2, 24, w, op, shape,
                                                                                k, ON.stream),
                     lambda O, g=g, op=op, shape=shape, k=k: {"dst": O.morph_u8(g, op, shape, k)})
    for w in (64, 70):
        b = blob_masks(2, 24, w, seed=w) * np.uint8(255)         # (blobs: neither op gives one value everywhere)
        for op, oname in ((0, "erode"), (1, "dilate")):
            # gates: va_morph.hip:531 (pack) `w % 32 == 0 && aligned(src, 16)`, :545 (unpack) `aligned(dst, 16)`
            _add("morph_bits_u8[%s,w%d]" % (oname, w), "va_morph_bits_u8",
                 "va_morph.hip:531 pack: w % 32 == 0 && aligned(src, 16); :545 unpack: w % 32 == 0 && aligned(dst, 16)",
                 [Arg("src", "in", b), out("dst", b.shape, np.uint8)],
                 lambda L, p, _, w=w, op=op: L.va_morph_bits_u8(p["src"], p["dst"], 2, 24, w, op, 0, 5, ON.stream),
                 lambda O, b=b, op=op: {"dst": O.morph_u8(b, op, 0, 5)})


_morph_cases()


# ---------------------------------------------------------------------------------------------- labelling
# the paths test_gpu_parity iterates (va_test_hook_labelling), and the library's choice
LABEL_PATHS = {"default": (0, 0), "frame-lds": (2, 0), "frame-staged": (4, 0), "frame-large": (2, 7), "chip-wide": (1, 0)}
LABEL_SHAPES = ((3, 16, 32), (3, 16, 64), (3, 16, 128), (3, 17, 70))


def _stats_rows(stats, refs):
    """the defined part of (n, max_labels, 16) statistics: rows below the frame's count, columns 0 .. 13"""
    counts = refs["counts"]
    return np.concatenate([stats[f, :int(counts[f]), :14].ravel() for f in range(len(counts))])


MAX_LABELS = 64                 # room for every frame's regions (asserted by the references)


def _label_reference(O, masks, conn):
    labels, counts = O.label_batch(masks, conn)
    assert 2 <= counts.min() and counts.max() <= MAX_LABELS, counts
    stats = np.zeros((len(masks), MAX_LABELS, 16), np.int64)
    for f in range(len(masks)):
        stats[f, :counts[f]] = O.region_stats(labels[f], int(counts[f]))
    return {"labels": labels, "counts": counts, "stats": stats}


def _largest_reference(O, masks, conn):
    """get_largest_region's choice (first maximum wins) for every frame"""
    r = _label_reference(O, masks, conn)
    areas = r["stats"][:, :, 0]
    largest = (np.argmax(areas, axis=1) + 1).astype(np.int32)
    area = areas[np.arange(len(masks)), largest - 1].astype(np.int64)
    sel = (r["labels"] == largest[:, None, None]).astype(np.uint8)
    return {"largest": largest, "area": area, "sel": sel}


def _label_cases():
    for shape in LABEL_SHAPES:
        n, h, w = shape
        masks = blob_masks(n, h, w, seed=w)
        tag = "x".join(map(str, shape))
        for conn in (4, 8):
            for path, (code, lds_runs) in sorted(LABEL_PATHS.items()):
                def setup(L, code=code, lds_runs=lds_runs):
                    assert L.va_test_hook_labelling(code, lds_runs) == 0

                def call(L, p, _, shape=shape, conn=conn):
                    n, h, w = shape
                    return _first(L.va_label_i32(p["mask"], p["labels"], p["counts"], n, h, w, conn, p["ws"],
                                                 L.va_label_workspace_bytes(n, h, w), ON.stream),
                                  L.va_moments_i64(p["labels"], n, h, w, MAX_LABELS, p["stats"], ON.stream))
                hooked = path != "default"
                # gates: the paint, va_ccl.hip:1804 `w % 4 == 0 && aligned(pl.labels, 16)` (16-byte stores), and the
                # statistics of va_moments_i64 on the late label planes, va_ccl.hip:1534 `x1 - x0 == 32 && (w & 3) == 0
                # && (labels & 15) == 0` (a thread's 32 labels as eight 16-byte loads).  w = 32, 64 and 128 take the
                # vector forms at aligned pointers, w = 70 never.  The mask is read by bytes (late by 1 and 4: control)
                _add("label_i32+moments_i64[%s,conn%d,%s]" % (tag, conn, path),
                     ("va_label_i32", "va_moments_i64") + (("va_test_hook_labelling",) if hooked else ()),
                     "va_ccl.hip:1804 paint: w % 4 == 0 && aligned(pl.labels, 16); va_ccl.hip:1534 statistics: (labels & 15) == 0",
                     [Arg("mask", "in", masks, decoy=blob_masks(n, h, w, seed=w + 1)),     # (other masks: other counts)
                      out("labels", shape, np.int32), out("counts", (n,), np.int32),
                      Arg("ws", "scratch", nbytes=lambda L, shape=shape: L.va_label_workspace_bytes(*shape)),
                      out("stats", (n, MAX_LABELS, 16), np.int64)],
                     call, lambda O, masks=masks, conn=conn: _label_reference(O, masks, conn),
                     setup=setup if hooked else None,
                     teardown=(lambda L, _: L.va_test_hook_labelling(0, 0)) if hooked else None,
                     project={"stats": _stats_rows})

            # va_largest_region on the late label planes of the same masks (no gate today: control)
            def given(key, masks=masks, conn=conn):
                return lambda O: _label_reference(O, masks, conn)[key]
            _add("largest_region[%s,conn%d]" % (tag, conn), "va_largest_region",
                 "none (va_moments.hip: control on the late label planes)",
                 [Arg("labels", "in", given("labels"), nbytes=n * h * w * 4, itemsize=4),
                  Arg("counts", "in", given("counts"), nbytes=n * 4, itemsize=4),
                  Arg("stats", "in", given("stats"), nbytes=n * MAX_LABELS * 128, itemsize=8),
                  out("largest", (n,), np.int32), out("area", (n,), np.int64), out("sel", shape, np.uint8)],
                 lambda L, p, _, shape=shape: L.va_largest_region(p["labels"], p["counts"], p["stats"], shape[0],
                                                                  shape[1], shape[2], MAX_LABELS, p["largest"],
                                                                  p["area"], p["sel"], ON.stream),
                 lambda O, masks=masks, conn=conn: _largest_reference(O, masks, conn))


_label_cases()


# ------------------------------------------------------------------------------------------ resize, rot90
def _resize_rot_cases():
    a = _u8(2440, 2, 24, 40)
    for dh, dw in ((12, 20), (13, 21)):
        for mode, name in ((0, "nearest"), (1, "linear"), (2, "cubic"), (3, "area")):
            # gate: va_resize.hip:438, `c == 1 && dw % 4 == 0 && dst % 4 == 0` (four outputs per thread)
            _add("resize_u8[24x40->%dx%d,%s]" % (dh, dw, name), "va_resize_u8",
                 "va_resize.hip:438: c == 1 && dw % 4 == 0 && dst % 4 == 0",
                 [Arg("src", "in", a), out("dst", (2, dh, dw), np.uint8)],
                 lambda L, p, _, dh=dh, dw=dw, mode=mode: L.va_resize_u8(p["src"], p["dst"], 2, 24, 40, 1, dh, dw, mode,
                                                                         ON.stream),
                 lambda O, dh=dh, dw=dw, name=name: {"dst": O.resize_u8(a, (dw, dh), name)})
    for eb in (1, 3):
        r = _u8(90 + eb, 2, 9, 14, eb)
        for k in (1, 2, 3):
            # no gate: elements are moved one by one (control); elem_bytes 3 is the odd-sized struct
            _add("rot90[elem%d,k%d]" % (eb, k), "va_rot90", "none (va_point.hip rot90_kernel: control)",
                 [Arg("src", "in", r), out("dst", np.rot90(r, k, axes=(1, 2)).shape, np.uint8)],
                 lambda L, p, _, eb=eb, k=k: L.va_rot90(p["src"], p["dst"], 2, 9, 14, eb, k, ON.stream),
                 lambda O, r=r, k=k: {"dst": np.rot90(r, k, axes=(1, 2))})


_resize_rot_cases()


# ----------------------------------------------------------------------------------------------- stencils
def _stencil_cases():
    for w in (32, 30):
        img = (_u8(w, 2, 12, w) // 32 * 32).astype(np.uint8)          # plateaus
        img[1] = _u8(w + 1, 12, w) % 6 * (_u8(w + 2, 12, w) % 2)
        for plateaus in (1, 0):
            # gate: va_stencil.hip:416, `w % 4 == 0 && src % 4 == 0 && dst % 4 == 0` (four pixels per thread)
            _add("detect_peaks_u8[w%d,plateaus%d]" % (w, plateaus), "va_detect_peaks_u8",
                 "va_stencil.hip:416: w % 4 == 0 && src % 4 == 0 && dst % 4 == 0",
                 [Arg("src", "in", img), out("dst", img.shape, np.uint8)],
                 lambda L, p, _, w=w, plateaus=plateaus: L.va_detect_peaks_u8(p["src"], p["dst"], 2, 12, w, plateaus, ON.stream),
                 lambda O, img=img, plateaus=plateaus: {"dst": np.stack([O.detect_peaks(f, bool(plateaus)) for f in img])
                                                        .astype(np.uint8)})
        yy, xx = np.mgrid[:20, :w]
        blob = ((((xx - 14) / 11.0) ** 2 + ((yy - 9) / 6.0) ** 2 <= 1) | (abs(xx - 24) + abs(yy - 8) < 6))
        m = blob.astype(np.uint8) * 255
        # gate: va_stencil.hip:468, `w % 4 == 0 && img % 4 == 0 && eroded % 4 == 0 && skel % 4 == 0`; the image is
        # consumed and the scratch is the caller's: both guarded, neither compared
        _add("mask_thinning_u8[w%d]" % w, "va_mask_thinning_u8",
             "va_stencil.hip:468: w % 4 == 0 && img % 4 == 0 && eroded % 4 == 0 && skel % 4 == 0",
             [Arg("img", "work", m), Arg("tmp", "work", nbytes=m.size), out("skel", m.shape, np.uint8)],
             lambda L, p, _, w=w: L.va_mask_thinning_u8(p["img"], p["tmp"], p["skel"], 20, w, C.byref(C.c_int()), ON.stream),
             lambda O, m=m: {"skel": O.mask_thinning(m)[0]})


_stencil_cases()


# ------------------------------------------------------------------------------------------------ Sobel
def _sobel_cases():
    AG = generator("make_golden_active_contour")
    for w in (16, 15):
        for dt, code in ((np.uint8, VA_U8), (np.float32, VA_F32)):
            x = np.stack([AG.sobel_input(9, w, dt, salt=s) for s in (1, 2)])
            # gate: va_gradients.hip:213, `fx_out % 16 == 0 && fy_out % 16 == 0` (two float64 per store), with a lead
            # element where the item offset is odd
            _add("sobel5_f64[w%d,%s]" % (w, np.dtype(dt).name), "va_sobel5_f64",
                 "va_gradients.hip:213: fx_out % 16 == 0 && fy_out % 16 == 0",
                 [Arg("src", "in", x), out("fx", x.shape, np.float64), out("fy", x.shape, np.float64)],
                 lambda L, p, _, w=w, code=code: L.va_sobel5_f64(p["src"], code, p["fx"], p["fy"], 2, 9, w, ON.stream),
                 lambda O, x=x: dict(zip(("fx", "fy"), AG.sobel5(x))))


_sobel_cases()


def _ragged_gradient_cases():
    AG = generator("make_golden_active_contour")
    # three items, the first of an odd size: item 1 starts at element 25, so its float64 planes are 8-byte aligned
    # only even in aligned buffers (the lead element of the kernel's paired stores)
    shapes = np.array([(5, 5), (6, 9), (3, 4)], np.int32)
    sizes = shapes.prod(axis=1)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sizes.sum())
    items = [AG.sobel_input(h, w, np.float32, salt=7 * k + 1) for k, (h, w) in enumerate(shapes)]
    packed = np.concatenate([p.ravel() for p in items])
    for sigma in (0.0, 1.0):
        def ref(O, sigma=sigma):
            fx, fy = np.zeros(total), np.zeros(total)
            for p, o in zip(items, offsets):
                gx, gy = AG.gradients(p, sigma)
                fx[o:o + p.size], fy[o:o + p.size] = gx.ravel(), gy.ravel()
            return {"fx": fx, "fy": fy, "status": np.zeros(3, np.int32)}
        _add("potential_gradients_ragged[s%g]" % sigma, "va_potential_gradients_ragged",
             "va_gradients.hip ragged kernel: fx_out, fy_out % 16 with a lead element where the item offset is odd",
             [Arg("src", "in", packed), Arg("shapes", "scratch", shapes), Arg("offsets", "scratch", offsets),
              out("fx", (total,), np.float64), out("fy", (total,), np.float64), out("status", (3,), np.int32)],
             lambda L, p, _, sigma=sigma: L.va_potential_gradients_ragged(p["src"], VA_F32, p["shapes"], p["offsets"], total,
                                                                          3, int(sizes.max()), sigma, p["fx"], p["fy"],
                                                                          p["status"], ON.stream),
             ref)


_ragged_gradient_cases()


def _guo_hall_cases():
    TG = generator("make_golden_thinning")
    for w in (32, 30):
        yy, xx = np.mgrid[:20, :w]
        blob = ((((xx - 14) / 11.0) ** 2 + ((yy - 9) / 6.0) ** 2 <= 1) | (abs(xx - 24) + abs(yy - 8) < 6))
        stack = np.stack([blob, blob[::-1, ::-1]]).astype(np.uint8) * np.uint8(255)
        # gate: va_thinning.hip:354, `(w & 3) == 0 && ((src | dst) & 3) == 0` (dword loads of the pack and stores of
        # the unpack)
        _add("guo_hall_thinning_u8[w%d]" % w, ("va_guo_hall_thinning_u8", "va_guo_hall_thinning_scratch_bytes"),
             "va_thinning.hip:354: (w & 3) == 0 && ((src | dst) & 3) == 0",
             [Arg("src", "in", stack, decoy=stack[:, :, ::-1]),     # (mirrored: reversed, this stack is itself)
              out("dst", stack.shape, np.uint8),
              Arg("scratch", "scratch", nbytes=lambda L, w=w: L.va_guo_hall_thinning_scratch_bytes(2, 20, w))],
             lambda L, p, _, w=w: L.va_guo_hall_thinning_u8(p["src"], p["scratch"],
                                                            L.va_guo_hall_thinning_scratch_bytes(2, 20, w), p["dst"], 2, 20,
                                                            w, 0, 0, None, None, ON.stream),
             lambda O, stack=stack: {"dst": np.stack([TG.guo_hall(f)[0] for f in stack])})


_guo_hall_cases()


# ------------------------------------------------------------------------------------------- region links
def _links_rows(links, refs):
    """the records the call wrote: the batch's total (totals[0]) of the capacity"""
    return links[:int(refs["totals"][0])]


def _region_links_cases():
    import region_links_checks as R
    shape = LABEL_SHAPES[-1]
    masks = blob_masks(*shape, seed=shape[2])

    def labels_of(O):
        return _label_reference(O, masks, 8)["labels"]
    n, h, w = shape[0] - 1, shape[1], shape[2]
    cap = h * w                                       # per pair: need <= the pixels that carry both labels

    def ref(O):
        labels = labels_of(O)
        rows, per = R.restate(labels[1:], labels[0])
        need = R.need_of(labels[1:], labels[0])
        assert 0 < len(rows) <= need <= n * cap
        links = np.zeros((n * cap, 4), np.int32)
        links[:len(rows)] = rows
        return {"nlinks": per, "totals": np.array([len(rows), need], np.int64), "links": links}
    # the late label planes of the labelling case: no gate (one pixel per lane: control).  The records and the
    # workspace must be 16-byte aligned (REJECTIONS), so they stay where they are
    _add("region_links[2x17x70]", ("va_region_links", "va_region_links_workspace_bytes"),
         "none (va_links.hip: control on the late label planes)",
         [Arg("prev", "in", lambda O: labels_of(O)[0], nbytes=h * w * 4, itemsize=4),
          Arg("labels", "in", lambda O: labels_of(O)[1:], nbytes=n * h * w * 4, itemsize=4),
          out("nlinks", (n,), np.int32), out("totals", (2,), np.int64),
          out("links", (n * cap, 4), np.int32, offsets=(0,)),
          Arg("ws", "scratch", nbytes=lambda L: L.va_region_links_workspace_bytes(n, h, w, n * cap))],
         lambda L, p, _: L.va_region_links(p["prev"], p["labels"], n, h, w, p["nlinks"], p["totals"], p["links"], n * cap,
                                           p["ws"], L.va_region_links_workspace_bytes(n, h, w, n * cap), ON.stream),
         ref, project={"links": _links_rows})


_region_links_cases()


# ----------------------------------------------------------------------------------------------- composer
def _compose_cases():
    import composer_checks as K
    from video import ops
    for w in (64, 61):
        for c in (1, 3):
            frames = _u8(w + c, 2, 8, w, c) if c == 3 else _u8(w + c, 2, 8, w)
            masks = [(np.random.default_rng(w + f).random((8, w)) < 0.6).astype(np.uint8) * np.uint8(1 + f) for f in (0, 1)]
            layers = [[("highlight", masks[f], None if c == 1 else ("g", None)[f], 100 + 50 * f)] for f in (0, 1)]
            table, off, _, packed = ops._compose_tables(layers, 2, 8, w, c, "compose")
            # gate: va_compose.hip:41 and :61, `valid == NB && (p & 3) == 0` on the 16-pixel lanes of frames and masks
            _add("compose_layers_u8[w%d,c%d]" % (w, c), "va_compose_layers_u8",
                 "va_compose.hip:41, :61: a lane's 16 pixels as dwords when (p & 3) == 0, bytes otherwise",
                 [Arg("src", "in", frames), out("dst", frames.shape, np.uint8), Arg("masks", "in", packed),
                  Arg("layers", "scratch", table.view(np.uint8)), Arg("off", "scratch", off)],
                 lambda L, p, _, w=w, c=c, nb=len(packed): L.va_compose_layers_u8(p["src"], c, p["dst"], 2, 8, w, c,
                                                                                  p["layers"], p["off"], 2, None, 0,
                                                                                  p["masks"], nb, ON.stream),
                 lambda O, frames=frames, layers=layers: {"dst": K.compose_layers(frames, layers)})


_compose_cases()


def _draw_control_cases():
    import composer_checks as K
    from video import ops
    for c in (1, 3):
        frames = _u8(610 + c, 2, 8, 61, c) if c == 3 else _u8(610 + c, 2, 8, 61)
        color = 200 if c == 1 else (10, 200, 90)
        commands = [[("polyline", np.array([(2, 1), (50, 6), (30, 2)]), True, color), ("circle", (20, 4), 3, False, color)],
                    [("circle", (40, 3), 2, True, color)]]
        recs, off, pts = ops._draw_tables(commands, 2, c, "draw")
        # no gate: va_draw_u8 writes single pixels into the frames, in place (control)
        _add("draw_u8[c%d]" % c, "va_draw_u8", "none (va_compose.hip draw kernel, one pixel per store: control)",
             [Arg("frames", "inout", frames, offsets=U8_LATE), Arg("cmds", "scratch", recs.view(np.uint8)),
              Arg("off", "scratch", off), Arg("points", "scratch", np.ascontiguousarray(pts, np.int32)),
              out("status", (2,), np.int32, (0,))],
             lambda L, p, _, c=c, nc=len(recs), npts=len(pts): L.va_draw_u8(p["frames"], 2, 8, 61, c, p["cmds"], p["off"], nc,
                                                                            p["points"], npts, p["status"], ON.stream),
             lambda O, frames=frames, commands=commands: {"frames": K.draw(frames, commands),
                                                         "status": np.zeros(2, np.int32)})


_draw_control_cases()


# ------------------------------------------------------------------------------------------- Motion-JPEG
def _jpeg_cases():
    import jpeg_checks as J
    import jpeg_decode_checks as D
    from video import ops
    for c in (1, 3):
        noise = _u8(160 + c, 2, 16, 24, c) if c == 3 else _u8(160 + c, 2, 16, 24)
        ramp = (np.arange(24) * 6).reshape((1, 1, 24) + ((1,) if c == 3 else ()))
        frames = (ramp + noise // 4).astype(np.uint8)                # a gradient with texture: AC and DC codes
        files = J.encode(frames, 90)
        blob = np.frombuffer(b"".join(files), np.uint8)
        file_off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        head = np.frombuffer(ops.jpeg_header(16, 24, c, 90), np.uint8)
        qt = np.concatenate(ops.jpeg_tables(90))
        # gate: va_jpeg.hip, the encoder's row loads: 8 bytes at once where `(p & 7) == 0`; frames late by 1 and 4
        _add("jpeg_encode_u8[2x16x24,c%d]" % c, "va_jpeg_encode_u8", "va_jpeg.hip:115 row loads: x0 + 8 <= w && (p & 7) == 0",
             [Arg("frames", "in", frames, offsets=(0, 1, 4)), Arg("qtables", "in", qt), Arg("header", "in", head),
              out("sizes", (2,), np.int64), out("offsets", (3,), np.int64), out("totals", (1,), np.int64),
              out("bytes", (len(blob),), np.uint8)],
             lambda L, p, _, c=c, nh=len(head), cap=len(blob): L.va_jpeg_encode_u8(
                 p["frames"], 2, 16, 24, c, p["qtables"], p["header"], nh, p["sizes"], p["offsets"], p["totals"],
                 p["bytes"], cap, ON.stream),
             lambda O, blob=blob, file_off=file_off: {"sizes": np.diff(file_off), "offsets": file_off,
                                                      "totals": file_off[-1:], "bytes": blob})
        # the decoder's pixel stores: 8 bytes at once where `(p & 7) == 0`; the output frames late by 1 and 4
        hd = ops.jpeg_parse_header(files[0])
        tables = np.frombuffer(b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in hd["huff"]),
                               np.uint8)
        scan_begin = np.full(2, hd["scan_begin"], np.int64)
        _add("jpeg_decode_u8[2x16x24,c%d]" % c, ("va_jpeg_decode_u8", "va_jpeg_decode_workspace_bytes"),
             "va_jpeg_decode.hip:321 pixel stores: x0 + 8 <= w && (dst & 7) == 0",
             [Arg("bytes", "in", blob, decoy=False), Arg("offsets", "scratch", file_off), Arg("scan_begin", "scratch", scan_begin),
              Arg("qtables", "in", np.ascontiguousarray(hd["qtables"])), Arg("huff", "scratch", tables),
              out("frames", frames.shape, np.uint8, offsets=(0, 1, 4)), out("status", (2,), np.int32, offsets=(0,)),
              Arg("ws", "scratch", nbytes=lambda L, c=c, ri=hd["ri"]: L.va_jpeg_decode_workspace_bytes(2, 16, 24, c, ri))],
             lambda L, p, _, c=c, ri=hd["ri"], nt=len(tables): L.va_jpeg_decode_u8(
                 p["bytes"], p["offsets"], p["scan_begin"], 2, 16, 24, c, ri, p["qtables"], p["huff"], nt, p["frames"],
                 p["status"], p["ws"], L.va_jpeg_decode_workspace_bytes(2, 16, 24, c, ri), ON.stream),
             lambda O, files=files: {"frames": np.stack([D.decode(f)[0] for f in files]), "status": np.zeros(2, np.int32)})


_jpeg_cases()


def _jpeg_sampled_cases():
    """4:2:0 files: the subsampled encoder's row loads and the subsampled decoder's pixel stores (controls: the
    same helpers as the 4:4:4 calls above, in kernels of their own)"""
    import jpeg_sampled_encode_checks as E
    import jpeg_subsampled_checks as SS
    from video import ops
    noise = _u8(420, 2, 16, 24, 3)
    frames = ((np.arange(24) * 6).reshape(1, 1, 24, 1) + noise // 4).astype(np.uint8)
    files = E.encode(frames, 90, (2, 2))
    blob = np.frombuffer(b"".join(files), np.uint8)
    file_off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    head = np.frombuffer(ops.jpeg_header(16, 24, 3, 90, (2, 2)), np.uint8)
    qt = np.concatenate(ops.jpeg_tables(90))
    _add("jpeg_encode_sampled_u8[2x16x24,4:2:0]", "va_jpeg_encode_sampled_u8", "none (va_jpeg.hip subsampled rows: control)",
         [Arg("frames", "in", frames, offsets=(0, 1, 4)), Arg("qtables", "in", qt), Arg("header", "in", head),
          out("sizes", (2,), np.int64), out("offsets", (3,), np.int64), out("totals", (1,), np.int64),
          out("bytes", (len(blob),), np.uint8)],
         lambda L, p, _: L.va_jpeg_encode_sampled_u8(p["frames"], 2, 16, 24, 3, 2, 2, p["qtables"], p["header"], len(head),
                                                     p["sizes"], p["offsets"], p["totals"], p["bytes"], len(blob), ON.stream),
         lambda O: {"sizes": np.diff(file_off), "offsets": file_off, "totals": file_off[-1:], "bytes": blob})
    hd = ops.jpeg_parse_header(files[0], sampling="any")
    assert tuple(hd["sampling"]) == (2, 2)
    tables = np.frombuffer(b"".join(ops._jpeg_decode_table(*dc) + ops._jpeg_decode_table(*ac) for dc, ac in hd["huff"]),
                           np.uint8)
    ri = hd["ri"]
    _add("jpeg_decode_sampled_u8[2x16x24,4:2:0]", ("va_jpeg_decode_sampled_u8", "va_jpeg_decode_sampled_workspace_bytes"),
         "none (va_jpeg_decode.hip subsampled reconstruction: control)",
         [Arg("bytes", "in", blob, decoy=False), Arg("offsets", "scratch", file_off),
          Arg("scan_begin", "scratch", np.full(2, hd["scan_begin"], np.int64)),
          Arg("qtables", "in", np.ascontiguousarray(hd["qtables"])), Arg("huff", "scratch", tables),
          out("frames", frames.shape, np.uint8, offsets=(0, 1, 4)), out("status", (2,), np.int32, offsets=(0,)),
          Arg("ws", "scratch", nbytes=lambda L: L.va_jpeg_decode_sampled_workspace_bytes(2, 16, 24, 3, ri, 2, 2))],
         lambda L, p, _: L.va_jpeg_decode_sampled_u8(
             p["bytes"], p["offsets"], p["scan_begin"], 2, 16, 24, 3, ri, 2, 2, p["qtables"], p["huff"], len(tables),
             p["frames"], p["status"], p["ws"], L.va_jpeg_decode_sampled_workspace_bytes(2, 16, 24, 3, ri, 2, 2), ON.stream),
         lambda O: {"frames": np.stack([SS.decode(f)[0] for f in files]), "status": np.zeros(2, np.int32)})


_jpeg_sampled_cases()


# ---------------------------------------------------------------------------------------- control cases
# Entry points with a uint8 or float32 plane argument and no pointer gate today: one case each with the plane late
# by 1 byte (uint8) or 4 (float32) at a small shape, so that the next vectorisation of it meets a test.


def _control_cases():
    none = "none (%s: control)"
    im = _u8(3370, 2, 33, 70)
    f = (np.random.default_rng(3371).random((2, 33, 70)) * 200 - 50).astype(np.float32)
    _add("gaussian_u8_rule[2x33x70,cv3]", "va_gaussian_u8_rule", "va_gauss.hip:370 gaussian_call (the cv3 tap set)",
         [Arg("src", "in", im, offsets=U8_LATE), out("dst", im.shape, np.uint8, U8_LATE)],
         lambda L, p, _: L.va_gaussian_u8_rule(p["src"], p["dst"], 2, 33, 70, 1, 2.0, 1, ON.stream),
         lambda O: {"dst": O.gaussian_u8(im, 2.0, tap_rule="cv3")})
    _add("gaussian_u8_generic[2x33x70]", "va_gaussian_u8_generic", none % "va_gauss.hip generic two-pass kernels",
         [Arg("src", "in", im, offsets=U8_LATE), out("dst", im.shape, np.uint8, U8_LATE)],
         lambda L, p, _: L.va_gaussian_u8_generic(p["src"], p["dst"], 2, 33, 70, 1, 2.0, ON.stream),
         lambda O: {"dst": O.gaussian_u8(im, 2.0)})
    peaks = np.random.default_rng(3372).normal(0, 1, (2, 12, 30)).astype(np.float32)
    peaks[1, 4:7, 10:16] = 2.5
    peaks[1][peaks[1] < 0] = 0
    for plateaus in (1, 0):
        _add("detect_peaks_f32[plateaus%d]" % plateaus, "va_detect_peaks_f32", none % "va_stencil.hip float peaks",
             [Arg("src", "in", peaks, offsets=F32_LATE), out("dst", peaks.shape, np.uint8, U8_LATE)],
             lambda L, p, _, plateaus=plateaus: L.va_detect_peaks_f32(p["src"], p["dst"], 2, 12, 30, plateaus, ON.stream),
             lambda O, plateaus=plateaus: {"dst": np.stack([O.detect_peaks(x, bool(plateaus)) for x in peaks])
                                           .astype(np.uint8)})
    for name, src, late in (("u8", im, U8_LATE), ("f32", f, F32_LATE)):
        for kernel, kname, ksize, prior, excl in ((0, "box", 3, 128, 0), (1, "ellipse", 4, 0, 1)):
            def ref(O, src=src, kname=kname, ksize=ksize, prior=prior, excl=excl):
                pairs = [O.image_statistics(x, kname, ksize, prior, bool(excl)) for x in src]
                return {"mean": np.stack([m for m, _ in pairs]), "var": np.stack([v for _, v in pairs])}
            _add("image_statistics_%s[%s%d]" % (name, kname, ksize), "va_image_statistics_" + name,
                 none % "va_stencil.hip window sums",
                 [Arg("src", "in", src, offsets=late), out("mean", src.shape, np.float64), out("var", src.shape, np.float64)],
                 lambda L, p, _, name=name, kernel=kernel, ksize=ksize, prior=prior, excl=excl: getattr(
                     L, "va_image_statistics_" + name)(p["src"], p["mean"], p["var"], 2, 33, 70, kernel, ksize, float(prior),
                                                       excl, ON.stream),
                 ref)
    # va_normalize: uint8 -> float32 and float32 -> uint8 (NumPy's types: float64 arithmetic on uint8 frames, float32 on
    # float32 frames)
    import special_values_checks as S
    unit = (f / 200).astype(np.float32)
    _add("normalize[u8->f32]", "va_normalize", none % "va_synth.hip normalize, one element per thread",
         [Arg("src", "in", im, offsets=U8_LATE), out("dst", im.shape, np.float32, F32_LATE)],
         lambda L, p, _: L.va_normalize(p["src"], VA_U8, p["dst"], VA_F32, im.size, 30.0, 200.0, 1.0 / 170.0, 0.0, ON.stream),
         lambda O: {"dst": ((np.clip(im.astype(np.float64), 30, 200) - 30) * (1.0 / 170.0) + 0).astype(np.float32)})
    _add("normalize[f32->u8]", "va_normalize", none % "va_synth.hip normalize, one element per thread",
         [Arg("src", "in", unit, offsets=F32_LATE), out("dst", im.shape, np.uint8, U8_LATE)],
         lambda L, p, _: L.va_normalize(p["src"], VA_F32, p["dst"], VA_U8, unit.size, 0.25, 0.75, 510.0, 0.0, ON.stream),
         lambda O: {"dst": S.normalize_numpy(unit, 0.25, 0.75, 510.0, 0.0, np.uint8)})
    rf = np.random.default_rng(3373).random((2, 24, 40), dtype=np.float32)
    _add("resize_f32[24x40->13x21,linear]", "va_resize_f32", none % "va_resize.hip float32 frames",
         [Arg("src", "in", rf, offsets=F32_LATE), out("dst", (2, 13, 21), np.float32, F32_LATE)],
         lambda L, p, _: L.va_resize_f32(p["src"], p["dst"], 2, 24, 40, 1, 13, 21, 1, ON.stream),
         lambda O: {"dst": O.resize_f32(rf, (21, 13), "linear")})

    # contours of blob masks: the mask plane late; the int32 / int64 tables stay aligned (REJECTIONS)
    masks = blob_masks(2, 17, 70, seed=71)

    def contours_ref(O):
        found = [O.find_contours_external_simple(m) for m in masks]
        per = np.array([len(c) for c in found], np.int32)
        flat = [np.asarray(c, np.int32).reshape(-1, 2) for frame in found for c in frame]
        off = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int64)
        assert 2 <= per.min() and per.sum() <= 64 and off[-1] <= 1024
        points, point_off = np.zeros((1024, 2), np.int32), np.zeros(65, np.int64)
        points[:off[-1]] = np.concatenate(flat)
        point_off[:len(off)] = off
        return {"ncontours": per, "totals": np.array([per.sum(), off[-1]], np.int64), "point_off": point_off,
                "points": points}
    _add("find_contours[2x17x70]", ("va_find_contours", "va_find_contours_workspace_bytes"),
         none % "va_contours.hip border following",
         [Arg("mask", "in", masks, offsets=U8_LATE, decoy=blob_masks(2, 17, 70, seed=72)),      # (a turn keeps the totals)
          out("ncontours", (2,), np.int32, (0,)),
          out("totals", (2,), np.int64, (0,)), Arg("info", "scratch", nbytes=64 * 48),
          out("point_off", (65,), np.int64, (0,)), out("points", (1024, 2), np.int32, (0,)),
          Arg("ws", "scratch", nbytes=lambda L: L.va_find_contours_workspace_bytes(2, 17, 70))],
         lambda L, p, _: L.va_find_contours(p["mask"], 2, 17, 70, p["ncontours"], p["totals"], p["info"], p["point_off"], 64,
                                            p["points"], 1024, p["ws"], L.va_find_contours_workspace_bytes(2, 17, 70), ON.stream),
         contours_ref,
         project={"point_off": lambda a, r: a[:int(r["totals"][0]) + 1], "points": lambda a, r: a[:int(r["totals"][1])]})

    def largest_ref(O):
        r = {"points": np.zeros((2, 256, 2), np.int32), "npoints": np.zeros(2, np.int32), "area": np.zeros(2),
             "ncomp": np.zeros(2, np.int32)}
        for k, m in enumerate(masks):
            contour, area = O.get_contour_from_largest_region(m, ret_area=True)
            pts = np.asarray(contour, np.int32).reshape(-1, 2)
            r["points"][k, :len(pts)], r["npoints"][k], r["area"][k] = pts, len(pts), area
            r["ncomp"][k] = O.label(m, 8)[1]
        return r
    _add("largest_contour[2x17x70]", ("va_largest_contour", "va_contour_workspace_bytes"),
         none % "va_contours.hip border following",
         [Arg("mask", "in", masks, offsets=U8_LATE), out("points", (2, 256, 2), np.int32, (0,)),
          out("npoints", (2,), np.int32, (0,)), out("area", (2,), np.float64, (0,)), out("ncomp", (2,), np.int32, (0,)),
          Arg("ws", "scratch", nbytes=lambda L: L.va_contour_workspace_bytes(2, 17, 70))],
         lambda L, p, _: L.va_largest_contour(p["mask"], 2, 17, 70, p["points"], 256, p["npoints"], p["area"], p["ncomp"],
                                              p["ws"], L.va_contour_workspace_bytes(2, 17, 70), ON.stream),
         largest_ref,
         project={"points": lambda a, r: np.concatenate([a[k, :int(r["npoints"][k])].ravel() for k in range(2)])})

    # Farneback flow of the smallest pair stack of the family's own test, uint8 and float32 frames late
    OG = generator("make_golden_optflow")
    params = OG.params_of({})
    for dt, code, late in ((np.uint8, VA_U8, U8_LATE), (np.float32, VA_F32, F32_LATE)):
        fr = OG.texture_frames(2, 9, 11, 104, step=(0, 1))
        fr = np.ascontiguousarray(fr if dt == np.uint8 else fr.astype(np.float32))
        args = (float(params["pyr_scale"]), int(params["levels"]), int(params["winsize"]), int(params["iterations"]),
                int(params["poly_n"]))
        _add("optical_flow_farneback[%s,2x9x11]" % np.dtype(dt).name,
             ("va_optical_flow_farneback", "va_farneback_workspace_bytes"), none % "va_optflow.hip",
             [Arg("frames", "in", fr, offsets=late), out("flow", (1, 9, 11, 2), np.float32, F32_LATE),
              out("mag", (1, 9, 11), np.float32, F32_LATE),
              Arg("ws", "scratch", nbytes=lambda L, args=args: L.va_farneback_workspace_bytes(2, 9, 11, *args))],
             lambda L, p, _, code=code, args=args: L.va_optical_flow_farneback(
                 p["frames"], code, 2, 9, 11, *args, float(params["poly_sigma"]), 0, p["flow"], p["mag"], p["ws"],
                 L.va_farneback_workspace_bytes(2, 9, 11, *args), ON.stream),
             lambda O, fr=fr: dict(zip(("flow", "mag"), OG.optical_flow(fr, **params))))


_control_cases()


def _ragged_control_cases():
    """the ragged packed layouts (shapes int32 (m, 2), element offsets int64): three items whose sizes are odd, so
    that the second and third start at odd addresses even in an aligned buffer"""
    none = "none (%s: control)"
    PG = generator("make_golden_polygon")
    TG = generator("make_golden_thinning")
    rng = np.random.default_rng(77)
    items = []
    for h, w in ((7, 9), (5, 13), (11, 6)):
        yy, xx = np.mgrid[:h, :w]
        m = ((xx - w / 2.0) ** 2 / (w / 2.2) ** 2 + (yy - h / 2.0) ** 2 / (h / 2.2) ** 2 <= 1) | (rng.random((h, w)) < 0.15)
        items.append(m.astype(np.uint8))
    shapes = np.array([a.shape for a in items], np.int32)
    sizes = [a.size for a in items]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sum(sizes))
    flat = np.concatenate([a.ravel() for a in items])
    tables = [Arg("shapes", "scratch", shapes), Arg("offsets", "scratch", offsets)]

    def packed(planes, dtype):
        return np.concatenate([np.asarray(p, dtype).ravel() for p in planes])
    _add("distance_transform_l2_5[3 items]", "va_distance_transform_l2_5", none % "va_polygon.hip",
         [Arg("masks", "in", flat, offsets=U8_LATE)] + tables
         + [out("out", (total,), np.float32, F32_LATE), out("status", (3,), np.int32, (0,))],
         lambda L, p, _: L.va_distance_transform_l2_5(p["masks"], p["shapes"], p["offsets"], total, 3,
                                                      int(shapes[:, 1].max()), p["out"], p["status"], ON.stream),
         lambda O: {"out": packed([PG.distance_transform(m) for m in items], np.float32), "status": np.zeros(3, np.int32)})
    _add("guo_hall_thinning_batch[3 items]", "va_guo_hall_thinning_batch", none % "va_thinning.hip resident kernel",
         [Arg("masks", "in", flat, offsets=U8_LATE)] + tables
         + [out("out", (total,), np.uint8, U8_LATE), out("iterations", (3,), np.int32, (0,)),
            out("status", (3,), np.int32, (0,))],
         lambda L, p, _: L.va_guo_hall_thinning_batch(p["masks"], p["shapes"], p["offsets"], total, 3,
                                                      max(h * ((w + 31) // 32) for h, w in shapes.tolist()), p["out"],
                                                      p["iterations"], p["status"], ON.stream),
         lambda O: {"out": packed([TG.guo_hall(m)[0] for m in items], np.uint8),
                    "iterations": np.array([TG.guo_hall(m)[1] for m in items], np.int32), "status": np.zeros(3, np.int32)})
    # va_fill_poly writes the ragged masks: uint8 planes late by 1, int32 planes by 4
    names = list(PG.FILL_POLYS)[:3]
    boxes = np.array([PG.bounding_rect(PG.FILL_POLYS[n], 1) for n in names], np.int64)
    contours = [np.asarray(PG.FILL_POLYS[n], np.float64).astype(np.int64).reshape(-1, 2) for n in names]
    verts = np.ascontiguousarray(np.concatenate(contours), np.int32)
    vert_off = np.concatenate([[0], np.cumsum([len(c) for c in contours])]).astype(np.int64)
    fsizes = (boxes[:, 2] * boxes[:, 3]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(fsizes)[:-1]]).astype(np.int64)
    ftotal = int(fsizes.sum())
    for dt, late in ((np.uint8, U8_LATE), (np.int32, F32_LATE)):
        _add("fill_poly[%s]" % np.dtype(dt).name, "va_fill_poly", none % "va_polygon.hip scanline fill",
             [Arg("verts", "in", verts, offsets=(0,)), Arg("vert_off", "scratch", vert_off),      # (coordinates: a decoy)
              Arg("boxes", "scratch", boxes.astype(np.int32)),
              Arg("out_off", "scratch", out_off), out("out", (ftotal,), dt, late), out("status", (3,), np.int32, (0,))],
             lambda L, p, _, dt=dt: L.va_fill_poly(p["verts"], p["vert_off"], len(verts), p["boxes"], p["out_off"], ftotal, 3,
                                                   np.dtype(dt).itemsize, p["out"], p["status"], ON.stream),
             lambda O, dt=dt: {"out": packed([PG.fill_poly(c, b) for c, b in zip(contours, boxes)], dt),
                               "status": np.zeros(3, np.int32)})


_ragged_control_cases()


def _warp_and_geodesic_control_cases():
    none = "none (%s: control)"
    from video import ops
    LG = generator("make_golden_line_scan")
    frames = _u8(2030, 2, 20, 30)
    # two warps of odd sizes: the second destination starts at an odd byte even in an aligned buffer
    sizes = np.array([(9, 13), (16, 21)], np.int64)
    mats = np.array([[[0.9, 0.3, 1.5], [-0.3, 0.9, 4.0]], [[1.1, -0.2, -2.0], [0.2, 1.1, 1.0]]])
    fidx = np.array([0, 1], np.int32)
    out_off = np.array([0, 9 * 13], np.int64)
    total = int(sizes.prod(axis=1).sum())
    tiles = np.maximum(1, (-(-sizes[:, 0] // ops.WARP_TILE_H)) * (-(-sizes[:, 1] // ops.WARP_TILE_W)))
    prefix, ntiles = ops._work_prefix(tiles, "warp")
    _add("warp_affine_u8[2 items]", "va_warp_affine_u8", none % "va_warp.hip",
         [Arg("frames", "in", frames, offsets=U8_LATE), Arg("fidx", "scratch", fidx), Arg("mats", "scratch", mats),
          Arg("shapes", "scratch", sizes.astype(np.int32)), Arg("flags", "scratch", np.zeros(2, np.int32)),
          Arg("out_off", "scratch", out_off), Arg("prefix", "scratch", prefix), out("out", (total,), np.uint8, U8_LATE),
          out("status", (2,), np.int32, (0,))],
         lambda L, p, _: L.va_warp_affine_u8(p["frames"], 2, 20, 30, 2, p["fidx"], p["mats"], p["shapes"], p["flags"],
                                             p["out_off"], p["prefix"], ntiles, total, p["out"], p["status"], ON.stream),
         lambda O: {"out": np.concatenate([LG.warp_affine(frames[f], M, (int(s[1]), int(s[0]))).ravel()
                                           for f, M, s in zip(fidx, mats, sizes)]), "status": np.zeros(2, np.int32)})
    p1, p2, hw = np.array([(3.0, 4.0), (25.0, 2.0)]), np.array([(26.0, 15.0), (6.0, 17.0)]), np.array([2.5, 3.0])
    smats, rows, cols = ops.line_scan_tables(p1, p2, hw)
    s_off = np.array([0, cols[0]], np.int64)
    stotal = int(cols.sum())
    sprefix, chunks = ops._work_prefix(np.maximum(1, -(-cols // ops.WARP_CHUNK)), "scan")
    _add("line_scan_u8[2 scans]", "va_line_scan_u8", none % "va_warp.hip",
         [Arg("frames", "in", frames, offsets=U8_LATE), Arg("fidx", "scratch", fidx), Arg("mats", "scratch", smats),
          Arg("shapes", "scratch", np.stack([rows, cols], 1).astype(np.int32)), Arg("out_off", "scratch", s_off),
          Arg("prefix", "scratch", sprefix), out("sums", (stotal,), np.int32, (0,)), out("status", (2,), np.int32, (0,))],
         lambda L, p, _: L.va_line_scan_u8(p["frames"], 2, 20, 30, 2, p["fidx"], p["mats"], p["shapes"], p["out_off"],
                                           p["prefix"], chunks, stotal, p["sums"], p["status"], ON.stream),
         lambda O: {"sums": np.concatenate([LG.line_scan_strip(frames[f], a, b, w)[1].sum(axis=0, dtype=np.int64)
                                            for f, a, b, w in zip(fidx, p1, p2, hw)]).astype(np.int32),
                    "status": np.zeros(2, np.int32)})

    # geodesic maps: the smallest mask of the family's fixture that has a path and a hundred pixels or more
    geo = np.load(os.path.join(ROOT, "tests", "golden", "geodesic_v1.npz"), allow_pickle=False)
    names = [n for n in geo["names"] if tuple(geo[n + "/path_end"]) != (-1, -1) and geo[n + "/mask"].any()
             and geo[n + "/mask"].size >= 100]
    name = sorted(names, key=lambda n: geo[n + "/mask"].size)[0]
    mask = geo[name + "/mask"]
    h, w = mask.shape
    fillable = (mask == 1).astype(np.uint8)
    starts = np.asarray(geo[name + "/starts"], np.int32).reshape(1, -1, 2)
    ends = np.asarray(geo[name + "/ends"], np.int32).reshape(1, -1, 2)
    tables = [Arg("starts", "scratch", starts), Arg("nstarts", "scratch", np.array([starts.shape[1]], np.int32))]
    if ends.shape[1]:
        tables += [Arg("ends", "scratch", ends), Arg("nends", "scratch", np.array([ends.shape[1]], np.int32))]
    ws = Arg("ws", "scratch", nbytes=lambda L: L.va_geodesic_workspace_bytes(1, h, w))
    _add("distance_map_i32[%s]" % name, ("va_distance_map_i32", "va_geodesic_workspace_bytes"), none % "va_geodesic.hip",
         [Arg("fillable", "in", fillable, offsets=U8_LATE, decoy=np.ones_like(fillable))] + tables + [out("map", (h, w), np.int32, F32_LATE), ws],
         lambda L, p, _: L.va_distance_map_i32(p["fillable"], 1, h, w, p["starts"], p["nstarts"], starts.shape[1],
                                               p.get("ends"), p.get("nends"), ends.shape[1], p["map"], p["ws"],
                                               L.va_geodesic_workspace_bytes(1, h, w), ON.stream),
         lambda O: {"map": np.where(fillable != 0, geo[name + "/map"], 0).astype(np.int32)})
    fg = (mask != 0).astype(np.uint8)            # (the decoys: no walls.  This corridor is its own mirror image)
    _add("farthest_points[%s]" % name, ("va_farthest_points", "va_geodesic_workspace_bytes"), none % "va_geodesic.hip",
         [Arg("mask", "in", fg, offsets=U8_LATE, decoy=np.ones_like(fg)), Arg("p1", "scratch", np.asarray(geo[name + "/fp_p1_in"], np.int32)),
          out("p1_out", (1, 2), np.int32, (0,)), out("p2_out", (1, 2), np.int32, (0,)), Arg("dist", "scratch", nbytes=4),
          Arg("rounds", "scratch", nbytes=8), ws],
         lambda L, p, _: L.va_farthest_points(p["mask"], 1, h, w, p["p1"], p["p1_out"], p["p2_out"], p["dist"], p["rounds"],
                                              None, 0, None, p["ws"], L.va_geodesic_workspace_bytes(1, h, w), ON.stream),
         lambda O: {"p1_out": np.asarray(geo[name + "/fp"][0], np.int32).reshape(1, 2),
                    "p2_out": np.asarray(geo[name + "/fp"][1], np.int32).reshape(1, 2)})


_warp_and_geodesic_control_cases()


def _skeleton_control_case():
    from video import ops
    SG = generator("make_golden_skeleton_graph")
    cases = sorted(SG.all_cases().items(), key=lambda kv: (-min(len(SG.skeleton_graph(kv[1])[1]), 1), kv[1].size, kv[0]))
    items = [np.ascontiguousarray(m, np.uint8) for _, m in cases[:3]]          # the three smallest that have an edge
    shapes = np.array([a.shape for a in items], np.int32)
    sizes = [a.size for a in items]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sum(sizes))
    graphs = [SG.skeleton_graph(m) for m in items]
    nn, ne = sum(len(g[0]) for g in graphs), sum(len(g[1]) for g in graphs)
    npts = sum(len(c) for g in graphs for c in g[3])
    assert ne >= 1 and nn >= 2

    def ref(O):
        nodes, edges = np.zeros(nn, ops.SKELETON_NODE_DTYPE), np.zeros(ne, ops.SKELETON_EDGE_DTYPE)
        counts, a, b = np.zeros((3, 2), np.int32), 0, 0
        for k, (gn, ge, gl, _) in enumerate(graphs):
            counts[k] = len(gn), len(ge)
            for name, col in (("x", 0), ("y", 1), ("degree", 2), ("pixels", 3)):
                nodes[name][a:a + len(gn)] = np.asarray(gn).reshape(-1, 4)[:, col]
            nodes["item"][a:a + len(gn)] = k
            for name, col in (("node_a", 0), ("node_b", 1), ("npoints", 2)):
                edges[name][b:b + len(ge)] = np.asarray(ge).reshape(-1, 3)[:, col]
            edges["item"][b:b + len(ge)], edges["length"][b:b + len(ge)] = k, gl
            a, b = a + len(gn), b + len(ge)
        curves = [np.asarray(c, np.int32).reshape(-1, 2) for g in graphs for c in g[3]]
        return {"counts": counts, "totals": np.array([nn, ne, npts], np.int64), "nodes": nodes.view(np.uint8),
                "edges": edges.view(np.uint8), "points": np.concatenate(curves),
                "point_off": np.concatenate([[0], np.cumsum([len(c) for c in curves])]).astype(np.int64)}
    _add("skeleton_graph[3 items]", ("va_skeleton_graph", "va_skeleton_graph_workspace_bytes"),
         "none (va_skeleton.hip: control)",
         [Arg("masks", "in", np.concatenate([a.ravel() for a in items]), offsets=U8_LATE, decoy=np.zeros(total, np.uint8)),
          Arg("shapes", "scratch", shapes),     # (the decoy: empty items.  Reversed, these items are themselves)
          Arg("offsets", "scratch", offsets), out("counts", (3, 2), np.int32, (0,)), out("totals", (3,), np.int64, (0,)),
          out("nodes", (nn * 20,), np.uint8, (0,)), out("edges", (ne * 24,), np.uint8, (0,)),
          out("point_off", (ne + 1,), np.int64, (0,)), out("points", (npts, 2), np.int32, (0,)),
          Arg("ws", "scratch", nbytes=lambda L: L.va_skeleton_graph_workspace_bytes(total, 3))],
         lambda L, p, _: L.va_skeleton_graph(p["masks"], p["shapes"], p["offsets"], total, 3, p["counts"], p["totals"],
                                             p["nodes"], nn, p["edges"], p["point_off"], ne, p["points"], npts, p["ws"],
                                             L.va_skeleton_graph_workspace_bytes(total, 3), ON.stream),
         ref)


_skeleton_control_case()


# ---------------------------------------------------------------------------------------------- pipelines
def pipeline_clip(n, h, w, seed=0):
    """noise around a drifting level with bright blobs: masks with several regions, with and without a model"""
    rng = np.random.default_rng(1000 + seed + w)
    yy, xx = np.mgrid[:h, :w]
    clip = np.empty((n, h, w), np.uint8)
    for t in range(n):
        f = rng.normal(90, 12, (h, w))
        for cx, cy, r in ((8 + 5 * t, 9, 5), (w - 14 - 3 * t, h - 10, 6), (w // 2, h // 2 + t, 3)):
            f[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] += 70
        clip[t] = np.clip(f, 0, 255).astype(np.uint8)
    return clip


def chain_reference(O, clip, background, sigma, thresh, close, conn, mean=None, n_seen=0):
    """filtered, mask, labels, counts and the background state of FilterBackground('mean') -> FilterBlur ->
    FilterThreshold -> 5 x 5 close -> labelling, stage by stage from the oracle"""
    state = None
    diff = clip
    if background:
        diff, state = O.bg_mean_u8(clip, mean=mean, n_seen=n_seen)
    r = {"filtered": O.gaussian_u8(diff, sigma), "state": state}
    m = O.threshold_u8(r["filtered"], thresh)
    if close:
        m = O.morph_u8(O.morph_u8(m, O.DILATE, O.RECT, 5), O.ERODE, O.RECT, 5)
    r["mask"] = m
    assert 0.02 < np.count_nonzero(m) / m.size < 0.9, np.count_nonzero(m) / m.size
    if conn:
        r["labels"], r["counts"] = O.label_batch(m, conn)
        assert r["counts"].min() >= 1
    return r


def make_pipeline(L, w, h, n, background, sigma, thresh, close, conn, dtype=VA_U8, channels=1, bg_rate=0.0):
    """va_pipeline_create through the C ABI; background: True (the running mean), False, or a VA_BG_* code; returns
    the handle"""
    from video import _hip
    cfg = _hip.va_config()
    cfg.struct_size = C.sizeof(_hip.va_config)
    cfg.width, cfg.height, cfg.channels, cfg.dtype, cfg.max_batch = w, h, channels, dtype, n
    cfg.bg_mode = BG_MEAN if background is True else int(background or 0)
    cfg.bg_rate, cfg.sigma, cfg.thresh, cfg.maxval = bg_rate, sigma, thresh, 255
    cfg.morph_count = 2 if close else 0
    for i, op in enumerate((1, 0) if close else ()):         # dilate, erode: a close
        cfg.morph_op[i], cfg.morph_shape[i], cfg.morph_ksize[i] = op, 0, 5
    cfg.connectivity, cfg.max_labels, cfg.tap_rule = conn, 0, 0
    handle = C.c_void_p()
    rc = L.va_pipeline_create(C.byref(cfg), C.byref(handle))
    assert rc == 0, L.va_last_error()
    return handle


PIPELINE_THRESH = {True: 25, False: 120}        # with a background model (difference images), without one


def _pipeline_cases():
    def add(name, gate, shape, background, outputs, close, conn, family, frame_offsets, offsets=None, rejects=None):
        n, h, w = shape
        clip = pipeline_clip(n, h, w)
        thresh = PIPELINE_THRESH[bool(background)]
        offsets = offsets or {}
        shapes = {"filtered": (shape, np.uint8), "mask": (shape, np.uint8), "labels": (shape, np.int32),
                  "counts": ((n,), np.int32)}

        def setup(L):
            p = make_pipeline(L, w, h, n, background, 1.0, thresh, close, conn)
            assert ("gauss=%s(" % family).encode() in L.va_pipeline_describe(p), L.va_pipeline_describe(p)
            return p

        def prepare(L, p):
            if background:
                assert L.va_bg_set_state(p, None, 0, 0) == 0              # every run starts a fresh model

        def call(L, ptr, p):
            return L.va_pipeline_run(p, ptr["frames"], n, ptr.get("filtered"), ptr.get("mask"), ptr.get("labels"),
                                     ptr.get("counts"), None, ON.stream)

        def ref(O):
            r = chain_reference(O, clip, background, 1.0, thresh, close, conn)
            return {k: r[k] for k in outputs}
        _add(name, ("va_pipeline_create", "va_pipeline_run", "va_pipeline_describe", "va_bg_set_state"), gate,
             # (the decoy under a model: the first frame twice, so the second frame's difference image is empty)
             [Arg("frames", "in", clip, offsets=frame_offsets, decoy=np.repeat(clip[:1], n, 0) if background else None)]
             + [out(k, shapes[k][0], shapes[k][1], offsets.get(k)) for k in outputs],
             call, ref, setup=setup, teardown=lambda L, p: p is not None and L.va_pipeline_destroy(p), rejects=rejects,
             prepare=prepare, rejoin=lambda L, p, stream: L.va_pipeline_fence(p, stream))

    for background in (True, False):
        bg = "mean" if background else "none"
        # the full chain on 32 x 64 at sigma = 1: the matrix-core Gaussian writes the bit mask itself.  Without a model
        # it reads frames_dev (va_gauss_mfma.hip:437: src % 16), so late frames are rejected at the top of
        # va_pipeline_run (va_api.hip); with one it reads the pipeline's difference image and late frames run.
        # mask_out: launch_unpack_bits (va_morph.hip:545); labels_out: the paint (va_ccl.hip: aligned(pl.labels, 16)).
        add("pipeline[32x64,%s,close,ccl4]" % bg,
            "va_api.hip va_pipeline_run: single-pass Gaussian needs frames_dev % 16 without a model; va_morph.hip:545; "
            "va_ccl.hip paint", (2, 32, 64), background, ("mask", "labels", "counts"), True, 4, "mfma-i8", (0, 1, 8),
            {"mask": (0, 1), "labels": (0, 4, 8), "counts": (0, 4)},
            rejects=None if background else (lambda late: late["frames"] % 16 != 0))
        # the same with filtered_out: 16-byte buffer stores (va_gauss_mfma.hip:408) at a dst that is 4-byte aligned
        # only; a dst that is not is rejected up front, whatever the background mode
        add("pipeline[32x64,%s,close,ccl4,filtered]" % bg,
            "va_api.hip va_pipeline_run: filtered_out_dev % 4 for mfma-i8; va_gauss_mfma.hip:408 16-byte stores",
            (2, 32, 64), background, ("filtered", "mask", "labels", "counts"), True, 4, "mfma-i8", (0, 1, 8),
            {"filtered": (0, 1, 4, 8, 12), "mask": (0, 1), "labels": (0, 4, 8), "counts": (0, 4)},
            rejects=lambda late, background=background: (late["filtered"] % 4 != 0
                                                         or (not background and late["frames"] % 16 != 0)))
        # the chain ends at the threshold: the byte-mask epilogue gate at va_api.hip:647 (mask_out % 4), whose slow
        # side is the bit mask and the unpack pass
        add("pipeline[32x64,%s,threshold]" % bg, "va_api.hip:647 byte-mask epilogue: mask_out % 4 == 0",
            (2, 32, 64), background, ("mask",), False, 0, "mfma-i8", (0,), {"mask": (0, 1, 4)})
        # 33 x 70: no single-pass family (planes), every pointer late, nothing to reject
        add("pipeline[33x70,%s,close,ccl4,filtered]" % bg,
            "va_point.hip:870 channel_planes_kernel; va_morph.hip:531 pack, :545 unpack; va_ccl.hip paint",
            (2, 33, 70), background, ("filtered", "mask", "labels", "counts"), True, 4, "mfma-i8-planes", (0, 1, 8),
            {"labels": (0, 4, 8), "counts": (0, 4)})


_pipeline_cases()


BY_NAME = {c.name: c for c in CASES}


# --------------------------------------------------------------------------------------------- rejections
# The calls whose header promises VA_ERR_INVALID for a misaligned pointer.  An argument list holds plain values and
# pointers ptr(name, alignment): alignment 0 for a pointer the call does not check.  Every list passes the guards in
# front of the alignment one, which runs before anything is enqueued, so the buffers need not hold meaningful data:
# the host test hands out made-up addresses, the GPU test sentinel-filled buffers that must come back untouched.
class ptr(object):
    def __init__(self, name, align=0):
        self.name, self.align = name, align


_I64 = [ptr("sizes_out", 8), ptr("offsets_out", 8), ptr("totals", 8)]
_DECODE = [ptr("bytes"), ptr("offsets", 8), ptr("scan_begin", 8)]
ROOM = 1 << 40      # workspace_bytes: the size guards come after the alignment ones
REJECTIONS = {
    "va_find_contours": [ptr("mask"), 1, 4, 4, ptr("ncontours"), ptr("totals", 8), ptr("info", 8), ptr("point_off", 8), 1,
                         ptr("points", 8), 1, ptr("workspace"), ROOM, None],
    "va_skeleton_graph": [ptr("masks"), ptr("shapes"), ptr("offsets"), 16, 1, ptr("counts", 4), ptr("totals", 8),
                          ptr("nodes", 4), 1, ptr("edges", 8), ptr("point_off", 8), 1, ptr("points", 8), 1,
                          ptr("workspace", 8), ROOM, None],
    "va_region_links": [ptr("prev", 4), ptr("labels", 4), 1, 4, 4, ptr("nlinks", 4), ptr("totals", 8), ptr("links", 16), 4,
                        ptr("workspace", 16), ROOM, None],
    "va_simplify_rdp": [ptr("points", 8), ptr("point_off", 8), 4, 1, ptr("eps", 8), ptr("keep"), ptr("out_count", 4),
                        ptr("status", 4), None],
    "va_simplify_visvalingam": [ptr("points", 8), ptr("point_off", 8), 4, 1, ptr("thr", 8), 0, ptr("keep"),
                                ptr("out_count", 4), ptr("status", 4), ptr("workspace", 8), ROOM, None],
    "va_curves_equidistant": [ptr("points", 8), ptr("point_off", 8), 4, 1, ptr("spacing", 8), ptr("count", 4),
                              ptr("translate", 8), ptr("out_count", 4), ptr("out_off", 8), ptr("in_length", 8),
                              ptr("status", 4), ptr("totals", 8), ptr("out_points", 8), 4, ptr("out_length", 8), None],
    "va_compose_layers_u8": [ptr("src"), 1, ptr("dst"), 1, 4, 4, 1, ptr("layers", 8), ptr("layer_off", 8), 1, None, 0,
                             ptr("masks"), 16, None],
    "va_draw_u8": [ptr("frames"), 1, 4, 4, 1, ptr("cmds", 8), ptr("cmd_off", 8), 1, ptr("points", 4), 1, ptr("status", 4),
                   None],
    "va_draw_contours_u8": [ptr("frames"), 1, 4, 4, 1, ptr("info", 8), ptr("point_off", 8), 1, ptr("points", 4), 1,
                            ptr("frame_map", 4), 1, 255, ptr("status", 4), None],
    "va_jpeg_encode_u8": [ptr("frames"), 1, 8, 8, 1, ptr("qtables"), ptr("header"), 16] + _I64 + [ptr("bytes_out"), 64,
                                                                                                  None],
    "va_jpeg_encode_sampled_u8": [ptr("frames"), 1, 8, 8, 3, 2, 2, ptr("qtables"), ptr("header"), 16] + _I64
    + [ptr("bytes_out"), 64, None],
    "va_jpeg_encode_optimized_u8": [ptr("frames"), 1, 8, 8, 3, 2, 2, ptr("qtables"), ptr("pre"), 8, ptr("post"), 8,
                                    ptr("bits_vals_out")] + _I64 + [ptr("bytes_out"), 64, None],
    "va_jpeg_optimal_tables": [ptr("freq", 8), 1, ptr("bits_vals_out"), None],
    "va_jpeg_decode_u8": _DECODE + [1, 8, 8, 1, 1, ptr("qtables"), ptr("huff", 4), 2 * 1416, ptr("frames_out"),
                                    ptr("status_out", 4), ptr("workspace", 16), ROOM, None],
    "va_jpeg_decode_sampled_u8": _DECODE + [1, 8, 8, 3, 1, 2, 2, ptr("qtables"), ptr("huff", 4), 6 * 1416,
                                            ptr("frames_out"), ptr("status_out", 4), ptr("workspace", 16), ROOM, None],
    "va_jpeg_decode_split_u8": _DECODE + [1, 8, 8, 3, 2, 2, ptr("qtables"), ptr("huff", 4), 6 * 1416, ptr("frames_out"),
                                          ptr("status_out", 4), ptr("workspace", 16), ROOM, 256, 16, 1024,
                                          ptr("rounds_out", 4), None],
}


def rejection_calls(entry):
    """[(name of the misaligned pointer, bytes it is moved by)] of an entry: every pointer the call checks, moved by
    half its alignment"""
    return [(a.name, a.align // 2) for a in REJECTIONS[entry] if isinstance(a, ptr) and a.align]


def rejection_args(entry, address, moved=None, by=0):
    """the argument list with address(name) for every pointer, the pointer `moved` late by `by` bytes"""
    return [a if not isinstance(a, ptr) else address(a.name) + (by if a.name == moved else 0) for a in REJECTIONS[entry]]
