#!/usr/bin/env python3
"""Generates tests/golden/reference_v1.npz -- results of the reference's OWN functions on the
cv2-free part of the analysis path.

    python tests/golden/make_golden_reference.py <reference checkout>      (or set $VA_REFERENCE)

The functions are lifted out of the checkout with `ast` at run time and executed in a namespace of
shims; none of their source is stored.  Without a checkout the script exits non-zero and writes
nothing: the point is the reference's own output, so there is no fallback restatement.

Lifted: video/analysis/video.py measure_mean, measure_mean_std; video/analysis/regions.py
rect_to_slices, find_bounding_box, get_largest_region; video/analysis/image.py detect_peaks,
regionprops; video/filters.py COLOR_CHANNELS, get_color_range, FilterNormalize, _check_coordinate,
FilterCrop, FilterMonochrome, FilterDiffBase, FilterTimeDifference.

Shims, and why none of them can change a result:
  np.int -> np.int64              NumPy 2 removed the alias of the platform integer (int64 here)
  xrange -> range                 the Python 3 name of the same iteration
  display_progress -> identity    it only wraps an iterator to report progress
  logger -> a no-op               logging only
  utils.math.get_number_range -> (-inf, inf)   it only feeds FilterNormalize's two warnings
  cached_property() -> property   caching only; each property is read once per instance here
  VideoFilterBase -> a stub that keeps `size`, `frame_count` and `_source` and whose
                     `_process_frame` returns the frame (the base only stores the geometry and
                     hands frames on)
  ndimage.measurements -> scipy.ndimage   the removed module path of the same `label`
  `local_max - eroded_background` in detect_peaks -> `local_max ^ eroded_background`, by an `ast`
                     transform of that one expression: boolean `-` was XOR before NumPy 1.9 and
                     raises since.  Every case asserts eroded_background <= local_max, where XOR
                     equals AND-NOT.

Casting.  The reference ran under legacy value-based casting; the installed NumPy 2 follows NEP 50.
The cases are chosen so that both rules give the same dtypes and values:
  * measure_mean `frame/(n + 1)`: uint8 / int16 frames give float64 under both rules, float32
    frames float32 under both (n + 1 <= 300 is exact in float32), float64 frames float64.
    measure_mean_std's `frame - mean` is float64 under both.
  * FilterNormalize `(frame - fmin)*alpha + tmin`: uint8 frames get integer bounds in 0..255 (learnt
    ones are uint8 scalars), so `frame - fmin` is uint8 and `*alpha` float64 under both.  float32
    frames compute in float32 under both: with learnt bounds alpha = int / float32 scalar is a
    float32 scalar under NEP 50 and a float64 one under legacy casting, which the float32 array
    product rounds to float32 -- the same value, since float32(float64(a/b)) is the correctly
    rounded float32 quotient of float32 a, b (53 >= 2*24 + 2).  Explicit bounds of float32 frames
    are Python floats, weak under both rules.
  * FilterTimeDifference: uint8 frames and dtype=int16, the only dtype the GPU path takes.

Large cases store no input: it is built from the integer hash `((i * 2654435761) >> 13) & 255` in
uint64 (`hashed`), and the case keeps the sha256 of the reference's output and a strided sample.
No RNG stream is used, so two runs write identical arrays.
"""
import ast
import hashlib
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_v1.npz")

SHIMS = ("np.int -> np.int64", "xrange -> range", "display_progress -> identity", "logger -> no-op",
         "utils.math.get_number_range -> (-inf, inf)", "cached_property() -> property",
         "VideoFilterBase -> stub (size, frame_count, _process_frame returns the frame)",
         "ndimage.measurements -> scipy.ndimage",
         "detect_peaks: local_max - eroded_background -> local_max ^ eroded_background")

HASHED_ABOVE = 256          # temporal outputs of more pixels than this are stored as sha256 + sample


# ---------------------------------------------------------------------------- inputs
def hashed(shape, salt=0):
    """uint8 array ((i * 2654435761) >> 13) & 255 over the flat index i (+ salt), in uint64"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(salt)
    return (((i * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(255)).astype(np.uint8).reshape(shape)


def hashed_wide(shape, salt=0):
    """the same hash with 32 useful bits (for the wider dtypes)"""
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(salt)
    return (((i * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFFFFFF)).reshape(shape)


def frames_of(gen, n, h, w, salt):
    """deterministic frames of every temporal-statistics dtype"""
    if gen in ("u8", "u8big"):
        return hashed((n, h, w), salt)
    k = hashed_wide((n, h, w), salt)
    if gen == "i16":                                     # FilterTimeDifference's range, +-255
        return ((k % 511).astype(np.int64) - 255).astype(np.int16)
    if gen == "i16x":                                    # the int16 extremes
        v = (k & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).copy()
        v.reshape(-1)[::7] = -32768
        v.reshape(-1)[3::7] = 32767
        return v
    if gen == "f32":                                     # negatives and non-trivial mantissas
        return (((k % 2000001).astype(np.float64) - 1000000) * 0.001).astype(np.float32)
    if gen == "f64":
        return ((k % 2000001).astype(np.float64) - 1000000) / 7.0
    raise ValueError(gen)


def digest(a):
    """sha256 over dtype, shape and bytes"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


# ---------------------------------------------------------------------------- lifting
class _NoLog(object):
    def __getattr__(self, name):
        return lambda *a, **k: None


class _FilterBaseStub(object):
    """what the lifted filters need of VideoFilterBase"""

    def __init__(self, source, size=None, frame_count=None, is_color=None):
        self._source = source
        self.size = tuple(size) if size is not None else tuple(source.size)
        self.frame_count = frame_count if frame_count is not None else getattr(source, "frame_count", None)
        self.is_color = is_color

    def _process_frame(self, frame):
        return frame


class _PeaksXor(ast.NodeTransformer):
    """`local_max - eroded_background` -> `local_max ^ eroded_background`, preceded by the subset check"""
    count = 0

    def visit_Assign(self, node):
        v = node.value
        if (isinstance(v, ast.BinOp) and isinstance(v.op, ast.Sub) and isinstance(v.left, ast.Name)
                and v.left.id == "local_max" and isinstance(v.right, ast.Name) and v.right.id == "eroded_background"):
            _PeaksXor.count += 1
            node.value = ast.copy_location(ast.BinOp(left=v.left, op=ast.BitXor(), right=v.right), v)
            check = ast.parse("_assert_subset(eroded_background, local_max)").body[0]
            return [ast.copy_location(check, node), node]
        return node


def _assert_subset(eroded_background, local_max):
    assert not np.any(eroded_background & ~local_max), "eroded background outside local_max: XOR != AND-NOT"


def _lift(path, names, ns, transformer=None):
    tree = ast.parse(open(path).read(), path)
    keep, found = [], set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            keep.append(node)
            found.add(node.name)
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in node.targets):
            keep.append(node)
            found.update(t.id for t in node.targets if isinstance(t, ast.Name))
    missing = set(names) - found
    if missing:
        raise SystemExit("%s: not found in the checkout: %s" % (path, sorted(missing)))
    mod = ast.Module(body=keep, type_ignores=[])
    if transformer is not None:
        mod = transformer.visit(mod)
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)


def load_reference(root):
    """namespace with the reference's functions, compiled from its source at run time"""
    import scipy.ndimage
    np_shim = type(sys)("np_shim")
    np_shim.__dict__.update(np.__dict__)
    np_shim.int = np.int64
    nd_shim = type(sys)("ndimage_shim")
    nd_shim.__dict__.update(scipy.ndimage.__dict__)
    nd_shim.measurements = scipy.ndimage
    ns = {"np": np_shim, "ndimage": nd_shim, "xrange": range, "display_progress": lambda it, *a, **k: it,
          "logger": _NoLog(), "get_number_range": lambda dtype: (-np.inf, np.inf),
          "cached_property": lambda *a, **k: property, "VideoFilterBase": _FilterBaseStub,
          "logging": logging, "_assert_subset": _assert_subset, "__name__": "reference_lifted"}
    a = os.path.join(root, "video", "analysis")
    _lift(os.path.join(a, "video.py"), ("measure_mean", "measure_mean_std"), ns)
    _lift(os.path.join(a, "regions.py"), ("rect_to_slices", "find_bounding_box", "get_largest_region"), ns)
    _PeaksXor.count = 0
    _lift(os.path.join(a, "image.py"), ("detect_peaks", "regionprops"), ns, _PeaksXor())
    if _PeaksXor.count != 1:
        raise SystemExit("detect_peaks: expected one `local_max - eroded_background`, found %d" % _PeaksXor.count)
    _lift(os.path.join(root, "video", "filters.py"),
          ("COLOR_CHANNELS", "get_color_range", "FilterNormalize", "_check_coordinate", "FilterCrop",
           "FilterMonochrome", "FilterDiffBase", "FilterTimeDifference"), ns)
    return ns


class Source(object):
    """a video as the lifted filters see it: `size` = (width, height) and `frame_count`"""

    def __init__(self, frames):
        self.frames = np.asarray(frames)
        self.size = (self.frames.shape[2], self.frames.shape[1])
        self.frame_count = len(self.frames)


# ---------------------------------------------------------------------------- cases
def temporal_specs():
    """(name, generator, n, h, w, salt) of the formula-built temporal cases"""
    specs = []
    for gen in ("u8", "i16", "f32", "f64"):
        for n in (1, 2, 3, 4, 31, 32, 33, 65, 300):
            specs.append(("%s_n%d_7x13" % (gen, n), gen, n, 7, 13))
        for h, w in ((1, 1), (3, 5), (17, 64)):
            specs.append(("%s_n33_%dx%d" % (gen, h, w), gen, 33, h, w))
        specs.append(("%s_n2_17x64" % gen, gen, 2, 17, 64))
    specs.append(("i16x_n65_7x13", "i16x", 65, 7, 13))
    specs.append(("i16x_n2_3x5", "i16x", 2, 3, 5))
    return [s + (1 + 977 * (k + 1),) for k, s in enumerate(specs)]


def temporal_cases(R, data, names):
    """measure_mean / measure_mean_std (video/analysis/video.py:26-55)"""
    for name, gen, n, h, w, salt in temporal_specs():
        put_temporal(R, data, names, name, frames_of(gen, n, h, w, salt), gen=gen, salt=salt)
    # constant and alternating uint8 videos (stored: they are tiny)
    for name, video in (("u8_const0_n33", np.zeros((33, 3, 5), np.uint8)),
                        ("u8_const255_n65", np.full((65, 3, 5), 255, np.uint8)),
                        ("u8_alt_n33", np.stack([np.full((3, 5), 255 * (k % 2), np.uint8) for k in range(33)])),
                        ("u8_alt_n300", np.stack([np.full((2, 3), 255 * (k % 2), np.uint8) for k in range(300)])),
                        ("u8_alt_rev_n31", np.stack([np.full((2, 3), 255 * ((k + 1) % 2), np.uint8)
                                                     for k in range(31)]))):
        put_temporal(R, data, names, name, video)
    put_temporal(R, data, names, "u8_hashed_40x1080x1920", frames_of("u8big", 40, 1080, 1920, 12345),
                 gen="u8big", salt=12345)


def put_temporal(R, data, names, name, video, gen=None, salt=None):
    key = "mean/" + name
    names.append(key)
    mean = R["measure_mean"](video)
    ms = R["measure_mean_std"](video)
    data[key + "/shape"] = np.array(video.shape, np.int64)
    data[key + "/dtype"] = np.array(video.dtype.str)
    if gen is None:
        data[key + "/input"] = video
    else:
        data[key + "/gen"] = np.array(gen)
        data[key + "/salt"] = np.array(salt, np.int64)
    for k, v in (("mean", np.asarray(mean)), ("ms_mean", np.asarray(ms[0])), ("ms_std", np.asarray(ms[1]))):
        if v.size > HASHED_ABOVE:
            data[key + "/" + k + "_sha256"] = np.array(digest(v))
            data[key + "/" + k + "_sample"] = v.reshape(-1)[::97].copy()
        else:
            data[key + "/" + k] = v


def region_masks():
    out = []
    m = np.zeros((20, 20), np.uint8)
    m[2:5, 3:6] = 1
    m[10:12, 12:15] = 1
    out.append(("two_blobs", m))                            # gaps in the occupied rows and columns
    t = np.zeros((9, 12), np.uint8)
    t[1:3, 1:3] = 1
    t[5:7, 7:9] = 1
    out.append(("tie_equal_area", t))                       # the first label wins
    t2 = np.zeros((9, 12), np.uint8)
    t2[6:8, 1:3] = 1
    t2[1:3, 8:10] = 1
    out.append(("tie_raster_order", t2))
    d = np.zeros((6, 6), np.uint8)
    d[1, 1] = d[2, 2] = d[3, 3] = d[3, 4] = 1
    out.append(("diagonal_contact", d))                     # separate regions under 4-connectivity
    c = np.zeros((7, 9), np.uint8)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = 1
    out.append(("corners", c))
    out.append(("full", np.ones((5, 8), np.uint8)))
    out.append(("row_1xN", (hashed((1, 37), 5) > 90).astype(np.uint8)))
    out.append(("col_Nx1", (hashed((29, 1), 6) > 90).astype(np.uint8)))
    g = np.zeros((10, 10), np.uint8)
    g[2, 3] = g[2, 7] = g[6, 3] = 1
    out.append(("gap_pixels", g))
    g2 = np.zeros((10, 10), np.uint8)
    g2[1:4, 2:8] = 1
    g2[6:9, 2:8] = 1
    g2[1:9, 2] = 1
    out.append(("c_shape", g2))                             # one region, contiguous rows and columns
    g3 = np.zeros((12, 14), np.uint8)
    g3[3:9, 4] = 1
    g3[3:9, 9] = 1
    g3[3, 4:10] = 1
    out.append(("u_shape", g3))
    s = np.zeros((11, 13), np.uint8)
    s[4, 5] = 1
    out.append(("single_pixel", s))
    out.append(("hashed_48x64", (hashed((48, 64), 77) > 150).astype(np.uint8)))
    b2 = np.zeros((40, 50), bool)
    b2[5:20, 8:30] = hashed((15, 22), 3) > 40
    out.append(("bool_block", b2))
    out.append(("empty", np.zeros((6, 7), np.uint8)))
    return out


def region_cases(R, data, names):
    """get_largest_region / find_bounding_box (video/analysis/regions.py:113-174)"""
    for name, mask in region_masks():
        key = "regions/" + name
        names.append(key)
        data[key + "/mask"] = mask
        try:
            data[key + "/bbox"] = np.array(R["find_bounding_box"](mask), np.int64)
        except IndexError:
            data[key + "/bbox_error"] = np.array("IndexError")
        try:
            region, area = R["get_largest_region"](mask, ret_area=True)
            assert np.array_equal(region, R["get_largest_region"](mask))
            data[key + "/largest"] = np.asarray(region)
            data[key + "/area"] = np.array(area, np.int64)
        except ValueError:
            data[key + "/largest_error"] = np.array("ValueError")


def peak_images():
    out = []
    for h in (1, 2, 3):
        for w in (4, 5, 6, 7):
            out.append(("u8_%dx%d" % (h, w), hashed((h, w), 31 * h + w) // 64))
    for w in (8, 9, 10, 11, 64, 67):
        out.append(("u8_13x%d" % w, hashed((13, w), w) // 32))
    p = np.zeros((9, 12), np.uint8)
    p[2:5, 2:6] = 7
    p[4, 8] = 3
    p[6:9, 9:12] = 200                                      # a plateau touching the border
    p[7, 0] = 1
    out.append(("u8_plateaus", p))
    z = hashed((16, 20), 9) // 128
    z[:, :3] = 0
    z[-4:, :] = 0                                           # zero background touching the border
    out.append(("u8_zero_border", z))
    out.append(("u8_zeros", np.zeros((5, 8), np.uint8)))
    out.append(("u8_const", np.full((6, 9), 17, np.uint8)))
    f = (hashed((11, 13), 21).astype(np.float32) - 128) / 8
    f[0, 0] = -0.0
    f[3, 4] = 0.0
    f[3, 5] = -0.0
    f[5, 6] = np.inf
    f[8, 1] = -np.inf
    f[10, 12] = np.inf
    f[2, 2:5] = 3.5
    out.append(("f32_signed", f))
    g = np.zeros((7, 10), np.float32)
    g[1, 1] = -0.0
    g[4, 5:8] = -2.0
    g[2, 8] = 1e-30
    g[6, 0] = -np.inf
    out.append(("f32_zeros_negzero", g))
    out.append(("f32_1x1", np.array([[-3.0]], np.float32)))
    out.append(("f32_1x5", np.array([[1.0, -np.inf, 2.0, 2.0, np.inf]], np.float32)))
    return out


def peak_cases(R, data, names):
    """detect_peaks (video/analysis/image.py:267-306), both include_plateaus"""
    for name, img in peak_images():
        key = "peaks/" + name
        names.append(key)
        data[key + "/img"] = img
        for plateaus in (1, 0):
            data[key + "/peaks_%d" % plateaus] = np.asarray(R["detect_peaks"](img, bool(plateaus)), bool)
    # batches whose h*w is not a multiple of 4: every frame is an image of its own
    for bname, (n, h, w) in (("batch_3x5x7", (3, 5, 7)), ("batch_4x3x3", (4, 3, 3)), ("batch_5x2x6", (5, 2, 6)),
                             ("batch_3x3x8", (3, 3, 8))):
        key = "peaks/" + bname
        names.append(key)
        imgs = hashed((n, h, w), 1000 + n * h * w) // 64
        imgs[1, 0, :] = 0
        data[key + "/img"] = imgs
        for plateaus in (1, 0):
            data[key + "/peaks_%d" % plateaus] = np.stack([np.asarray(R["detect_peaks"](im, bool(plateaus)), bool)
                                                           for im in imgs])
    key = "peaks/u8_hashed_1080x1920"
    names.append(key)
    img = hashed((1080, 1920), 4242) // 16
    data[key + "/salt"] = np.array(4242, np.int64)
    for plateaus in (1, 0):
        r = np.asarray(R["detect_peaks"](img, bool(plateaus)), bool)
        data[key + "/peaks_%d_sha256" % plateaus] = np.array(digest(r))
        data[key + "/peaks_%d_sample" % plateaus] = r.reshape(-1)[::997].copy()


def normalize_cases(R, data, names):
    """FilterNormalize._process_frame (video/filters.py:101-135); frame 0 supplies what is not given"""
    specs = []
    u8 = hashed((3, 6, 40), 55)
    u8[1, 0, :4] = (0, 255, 1, 254)
    for fmax in (3, 7, 51, 200, 255):
        specs.append(("u8_to_u8_0_%d" % fmax, u8, 0, fmax, None))
    for fmin, fmax in ((10, 17), (20, 220), (1, 254), (100, 107)):
        specs.append(("u8_to_u8_%d_%d" % (fmin, fmax), u8, fmin, fmax, np.uint8))
    learn = hashed((3, 6, 40), 56)
    learn[0] = np.clip(learn[0], 30, 190)                  # later frames hold values outside the learnt bounds
    specs.append(("u8_learnt", learn, None, None, None))
    specs.append(("u8_learnt_to_f32", learn, None, None, np.float32))
    specs.append(("u8_learnt_to_f64", learn, None, None, np.float64))
    specs.append(("u8_to_f32_7_250", u8, 7, 250, np.float32))
    specs.append(("u8_to_f64_3_9", u8, 3, 9, np.float64))
    f = (hashed((3, 6, 40), 57).astype(np.float32) - 100) / np.float32(37)
    f[0, 0, 0], f[0, 0, 1] = np.float32(-1.25), np.float32(3.75)
    specs.append(("f32_learnt", f, None, None, None))
    specs.append(("f32_learnt_to_u8", f, None, None, np.uint8))
    specs.append(("f32_learnt_to_f64", f, None, None, np.float64))
    specs.append(("f32_to_u8_0_1.5", f, 0.0, 1.5, np.uint8))
    specs.append(("f32_to_u8_-0.3_0.7", f, -0.3, 0.7, np.uint8))
    specs.append(("f32_to_f32_-1_2", f, -1.0, 2.0, np.float32))
    specs.append(("f32_to_f64_-0.9_2.1", f, -0.9, 2.1, np.float64))
    # ramps whose (f - fmin)*alpha lands on an integer or one ulp below one
    g = np.tile(np.arange(0, 256, dtype=np.uint8), (2, 1, 1))
    for fmin, fmax in ((0, 3), (0, 5), (0, 7), (0, 9), (0, 11), (0, 13), (0, 49), (0, 51), (0, 99), (0, 127),
                       (2, 9), (5, 12), (60, 109)):
        specs.append(("u8_ramp_%d_%d" % (fmin, fmax), g, fmin, fmax, np.uint8))
    odd = np.tile(np.arange(0, 255, dtype=np.uint8), (2, 1, 1)).reshape(2, 3, 85)     # no 4-byte rows
    for fmin, fmax in ((0, 7), (0, 13), (5, 12)):
        specs.append(("u8_odd_ramp_%d_%d" % (fmin, fmax), odd, fmin, fmax, np.uint8))
    fr = (np.arange(0, 512, dtype=np.float32) / np.float32(64)).reshape(2, 1, 256)
    for fmin, fmax in ((0.0, 0.75), (0.0, 3.0), (0.125, 2.875), (0.3, 7.3)):
        specs.append(("f32_ramp_%g_%g" % (fmin, fmax), fr, fmin, fmax, np.uint8))
    for name, frames, vmin, vmax, dtype in specs:
        key = "normalize/" + name
        names.append(key)
        filt = R["FilterNormalize"](Source(frames), vmin, vmax, dtype)
        outs = [filt._process_frame(np.array(x)) for x in frames]
        data[key + "/frames"] = frames
        data[key + "/vmin"] = np.array(np.nan if vmin is None else vmin, np.float64)
        data[key + "/vmax"] = np.array(np.nan if vmax is None else vmax, np.float64)
        data[key + "/dtype"] = np.array("" if dtype is None else np.dtype(dtype).str)
        data[key + "/out"] = np.stack(outs)


CROPS = [("rect_int", "mono", [dict(rect=[4, 2, 10, 8])]),
         ("rect_fraction", "mono", [dict(rect=[0.25, 0.5, 0.5, 0.25])]),
         ("rect_negative", "mono", [dict(rect=[-10, -6, 7, 5])]),
         ("rect_neg_fraction", "mono", [dict(rect=[-0.5, -0.75, 0.3, 0.2])]),
         ("upper_left", "mono", [dict(region="upper left")]),
         ("lower_right", "mono", [dict(region="lower right")]),
         ("region_right", "col3", [dict(region="right")]),
         ("channel_name", "col3", [dict(rect=[3, 4, 12, 9], color_channel="green")]),
         ("channel_r", "col3", [dict(region="lower", color_channel="r")]),
         ("channel_idx4", "col4", [dict(rect=[2, 2, 9, 9], color_channel=2)]),
         ("align4", "mono", [dict(rect=[1, 3, 13, 10], size_alignment=4)]),
         ("align3", "mono", [dict(rect=[0, 0, 11, 7], size_alignment=3)]),
         ("nested", "mono", [dict(rect=[4, 2, 20, 18]), dict(rect=[1, 3, 9, 6])]),
         ("nested_channel", "col3", [dict(rect=[5, 4, 20, 16], color_channel="b"), dict(region="upper right")]),
         ("nested_three", "col3", [dict(rect=[2, 1, 25, 20]), dict(rect=[3, 2, 0.5, 0.5]),
                                   dict(rect=[1, 1, 6, 4], color_channel=1)])]
MONOS = [("mean3", "col3", "mean"), ("mean4", "col4", "mean"), ("red3", "col3", "red"), ("g3", "col3", "g"),
         ("b4", "col4", "B"), ("green4", "col4", "Green")]


def crop_sources():
    return {"mono": hashed((3, 24, 30), 73), "col3": hashed((3, 24, 30, 3), 71), "col4": hashed((3, 24, 30, 4), 72)}


def crop_cases(R, data, names):
    """FilterCrop (video/filters.py:161-249) incl. nested crops, FilterMonochrome (:348-374),
    FilterTimeDifference._compare_frames (:564-568)"""
    srcs = crop_sources()
    for k, v in srcs.items():
        data["crop_source/" + k] = v
    for name, src, chain in CROPS:
        key = "crop/" + name
        names.append(key)
        frames = srcs[src]
        filt = Source(frames)
        for kw in chain:
            filt = R["FilterCrop"](filt, **kw)
        data[key + "/source"] = np.array(src)
        data[key + "/chain"] = np.array(json.dumps(chain))
        data[key + "/rect"] = np.array(filt.rect, np.int64)
        data[key + "/out"] = np.stack([filt._process_frame(x) for x in frames])
    for name, src, mode in MONOS:
        key = "mono/" + name
        names.append(key)
        frames = srcs[src]
        filt = R["FilterMonochrome"](Source(frames), mode)
        data[key + "/source"] = np.array(src)
        data[key + "/mode"] = np.array(mode)
        data[key + "/out"] = np.stack([filt._process_frame(x) for x in frames])
    key = "timediff/u8"
    names.append(key)
    frames = hashed((5, 9, 17), 81)
    frames[2] = 255
    frames[3] = 0
    td = R["FilterTimeDifference"](Source(frames))
    data[key + "/frames"] = frames
    data[key + "/out"] = np.stack([td._compare_frames(frames[k + 1], frames[k]) for k in range(len(frames) - 1)])


def regionprops_moments():
    """(name, m00 m10 m01 m20 m11 m02) of pixel sets"""
    sets = [("line_slanted", [(0, 0), (1, 2), (2, 4)]),            # e2 rounds to -4.4e-16
            ("diag_b_pos", [(0, 0), (1, 1)]),                      # a - c == 0 with b > 0
            ("antidiag_b_neg", [(1, 0), (0, 1)]),                  # a - c == 0 with b < 0
            ("square_b_zero", [(x, y) for x in range(3) for y in range(3)]),     # a - c == 0 with b == 0
            ("single", [(4, 7)]),
            ("row", [(x, 2) for x in range(5)]),
            ("blob", [(x, y) for y in range(9) for x in range(11) if (x - 4.3) ** 2 + 2 * (y - 3.9) ** 2 < 17])]
    out = []
    for name, pts in sets:
        p = np.array(pts, np.float64)
        x, y = p[:, 0], p[:, 1]
        out.append((name, np.array([len(p), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()])))
    return out


REGIONPROPS_KEYS = ("m00", "m10", "m01", "m20", "m11", "m02", "mu20", "mu11", "mu02")
REGIONPROPS_OUT = ("area", "centroid_x", "centroid_y", "orientation", "e1", "e2", "major_axis_length",
                   "minor_axis_length")


def central(sp):
    """the moments regionprops reads, central ones in the operation order of OpenCV's completeMomentState"""
    m00, m10, m01, m20, m11, m02 = (float(v) for v in sp)
    inv = 1.0 / m00
    cx, cy = m10 * inv, m01 * inv
    return {"m00": m00, "m10": m10, "m01": m01, "m20": m20, "m11": m11, "m02": m02,
            "mu20": m20 - m10 * cx, "mu11": m11 - m10 * cy, "mu02": m02 - m01 * cy}


def regionprops_cases(R, data, names):
    """regionprops(moments=...) (video/analysis/image.py:349-405); eccentricity is left out (the
    reference calls a property as a method there)"""
    with np.errstate(invalid="ignore"):
        for name, sp in regionprops_moments():
            key = "regionprops/" + name
            names.append(key)
            m = central(sp)
            rp = R["regionprops"](moments=dict(m))
            e1, e2 = rp.inertia_tensor_eigvals
            vals = [rp.area, rp.centroid[0], rp.centroid[1], rp.orientation, e1, e2,
                    rp.major_axis_length, rp.minor_axis_length]
            data[key + "/spatial"] = np.asarray(sp, np.float64)
            data[key + "/moments"] = np.array([m[k] for k in REGIONPROPS_KEYS], np.float64)
            data[key + "/out"] = np.array(vals, np.float64)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_reference.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        return 2
    R = load_reference(root)
    data, names = {}, []
    temporal_cases(R, data, names)
    region_cases(R, data, names)
    peak_cases(R, data, names)
    normalize_cases(R, data, names)
    crop_cases(R, data, names)
    regionprops_cases(R, data, names)
    data["names"] = np.array(names)
    data["shims"] = np.array(SHIMS)
    data["regionprops_keys"] = np.array(REGIONPROPS_KEYS)
    data["regionprops_out"] = np.array(REGIONPROPS_OUT)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d cases, %d arrays" % (OUT, len(names), len(data)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
