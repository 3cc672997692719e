#!/usr/bin/env python3
"""Generates tests/golden/composer_v1.npz.

    python tests/golden/make_golden_composer.py <reference checkout>      (or set $VA_REFERENCE)

Two kinds of entries, told apart by their prefix:

  ref_*       results of the reference's OWN code.  `highlight_mask` is the one method of video/io/composer.py whose
              arithmetic is pure NumPy; it, CHANNEL_NAMES and get_color are lifted out of the checkout with `ast`
              at run time and executed in a namespace of shims; none of their source is stored.  Without a checkout
              the script exits non-zero and writes nothing.
  restated_*  results of tests/composer_checks.py (drawing, add, blend): cv2 is not installed, so these pin the
              restatement against itself over time, nothing more.

Shims, and why none of them can change a result:
  the @skip_if_no_output decorator is dropped     it only skips frames that are not written; every case is written
  VideoComposer -> a stub with is_color, zoom_factor = 1 and _frame     highlight_mask reads nothing else (the
              zoom branch, with its removed np.bool alias, is not reached at zoom 1)
  a monochrome frame is handed in as (h, w, 1)    the reference indexes `_frame[mask, 0]` for a monochrome video,
              which a 2-d frame does not have (an IndexError); the stored result is the (h, w) plane
  the mask is handed in as a boolean array         the reference indexes with it as it is
  `from __future__ import division`                Python 3's division already

Inputs come from the integer hash `((i * 2654435761) >> 13) & 255`, so two runs write identical arrays.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "composer_v1.npz")
sys.path.insert(0, os.path.dirname(HERE))

SHIMS = ("@skip_if_no_output dropped", "VideoComposer -> stub (is_color, zoom_factor = 1, _frame)",
         "monochrome frames as (h, w, 1)", "boolean masks", "true division")
STRENGTHS = (0, 1, 128, 254, 255)
MONO_CHANNELS = ("all", None)
COLOR_CHANNELS = ("all", None, 0, 1, 2, "r", "g", "b", "red", "green", "blue")
COLOR_NAMES = ("w", "k", "r", "g", "b", "c", "m", "y", "white", "black")
H, W = 12, 16


def hashed(shape, salt=0):
    i = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(salt)
    return (((i * np.uint64(2654435761)) >> np.uint64(13)) & np.uint64(255)).astype(np.uint8).reshape(shape)


def channel_key(ch):
    return "none" if ch is None else str(ch)


def lift(root):
    """(get_color, CHANNEL_NAMES, highlight_mask as a plain function of (self, mask, channel, strength))"""
    path = os.path.join(root, "video", "io", "composer.py")
    tree = ast.parse(open(path).read(), path)
    keep = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "get_color":
            keep.append(node)
        elif isinstance(node, ast.Assign):
            t = node.targets[0]
            if (isinstance(t, ast.Name) and t.id == "CHANNEL_NAMES") or (
                    isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "get_color"):
                keep.append(node)
        elif isinstance(node, ast.ClassDef) and node.name == "VideoComposer":
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == "highlight_mask":
                    sub.decorator_list = []
                    keep.append(sub)
    names = [getattr(n, "name", None) for n in keep]
    assert "get_color" in names and "highlight_mask" in names and len(keep) == 4, names
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    from matplotlib.colors import ColorConverter
    ns = {"np": np, "ColorConverter": ColorConverter}
    exec(compile(mod, path, "exec"), ns)
    return ns["get_color"], ns["CHANNEL_NAMES"], ns["highlight_mask"]


class Stub(object):
    zoom_factor = 1

    def __init__(self, frame):
        self.is_color = frame.ndim == 3
        self._frame = frame.copy() if self.is_color else frame.copy()[:, :, None]


def draw_commands(c):
    """the command list of the restated_draw_* entries for frames of c channels (tests/test_composer_host.py
    redraws the entries from it)"""
    cmds = [("polyline", [(-5, 3), (30, 50), (70, 10), (20, -4)], True, 200),
            ("polyline", [(2, 2), (61, 2), (61, 45), (2, 45)], True, 90),
            ("circle", (32, 24), 20, False, 255), ("circle", (60, 40), 6, True, 10),
            ("polyline", [(10, 40), (50, 41)], False, 77), ("circle", (0, 0), 3, True, 33)]
    if c == 1:
        return cmds
    return [cmd[:-1] + ((cmd[-1], 255 - cmd[-1], cmd[-1] // 2),) for cmd in cmds]


def restated_cases():
    import composer_checks as K
    out = {}
    mono, rgb = hashed((48, 64), 5), hashed((48, 64, 3), 6)
    image, image3 = hashed((48, 64), 7), hashed((48, 64, 3), 8)
    mask = (hashed((48, 64), 9) > 100)
    out["restated_in_mono"], out["restated_in_rgb"] = mono, rgb
    out["restated_in_image"], out["restated_in_image3"], out["restated_in_mask"] = image, image3, mask
    for w in (0.0, 1.0, 0.5, 0.3):
        out["restated_blend_mono_%g" % w] = K.blend(mono.copy(), image, w, None)
        out["restated_blend_rgb_%g" % w] = K.blend(rgb.copy(), image3, w, mask)
    out["restated_add_mono"] = K.add(mono.copy(), image, mask)
    out["restated_add_rgb"] = K.add(rgb.copy(), image, None)
    out["restated_draw_mono"] = K.draw_frame(mono.copy(), draw_commands(1))
    out["restated_draw_rgb"] = K.draw_frame(rgb.copy(), draw_commands(3))
    return out


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.exists(os.path.join(root, "video", "io", "composer.py")):
        sys.stderr.write("usage: make_golden_composer.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        return 1
    get_color, channel_names, highlight_mask = lift(root)
    out = {"shims": np.array(SHIMS)}
    mono, rgb = hashed((H, W), 1), hashed((H, W, 3), 2)
    mask = hashed((H, W), 3) > 90
    out["ref_in_mono"], out["ref_in_rgb"], out["ref_in_mask"] = mono, rgb, mask
    for frame, channels, tag in ((mono, MONO_CHANNELS, "mono"), (rgb, COLOR_CHANNELS, "rgb")):
        for ch in channels:
            for s in STRENGTHS:
                stub = Stub(frame)
                highlight_mask(stub, mask, ch, s)
                out["ref_highlight_%s_%s_%d" % (tag, channel_key(ch), s)] = stub._frame.reshape(frame.shape)
    out["ref_channel_keys"] = np.array([str(k) for k in channel_names])
    out["ref_channel_values"] = np.array([channel_names[k] for k in channel_names], np.int64)
    out["ref_color_names"] = np.array(COLOR_NAMES)
    out["ref_color_values"] = np.array([get_color(n) for n in COLOR_NAMES], np.int64)
    out["ref_color_float_in"] = np.array([0.5, 0.25, 1.0])
    out["ref_color_float_out"] = np.array(get_color((0.5, 0.25, 1.0)), np.int64)
    out.update(restated_cases())
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
