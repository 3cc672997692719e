#!/usr/bin/env python3
"""Generates tests/golden/thinning_v1.npz -- the `guo-hall` method of mask_thinning (video/analysis/image.py:214-263)
and Polygon.get_skeleton / get_skeleton_points (video/analysis/shapes.py:600-625) as the reference's own code
computes them over the NumPy restatement of the pinned Guo-Hall definition ("Guo-Hall thinning").

    python tests/golden/make_golden_thinning.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout: the tests take the restatement (`guo_hall`, and the pixel-by-pixel
`guo_hall_literal`), the case tables and the seeded generators (`blob`, `worm_mask`, `ring`, `comb`,
`resident_batch`) from it.  Writing the fixture lifts the reference's mask_thinning (image.py) and, through
make_golden_polygon.load_reference, its Rectangle and Polygon (shapes.py) with `ast` at run time and runs them in
a namespace of shims; none of their source is stored.

Shims, and why none of them can change a result:
  module `thinning`                         its guo_hall_thinning(img) is `guo_hall` below, written back into img
                                            and returned, as the module thins in place (the module is not
                                            installed; agreement of the restatement with it is expected from its
                                            C source as known, and unverified).  With the shim importable the
                                            reference's own dispatch makes 'auto' mean 'guo-hall'.
  cv2 (mask_thinning's `python` branch)     never reached by the calls made here; a module without attributes, so
                                            that reaching it would raise
  everything make_golden_polygon.py lists   np.int, zip, cv2.fillPoly (restated), shapely, cached_property ...:
                                            the masks and offsets of Polygon.get_mask, pinned by polygon_v1.npz
Every case is compared exactly; none is dropped.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "thinning_v1.npz")
RESIDENT_MAX_WORDS = 15360          # VA_THIN_RESIDENT_MAX_WORDS, include/videoanalysis_hip.h


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


POL = _sibling("make_golden_polygon")


# ------------------------------------------------------------------------------------- restatement
def _flags(fg, sub):
    """deletion flags of the pixels 1 <= y <= h - 2, 1 <= x <= w - 2 of a boolean image with h, w >= 3"""
    p2, p3, p4, p5 = fg[:-2, 1:-1], fg[:-2, 2:], fg[1:-1, 2:], fg[2:, 2:]
    p6, p7, p8, p9 = fg[2:, 1:-1], fg[2:, :-2], fg[1:-1, :-2], fg[:-2, :-2]
    i = lambda a: a.astype(np.int32)
    C = i(~p2 & (p3 | p4)) + i(~p4 & (p5 | p6)) + i(~p6 & (p7 | p8)) + i(~p8 & (p9 | p2))
    N1 = i(p9 | p2) + i(p3 | p4) + i(p5 | p6) + i(p7 | p8)
    N2 = i(p2 | p3) + i(p4 | p5) + i(p6 | p7) + i(p8 | p9)
    N = np.minimum(N1, N2)
    m = ((p2 | p3 | ~p5) & p4) if sub else ((p6 | p7 | ~p9) & p8)
    return fg[1:-1, 1:-1] & (C == 1) & (N >= 2) & (N <= 3) & ~m


def guo_hall(img):
    """(skeleton uint8, iterations) of the pinned definition: parallel sub-iterations 0 and 1 until one whole
    iteration deletes nothing (that one is counted); the first and last row and column are never tested; the
    skeleton keeps the input's own values.  The input is left alone."""
    img = np.asarray(img)
    if img.ndim != 2:
        raise ValueError("mask must be 2-d")
    fg = img != 0
    h, w = fg.shape
    iterations = 0
    while True:
        iterations += 1
        changed = False
        if h >= 3 and w >= 3:
            for sub in (0, 1):
                flag = _flags(fg, sub)
                if flag.any():
                    fg = fg.copy()
                    fg[1:-1, 1:-1] &= ~flag
                    changed = True
        if not changed:
            break
    return np.where(fg, img, 0).astype(np.uint8), iterations


def guo_hall_literal(img):
    """the same, pixel by pixel in the definition's own words (slow; cross-checks the vector form)"""
    img = np.asarray(img)
    cur = [[1 if v else 0 for v in row] for row in (img != 0)]
    h, w = img.shape
    iterations = 0
    while True:
        iterations += 1
        changed = False
        for sub in (0, 1):
            marked = []
            for y in range(1, h - 1):
                for x in range(1, w - 1):
                    if not cur[y][x]:
                        continue
                    p2, p3, p4, p5 = cur[y - 1][x], cur[y - 1][x + 1], cur[y][x + 1], cur[y + 1][x + 1]
                    p6, p7, p8, p9 = cur[y + 1][x], cur[y + 1][x - 1], cur[y][x - 1], cur[y - 1][x - 1]
                    C = ((1 - p2) & (p3 | p4)) + ((1 - p4) & (p5 | p6)) + ((1 - p6) & (p7 | p8)) + \
                        ((1 - p8) & (p9 | p2))
                    N1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8)
                    N2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
                    N = min(N1, N2)
                    m = ((p2 | p3 | (1 - p5)) & p4) if sub else ((p6 | p7 | (1 - p9)) & p8)
                    if C == 1 and 2 <= N <= 3 and m == 0:
                        marked.append((y, x))
            for y, x in marked:
                cur[y][x] = 0
            changed = changed or bool(marked)
        if not changed:
            break
    return np.where(np.array(cur, bool).reshape(h, w), img, 0).astype(np.uint8), iterations


# --------------------------------------------------------------------------------------- generators
def blob(seed, h, w, sigma=4.0, level=0.0):
    """Gaussian-filtered seeded noise above `level` standard deviations (0 / 1 uint8)"""
    from scipy import ndimage
    g = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((h, w)), sigma, mode="reflect")
    return (g > level * g.std()).astype(np.uint8)


def worm_mask(seed, margin=5):
    """the mask of a seeded bent band (make_golden_polygon.worm, filled by its restated fillPoly)"""
    rng = np.random.default_rng(seed)
    c = POL.worm(length=float(rng.uniform(40, 110)), width=float(rng.uniform(4, 12)), bend=float(rng.uniform(0, 18)),
                 n=int(rng.integers(20, 48)), x0=float(rng.uniform(0, 20)), y0=float(rng.uniform(20, 30)),
                 phase=float(rng.uniform(0, 6.28)))
    return POL.get_mask(c, margin)[0]


def ring(h, w, holes=1, seed=0):
    """an ellipse with `holes` round holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    m = ((yy - h / 2.0) / (h / 2.0 - 1.5)) ** 2 + ((xx - w / 2.0) / (w / 2.0 - 1.5)) ** 2 <= 1
    for k in range(holes):
        cy = h / 2.0 + (rng.uniform(-0.2, 0.2) * h if holes > 1 else 0)
        cx = w * (k + 1.0) / (holes + 1.0)
        r = min(h, w / (holes + 1.0)) * 0.22
        m &= (yy - cy) ** 2 + (xx - cx) ** 2 > r * r
    return m.astype(np.uint8)


def comb(h, w, teeth=4, thick=3):
    """a spine along the bottom with `teeth` upright teeth"""
    m = np.zeros((h, w), np.uint8)
    m[h - 2 - thick:h - 2, 2:w - 2] = 1
    for k in range(teeth):
        x = 2 + int((w - 4 - thick) * k / max(teeth - 1, 1))
        m[2:h - 2, x:x + thick] = 1
    return m


def _field(h, w, rows, cols):
    m = np.zeros((h, w), np.uint8)
    m[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = 1
    return m


def _plus():
    m = np.zeros((7, 7), np.uint8)
    m[3, 1:6] = 1
    m[1:6, 3] = 1
    return m


# hand cases: (mask, expected skeleton, iterations), results of the restatement run on the CPU
HAND_CASES = {
    "block2": (_field(4, 4, (1, 2), (1, 2)), _field(4, 4, (1, 1), (2, 2)), 2),
    "bar3x7": (_field(5, 9, (1, 3), (1, 7)), _field(5, 9, (2, 2), (2, 6)), 2),
    "ones5x9": (np.ones((5, 9), np.uint8), np.ones((5, 9), np.uint8), 1),
    "plus7": (_plus(), _plus(), 1),
}


def fixture_masks():
    """name -> mask of every mask case of the fixture"""
    cases = {name: c[0] for name, c in HAND_CASES.items()}
    for k, (h, w, sigma, level) in enumerate([(24, 31, 2.0, 0.0), (40, 40, 3.0, 0.3), (33, 65, 2.5, -0.3),
                                              (64, 96, 4.0, 0.0), (96, 128, 4.0, -0.5), (17, 130, 2.0, 0.0),
                                              (70, 33, 3.0, 0.2), (50, 64, 6.0, -0.8)]):
        cases["blob%d" % k] = blob(100 + k, h, w, sigma, level)
    for k in range(4):
        cases["worm%d" % k] = worm_mask(200 + k)
    cases["ring1"] = ring(31, 45, 1)
    cases["ring3"] = ring(40, 90, 3, seed=3)
    cases["comb4"] = comb(30, 41, 4, 3)
    cases["comb7"] = comb(26, 70, 7, 4)
    cases["blob255"] = blob(120, 30, 50, 2.5) * np.uint8(255)
    rng = np.random.default_rng(121)
    cases["blob_mixed"] = blob(121, 36, 44, 2.5) * rng.integers(1, 256, (36, 44)).astype(np.uint8)
    cases["touching"] = np.pad(blob(122, 30, 38, 3.0, -0.4)[1:-1, 1:-1], 1, constant_values=1)
    cases["empty"] = np.zeros((9, 12), np.uint8)
    for h, w in ((1, 9), (2, 9), (9, 1), (9, 2), (1, 1), (2, 2)):
        cases["thin%dx%d" % (h, w)] = np.ones((h, w), np.uint8)
    return cases


POLYGONS = ("worm", "worm_steep", "mouse", "hexagon", "star", "u_shape", "l_shape", "fractional", "negative", "tiny")


def resident_batch():
    """the ragged batch of the GPU test: (name, mask) pairs, every one within the resident limit"""
    rng = np.random.default_rng(7)
    out = []
    for w in range(1, 71):                                   # every w % 32 and the word boundaries
        h = 1 + (w - 1) % 5
        out.append(("w%d_h%d" % (w, h), (rng.random((h, w)) < 0.8).astype(np.uint8)))
        out.append(("w%d_tall" % w, blob(1000 + w, 12 + w % 9, w, 1.5, -0.5) if w >= 3 else
                    np.ones((12, w), np.uint8)))
    for k in range(60):
        out.append(("worm%d" % k, worm_mask(300 + k, margin=int(rng.integers(0, 6)))))
    for k in range(60):
        h, w = int(rng.integers(8, 160)), int(rng.integers(8, 200))
        out.append(("blob%d" % k, blob(400 + k, h, w, float(rng.uniform(1.5, 5.0)), float(rng.uniform(-0.8, 0.5)))))
    for k in range(8):
        m = blob(500 + k, 40 + 3 * k, 61 + 5 * k, 3.0, -0.3)
        out.append(("v255_%d" % k, m * np.uint8(255)))
        out.append(("mixed_%d" % k, m * rng.integers(1, 256, m.shape).astype(np.uint8)))
        out.append(("bool_%d" % k, m.astype(bool)))
        out.append(("touch_%d" % k, np.pad(m[1:-1, 1:-1], 1, constant_values=1)))
    out.append(("empty", np.zeros((20, 45), np.uint8)))
    out.append(("empty_1x1", np.zeros((1, 1), np.uint8)))
    out.append(("full", np.ones((33, 64), np.uint8)))
    out.append(("full_65", np.ones((40, 65), np.uint8)))
    out.append(("ring", ring(120, 200, 3, seed=1)))
    out.append(("comb", comb(90, 257, 9, 6)))
    out.append(("big_blob", blob(600, 300, 700, 5.0, -0.2)))             # 300 * 22 words
    out.append(("at_limit", blob(601, 480, 1024, 6.0, -0.4)))            # 480 * 32 = RESIDENT_MAX_WORDS
    out.append(("at_limit_tall", blob(602, 15360, 32, 3.0, -0.6)))       # one word per row
    return out


# -------------------------------------------------------------------------------------------- lifting
def thinning_shim():
    mod = types.ModuleType("thinning")

    def guo_hall_thinning(img):
        img[...] = guo_hall(img)[0]
        return img
    mod.guo_hall_thinning = guo_hall_thinning
    return mod


def load_reference(root):
    """(mask_thinning, Polygon) of the reference, lifted; Polygon's `image` module gets the lifted mask_thinning"""
    RP = POL.load_reference(root)[0]
    ns = {"np": np, "cv2": types.ModuleType("cv2_unused"), "__name__": "ref_image"}
    POL._lift(os.path.join(root, "video", "analysis", "image.py"), ("mask_thinning",), ns)
    RP.get_skeleton.__globals__["image"].mask_thinning = ns["mask_thinning"]
    return ns["mask_thinning"], RP


def generate(root):
    mask_thinning, RP = load_reference(root)
    data = {"shims": np.array(["thinning.guo_hall_thinning -> the restatement, in place",
                               "cv2 of the python branch -> never reached",
                               "Polygon: the shims of make_golden_polygon.py"])}
    with POL._modules(thinning=thinning_shim()):
        for name, mask in fixture_masks().items():
            skel, it = guo_hall(mask)
            if mask.size <= 4096:
                lit, lit_it = guo_hall_literal(mask)
                assert np.array_equal(lit, skel) and lit_it == it, name
            for method in ("auto", "guo-hall"):              # with `thinning` importable, auto is guo-hall
                arg = mask.copy()
                ref = mask_thinning(arg, method)
                assert ref is arg and ref.dtype == np.uint8 and np.array_equal(ref, skel), (name, method)
            data["mask/%s" % name] = mask
            data["skel/%s" % name] = ref
            data["iters/%s" % name] = np.int32(it)
        for name, (mask, want, it) in HAND_CASES.items():
            assert np.array_equal(data["skel/%s" % name], want) and int(data["iters/%s" % name]) == it, name
        for name in POLYGONS:
            c = POL.FILL_POLYS[name]
            poly = RP(c)
            skel = poly.get_skeleton()
            assert np.array_equal(skel, guo_hall(POL.get_mask(c, 0)[0])[0]), name
            skel_off, off = poly.get_skeleton(ret_offset=True)
            mask5, off5 = POL.get_mask(c, 5)
            assert np.array_equal(skel_off, guo_hall(mask5)[0]) and tuple(off) == off5, name
            data["poly/%s" % name] = c
            data["skeleton/%s" % name] = skel
            data["skeleton5/%s" % name] = skel_off
            data["skeleton5/%s/offset" % name] = np.array(off, np.int64)
            data["points/%s" % name] = np.asarray(poly.get_skeleton_points(), np.int64)
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_thinning.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
