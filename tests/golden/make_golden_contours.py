#!/usr/bin/env python3
"""Generates tests/golden/contours_v1.npz -- every outer contour (cv2.findContours RETR_EXTERNAL /
CHAIN_APPROX_SIMPLE) of the seeded masks built here, as the CPU oracle's Suzuki-Abe scanner lists them, and
get_external_contour (video/analysis/regions.py:201-232) as the reference's own code computes it.

    python tests/golden/make_golden_contours.py <reference checkout>      (or set $VA_REFERENCE)

Importing this module needs no checkout and no oracle: the CPU and GPU tests take the mask builders, the case
tables and the topological restatement (`topological_starts`) from it.  Writing the fixture lifts the reference's
get_external_contour and curves.point_distance with `ast` at run time and runs them over shims; none of their
source is stored.

Shims:
  np.int -> np.int64                 NumPy 2 removed the alias
  itertools.izip -> zip              Python 2's lazy zip
  cv2.fillPoly                       the restated fill of make_golden_polygon.py (`fill_poly`), colour 255
  cv2.findContours                   oracle.find_contours_external_simple, its `offset` added to every point
  shapely LinearRing.bounds          (min x, min y, max x, max y) of the ring's integer points
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "contours_v1.npz")

WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 97)        # around the 32-bit words of the packed mask
HEIGHTS = (1, 2, 7)
DENSITIES = (0.2, 0.5, 0.8)
BATCH_SHAPE = (9, 37, 45)
BLOB_SHAPE = (3, 203, 331)


# -------------------------------------------------------------------------------------------- masks
def random_mask(seed, h, w, density):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def word_boundary_cases():
    """name -> mask for every width x height x density, seeded by the three"""
    out = {}
    for w in WIDTHS:
        for h in HEIGHTS:
            for d in DENSITIES:
                out["rand/%dx%d/%g" % (h, w, d)] = random_mask(1000 * w + 10 * h + int(10 * d), h, w, d)
    return out


def fixed_cases():
    """masks with known answers: name -> (mask, list of point counts of the contours)"""
    return {
        "zeros": (np.zeros((7, 33), np.uint8), []),
        "ones": (np.ones((7, 33), np.uint8), [4]),
        "1x1": (np.ones((1, 1), np.uint8), [1]),
        "1xw": (np.ones((1, 65), np.uint8), [2]),
    }


def nested_rings(kind, size=41, depth=3, seed=0, add=0.08, remove=0.03):
    """`depth` one-pixel rings ('square', 'diamond', 'round') inside each other around a centre blob, 8 % of the
    pixels set and 3 % cleared at random"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:size, :size]
    c = size // 2
    dx, dy = np.abs(xx - c), np.abs(yy - c)
    r = {"square": np.maximum(dx, dy), "diamond": dx + dy, "round": np.rint(np.hypot(dx, dy)).astype(int)}[kind]
    m = np.zeros((size, size), bool)
    for k in range(depth):
        m |= r == c - 1 - 5 * k
    m |= r <= 1
    m |= rng.random(m.shape) < add
    m &= rng.random(m.shape) >= remove
    return m.astype(np.uint8)


def externality_cases():
    """name -> mask: components inside holes, which RETR_EXTERNAL leaves out"""
    out = {}
    for k, kind in enumerate(("square", "diamond", "round")):
        out["rings/%s/clean" % kind] = nested_rings(kind, add=0.0, remove=0.0)
        out["rings/%s/noise" % kind] = nested_rings(kind, seed=7 + k)
    # a blob in a hole whose only opening to the outside is diagonal: the background is 4-connected, so the hole
    # stays closed and the blob is not external
    m = np.zeros((12, 40), np.uint8)
    m[2:10, 30:38] = 1
    m[3:9, 31:37] = 0
    m[5:7, 33:35] = 1
    m[2, 30] = 0                   # corner removed: (30, 2) touches the hole's (31, 3) only diagonally
    out["diagonal_opening"] = m
    m = np.zeros((9, 34), np.uint8)
    m[3:6, 0:3] = 1                # first pixel in column 0
    m[1, 31:34] = 1
    out["column0"] = m
    m = np.zeros((10, 33), np.uint8)
    m[0:10, 20:33] = 1             # a ring that touches the frame edge on three sides, a blob inside
    m[2:8, 22:31] = 0
    m[4:6, 25:28] = 1
    out["edge_ring"] = m
    yy, xx = np.mgrid[:9, :35]
    out["checkerboard"] = ((yy + xx) % 2 == 0).astype(np.uint8)   # one 8-connected component, many holes
    return out


def smooth_field(rng, h, w, passes=3, radius=6):
    """white noise, box-blurred `passes` times (cumulative sums)"""
    f = rng.random((h, w))
    for _ in range(passes):
        for axis in (0, 1):
            p = np.concatenate([np.repeat(np.take(f, [0], axis), radius, axis), f,
                                np.repeat(np.take(f, [-1], axis), radius, axis)], axis)
            c = np.cumsum(p, axis)
            zero = np.zeros_like(np.take(c, [0], axis))
            c = np.concatenate([zero, c], axis)
            n = f.shape[axis]
            f = (np.take(c, np.arange(2 * radius + 1, 2 * radius + 1 + n), axis) -
                 np.take(c, np.arange(n), axis)) / (2 * radius + 1)
    return f


def blob_stack(shape=BLOB_SHAPE, seed=5):
    """blob masks: a thresholded smooth field with a little salt, so that outlines run to thousands of steps"""
    rng = np.random.default_rng(seed)
    n, h, w = shape
    out = np.zeros(shape, np.uint8)
    for f in range(n):
        field = smooth_field(rng, h, w)
        m = field > np.quantile(field, 0.55)
        m |= rng.random((h, w)) < 0.002
        out[f] = m
    return out


def batch9():
    """9 frames of 37 x 45 with different numbers of contours: two empty frames (the middle one and the last) and
    one of isolated pixels on every other row and column (19 x 23 = 437 one-point contours)"""
    n, h, w = BATCH_SHAPE
    out = np.zeros(BATCH_SHAPE, np.uint8)
    out[0] = random_mask(90, h, w, 0.3)
    out[1, ::2, ::2] = 1
    out[2] = nested_rings("square", 37, seed=3)[:, :37].repeat(2, axis=1)[:, :w]
    out[3] = random_mask(93, h, w, 0.7)
    # 4: empty
    out[5] = blob_stack((1, h, w), seed=95)[0]
    out[6] = random_mask(96, h, w, 0.05)
    out[7] = 1
    # 8: empty
    return out


def all_cases():
    """name -> 2-d mask, every mask whose oracle contours the fixture holds"""
    out = dict(word_boundary_cases())
    out.update({"fixed/" + k: v[0] for k, v in fixed_cases().items()})
    out.update({"ext/" + k: v for k, v in externality_cases().items()})
    out.update({"batch9/%d" % f: m for f, m in enumerate(batch9())})
    out.update({"blobs/%d" % f: m for f, m in enumerate(blob_stack())})
    return out


def seeded_check_masks(count=300, seed=11):
    """small random and ring masks for the comparison of the topological rule with the oracle"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        if k % 3 == 2:
            yield nested_rings(("square", "diamond", "round")[k % 9 // 3], size=int(rng.integers(17, 36)),
                               seed=int(rng.integers(1 << 30)))
        elif k % 3 == 1:
            h, w = rng.integers(20, 48, 2)
            yield random_mask(int(rng.integers(1 << 30)), int(h), int(w), float(rng.uniform(0.55, 0.7)))
        else:
            h, w = rng.integers(1, 28, 2)
            yield random_mask(int(rng.integers(1 << 30)), int(h), int(w), float(rng.uniform(0.1, 0.9)))


# ------------------------------------------------------------------------------- topological rule
def topological_starts(mask):
    """the GPU path's definition in SciPy: the first raster pixel of every 8-connected component whose left
    neighbour lies in a 4-connected background component that touches the frame edge (or that is in column 0),
    by descending pixel index; (k, 2) int64 (x, y).  Also returns the number of 8-connected components."""
    from scipy import ndimage
    m = np.asarray(mask) != 0
    h, w = m.shape
    lab, num = ndimage.label(m, structure=np.ones((3, 3), int))
    bg, _ = ndimage.label(~m)
    edge = np.zeros(bg.max() + 1, bool)
    for border in (bg[0], bg[-1], bg[:, 0], bg[:, -1]):
        edge[border] = True
    edge[0] = False
    flat = lab.reshape(-1)
    idx = np.arange(flat.size)
    firsts = ndimage.minimum(idx, flat, np.arange(1, num + 1)).astype(np.int64) if num else np.zeros(0, np.int64)
    keep = [i for i in firsts if i % w == 0 or edge[bg.reshape(-1)[i - 1]]]
    keep = np.array(sorted(keep, reverse=True), np.int64)
    return np.stack([keep % w, keep // w], 1).reshape(-1, 2), num


# -------------------------------------------------------------------------------- fixture layout
def flatten(contours):
    """list of (N, 1, 2) arrays -> (points (k, 2) int32, sizes int32)"""
    sizes = np.array([len(c) for c in contours], np.int32)
    pts = np.concatenate([c.reshape(-1, 2) for c in contours]) if contours else np.zeros((0, 2), np.int32)
    return pts.astype(np.int32), sizes


def unflatten(pts, sizes):
    o = np.concatenate([[0], np.cumsum(sizes)])
    return [pts[o[k]:o[k + 1]].reshape(-1, 1, 2) for k in range(len(sizes))]


# ------------------------------------------------------------------------- get_external_contour
def figure_eight(n=40, a=30.0):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([40.3 + a * np.sin(t), 25.8 + a * np.sin(t) * np.cos(t)], 1)


RINGS = {
    "convex": np.array([[10.5, 2.25], [20.0, 2.0], [25.75, 10.0], [20.0, 18.5], [10.0, 18.0], [5.25, 10.0]]),
    "concave": np.array([[0.0, 0.0], [6.0, 0.0], [6.0, 20.0], [14.0, 20.0], [14.0, 0.0], [20.0, 0.0], [20.0, 26.0],
                         [0.0, 26.0]]) * 1.3 - 7.1,
    "bowtie": np.array([[0.0, 0.0], [20.0, 12.0], [20.0, 0.0], [0.0, 12.0]]) * 2.5,
    "figure_eight": figure_eight(),
}
RESOLUTIONS = {"convex": 0.5, "concave": 1.0, "bowtie": 0.7, "figure_eight": 0.4}    # the explicit ones


def ring_cases():
    """(key, ring, resolution or None)"""
    for name, ring in RINGS.items():
        yield "ring/%s/default" % name, ring, None
        yield "ring/%s/explicit" % name, ring, RESOLUTIONS[name]


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lift(path, names, ns):
    tree = ast.parse(open(path).read(), path)
    keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
    missing = set(names) - {node.name for node in keep}
    if missing:
        raise SystemExit("%s: not found in the checkout: %s" % (path, sorted(missing)))
    mod = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)


def load_reference(root, oracle):
    """the reference's get_external_contour, lifted and shimmed"""
    import itertools
    import math
    poly = _sibling("make_golden_polygon")
    a = os.path.join(root, "video", "analysis")
    np_shim = types.ModuleType("np_shim")
    np_shim.__dict__.update(np.__dict__)
    np_shim.int = np.int64
    it_shim = types.ModuleType("itertools_shim")
    it_shim.__dict__.update(itertools.__dict__)
    it_shim.izip = zip
    cns = {"math": math, "np": np_shim, "__name__": "ref_curves"}
    _lift(os.path.join(a, "curves.py"), ("point_distance",), cns)
    curves = types.ModuleType("curves")
    curves.__dict__.update(cns)

    cv2 = types.ModuleType("cv2_shim")
    cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE = 0, 2

    def fill(mask, contours, color, offset=(0, 0)):
        assert len(contours) == 1 and color == 255
        h, w = mask.shape
        mask[...] = poly.fill_poly(np.asarray(contours[0]), (-offset[0], -offset[1], w, h), mask.dtype) * 255
    cv2.fillPoly = fill

    def find(mask, mode, method, offset=(0, 0)):
        assert mode == cv2.RETR_EXTERNAL and method == cv2.CHAIN_APPROX_SIMPLE
        return None, [c + np.array(offset, np.int32) for c in oracle.find_contours_external_simple(mask)]
    cv2.findContours = find

    geometry = types.ModuleType("geometry_shim")

    class Ring(object):
        def __init__(self, pts):
            p = np.asarray(pts)
            self.bounds = (int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max()))
    geometry.LinearRing = Ring
    rns = {"np": np_shim, "itertools": it_shim, "cv2": cv2, "curves": curves, "geometry": geometry,
           "__name__": "ref_regions"}
    _lift(os.path.join(a, "regions.py"), ("get_external_contour",), rns)
    return rns["get_external_contour"]


# ----------------------------------------------------------------------------------------------- main
def generate(root):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import oracle as O
    O.build()
    data = {"shims": np.array(["np.int -> int64", "itertools.izip -> zip", "cv2.fillPoly -> restated fill",
                               "cv2.findContours -> oracle + offset", "LinearRing.bounds -> min/max"])}
    nested = 0
    for name, mask in all_cases().items():
        contours = O.find_contours_external_simple(mask)
        starts, ncomp = topological_starts(mask)
        assert np.array_equal(starts, np.array([c[0, 0] for c in contours], np.int64).reshape(-1, 2)), name
        nested += ncomp > len(contours)
        data["c/%s/points" % name], data["c/%s/sizes" % name] = flatten(contours)
    for name, (mask, sizes) in fixed_cases().items():
        assert list(data["c/fixed/%s/sizes" % name]) == sizes, name
    assert nested >= 6
    ref = load_reference(root, O)
    for key, ring, res in ring_cases():
        out = np.asarray(ref(ring.copy(), res), np.float64)
        assert out.ndim == 2 and out.shape[1] == 2 and len(out) > 2, key
        data[key + "/points"] = ring
        data[key + "/resolution"] = np.float64(np.nan if res is None else res)
        data[key] = out
    return data


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    if not root or not os.path.isdir(os.path.join(root, "video", "analysis")):
        sys.stderr.write("usage: make_golden_contours.py <reference checkout> (or $VA_REFERENCE); nothing written\n")
        raise SystemExit(2)
    data = generate(root)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
