#!/usr/bin/env python3
"""Generates tests/golden/geodesic_v1.npz -- known answers for make_distance_map,
shortest_path_in_distance_map and get_farthest_points (video/analysis/regions.py:455-611).

    python tests/golden/make_golden_geodesic.py [path of a reference checkout]

Sources of truth:
  * distance maps: an exact-pair Dijkstra (heapq) restated below.  A geodesic distance on the
    8-neighbour grid is a + b*sqrt2 (a straight, b diagonal steps); the pair of the shortest one is
    unique, and the reference's int(2 + d) is 2 + a + isqrt(2 b^2).  Cross-checked against
    scipy.sparse.csgraph.dijkstra on the same graph.
  * paths: the reference's walk restated step for step (int64 map, float64 weights).
  * farthest points: the reference's loop over the two restatements, from a given p1.
If a reference checkout is given (or found at $VA_REFERENCE), its own make_distance_map and
shortest_path_in_distance_map are lifted out of regions.py with `ast` at run time (np.int shimmed
to int64) and must agree on every case; none of its source is stored.
Importable: tests/test_geodesic_host.py checks the restatements against the committed fixture.
"""
import ast
import heapq
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "geodesic_v1.npz")
SQRT2 = np.sqrt(2)
INT64_MAX = np.iinfo(np.int64).max


# ---------------------------------------------------------------------------- restatements
def isqrt2b2(b):
    """floor(b * sqrt2) for a non-negative integer b"""
    import math
    return math.isqrt(2 * b * b)


def exact_pairs(fill, starts):
    """{(x, y): (a, b)} of the shortest geodesic from any valid start over the fillable pixels"""
    h, w = fill.shape
    best = {}
    heap = []
    for x, y in starts:
        x, y = int(x), int(y)
        if 0 <= x < w and 0 <= y < h and fill[y, x]:
            heapq.heappush(heap, (0.0, 0, 0, x, y))
    while heap:
        _, a, b, x, y = heapq.heappop(heap)
        if (x, y) in best:
            continue
        best[(x, y)] = (a, b)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                nx, ny = x + dx, y + dy
                if 0 <= nx < w and 0 <= ny < h and fill[ny, nx] and (nx, ny) not in best:
                    na, nb = (a, b + 1) if dx and dy else (a + 1, b)
                    heapq.heappush(heap, (na + nb * SQRT2, na, nb, nx, ny))
    return best


def distance_map(mask, starts, ends=None):
    """the contract of make_distance_map on a copy of the integer array `mask`"""
    out = np.array(mask, copy=True)
    fill = out == 1
    pairs = exact_pairs(fill, starts)
    key = lambda p: p[0] + p[1] * SQRT2          # noqa: E731 (distinct values differ by >> rounding here)
    limit = end_xy = None
    if ends is not None:
        for x, y in ends:
            p = pairs.get((int(x), int(y)))
            if p is not None and (limit is None or key(p) < key(limit)):
                limit, end_xy = p, (int(x), int(y))
    for (x, y), p in pairs.items():
        if limit is None or key(p) < key(limit) or (x, y) == end_xy:
            out[y, x] = 2 + p[0] + isqrt2b2(p[1])
    return out


DIST_LOCAL = np.full((3, 3), 1 / np.sqrt(2), np.double)
DIST_LOCAL[1, :] = DIST_LOCAL[:, 1] = 1


def shortest_path(distance_map_, end_point):
    """the reference's walk (regions.py:513-565), with int64 for the np.int NumPy 2 removed"""
    h, w = distance_map_.shape
    D = np.zeros((h + 2, w + 2), np.int64)
    D[1:-1, 1:-1] = distance_map_
    D[D <= 1] = INT64_MAX
    x, y = int(end_point[0]) + 1, int(end_point[1]) + 1
    points = [(x, y)]
    d = D[y, x]
    while True:
        S = D[y - 1:y + 2, x - 1:x + 2]
        if S.shape != (3, 3):
            break
        dy, dx = np.unravel_index(((S - d) * DIST_LOCAL).argmin(), (3, 3))
        x += dx - 1
        y += dy - 1
        if D[y, x] < d:
            d = D[y, x]
        elif D[y, x] == d:
            if (x, y) in points:
                break
        else:
            break
        points.append((x, y))
    return np.array(points, np.int64) - 1


def farthest_points(mask, p1, ret_path=False):
    """the reference's loop (regions.py:585-611) from a given p1"""
    mask_int = np.clip(np.asarray(mask).astype(np.int64), 0, 1)
    dist_prev = 0
    while True:
        dmap = distance_map(mask_int, [p1])
        idx = np.unravel_index(dmap.argmax(), dmap.shape)
        dist = dmap[idx]
        p2 = (int(idx[1]), int(idx[0]))
        if dist <= dist_prev:
            break
        dist_prev = dist
        p1 = p2
    if ret_path:
        return shortest_path(dmap, p2)
    return (int(p1[0]), int(p1[1])), p2


# ---------------------------------------------------------------------------- cross-checks
def check_csgraph(mask, starts):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    fill = np.asarray(mask) == 1
    h, w = fill.shape
    idx = -np.ones((h, w), np.int64)
    ys, xs = np.nonzero(fill)
    idx[ys, xs] = np.arange(len(ys))
    rows, cols, wts = [], [], []
    for dy, dx, c in ((0, 1, 1.0), (1, 0, 1.0), (1, 1, SQRT2), (1, -1, SQRT2)):
        ny, nx = ys + dy, xs + dx
        ok = (ny < h) & (nx >= 0) & (nx < w)
        ok[ok] &= fill[ny[ok], nx[ok]]
        rows.append(idx[ys[ok], xs[ok]])
        cols.append(idx[ny[ok], nx[ok]])
        wts.append(np.full(ok.sum(), c))
    g = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))),
                   shape=(len(ys),) * 2).tocsr()
    src = [idx[int(y), int(x)] for x, y in starts
           if 0 <= int(x) < w and 0 <= int(y) < h and fill[int(y), int(x)]]
    pairs = exact_pairs(fill, starts)
    if not src:
        assert not pairs
        return
    d = dijkstra(g, directed=False, indices=src, min_only=True)
    for (x, y), (a, b) in pairs.items():
        assert abs(d[idx[y, x]] - (a + b * SQRT2)) < 1e-9, (x, y)
    assert np.isinf(d).sum() == len(ys) - len(pairs)


def load_reference(root):
    """the reference's make_distance_map / shortest_path_in_distance_map, compiled from its source
    at run time (nothing is copied)"""
    from collections import defaultdict
    path = os.path.join(root, "video", "analysis", "regions.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body
            if (isinstance(n, ast.FunctionDef) and n.name in ("make_distance_map", "shortest_path_in_distance_map"))
            or (isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "DIST_LOCAL" for t in n.targets))
            or (isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Subscript))]
    np_shim = type(sys)("np_shim")
    np_shim.__dict__.update(np.__dict__)
    np_shim.int = np.int64
    ns = {"np": np_shim, "defaultdict": defaultdict}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["make_distance_map"], ns["shortest_path_in_distance_map"]


# ---------------------------------------------------------------------------- cases
def blobs(rng, h, w, frac=0.5, passes=3):
    a = rng.random((h, w))
    for _ in range(passes):
        p = np.pad(a, 1, mode="edge")
        a = sum(p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9
    return (a > np.quantile(a, 1 - frac)).astype(np.int64)


def spiral(n):
    m = np.zeros((n, n), np.int64)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    while x0 <= x1 and y0 <= y1:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 - y0 >= 2:
            m[y1, x0 + 2:x1 + 1] = 1
        if x1 - x0 >= 2:
            m[y0 + 2:y1 + 1, x0 + 2] = 1
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
    return m


def maze(rng, cells_h, cells_w):
    h, w = 2 * cells_h + 1, 2 * cells_w + 1
    m = np.zeros((h, w), np.int64)
    seen = np.zeros((cells_h, cells_w), bool)
    stack = [(0, 0)]
    seen[0, 0] = True
    m[1, 1] = 1
    while stack:
        cy, cx = stack[-1]
        nb = [(cy + dy, cx + dx) for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0))
              if 0 <= cy + dy < cells_h and 0 <= cx + dx < cells_w and not seen[cy + dy, cx + dx]]
        if not nb:
            stack.pop()
            continue
        ny, nx = nb[rng.integers(len(nb))]
        seen[ny, nx] = True
        m[2 * ny + 1, 2 * nx + 1] = 1
        m[cy + ny + 1, cx + nx + 1] = 1
        stack.append((ny, nx))
    return m


def first_fill(m):
    ys, xs = np.nonzero(np.asarray(m) == 1)
    return (int(xs[0]), int(ys[0]))


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    b = blobs(rng, 120, 160)
    out.append(("blobs", b, [first_fill(b)], None))
    b2 = blobs(rng, 97, 131, frac=0.6)
    ys, xs = np.nonzero(b2)
    out.append(("blobs_mid", b2, [(int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))], None))
    s = spiral(61)
    out.append(("spiral", s, [(30, 30)], None))
    mz = maze(rng, 20, 25)
    out.append(("maze", mz, [(1, 1)], None))
    diag = np.zeros((40, 40), np.int64)
    for i in range(40):
        diag[i, i] = 1
        diag[i, 39 - i] = 1
    diag[::7, :] = 0
    diag[5, 5:30:3] = 1
    out.append(("diagonal", diag, [(0, 0), (39, 0)], None))
    out.append(("single", np.ones((1, 1), np.int64), [(0, 0)], None))
    one = np.zeros((5, 5), np.int64)
    one[2, 3] = 1
    out.append(("single_in_frame", one, [(3, 2)], None))
    b3 = blobs(rng, 64, 80)
    ys0, xs0 = np.nonzero(b3 == 0)
    ys1, xs1 = np.nonzero(b3 == 1)
    out.append(("starts_mixed", b3, [(-1, 3), (int(xs0[5]), int(ys0[5])), (int(xs1[3]), int(ys1[3])),
                                     (1000, 1000), (int(xs1[-7]), int(ys1[-7])), (3, -2)], None))
    out.append(("starts_none_valid", b3, [(-1, 3), (int(xs0[5]), int(ys0[5]))], None))
    row = (rng.random((1, 37)) < 0.8).astype(np.int64)
    out.append(("height1", row, [first_fill(row)], None))
    col = (rng.random((29, 1)) < 0.8).astype(np.int64)
    out.append(("width1", col, [first_fill(col)], None))
    odd = blobs(rng, 33, 47, frac=0.7)
    out.append(("odd_width", odd, [first_fill(odd)], None))
    vals = rng.choice(np.array([0, 1, 1, 1, 5, -3, 2, 7]), size=(50, 61)).astype(np.int64)
    out.append(("int64_values", vals, [first_fill(vals), (0, 0)], None))
    # end points: a corridor where the equal-distance shell of the end is the end alone
    cor = np.zeros((9, 60), np.int64)
    cor[4, :] = 1
    out.append(("end_corridor", cor, [(0, 4)], [(41, 4), (55, 4)]))
    b4 = blobs(rng, 70, 90, frac=0.65)
    ys, xs = np.nonzero(b4)
    st = (int(xs[0]), int(ys[0]))
    keys = {}
    for q, p in exact_pairs(b4 == 1, [st]).items():
        keys.setdefault(p, []).append(q)
    uniq = sorted((p[0] + p[1] * SQRT2, q[0]) for p, q in keys.items() if len(q) == 1)
    out.append(("end_blob", b4, [st], [uniq[len(uniq) // 2][1], (-5, 2), uniq[-1][1]]))
    return out


def check_end_shell(mask, starts, ends):
    fill = np.asarray(mask) == 1
    pairs = exact_pairs(fill, starts)
    reach = [pairs[(int(x), int(y))] for x, y in ends if (int(x), int(y)) in pairs]
    if not reach:
        return
    lim = min(p[0] + p[1] * SQRT2 for p in reach)
    shell = [q for q, p in pairs.items() if abs(p[0] + p[1] * SQRT2 - lim) < 1e-9]
    assert len(shell) == 1, "the end point's equal-distance shell must be the end point alone"


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VA_REFERENCE")
    ref = load_reference(ref_root) if ref_root and os.path.isdir(ref_root) else None
    data = {}
    names = []
    for name, mask, starts, ends in cases():
        names.append(name)
        mask = np.asarray(mask, np.int64)
        check_csgraph(mask, starts)
        dmap = distance_map(mask, starts, ends)
        if ends is not None:
            check_end_shell(mask, starts, ends)
        data[name + "/mask"] = mask
        data[name + "/starts"] = np.array(starts, np.int64).reshape(-1, 2)
        data[name + "/ends"] = np.array(ends if ends else [], np.int64).reshape(-1, 2)
        data[name + "/map"] = dmap
        filled = np.argwhere(dmap >= 2)
        if len(filled):
            y, x = filled[np.argmax(dmap[dmap >= 2])]
            end = (int(x), int(y))
            path = shortest_path(dmap, end)
        else:
            end, path = (-1, -1), np.zeros((0, 2), np.int64)
        data[name + "/path_end"] = np.array(end, np.int64)
        data[name + "/path"] = path
        fg = np.asarray(mask) != 0
        p1 = first_fill(fg.astype(np.int64)) if fg.any() else (0, 0)
        (a, b) = farthest_points(fg.astype(np.uint8), p1)
        data[name + "/fp_p1_in"] = np.array(p1, np.int64)
        data[name + "/fp"] = np.array([a, b], np.int64)
        data[name + "/fp_path"] = farthest_points(fg.astype(np.uint8), p1, ret_path=True) if fg.any() else \
            np.zeros((0, 2), np.int64)
        if ref is not None:
            r = mask.copy()
            ref[0](r, starts, ends)
            assert np.array_equal(r, dmap), name
            if len(filled):
                assert np.array_equal(ref[1](dmap, end), path), name
    data["names"] = np.array(names)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d cases%s" % (OUT, len(names), " (reference checked)" if ref else ""))


if __name__ == "__main__":
    main()
