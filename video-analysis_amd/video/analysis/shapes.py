"""Shapes: the reference's Rectangle and Polygon (video/analysis/shapes.py:49-227, 418-823) as the analysis path
uses them.

The reference's shapes module is geometry on top of shapely (out of the hot-path scope).
What runs here: `Polygon.moments` / `eccentricity` (cv2.moments of the contour), the mask (cv2.fillPoly,
va_fill_poly), the skeleton (mask_thinning) and the centre lines.  The estimate runs on the geodesic kernels; the
optimized centre line chains fill -> cv2.distanceTransform (va_distance_transform_l2_5) -> ActiveContour.  The
equidistant resampling, the translations and the smoothing spline stay on the host, as in the reference.

Batched forms: `get_masks` fills many polygons in one launch, `get_centerline_estimates` runs the estimates of
many polygons on padded stacks, one geodesic call per stack, and `get_centerlines_optimized` (with
`get_centerlines_smoothed` and `get_centerlines` on top) keeps the masks, distance maps and gradient planes of
many polygons on the device as ragged buffers and runs all their snakes in one launch.

Deviations ("Polygons"):
  * `bounds` is a fresh Rectangle on every read.  The reference caches it and get_bounding_rect buffers it in
    place, so margins accumulate across calls (get_mask(1) then get_mask(2) gives a margin of 3).
  * the constructor keeps the contour's orientation (the reference reverses counter-clockwise contours); every
    method here gives the same result for either orientation, and `moments` keeps its bits.
  * the end-point deviation of make_distance_map carries over to the estimate with two or more end points, and
    that of shortest_path_in_distance_map to every estimate: an end point that is not a reached pixel of the
    mask raises ValueError, where the reference walks through its sentinels.
  * `position` restates GEOS's InteriorPointArea (shapely's representative_point) without shapely; unverified
    against GEOS itself.
"""
import math

import numpy as np

from . import curves as _curves
from .image import contour_moments

GEODESIC_MAX_WIDTH = 8192        # the widest frame the geodesic kernels take


class Rectangle(object):
    """ class that represents a rectangle (reference :49-227, the members the polygons use) """

    def __init__(self, x, y, width, height):
        self.x = x
        self.y = y
        self.width = width
        self.height = height

    @classmethod
    def from_points(cls, p1, p2):
        x1, x2 = min(p1[0], p2[0]), max(p1[0], p2[0])
        y1, y2 = min(p1[1], p2[1]), max(p1[1], p2[1])
        return cls(x1, y1, x2 - x1, y2 - y1)

    def copy(self):
        return self.__class__(self.x, self.y, self.width, self.height)

    def __repr__(self):
        return ("%s(x=%g, y=%g, width=%g, height=%g)"
                % (self.__class__.__name__, self.x, self.y, self.width, self.height))

    @property
    def data(self):
        return self.x, self.y, self.width, self.height

    @property
    def data_int(self):
        return (int(self.x), int(self.y), int(self.width), int(self.height))

    def buffer(self, amount):
        """ dilate the rectangle by a certain amount in all directions """
        self.x -= amount
        self.y -= amount
        self.width += 2 * amount
        self.height += 2 * amount


def interior_point(contour):
    """a point inside a simple polygon -- shapely's representative_point(), GEOS's InteriorPointArea restated:
    the scan line y is the mean of the nearest vertex ordinates at or below and above the centre of the
    envelope; its crossings with the edges (a vertex on the scan line counts only as the lower end of an edge,
    horizontal edges not at all) are sorted and paired, and the middle of the widest pair is the point.  Without
    a pair of positive width: the first vertex."""
    p = [(float(a), float(b)) for a, b in np.asarray(contour, np.float64)]
    ys = [q[1] for q in p]
    lo, hi = min(ys), max(ys)
    centre = (lo + hi) / 2.0
    for y in ys:
        if y <= centre:
            if y > lo:
                lo = y
        elif y < hi:
            hi = y
    scan = (hi + lo) / 2.0
    ring = p + [p[0]]
    crossings = []
    for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]):
        if (y0 > scan and y1 > scan) or (y0 < scan and y1 < scan):
            continue
        if y0 == y1 or (y0 == scan and y1 < scan) or (y1 == scan and y0 < scan):
            continue
        crossings.append(x0 if x0 == x1 else x0 + (scan - y0) / ((y1 - y0) / (x1 - x0)))
    crossings.sort()
    best, width = p[0], 0.0
    for k in range(0, len(crossings) - 1, 2):
        if crossings[k + 1] - crossings[k] > width:
            width = crossings[k + 1] - crossings[k]
            best = ((crossings[k] + crossings[k + 1]) / 2.0, scan)
    return np.array(best)


class Polygon(object):
    """a closed polygon given by its contour, an (N, 2) sequence of (x, y) points"""

    def __init__(self, contour):
        contour = np.asarray(contour, np.double)
        if contour.ndim != 2 or contour.shape[1] != 2 or len(contour) < 3:
            raise ValueError("a polygon needs an (N, 2) contour with at least three points")
        self.contour = contour
        self._moments = None
        self._position = None

    def __repr__(self):
        return '%s(%r)' % (self.__class__.__name__, self.contour)

    @property
    def moments(self):
        """all moments up to third order: cv2.moments(np.asarray(contour, np.float32))
        (reference :527-533; the float32 cast is the reference's own)"""
        if self._moments is None:
            self._moments = contour_moments(np.asarray(self.contour, np.float32))
        return self._moments

    @property
    def area(self):
        return self.moments["m00"]

    @property
    def centroid(self):
        m = self.moments
        return (m["m10"] / m["m00"], m["m01"] / m["m00"])

    @property
    def eccentricity(self):
        """0 for a circle ... 1 for a line (reference :537-549)"""
        m = self.moments
        a, b, c = m["mu20"], -m["mu11"], m["mu02"]
        root = math.sqrt(4 * b ** 2 + (a - c) ** 2)
        e1, e2 = (a + c) + root, (a + c) - root
        if e1 == 0:
            return 0
        return math.sqrt(1 - e2 / e1)

    @property
    def position(self):
        """a representative point inside the polygon (reference :510-512, shapely's representative_point();
        see interior_point)"""
        if self._position is None:
            self._position = interior_point(self.contour)
        return self._position

    @property
    def bounds(self):
        """the bounding rectangle (reference :557-560).  Deviation: a fresh Rectangle on every read, so that
        get_bounding_rect's buffer does not accumulate across calls"""
        c = self.contour
        return Rectangle.from_points((c[:, 0].min(), c[:, 1].min()), (c[:, 0].max(), c[:, 1].max()))

    def contains(self, point):
        """whether the point (x, y) lies strictly inside the polygon (reference :552-554, shapely's contains; the
        definition is pinned in DESIGN.md §9, "Outline queries": the boundary is outside)"""
        return bool(contains_points([self], [point])[0])

    def contains_points(self, points):
        """contains for (q, 2) points in one launch: a (q,) bool array"""
        return contains_points([self], points)

    def get_bounding_rect(self, margin=0):
        """ returns the bounding rectangle of the polygon, (x, y, width, height) truncated to integers """
        bound_rect = self.bounds
        if margin:
            bound_rect.buffer(margin)
        return np.asarray(bound_rect.data).astype(np.int64)

    def get_mask(self, margin=0, dtype=np.uint8, ret_offset=False):
        """ builds a mask of the polygon (cv2.fillPoly on the GPU, reference :577-597).

        `margin` adds an extra margin to the boundary
        `dtype` determines the dtype of the output
        `ret_offset` determines whether the coordinates of the upper left point
            of the mask are returned
        """
        masks, offsets = get_masks([self], margin, dtype, ret_offset=True)
        return (masks[0], offsets[0]) if ret_offset else masks[0]

    def get_skeleton(self, ret_offset=False, method="auto"):
        """ gets the binary skeleton image of the polygon (mask_thinning on the GPU, reference :600-616)

        `ret_offset` determines whether the coordinates of the upper left point
            of the skeleton mask are returned
        `method` is mask_thinning's: 'auto' / 'python' (cross erosions) or 'guo-hall'
        """
        from .image import mask_thinning
        if ret_offset:
            mask, offset = self.get_mask(margin=5, ret_offset=True)
        else:
            mask = self.get_mask(ret_offset=False)
        skeleton = mask_thinning(mask, method)
        if ret_offset:
            return skeleton, offset
        return skeleton

    def get_skeleton_points(self, method="auto"):
        """ returns points along the skeleton of the shape """
        skeleton, offset = self.get_skeleton(ret_offset=True, method=method)
        y, x = np.nonzero(skeleton)
        return np.c_[x, y] + offset

    def get_morphological_graph(self, simplify_epsilon=0.1, method="guo-hall"):
        """the polygon's skeleton as a MorphologicalGraph in the polygon's own coordinates (reference :628-646):
        the mask with a margin of 5 is thinned (`method` is mask_thinning's), MorphologicalGraph.from_skeleton
        builds and post-processes the graph by the definition pinned in DESIGN.md §9, "Skeleton graphs", a
        positive `simplify_epsilon` thins its curves, and the mask's offset is added"""
        from .morphological_graph import MorphologicalGraph
        skeleton, offset = self.get_skeleton(ret_offset=True, method=method)
        graph = MorphologicalGraph.from_skeleton(skeleton, copy=False)
        return _finish_morphological_graph(graph, simplify_epsilon, offset)

    def get_centerline_estimate(self, end_points=None):
        """ determines an estimate to a center line of the polygon (reference :649-724)
        `end_points` can either be None, a single point, two points or n points (the two of them whose path
        is the longest are taken).  Returns the (K, 2) int64 path of (x, y) points. """
        return get_centerline_estimates([self], None if end_points is None else [end_points])[0]

    def get_centerline_optimized(self, alpha=1e3, beta=1e6, gamma=0.01, spacing=20, max_iterations=1000,
                                 endpoints=None):
        """ determines the center line of the polygon using an active contour algorithm (reference :727-757):
        the snake climbs the distance transform of the mask, from the estimate, with both ends anchored """
        from .. import ops
        from .active_contour import ActiveContour
        ac = ActiveContour(blur_radius=1, alpha=alpha, beta=beta, gamma=gamma, closed_loop=False)
        ac.max_iterations = max_iterations

        # set the potential from the distance map
        mask, offset = self.get_mask(1, ret_offset=True)
        potential = ops.distance_transform([mask])[0]
        ac.set_potential(potential)

        # initialize the centerline from the estimate
        points = self.get_centerline_estimate(endpoints)
        points = _curves.make_curve_equidistant(points, spacing=spacing)
        points = _curves.translate_points(points, -offset[0], -offset[1])
        # anchor the end points
        anchor = np.zeros(len(points), bool)
        anchor[0] = anchor[-1] = True

        # find the best contour
        points = ac.find_contour(points, anchor, anchor)

        points = _curves.make_curve_equidistant(points, spacing=spacing)
        return _curves.translate_points(points, *offset)

    def get_centerline_smoothed(self, points=None, spacing=10, skip_length=90, **kwargs):
        """ determines the center line of the polygon using an active contour algorithm, smoothed by a spline
        (reference :760-810, host code).  If `points` are given, they are used for getting the smoothed
        centerline; otherwise the optimized centerline with the additional keyword arguments.
        `skip_length` is the length that is skipped at either end of the center
            line when the smoothed variant is calculated
        """
        if points is None:
            points = self.get_centerline_optimized(spacing=spacing, **kwargs)
        return smooth_centerline(points, spacing, skip_length)

    def get_centerline(self, method='smoothed', **kwargs):
        """ get the centerline of the polygon """
        if method == 'smoothed':
            return self.get_centerline_smoothed(**kwargs)
        elif method == 'optimized':
            return self.get_centerline_optimized(**kwargs)
        elif method == 'estimate':
            return self.get_centerline_estimate(**kwargs)
        else:
            raise ValueError('Unknown method `%s`' % method)


def smooth_centerline(points, spacing=10, skip_length=90):
    """ the spline part of get_centerline_smoothed (reference :775-810, host code): resamples the centre line
    `points`, skips `skip_length` at either end, fits a smoothing spline and restricts it to the section between
    the centre line's end points """
    from scipy import interpolate, spatial

    # get properties of the line
    length = _curves.curve_length(points)
    endpoints = points[0], points[-1]

    # get the points to interpolate
    points = _curves.make_curve_equidistant(points, spacing=spacing)
    skip_points = int(skip_length / spacing)
    points = points[skip_points:-skip_points]

    # do spline fitting to smooth the line
    try:
        tck, _ = interpolate.splprep(np.transpose(points), k=3, s=length)
    except (ValueError, TypeError):
        # do not interpolate if there are problems
        pass
    else:
        # extend the center line in both directions to make sure that it crosses the outline
        overshoot = 20 * skip_length  #< absolute overshoot
        num_points = (length + 2 * overshoot) / spacing
        overshoot /= length  #< overshoot relative to total length
        s = np.linspace(-overshoot, 1 + overshoot, int(num_points))
        points = list(zip(*interpolate.splev(s, tck)))

        # restrict center line to the section between the end points (the reference's LineString only
        # wraps the point list)
        dists = spatial.distance.cdist(endpoints, points)
        ks = sorted(np.argmin(dists, axis=1))
        points = np.array(points[ks[0]:ks[1] + 1])

    return points


# ---------------------------------------------------------------------------------------- batched
def contains_points(polygons, points, index=None):
    """Polygon.contains for many points and polygons in one launch.  polygons: Polygons, or (N, 2) rings (closed
    with the edge from the last point to the first); points: (q, 2); index: the polygon of each point (None: the
    one polygon for all points, else point k in polygon k, which needs as many points as polygons).  Returns a
    (q,) bool array."""
    from .. import ops
    rings = [p.contour if isinstance(p, Polygon) else p for p in polygons]
    return ops.points_in_outlines(rings, points, index)


def get_masks(polygons, margin=0, dtype=np.uint8, ret_offset=False):
    """Polygon.get_mask(margin, dtype) of every polygon of a list, in one fill launch.  uint8 and int32 masks
    are written by the kernel; other dtypes are converted from uint8.  Returns the list of masks, and with
    ret_offset also the list of (x, y) offsets of their upper left corners."""
    from .. import ops
    dtype = np.dtype(dtype)
    rects = [p.get_bounding_rect(margin=margin) for p in polygons]
    contours = [np.asarray(p.contour).astype(np.int64) for p in polygons]
    fill_dtype = dtype if dtype in (np.uint8, np.int32) else np.uint8
    masks = ops.fill_polys(contours, rects, fill_dtype) if polygons else []
    if fill_dtype != dtype:
        masks = [m.astype(dtype) for m in masks]
    offsets = [(int(r[0]), int(r[1])) for r in rects]
    return (masks, offsets) if ret_offset else masks


def get_skeletons(polygons, method="guo-hall", ret_offset=False):
    """Polygon.get_skeleton(ret_offset, method) of every polygon of a list: one fill launch for the masks (margin 5
    with offsets, 0 without, as the reference's get_skeleton, :606-609) and, for 'guo-hall', one thinning call for
    all of them.  Returns the list of skeletons, and with ret_offset also the list of (x, y) offsets."""
    from .. import ops
    from .image import mask_thinning
    if method not in ("auto", "python", "guo-hall"):
        raise ValueError("Unknown thinning method `%s`" % method)
    masks, offsets = get_masks(polygons, 5 if ret_offset else 0, ret_offset=True)
    if method == "guo-hall":
        skeletons = ops.guo_hall_thinning(masks)
    else:
        skeletons = [mask_thinning(m, method) for m in masks]
    return (skeletons, offsets) if ret_offset else skeletons


def _bucket(shape):
    """stack key of a box: its sides rounded up to powers of two, so that padding at most doubles a side"""
    return tuple(1 << max(int(s) - 1, 0).bit_length() for s in shape)


def _stacks(frames):
    """[(indices, (N, H, W) int32 stack zero-padded at the right and bottom)] of 2-d frames grouped by _bucket"""
    groups = {}
    for k, f in enumerate(frames):
        groups.setdefault(_bucket(f.shape), []).append(k)
    out = []
    for idx in groups.values():
        H = max(frames[k].shape[0] for k in idx)
        W = max(frames[k].shape[1] for k in idx)
        stack = np.zeros((len(idx), H, W), np.int32)
        for r, k in enumerate(idx):
            h, w = frames[k].shape
            stack[r, :h, :w] = frames[k]
        out.append((idx, stack))
    return out


def _integral(p):
    return all(float(v) == int(v) for v in p)


def get_centerline_estimates(polygons, end_points=None):
    """Polygon.get_centerline_estimate for every polygon of a list: one fill launch for the int32 masks (margin
    2), which are packed into (N, H_max, W_max) stacks padded with zeros at the right and bottom, and one
    geodesic call per stack and kind of estimate.  Padding with walls is exact: no geodesic passes a wall, the
    first raster-order maximum of a padded map lies in its box, and the path walk stops at values <= 1.
    Polygons are grouped by box size (sides rounded up to powers of two) so that one large box does not inflate
    every stack.  end_points: None, or one entry per polygon (None, (2,), (2, 2) or (n, 2) points).
    Returns the list of (K, 2) int64 paths (None where n end points give no path longer than 0)."""
    from .. import ops
    m = len(polygons)
    eps = [None] * m if end_points is None else list(end_points)
    if len(eps) != m:
        raise ValueError("need one end-point entry per polygon (%d polygons, %d entries)" % (m, len(eps)))
    masks, offsets = get_masks(polygons, 2, np.int32, ret_offset=True)
    for mk in masks:
        if mk.shape[1] > GEODESIC_MAX_WIDTH:
            raise ValueError("a polygon's box of %d columns exceeds the geodesic kernels' %d"
                             % (mk.shape[1], GEODESIC_MAX_WIDTH))

    # jobs: (polygon, kind, p1, p2) in the box's coordinates; kind 'far' (no end points), 'one' (one), 'pair'
    jobs, pairs_of = [], {}
    for k, (poly, ep) in enumerate(zip(polygons, eps)):
        ox, oy = offsets[k]
        rel = lambda p: (p[0] - ox, p[1] - oy)            # noqa: E731
        if ep is None:
            jobs.append((k, "far", rel(poly.position), None))
            continue
        ep = np.squeeze(ep)
        if ep.shape == (2,):
            jobs.append((k, "one", rel(ep), None))
        elif ep.shape == (2, 2):
            jobs.append((k, "pair", rel(ep[0]), rel(ep[1])))
        elif ep.ndim == 2 and ep.shape[1] == 2:
            pairs_of[k] = []
            for k1, p1 in enumerate(ep):
                for p2 in ep[:k1]:
                    pairs_of[k].append(len(jobs))
                    jobs.append((k, "pair", rel(p1), rel(p2)))
        else:
            raise TypeError('`end_points` must have shape (2,) or (n, 2), but we found %s' % str(ep.shape))

    paths = [None] * len(jobs)
    for kind in ("far", "one", "pair"):
        sel = [j for j, job in enumerate(jobs) if job[1] == kind]
        for idx, stack in _stacks([masks[jobs[j][0]] for j in sel]):
            js = [sel[i] for i in idx]
            starts = [jobs[j][2] for j in js]
            if kind == "far":
                res = ops.farthest_points(stack, starts, ret_path=True)
            elif kind == "one":
                maps = ops.distance_map(stack, [[p] for p in starts])
                ends = []
                for r, j in enumerate(js):
                    h, w = masks[jobs[j][0]].shape
                    iy, ix = np.unravel_index(maps[r, :h, :w].argmax(), (h, w))
                    ends.append((int(ix), int(iy)))
                res = ops.distance_map_path(maps, ends)
            else:
                ends = [jobs[j][3] for j in js]
                # a non-integral end point is never met: the reference fills the whole map
                maps = ops.distance_map(stack, [[p] for p in starts], [[e] if _integral(e) else [] for e in ends])
                res = ops.distance_map_path(maps, ends)
            for j, path in zip(js, res):
                if len(path) == 0:
                    k, _, p1, p2 = jobs[j]
                    raise ValueError("polygon %d: no path from %s, which is not a reached pixel of the polygon's "
                                     "mask (shortest_path_in_distance_map's deviation)"
                                     % (k, tuple(np.add(p2 if p2 is not None else p1, offsets[k]))))
                paths[j] = path

    out = [None] * m
    for j, (k, kind, _, _) in enumerate(jobs):
        if k not in pairs_of:
            out[k] = _curves.translate_points(paths[j], *offsets[k])
    for k, js in pairs_of.items():
        longest_path, length = None, 0
        for j in js:
            path = _curves.translate_points(paths[j], *offsets[k])
            path_len = _curves.curve_length(path)
            if path_len > length:
                longest_path, length = path, path_len
        out[k] = longest_path
    return out


def get_centerlines_optimized(polygons, alpha=1e3, beta=1e6, gamma=0.01, spacing=20, max_iterations=1000,
                              endpoints=None):
    """Polygon.get_centerline_optimized (reference :727-757) for every polygon of a list, as one batch: the masks
    (margin 1), their distance transforms and the gradients of the blurred maps are computed back to back on the
    device and stay there as ragged planes (ops.centerline_gradients), the estimates come from
    get_centerline_estimates, and one find_contours call runs every snake, both ends anchored, each on its own
    polygon's planes.  Both equidistant resamplings are batched calls with the translations fused into them
    (curves.resample_many).  endpoints: None, or one entry per polygon as get_centerline_estimates takes them.
    Returns the list of (K, 2) float64 centre lines, each with the bits the per-polygon method gives."""
    from .. import ops
    from .active_contour import ActiveContour
    m = len(polygons)
    eps = [None] * m if endpoints is None else list(endpoints)
    if len(eps) != m:
        raise ValueError("need one end-point entry per polygon (%d polygons, %d entries)" % (m, len(eps)))
    ac = ActiveContour(blur_radius=1, alpha=alpha, beta=beta, gamma=gamma, closed_loop=False)
    ac.max_iterations = max_iterations

    # set the potentials from the distance maps
    rects = [p.get_bounding_rect(margin=1) for p in polygons]
    contours = [np.asarray(p.contour).astype(np.int64) for p in polygons]
    ac._set_gradients(*ops.centerline_gradients(contours, rects, sigma=ac.blur_radius))
    if m == 0:
        return []
    offsets = [(int(r[0]), int(r[1])) for r in rects]

    # initialize the centerlines from the estimates, the end points anchored
    curves = _curves.resample_many(get_centerline_estimates(polygons, eps), spacing=spacing,
                                   offsets=[(-x, -y) for x, y in offsets])[0]
    anchors = []
    for points in curves:
        anchor = np.zeros(len(points), bool)
        anchor[0] = anchor[-1] = True
        anchors.append(anchor)

    # find the best contours
    found = ac.find_contours(curves, list(range(m)), anchors, anchors)
    return _curves.resample_many(found, spacing=spacing, offsets=offsets)[0]


def get_centerlines_smoothed(polygons, spacing=10, skip_length=90, **kwargs):
    """Polygon.get_centerline_smoothed(spacing=, skip_length=, **kwargs) for every polygon of a list: the batched
    get_centerlines_optimized, then the smoothing spline of each centre line on the host"""
    return [smooth_centerline(points, spacing, skip_length)
            for points in get_centerlines_optimized(polygons, spacing=spacing, **kwargs)]


def get_centerlines(polygons, method='smoothed', **kwargs):
    """ Polygon.get_centerline(method, **kwargs) for every polygon of a list, batched """
    if method == 'smoothed':
        return get_centerlines_smoothed(polygons, **kwargs)
    elif method == 'optimized':
        return get_centerlines_optimized(polygons, **kwargs)
    elif method == 'estimate':
        return get_centerline_estimates(polygons, **kwargs)
    else:
        raise ValueError('Unknown method `%s`' % method)


# ------------------------------------------------------------------------------- morphological graphs
def _finish_morphological_graph(graph, simplify_epsilon, offset):
    """the last two steps of Polygon.get_morphological_graph: curves thinned by a positive epsilon, then the
    mask's offset added"""
    if simplify_epsilon > 0:
        graph.simplify(simplify_epsilon)
    graph.translate(*offset)
    return graph


def get_morphological_graphs(polygons, simplify_epsilon=0.1, batched_simplify=False):
    """Polygon.get_morphological_graph(simplify_epsilon, 'guo-hall') of every polygon of a list, as one batch: the
    masks (margin 5), their Guo-Hall skeletons and the skeleton graphs are computed back to back on the device
    (ops.polygon_skeleton_graphs); the post-processing, the simplification and the translation stay on the host.
    Returns the list of MorphologicalGraphs, each with the bits the per-polygon method gives.
    batched_simplify=True thins the curves of all graphs in one device call after the merge step
    (curves.simplify_curves, DESIGN.md §9, "Simplification") instead of one curves.simplify_curve call per curve.
    That is the pinned distance |ax*by - ay*bx| / sqrt(ax*ax + ay*ay), not simplify_curve's np.linalg.det, and the
    results are not always the same: where an exact distance equals epsilon, or is 0, or two maxima tie exactly,
    simplify_curve's answer is rounding noise and the pinned one is exact.  On 1000 random integer curves each, at
    epsilon 0 / 0.1 / 1, the two differed on 19 / 11 / 504 free unit-step walks, on 242 / 0 / 416 unit-step curves
    with one point per column, and on no curve of random vertices in 0..1919.  Hence the default, False."""
    from .. import ops
    from . import curves
    from .morphological_graph import MorphologicalGraph
    rects = [p.get_bounding_rect(margin=5) for p in polygons]
    contours = [np.asarray(p.contour).astype(np.int64) for p in polygons]
    res = ops.polygon_skeleton_graphs(contours, rects) if polygons else []
    graphs = [MorphologicalGraph.from_arrays(g.nodes, g.edges, g.curves) for g in res]
    if not (batched_simplify and simplify_epsilon > 0):
        return [_finish_morphological_graph(graph, simplify_epsilon, (int(r[0]), int(r[1])))
                for graph, r in zip(graphs, rects)]
    for graph in graphs:
        graph.merge_pass_through_nodes()
    given = [[data['curve'] for _, _, data in graph.edges(data=True)] for graph in graphs]
    thinned = curves.simplify_curves([c for cs in given for c in cs], simplify_epsilon)
    at = 0
    for graph, cs, r in zip(graphs, given, rects):
        graph.set_curves(thinned[at:at + len(cs)])
        at += len(cs)
        graph.translate(int(r[0]), int(r[1]))
    return graphs
