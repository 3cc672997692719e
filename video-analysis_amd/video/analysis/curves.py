"""Curve helpers that ActiveContour needs (reference: video/analysis/curves.py).

Host NumPy: these run on at most a few hundred points per curve.  The one batched exception is the equidistant
resampling: make_curves_equidistant resamples many curves in one device call (ops.curves_equidistant, DESIGN.md §9,
"Equidistant curves"), with the bits of make_curve_equidistant.  `curve_length` restates
cv2.arcLength(float32 points, closed=False) (curves.py:66-71) without OpenCV: each segment is a float32
dx*dx + dy*dy (two rounded products, one rounded sum), its float32 square root, and the roots are added
in double in point order.  ActiveContour's point spacing -- and with it the evolution matrix and its
cache key -- comes from this value, so np.hypot (a different rounding) would not do.
"""
import math

import numpy as np


def point_distance(p1, p2):
    """calculates the distance between point p1 and p2 (curves.py:27-29)"""
    return math.hypot(p1[0] - p2[0], p1[1] - p2[1])


def translate_points(points, xoff, yoff):
    """translate points by a certain offset (curves.py:54-63)"""
    if isinstance(points, np.ndarray):
        offset = np.array([xoff, yoff])
        return points + offset[..., :]
    return [(p[0] + xoff, p[1] + yoff) for p in points]


def curve_length(points):
    """returns the total arc length of a curve defined by a number of points (cv2.arcLength of the
    float32 points, open curve)"""
    if len(points) < 2:
        return 0
    p = np.asarray(points, np.float32).reshape(-1, 2)
    d = p[1:] - p[:-1]
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])             # float32 throughout
    return float(np.cumsum(seg.astype(np.float64))[-1])              # double, in point order


def curve_segment_lengths(points):
    """returns the length of all segments of a curve (curves.py:78-81)"""
    dp = np.diff(points, axis=0)
    return np.hypot(dp[:, 0], dp[:, 1])


def make_curve_equidistant(points, spacing=None, count=None):
    """returns a new parameterization of the same curve where points have been chosen equidistantly
    (curves.py:99-148).  With `spacing` the curve is walked and a point dropped every `spacing` (rounded
    so that the length divides evenly); otherwise `count` points (default: as many as given) are placed
    at equal arc length by linear interpolation."""
    points = np.asarray(points, np.double)

    if spacing is not None:
        profile_length = curve_length(points)
        if profile_length < spacing:
            return points

        dx = profile_length / np.round(profile_length / spacing)
        dist = 0
        result = [points[0]]
        for p1, p2 in zip(points[:-1], points[1:]):
            dp = np.linalg.norm(p2 - p1)
            while dist + dp > dx:
                p1 = p1 + (dx - dist) / dp * (p2 - p1)
                result.append(p1.copy())
                dp = np.linalg.norm(p2 - p1)
                dist = 0
            dist += dp

        if dist > 1e-8:
            result.append(points[-1])

    else:
        if count is None:
            count = len(points)
        s = np.cumsum([point_distance(p1, p2) for p1, p2 in zip(points, points[1:])])
        s = np.insert(s, 0, 0)
        sp = np.linspace(s[0], s[-1], count)
        result = np.transpose((np.interp(sp, s, points[:, 0]), np.interp(sp, s, points[:, 1])))

    return result


def resample_many(curves, spacing=None, count=None, offsets=None):
    """make_curve_equidistant(curve, spacing, count) of every curve of a list, then translate_points by its entry
    of `offsets` (None: no translation): (list of (K, 2) float64 arrays, (m,) float64 curve_length of each).  This
    is where the batched callers choose: one device call (ops.curves_equidistant) from ops.CURVES_DEVICE_MIN_BATCH
    curves on, provided the host's np.linalg.norm is the form the device is pinned to (ops.host_norm_is_pinned);
    else the per-curve loop on the host.  The results are the same bits either way.  spacing: None or one positive
    finite number (anything else is a ValueError); count: None, one integer or one per curve."""
    from .. import ops
    curves = list(curves)
    m = len(curves)
    if spacing is not None and not (spacing > 0 and math.isfinite(spacing)):
        raise ValueError("make_curves_equidistant: spacing must be a positive finite number, got %r" % (spacing,))
    if m >= ops.CURVES_DEVICE_MIN_BATCH and ops.host_norm_is_pinned():
        return ops.curves_equidistant(curves, spacing, count, offsets, ret_lengths=True)
    counts = [count] * m if count is None or np.ndim(count) == 0 else list(count)
    if len(counts) != m:
        raise ValueError("make_curves_equidistant: %d count entries for %d curves" % (len(counts), m))
    results, lengths = [], np.zeros(m, np.float64)
    for k, curve in enumerate(curves):
        points = np.asarray(make_curve_equidistant(curve, spacing=spacing, count=counts[k]), np.float64)
        if offsets is not None:
            points = translate_points(points, offsets[k][0], offsets[k][1])
        results.append(points)
        lengths[k] = curve_length(points)
    return results, lengths


def make_curves_equidistant(curves, spacing=None, count=None):
    """make_curve_equidistant for every curve of a list, batched on the device: the list of (K, 2) float64 arrays,
    each with the bits the per-curve function gives.  count may be one integer or one per curve."""
    return resample_many(curves, spacing, count)[0]


def merge_curves(points1, points2):
    """one curve out of two that share an end point (curves.py:87-99): points1, turned so that it ends at the
    shared point, followed by points2, turned so that it starts there; the shared point appears twice.  The pairs
    of ends are tried in the order (last, first), (first, first), (first, last), (last, last), as the reference
    tries them; ValueError if no pair coincides"""
    a, b = np.asarray(points1), np.asarray(points2)
    for a_end, b_end in ((-1, 0), (0, 0), (0, -1), (-1, -1)):
        if np.allclose(a[a_end], b[b_end]):
            return np.concatenate([a if a_end == -1 else a[::-1], b if b_end == 0 else b[::-1]])
    raise ValueError("merge_curves: no end point of the first curve coincides with one of the second")


def simplify_curve(points, epsilon=0):
    """Ramer-Douglas-Peucker simplification of an (N, 2) curve (curves.py:22, the rdp of
    external/simplify_polygon_rdp.py) with that module's arithmetic: a point's distance from the chord is
    |det([x2 - x1, x1 - x0])| / |x2 - x1| (np.linalg.det and norm), or |x0[0] - x1[0]| when the chord's ends have
    equal x; the first point of largest distance splits the curve when that distance exceeds epsilon.  Returns
    the kept points, an array of the input's dtype.
    One deviation: the module also measures the chord's own end point, whose distance is 0 in exact arithmetic;
    where rounding makes it the largest distance above epsilon (float curves with epsilon = 0) the module recurses
    without end, and this function does not test that point."""
    M = np.asarray(points)
    if M.ndim != 2 or len(M) == 0:
        raise ValueError("simplify_curve: expected an (N, 2) curve, got shape %r" % (M.shape,))
    keep = np.zeros(len(M), bool)
    keep[0] = keep[-1] = True
    todo = [(0, len(M) - 1)]
    while todo:
        i0, i1 = todo.pop()
        if i1 - i0 < 2:
            continue
        x1, x2 = M[i0], M[i1]
        x0 = M[i0 + 1:i1]                          # (the module also tests the chord's own end: see below)
        if x1[0] == x2[0]:
            d = np.abs(x0[:, 0] - x1[0])
        else:
            mats = np.empty((len(x0), 2, 2), np.result_type(M.dtype, np.float64))
            mats[:, 0] = x2 - x1
            mats[:, 1] = x1 - x0
            d = np.abs(np.linalg.det(mats)) / np.linalg.norm(x2 - x1)
        k = int(np.argmax(d))                      # the first of the largest
        if d[k] > max(epsilon, 0.0):
            keep[i0 + 1 + k] = True
            todo.append((i0, i0 + 1 + k))
            todo.append((i0 + 1 + k, i1))
    if len(M) == 1:
        return np.vstack((M[0], M[0]))             # the module returns both ends of the chord, here the same point
    return M[keep]


def simplify_curves(curves, epsilon=0):
    """Ramer-Douglas-Peucker simplification of every (N, 2) curve of a list in one device call
    (ops.simplify_curves, DESIGN.md §9, "Simplification"): the list of kept points, each an array of its input's
    dtype.  epsilon: one number or one per curve.
    This is the pinned form, not simplify_curve's bits: a point's distance from the chord is
    |ax*by - ay*bx| / sqrt(ax*ax + ay*ay), every operation rounded once, where simplify_curve goes through
    np.linalg.det, which computes sign * exp(sum(log|u_ii|)).  The two agree on all the curves the reference's own rdp
    was recorded on; they differ where an exact distance equals epsilon, or is 0, or two maxima tie exactly, where
    simplify_curve's answer is rounding noise and this one is exact.  Measured on 1000 random integer curves each,
    at epsilon 0 / 0.1 / 1: free unit-step walks 19 / 11 / 504 differ, unit steps with one point per column
    242 / 0 / 416, random vertices in 0..1919 none.  A curve of one point comes back as that one point, not the two
    equal rows simplify_curve returns."""
    from .. import ops
    return ops.simplify_curves(curves, epsilon, method="rdp")
