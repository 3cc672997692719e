"""Curve helpers that ActiveContour needs (reference: video/analysis/curves.py).

Host NumPy: these run on at most a few hundred points per curve.  `curve_length` restates
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
