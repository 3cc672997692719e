"""Image operations: region properties from image moments, morphology, statistics.

Reference: video/analysis/image.py -- subpixel(s) :23-57, get_subimage :61-85, line_scan :89-106,
get_steepest_point :110-127, set_image_border :205-210, regionprops :310-405.
The ten spatial moments are accumulated on the GPU from run segments (exact integers); the
central / normalised moments and the derived scalars are the reference's formulas evaluated in
float64 on the host (a few dozen flops per region).
"""
import math

import numpy as np

_SPATIAL = ("m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03")


def set_image_border(img, size=1, color=0):
    """sets the border of an image to `color` (in place)"""
    img[:size, :] = color
    img[-size:, :] = color
    img[:, :size] = color
    img[:, -size:] = color


def subpixel(img, pt):
    """gets image intensities at a single point with sub pixel accuracy (image.py:23-38)"""
    x, y = pt
    xi = int(x)
    yi = int(y)
    dx = x - xi
    dy = y - int(y)

    weight_tl = (1.0 - dx) * (1.0 - dy)
    weight_tr = (dx) * (1.0 - dy)
    weight_bl = (1.0 - dx) * (dy)
    weight_br = (dx) * (dy)
    return (weight_tl * img[yi, xi] +
            weight_tr * img[yi, xi + 1] +
            weight_bl * img[yi + 1, xi] +
            weight_br * img[yi + 1, xi + 1])


def subpixels(img, pts):
    """gets image intensities of multiple points with sub pixel accuracy (image.py:42-57); the snake
    kernel of ActiveContour gathers its forces with this arithmetic"""
    x, y = pts[:, 0], pts[:, 1]
    xi = x.astype(np.int64)
    yi = y.astype(np.int64)
    dx = x - xi
    dy = y - yi

    weight_tl = (1.0 - dx) * (1.0 - dy)
    weight_tr = (dx) * (1.0 - dy)
    weight_bl = (1.0 - dx) * (dy)
    weight_br = (dx) * (dy)
    return (weight_tl * img[yi, xi] +
            weight_tr * img[yi, xi + 1] +
            weight_bl * img[yi + 1, xi] +
            weight_br * img[yi + 1, xi + 1])


def _round_half_away(x):
    """Python 2's round(x), which the reference's get_subimage sizes its result with"""
    x = float(x)
    f = math.floor(abs(x))
    if abs(x) - f >= 0.5:
        f += 1.0
    return math.copysign(f, x)


def _uint8_image(img, what, ndims=(2,)):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in ndims:
        raise TypeError("%s: single-channel uint8 images only (float, int16 and colour images are not supported on "
                        "the GPU path), got %s of shape %r" % (what, img.dtype, img.shape))
    return img


def get_subimage(img, slice_x, slice_y, width=None, height=None):
    """extracts the subimage specified by `slice_x` and `slice_y`, optionally resampled to `width` x `height`
    pixels (reference :61-85), through the batched cv2.warpAffine of the GPU path (ops.warp_affine; DESIGN.md §9,
    "Affine warps and line scans").  The reference's transposed naming is kept: the result has int(round(width))
    rows and int(round(height)) columns, `round` being Python 2's (halves away from zero).
    Deviations: uint8 images only (TypeError otherwise); an empty result (a rounded side of 0) and a degenerate
    slice raise ValueError, where OpenCV would warp to the source's size or return an arbitrary matrix."""
    from .. import ops
    img = _uint8_image(img, "get_subimage")
    p1_x, p2_x = slice_x[:2]
    p1_y, p2_y = slice_y[:2]

    if width is None:
        width = p2_x - p1_x

    if height is None:
        if p2_x == p1_x:
            raise ValueError("get_subimage: slice_x is empty")
        height = (p2_y - p1_y) * width / (p2_x - p1_x)

    # get corresponding points between the two images
    pts1 = np.array(((p1_x, p1_y), (p1_x, p2_y), (p2_x, p1_y)), np.float32)
    pts2 = np.array(((0, 0), (height, 0), (0, width)), np.float32)

    # determine and apply the affine transformation
    matrix = ops.affine_transforms(pts1, pts2)
    cols, rows = int(_round_half_away(height)), int(_round_half_away(width))
    if cols < 1 or rows < 1:
        raise ValueError("get_subimage: empty result (%d rows, %d columns)" % (rows, cols))
    return ops.warp_affine(img, matrix, [(rows, cols)])[0]


def line_scan(img, p1, p2, half_width=5):
    """returns the average intensity of an image along a strip of a given half_width, ranging from point p1 to p2
    (reference :89-106): the strip is cv2.warpAffine's, int(2*half_width) rows of int(length) columns, averaged
    over its rows (ops.line_scans; DESIGN.md §9, "Affine warps and line scans").  One scan is one launch: many
    scans of a frame or a stack belong in `line_scans`.
    Deviations: uint8 images only (TypeError otherwise); an empty strip (length < 1 or 2*half_width < 1) and
    p1 == p2 raise ValueError, where the reference returns the column means of a warp to the source's size."""
    from .. import ops
    return ops.line_scans(_uint8_image(img, "line_scan"), [p1], [p2], half_width)[0]


def line_scans(img_or_stack, p1s, p2s, half_width=5):
    """line_scan for many strips in one launch.  With one (h, w) image, p1s and p2s are (m, 2) points and the
    result is the list of m profiles.  With an (n, h, w) stack they hold one (m_f, 2) array per frame, and the
    result is one list of profiles per frame.  half_width: one number for all scans."""
    from .. import ops
    img = _uint8_image(img_or_stack, "line_scans", (2, 3))
    if img.ndim == 2:
        return ops.line_scans(img, p1s, p2s, half_width)
    if len(p1s) != len(img) or len(p2s) != len(img):
        raise ValueError("line_scans: a stack of %d frames needs %d point arrays" % (len(img), len(img)))
    a = [np.asarray(p, np.float64).reshape(-1, 2) for p in p1s]
    b = [np.asarray(p, np.float64).reshape(-1, 2) for p in p2s]
    counts = [len(p) for p in a]
    if counts != [len(p) for p in b]:
        raise ValueError("line_scans: start and end points differ in number")
    if sum(counts) == 0:
        return [[] for _ in counts]
    flat = ops.line_scans(img, np.concatenate(a), np.concatenate(b), half_width,
                          frame_index=np.repeat(np.arange(len(img)), counts))
    ends = np.cumsum(counts).tolist()
    return [flat[e - c:e] for c, e in zip(counts, ends)]


def get_steepest_point(profile, direction=1, smoothing=0):
    """returns the index where the profile is steepest (reference :110-127; host arithmetic).

    profile is a 1D array of intensities
    direction determines whether ascending (direction=1) or descending (direction=-1) slopes are search for
    smoothing determines the standard deviation of a Gaussian smoothing filter that is applied before looking
        for the slope"""
    if len(profile) < 2:
        return np.nan

    if smoothing > 0:
        from scipy.ndimage import gaussian_filter1d
        profile = gaussian_filter1d(profile, smoothing)

    i_max = np.argmax(direction * np.diff(profile))

    return i_max + 0.5


def moments_from_spatial(spatial):
    """dict with the 24 entries of cv2.moments() from the ten spatial moments, evaluated in the
    operation order of OpenCV's completeMomentState"""
    m = {k: float(v) for k, v in zip(_SPATIAL, spatial)}
    cx = cy = inv_m00 = 0.0
    if abs(m["m00"]) > 2.220446049250313e-16:
        inv_m00 = 1.0 / m["m00"]
        cx = m["m10"] * inv_m00
        cy = m["m01"] * inv_m00
    mu20 = m["m20"] - m["m10"] * cx
    mu11 = m["m11"] - m["m10"] * cy
    mu02 = m["m02"] - m["m01"] * cy
    m["mu20"], m["mu11"], m["mu02"] = mu20, mu11, mu02
    m["mu30"] = m["m30"] - cx * (3 * mu20 + cx * m["m10"])
    mu11 += mu11
    m["mu21"] = m["m21"] - cx * (mu11 + cx * m["m01"]) - cy * mu20
    m["mu12"] = m["m12"] - cy * (mu11 + cy * m["m10"]) - cx * mu02
    m["mu03"] = m["m03"] - cy * (3 * mu02 + cy * m["m01"])
    inv_sqrt_m00 = math.sqrt(abs(inv_m00))
    s2 = inv_m00 * inv_m00
    s3 = s2 * inv_sqrt_m00
    for k in ("20", "11", "02"):
        m["nu" + k] = m["mu" + k] * s2
    for k in ("30", "21", "12", "03"):
        m["nu" + k] = m["mu" + k] * s3
    return m


def image_moments(mask):
    """cv2.moments(mask.astype(np.uint8)) for a 0/1 mask (image.py:353)"""
    from .. import ops
    m = (np.asarray(mask) != 0).astype(np.int32)
    if m.ndim != 2:
        raise ValueError("mask must be 2-d")
    return moments_from_spatial(ops.region_stats(m, 1)[0][:10])


def contour_moments(contour):
    """cv2.moments(contour) (image.py:355; shapes.py:533): Green's-theorem moments of a closed
    polygon given as (N, 2) / (N, 1, 2) points.  Integer arrays are read as int32 points, all
    other dtypes as float32 points, like Polygon.moments' explicit cast in the reference."""
    from .. import ops
    return moments_from_spatial(ops.contour_moments(contour))


class regionprops(object):
    """properties of a region given by a boolean mask, by its contour or by precomputed moments
    (reference :310-405; the formulas follow scikit-image, as the reference notes)"""

    def __init__(self, mask=None, contour=None, moments=None):
        if moments is not None:
            self.moments = moments
        elif mask is not None:
            self.moments = image_moments(mask)
        elif contour is not None:
            self.moments = contour_moments(contour)
        else:
            raise ValueError("Either the mask or the moments must be given")

    @property
    def area(self):
        return self.moments["m00"]

    @property
    def centroid(self):
        m = self.moments
        return (m["m10"] / m["m00"], m["m01"] / m["m00"])

    @property
    def orientation(self):
        m = self.moments
        a, b, c = m["mu20"], m["mu11"], m["mu02"]
        if a - c == 0:
            return -np.pi / 4 if b > 0 else np.pi / 4
        return -np.arctan2(2 * b, (a - c)) / 2

    # NumPy's sqrt, as in the reference: an eigenvalue that rounding made slightly negative (a
    # degenerate region such as a slanted line of pixels) gives NaN, not an exception
    @property
    def inertia_tensor_eigvals(self):
        m = self.moments
        a, b, c = m["mu20"] / m["m00"], -m["mu11"] / m["m00"], m["mu02"] / m["m00"]
        root = np.sqrt(4 * b ** 2 + (a - c) ** 2)
        return (a + c) + root, (a + c) - root

    @property
    def eccentricity(self):
        e1, e2 = self.inertia_tensor_eigvals
        return 0 if e1 == 0 else np.sqrt(1 - e2 / e1)

    @property
    def major_axis_length(self):
        with np.errstate(invalid="ignore"):
            return 4 * np.sqrt(self.inertia_tensor_eigvals[0])

    @property
    def minor_axis_length(self):
        with np.errstate(invalid="ignore"):
            return 4 * np.sqrt(self.inertia_tensor_eigvals[1])


def detect_peaks(img, include_plateaus=True):
    """boolean mask of the pixels that are maximal in their 8-neighbourhood; with plateaus the
    eroded zero-background is removed (reference :267-306)"""
    from .. import ops
    return ops.detect_peaks(img, include_plateaus)


def mask_thinning(img, method="auto"):
    """skeleton (thinned image) of a mask (reference :214-263).

    `method`: 'guo-hall' is thinning.guo_hall_thinning (reference :236-241) on the GPU: a connected, one pixel
        wide curve that keeps the mask's topology (ops.guo_hall_thinning; DESIGN.md §9 pins the definition).
        'python' is the reference's fallback of iterated 3x3-cross erosions (:243-258), a different skeleton of
        disconnected ridge pixels.  'auto' is 'python' here, what the reference does without the `thinning` module;
        where that module is installed the reference's 'auto' means 'guo-hall', so ask for it by name.
    Deviation: 'guo-hall' returns a new array and leaves `img` alone (the module thins its argument in place)."""
    from .. import ops
    if method == "guo-hall":
        return ops.guo_hall_thinning([img])[0]
    if method not in ("auto", "python"):
        raise ValueError("Unknown thinning method `%s`" % method)
    return ops.mask_thinning(img)[0]


def get_image_statistics(img, kernel="box", ksize=5, ret_var=True, prior=None,
                         exclude_center=False):
    """mean and variance in a window around every point of an image (reference :131-201).
    `prior` is subtracted before summing (default: the image mean)."""
    from .. import ops
    img = np.asarray(img)
    if prior is None:
        prior = img.mean()
    if kernel not in ("box", "ellipse", "circle"):
        raise ValueError("Unknown filter kernel `%s`" % kernel)
    return ops.image_statistics(img, kernel, int(ksize), prior, exclude_center, ret_var)


def template_search_window(search_rect, t_shape, i_shape):
    """(x0, y0, nx, ny): the positions of a template's top-left corner that keep the template inside the part of
    `search_rect` = (left, top, width, height) that lies in an image of `i_shape` = (height, width); None is the whole
    image.  The rectangle is clipped with the arithmetic of regions.get_overlapping_slices (RuntimeError where it
    misses the image); ValueError where what is left does not hold the template of `t_shape` = (height, width)."""
    from .regions import get_overlapping_slices
    th, tw = int(t_shape[0]), int(t_shape[1])
    if search_rect is None:
        search_rect = (0, 0, i_shape[1], i_shape[0])
    left, top, width, height = (int(v) for v in search_rect)
    if width < 1 or height < 1:
        raise ValueError("the search rectangle %r is empty" % (tuple(search_rect),))
    _, (x0, y0, w, h) = get_overlapping_slices((left, top), (height, width), i_shape, anchor="upper left",
                                               ret_rect=True)
    if w < tw or h < th:
        raise ValueError("the search rectangle %r leaves %d x %d pixels of the image, the template has %d x %d"
                         % (tuple(search_rect), w, h, tw, th))
    return x0, y0, w - tw + 1, h - th + 1


def match_template(img, template, method="ccoeff_normed"):
    """cv2.matchTemplate(img, template, cv2.TM_*) for a monochrome uint8 image: the (h - th + 1, w - tw + 1) float64
    map of scores (ops.match_templates; DESIGN.md §9, "Template matching", pins the arithmetic, which is exact up to
    the final float64 operations where cv2 returns float32 from a DFT).  method: 'sqdiff', 'sqdiff_normed', 'ccorr',
    'ccorr_normed', 'ccoeff' or 'ccoeff_normed'."""
    from .. import ops
    img = _uint8_image(img, "match_template")
    template = _uint8_image(template, "match_template")
    window = template_search_window(None, template.shape, img.shape)
    _, maps = ops.match_templates(img[None], [template], [(0, 0) + window], method=method, maps=True)
    return maps[0]


def find_template(img_or_stack, template, search_rect=None, method="ccoeff_normed"):
    """the best match of `template` in an image: cv2.minMaxLoc of cv2.matchTemplate, restricted to the part of the
    image inside search_rect = (left, top, width, height) (None: the whole image; template_search_window clips it).
    Returns ((x, y), score), the top-left corner of the best position -- the minimum for the sqdiff methods, the
    maximum otherwise, the first in raster order among equals -- and its score.  For a stack (n, h, w), or an
    ops.DeviceFrames, every frame is searched in the same rectangle by one call, and the result is ((n, 2) int32
    positions, (n,) float64 scores).  Only the best records cross to the host."""
    from .. import ops
    template = _uint8_image(template, "find_template")
    if isinstance(img_or_stack, ops.DeviceFrames):
        frames, single = img_or_stack, False
        n, shape = frames.n, (frames.h, frames.w)
    else:
        frames = _uint8_image(img_or_stack, "find_template", ndims=(2, 3))
        single = frames.ndim == 2
        frames = frames[None] if single else frames
        n, shape = len(frames), frames.shape[1:]
    window = template_search_window(search_rect, template.shape, shape)
    best = ops.match_templates(frames, [template], [(f, 0) + window for f in range(n)], method=method)
    positions = np.stack([best["x"], best["y"]], axis=1)
    if single:
        return (int(positions[0, 0]), int(positions[0, 1])), float(best["score"][0])
    return positions, best["score"].copy()
