"""Active contours (snakes) fitted to the gradient of a potential (reference:
video/analysis/active_contour.py).

set_potential blurs the potential and takes both 5-tap Sobel gradients on the GPU, and keeps the two
float64 planes there; find_contours runs every iteration of every contour of a call in one kernel launch
(va_snake.hip).  The potential is one image, a stack of equal-sized frames, or a list of images of different
shapes (the distance maps of many polygons), which is kept as one ragged buffer (va_gradients.hip).  The
equidistant points and the point spacing of all contours of a call come from one batched resampling
(curves.resample_many); the host keeps the rest of the per-contour preparation: the evolution matrix (NumPy,
the reference's formula and np.linalg.inv, cached by (N, ds)) and the anchors.

Arithmetic ("Active contours"): the forces, the update and the clip are the reference's; the
matrix-vector product sums in ascending column order, where the reference's np.dot goes through BLAS in an
order of its own, so points agree with the reference to ~1e-11 px rather than bit for bit, and the residual
is summed in a fixed order of its own.
"""
import numpy as np

from . import curves as _curves


class ActiveContour(object):
    """ class that manages an algorithm for using active contours for edge
    detection [http://en.wikipedia.org/wiki/Active_contour_model]

    This implementation is inspired by the following articles:
        http://www.pagines.ma1.upc.edu/~toni/files/SnakesAivru86c.pdf
        http://www.cb.uu.se/~cris/blog/index.php/archives/217
    """

    max_iterations = 50  #< maximal number of iterations
    max_cache_count = 20  #< maximal number of cache entries
    residual_tolerance = 1  #< stop iteration when reaching this residual value

    def __init__(self, blur_radius=10, alpha=0, beta=1e2, gamma=0.001, closed_loop=False):
        """ initializes the active contour model
        blur_radius sets the length scale of the attraction to features.
        alpha is the line tension of the contour (high alpha leads to shorter contours)
        beta is the stiffness of the contour (high beta leads to straighter contours)
        gamma is the time scale of the convergence (high gamma might lead to overshoot)
        closed_loop indicates whether the contour is a closed loop
        """
        self.blur_radius = blur_radius
        self.alpha = float(alpha)  #< line tension
        self.beta = float(beta)  #< stiffness
        self.gamma = float(gamma)  #< convergence rate
        self.closed_loop = closed_loop

        self.clear_cache()  #< also initializes the cache
        self._grad = None  #< (fx, fy, (n, h, w)) on the device; ragged: (fx, fy, (shapes, offsets))
        self._ragged = False  #< the potential is a list of images of different shapes
        self._host = {}  #< downloaded planes
        self.info = {}

    def clear_cache(self):
        """ clears the cache. This method should be called if any of the
        parameters of the model are changed """
        self._Pinv_cache = {}

    def _cache_put(self, key, value):
        """insertion-ordered, at most max_cache_count entries (the oldest go first)"""
        while len(self._Pinv_cache) >= max(int(self.max_cache_count), 1):
            del self._Pinv_cache[next(iter(self._Pinv_cache))]
        self._Pinv_cache[key] = value

    def get_evolution_matrix(self, N, ds):
        """ calculates the evolution matrix """
        # scale parameters
        alpha = self.alpha / ds**2  # tension ~1/ds^2
        beta = self.beta / ds**4  # stiffness ~ 1/ds^4

        # calculate matrix entries
        a = self.gamma * (2 * alpha + 6 * beta) + 1
        b = self.gamma * (-alpha - 4 * beta)
        c = self.gamma * beta

        if self.closed_loop:
            # matrix for closed loop
            P = (
                np.diag(np.zeros(N) + a) +
                np.diag(np.zeros(N - 1) + b, 1) + np.diag([b], -N + 1) +
                np.diag(np.zeros(N - 1) + b, -1) + np.diag([b], N - 1) +
                np.diag(np.zeros(N - 2) + c, 2) + np.diag([c, c], -N + 2) +
                np.diag(np.zeros(N - 2) + c, -2) + np.diag([c, c], N - 2)
            )

        else:
            # matrix for open end with vanishing derivatives
            P = (
                np.diag(np.zeros(N) + a) +
                np.diag(np.zeros(N - 1) + b, 1) +
                np.diag(np.zeros(N - 1) + b, -1) +
                np.diag(np.zeros(N - 2) + c, 2) +
                np.diag(np.zeros(N - 2) + c, -2)
            )
            P[0, 1] = P[-1, -2] = 2 * b
            P[0, 2] = P[-1, -3] = 2 * c
            P[1, 1] = P[-2, -2] = a + c

        # create inverse matrix for iteration
        return np.linalg.inv(P)

    # ------------------------------------------------------------------------------- potential
    def set_potential(self, potential):
        """ sets the potential and calculates the associated derivatives.  `potential` is one (h, w)
        image or an (n, h, w) stack, uint8 or float32; find_contour(..., frame=k) picks a frame.  A list or
        tuple of 2-d potentials of different shapes (one dtype) is kept as it is: every item is blurred and
        differentiated as an image of its own, fx and fy are then lists, and frame=k picks item k """
        from .. import ops
        if isinstance(potential, (list, tuple)) and len(potential) > 0:
            items = [np.asarray(q) for q in potential]
            if all(q.ndim == 2 for q in items) and len(set(q.shape for q in items)) > 1:
                return self._set_ragged_potential(items)
        p = np.asarray(potential)
        if p.dtype not in (np.uint8, np.float32):
            raise TypeError("ActiveContour: potentials must be uint8 or float32, got %s" % p.dtype)
        if p.ndim == 4 or (p.ndim == 3 and p.shape[-1] in (3, 4)):
            raise ValueError("ActiveContour: colour potentials are not supported (shape %r); an (n, h, w) "
                             "stack with w = 3 or 4 is read as colour" % (p.shape,))
        if p.ndim not in (2, 3):
            raise ValueError("ActiveContour: expected an (h, w) potential or an (n, h, w) stack, got shape %r"
                             % (p.shape,))
        if p.shape[-1] < 2 or p.shape[-2] < 2 or (p.ndim == 3 and p.shape[0] < 1):
            raise ValueError("ActiveContour: the potential needs h, w >= 2 (got shape %r)" % (p.shape,))
        grad = ops.potential_gradients(p, self.blur_radius if self.blur_radius > 0 else 0.0)
        self._release()
        self._grad = grad
        self._single = p.ndim == 2

    def _set_ragged_potential(self, items):
        from .. import ops
        for q in items:
            if q.dtype not in (np.uint8, np.float32):
                raise TypeError("ActiveContour: potentials must be uint8 or float32, got %s" % q.dtype)
            if q.shape[0] < 2 or q.shape[1] < 2:
                raise ValueError("ActiveContour: the potential needs h, w >= 2 (got shape %r)" % (q.shape,))
        self._set_gradients(*ops.potential_gradients_ragged(items, self.blur_radius if self.blur_radius > 0 else 0.0))

    def _set_gradients(self, fx, fy, shapes, offsets):
        """takes over the ragged gradient planes (fx, fy float64 DeviceBuffers, item k of shape shapes[k] at
        element offset offsets[k]) as ops.potential_gradients_ragged / ops.centerline_gradients return them"""
        self._release()
        self._grad = (fx, fy, (np.asarray(shapes, np.int32).reshape(-1, 2), np.asarray(offsets, np.int64).reshape(-1)))
        self._ragged = True
        self._single = False

    def _release(self):
        if self._grad is not None:
            self._grad[0].free()
            self._grad[1].free()
        self._grad = None
        self._ragged = False
        self._host = {}

    def _plane(self, k):
        if self._grad is None:
            return None
        if k not in self._host and self._ragged:
            shapes, offsets = self._grad[2]
            sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
            flat = self._grad[k].download((int(sizes.sum()),), np.float64)
            self._host[k] = [flat[o:o + s].reshape(hw) for o, s, hw in zip(offsets.tolist(), sizes.tolist(),
                                                                           shapes.tolist())]
        if k not in self._host:
            n, h, w = self._grad[2]
            v = self._grad[k].download((n, h, w), np.float64)
            self._host[k] = v[0] if self._single else v
        return self._host[k]

    @property
    def fx(self):
        """the x gradient (h, w) -- or (n, h, w) for a stack, a list of arrays for a list of potentials --
        float64, downloaded when read; None before set_potential"""
        return self._plane(0)

    @property
    def fy(self):
        """the y gradient, like fx"""
        return self._plane(1)

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---------------------------------------------------------------------------------- contours
    def _matrix(self, N, ds):
        cache_key = (N, ds)
        Pinv = self._Pinv_cache.get(cache_key, None)
        if Pinv is None:
            Pinv = self.get_evolution_matrix(N, ds)
            self._cache_put(cache_key, Pinv)
        return Pinv

    def find_contour(self, curve, anchor_x=None, anchor_y=None, frame=0):
        """ adapts the contour given by points to the potential image
        anchor_x can be a list of indices for those points whose x-coordinate
            should be kept fixed.
        anchor_y is the respective argument for the y-coordinate
        frame picks the frame of a potential stack
        """
        info = dict(self.info)
        points = self.find_contours([curve], [frame], [anchor_x], [anchor_y])[0]
        if len(points) <= 2:
            self.info.clear()
            self.info.update(info)     # the reference returns before it touches info
        else:
            self.info['iteration_count'] = int(self.info['iteration_count'][0])
            self.info['total_variation'] = float(self.info['total_variation'][0])
        return points

    def find_contours(self, curves, frames=None, anchor_x=None, anchor_y=None):
        """ adapts every curve of `curves` to its frame of the potential, all in one kernel launch.
        frames: None (frame 0 for all) or one frame index per curve; anchor_x, anchor_y: None or one entry
        per curve, each as find_contour takes it.  Returns a list of (N, 2) point arrays and sets
        info['iteration_count'] and info['total_variation'] to arrays with one entry per curve (0 for
        curves of two points or fewer, which come back equidistant and untouched) """
        from .. import _hip, ops
        if self._grad is None:
            raise RuntimeError('Potential must be set before the contour can be adapted.')
        fxb, fyb, shape = self._grad
        n = len(shape[0]) if self._ragged else shape[0]
        m = len(curves)
        frames = [0] * m if frames is None else [int(f) for f in frames]
        anchor_x = [None] * m if anchor_x is None else list(anchor_x)
        anchor_y = [None] * m if anchor_y is None else list(anchor_y)
        if not len(frames) == len(anchor_x) == len(anchor_y) == m:
            raise ValueError("find_contours: frames and anchors need one entry per curve")

        # every curve up to the first bad frame is resampled in one call; the checks then run curve by curve.  If a
        # curve makes that call raise, each is resampled where the loop reaches it, so that the first failing curve
        # raises after the checks of the curves before it, as it always did
        good = next((k for k in range(m) if not 0 <= frames[k] < n), m)
        inputs = [np.asarray(curves[k]) for k in range(good)]
        try:
            resampled, lengths = _curves.resample_many(inputs)
        except _hip.HipError:                   # the device or the library is missing, or a call failed: an error
            raise
        except Exception:
            resampled = lengths = None
        results, jobs = [], []
        for k in range(m):
            if not 0 <= frames[k] < n:
                raise IndexError("find_contours: frame %d of a potential of %d frame(s)" % (frames[k], n))
            curve = inputs[k]
            if resampled is not None:
                points, length = resampled[k], float(lengths[k])
            else:
                points = _curves.make_curve_equidistant(curve)
                length = float(_curves.curve_length(points))
            results.append(points)
            if len(points) <= 2:
                continue
            if not np.all(np.isfinite(points)):
                raise ValueError("find_contours: curve %d has non-finite points" % k)
            if len(points) > ops.SNAKE_MAX_POINTS:
                raise ValueError("find_contours: curve %d has %d points; at most %d are supported"
                                 % (k, len(points), ops.SNAKE_MAX_POINTS))
            jobs.append((k, points) + self._anchors(curve, points, anchor_x[k], anchor_y[k]) + (length,))

        iterations = np.zeros(m, np.int64)
        variation = np.zeros(m, np.float64)
        if jobs:
            max_points = max(len(j[1]) for j in jobs)
            pts = np.zeros((len(jobs), max_points, 2))
            flags = np.zeros((len(jobs), max_points), np.uint8) if any(j[2] is not None for j in jobs) else None
            vals = np.zeros((len(jobs), max_points, 2)) if flags is not None else None
            offsets, mats, where = [], [], {}
            for r, (k, points, f, v, length) in enumerate(jobs):
                N = len(points)
                pts[r, :N] = points
                if f is not None:
                    flags[r, :N] = f
                    vals[r, :N] = v
                ds = length / (N - 1)
                key = (N, ds)
                if key not in where:             # contours of equal (N, ds) share one matrix
                    where[key] = sum(a.size for a in mats)
                    mats.append(np.ascontiguousarray(self._matrix(N, ds).T).reshape(-1))
                offsets.append(where[key])
            planes = (fxb, fyb) + shape if self._ragged else (fxb, fyb, shape)
            out, its, tvs = (ops.active_contour_ragged if self._ragged else ops.active_contour)(
                *planes, pts, [len(j[1]) for j in jobs], [frames[j[0]] for j in jobs],
                np.concatenate(mats), offsets, flags, vals, self.gamma, self.residual_tolerance * self.gamma,
                self.max_iterations)
            if np.any(its < 0):
                raise RuntimeError("find_contours: the snake kernel refused a contour")
            for r, (k, points, f, v, length) in enumerate(jobs):
                results[k] = out[r, :len(points)].copy()
                iterations[k] = its[r]
                variation[k] = tvs[r]

        # collect additional information
        self.info['iteration_count'] = iterations
        self.info['total_variation'] = variation
        return results

    @staticmethod
    def _anchors(curve, points, anchor_x, anchor_y):
        """(flags, values) of the anchored coordinates, or (None, None): each anchor fixes the coordinate of
        the equidistant point nearest to it (the first of equally near ones) at the curve's value; when two
        anchors pick one point, the later one wins, as NumPy's fancy assignment in the reference"""
        if anchor_x is None and anchor_y is None:
            return None, None
        flags = np.zeros(len(points), np.uint8)
        vals = np.zeros((len(points), 2))
        for coord, indices in ((0, anchor_x), (1, anchor_y)):
            if indices is None or len(indices) == 0:
                continue
            ps = curve[indices, :]
            # spatial.distance.cdist(points, ps): sqrt of dx*dx + dy*dy, summed in this order
            d = points[:, None, :] - np.asarray(ps, np.float64)[None, :, :]
            dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
            idx = np.argmin(dist, axis=0)
            vals[idx, coord] = ps[:, coord]
            flags[idx] |= np.uint8(1 << coord)
        return flags, vals
