"""GPU, opportunistic: ActiveContour.set_potential's gradients against REAL OpenCV.  The GPU path is pinned to
FilterEngine's scalar order for the CV_64F Sobel ("Active contours"), which is written from
upstream knowledge: agreement with a given cv2 build is checked here, and not assumed.  The bar for the
blurred case is a judgement: builds whose GaussianBlur dispatches to IPP or wider SIMD round differently.
Skips cleanly without cv2."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_active_contour", os.path.join(ROOT, "tests", "golden", "make_golden_active_contour.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sobel_matches_cv2():
    from video import ops
    G = _generator()
    print("cv2", cv2.__version__)
    for dt in (np.uint8, np.float32):
        for h, w in G.SOBEL_SIZES + ((120, 160),):
            x = G.sobel_input(h, w, dt, salt=3)
            gx, gy = ops.sobel5_f64(x)
            assert np.array_equal(gx, cv2.Sobel(x, cv2.CV_64F, 1, 0, ksize=5)), (dt, h, w)
            assert np.array_equal(gy, cv2.Sobel(x, cv2.CV_64F, 0, 1, ksize=5)), (dt, h, w)


def test_set_potential_matches_cv2():
    from video.analysis.active_contour import ActiveContour
    G = _generator()
    for kind in ("f32",):       # uint8 blurs round to integers, where one level moves a gradient by 6 * 16
        p = G.potential(kind)
        for sigma in (1, 10):
            ac = ActiveContour(blur_radius=sigma)
            ac.set_potential(p)
            b = cv2.GaussianBlur(p, (0, 0), sigma)
            for got, want in ((ac.fx, cv2.Sobel(b, cv2.CV_64F, 1, 0, ksize=5)),
                              (ac.fy, cv2.Sobel(b, cv2.CV_64F, 0, 1, ksize=5))):
                scale = max(1.0, np.abs(want).max())
                assert np.abs(got - want).max() <= 1e-4 * scale, (kind, sigma)
