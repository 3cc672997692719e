"""GPU vs a real cv2, where one is installed: cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), cv2.contourArea,
cv2.arcLength, cv2.boundingRect and cv2.moments on the masks of test_gpu_contours.py.  Skips cleanly without cv2."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_contours", os.path.join(ROOT, "tests", "golden", "make_golden_contours.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


def test_contours_and_records_match_cv2():
    from video import ops
    print("\n[cv2 parity] OpenCV %s" % cv2.__version__)
    for name, mask in G.all_cases().items():
        want = cv2.findContours(mask, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)[-2]
        got, info, moments = ops.find_contours(mask, ret_info=True, moments=True)
        assert len(got) == len(want), name
        for g, c, rec, mom in zip(got, want, info, moments):
            assert np.array_equal(g, c), name
            assert rec["area"] == cv2.contourArea(c) and rec["perimeter"] == cv2.arcLength(c, True), name
            assert tuple(rec["rect"]) == tuple(cv2.boundingRect(c)), name
            m = cv2.moments(c)
            assert mom.tolist() == [m[k] for k in ("m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12",
                                                   "m03")], name
