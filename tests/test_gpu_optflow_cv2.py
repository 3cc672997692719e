"""GPU, opportunistic: FilterOpticalFlow's Farneback flow against REAL OpenCV on textured 640x480 pairs.
The bars (|d magnitude| <= 1e-3 px on 99.9 % of pixels, <= 0.05 px everywhere) are a judgement: builds with
IPP or AVX2/FMA dispatch in GaussianBlur, resize or magnitude differ from the pinned scalar arithmetic
("Optical flow").  Skips cleanly without cv2."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cv2 = pytest.importorskip("cv2", reason="OpenCV is not installed on this box")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_optflow", os.path.join(ROOT, "tests", "golden", "make_golden_optflow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_magnitudes_match_cv2():
    from video import ops
    G = _generator()
    print("cv2", cv2.__version__)
    for seed, step in ((1, (1, 0)), (2, (2, -1)), (3, (0, 3))):
        frames = G.texture_frames(2, 480, 640, seed, step=step, cell=12)
        flow = cv2.calcOpticalFlowFarneback(frames[0], frames[1], None, 0.5, 3, 2, 3, 5, 1.2, 0)
        want, _ = cv2.cartToPolar(flow[..., 0], flow[..., 1])
        got = ops.optical_flow_farneback(frames)[0]
        d = np.abs(got.astype(np.float64) - want)
        print("seed %d: max |d mag| %.3g, 99.9th percentile %.3g, exact %.4f" % (
            seed, d.max(), np.percentile(d, 99.9), np.mean(d == 0)))
        assert np.mean(d <= 1e-3) >= 0.999
        assert d.max() <= 0.05
