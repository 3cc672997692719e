"""Writes tests/golden/sliding_median_v1.npz: uint8 clips with the sliding-window median planes of every frame
("Sliding median"): lower[k] / upper[k] = the sorted window max(0, k - W) .. k - 1 at ranks
(cnt - 1) // 2 and cnt // 2, cnt = min(k, W), both 0 for the empty window; diff[k] = min(255, |2 frame[k] - lower[k] -
upper[k]| >> 1).

The definition is restated twice in tests/sliding_median_checks.py, independently of each other and of the package:
a sort of every window, and a histogram per pixel read off by cumulative sums.  The script asserts that the two agree
on every case while it writes the fixture.  Per case `name` = w<W>_px<px>_<content>: frames_<name> (3 W + 5, px)
uint8, and lower_<name>, upper_<name>, diff_<name> of the same shape.  The windows sit at 1, 2, 3, 64, on both sides
of the switch of the counters from uint8 to uint16 (255 | 256) and at 300; the plane sizes at 1, at odd and even
sizes, and on both sides of the 128 pixels of a workgroup.  Run: python tests/golden/make_golden_sliding_median.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import sliding_median_checks as K  # noqa: E402


def main():
    rng = np.random.default_rng(20261021)
    data = {}
    for window, px, kind in K.CASES:
        frames = K.content(kind, K.frames_of(window), px, rng)
        first, second = K.restate_sorted(frames, window), K.restate_histogram(frames, window)
        for a, b in zip(first, second):
            assert a.dtype == np.uint8 and np.array_equal(a, b), (window, px, kind)
        name = "w%d_px%d_%s" % (window, px, kind)
        assert "frames_" + name not in data
        data["frames_" + name] = frames
        data["lower_" + name], data["upper_" + name], data["diff_" + name] = first
    assert {w for w, _, _ in K.CASES} == set(K.WINDOWS) and {c for _, _, c in K.CASES} == set(K.CONTENTS)
    path = os.path.join(HERE, "sliding_median_v1.npz")
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d bytes" % (path, len(K.CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
