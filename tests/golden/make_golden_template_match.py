"""Writes tests/golden/template_match_v1.npz: uint8 frames, a ragged batch of templates, queries, and for each of the
six methods the best record and the score map of every query ("Template matching").

The definition is restated twice in tests/template_match_checks.py, independently of each other and of the package:
every window through sliding_window_view summed in int64, and integral images with scipy.signal.correlate2d in
int64.  The script asserts that the two agree to the byte on every query and method while it writes the fixture.
Keys: frames (n, h, w) uint8; templates (bytes), template_shapes (m, 2) int32, template_offsets (m + 1,) int64;
queries (q, 6) int32 (frame, templ, x0, y0, nx, ny); status (q,) int32; per method score_<m> (q,) float64, x_<m>,
y_<m> (q,) int32 (zeros for a flagged query) and maps_<m>, the (ny, nx) float64 maps of the queries with status 0,
flattened one behind the other.  Run: python tests/golden/make_golden_template_match.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import template_match_checks as K  # noqa: E402


def main():
    frames, templates, queries = K.fixture_inputs()
    tbytes, shapes, offsets = K.pack_templates(templates)
    data = dict(frames=frames, templates=tbytes, template_shapes=shapes, template_offsets=offsets, queries=queries)
    for method in K.METHODS:
        first = K.restate(frames, templates, queries, method, K.sums_windows)
        second = K.restate(frames, templates, queries, method, K.sums_integral)
        K.same_results(first, second, method)
        best, maps = first
        data["status"] = best["status"]
        data["score_" + method], data["x_" + method], data["y_" + method] = best["score"], best["x"], best["y"]
        data["maps_" + method] = np.concatenate([m.reshape(-1) for m in maps if m is not None])
    kinds = set(data["status"].tolist())
    assert {0, K.BAD_FRAME, K.BAD_TEMPLATE, K.EMPTY, K.OUTSIDE} <= kinds, kinds
    path = os.path.join(HERE, "template_match_v1.npz")
    np.savez_compressed(path, **data)
    print("%s: %d queries, %d positions, %d bytes" % (path, len(queries), data["maps_sqdiff"].size, os.path.getsize(path)))


if __name__ == "__main__":
    main()
