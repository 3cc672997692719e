"""CPU: the region intensity of DESIGN.md §9, "Region intensity".  The restatement of tests/region_intensity_checks.py
equals the fixture that two other restatements agreed on (tests/golden/make_golden_region_intensity.py);
ops.RegionIntensity completes the table as NumPy does on the pixel lists of each region; va_intensity_math.h, compiled
with the host compiler under sanitizers into a stand-alone program, gives the same tables, histograms and
percentiles."""
import math

import numpy as np
import pytest

import region_intensity_checks as K


@pytest.fixture(scope="module")
def cases():
    fix = K.fixture()
    assert len(fix) >= 35 and sum(hist is not None for _, _, _, _, hist in fix.values()) >= 5
    return fix


def test_restatement_equals_the_fixture(cases):
    for name, (labels, frames, max_labels, table, hist) in cases.items():
        got_table, got_hist = K.restate(labels, frames, max_labels)
        assert got_table.dtype == table.dtype == np.int64 and np.array_equal(got_table, table), name
        if hist is not None:
            assert got_hist.dtype == hist.dtype == np.uint32 and np.array_equal(got_hist, hist), name
        # the histogram carries the count, the sum and the sum of squares again
        v = np.arange(256, dtype=np.int64)
        assert np.array_equal(got_hist.sum(-1), table[..., 6]), name
        assert np.array_equal((got_hist * v).sum(-1), table[..., 0]) and np.array_equal((got_hist * v * v).sum(-1), table[..., 1]), name
        assert (table[..., 7] == 0).all() and np.array_equal(table[..., 6], np.broadcast_to(table[..., :1, 6], table.shape[:-1])), name
    empty = cases["background_3"][3]
    assert (empty[..., 4] == 256).all() and (empty[..., 5] == -1).all() and not empty[..., [0, 1, 2, 3, 6, 7]].any()
    full = cases["one_label_full_1"][3]
    assert full[0, 0, 0].tolist() == [255 * 126, 255 * 255 * 126, 255 * 9 * sum(range(14)), 255 * 14 * sum(range(9)), 255, 255, 126, 0]


def test_completion_equals_numpy_on_the_pixel_lists(cases):
    """min, max, count and the percentiles are integers and compared exactly.  The float64 results:
    mean = S0 / N and centroid = S2 / S0, S3 / S0 are one correctly rounded division of two exact integers; NumPy's
    v.mean() and (v * x).sum() / v.sum() form the same integers exactly in float64 (all below 2^53) and divide once:
    one rounding each, so the two lie within one unit in the last place of a result <= 255 resp. <= max(h, w):
    tolerance 2^-52 times that bound.  var = S1 / N - mean^2: S1 / N <= 255^2 and mean^2 <= 255^2 each carry at most
    1.5 roundings of 2^-53 * 255^2 (the quotient; the mean's error doubled by the square, and the square's own), the
    difference one more; np.var sums N squared differences, each off by at most 3 * 2^-53 * 255^2 (the mean, doubled,
    and the square), with at most log2(N) + 1 roundings of a pairwise sum and one of the division.  Together below
    (10 + log2 N) * 255^2 * 2^-53."""
    from video import ops
    run = {name: case[:3] for name, case in cases.items()}
    run.update(("content_" + name, case) for name, case in K.content_cases().items() if "own_label" not in name)
    regions = 0
    for name, (labels, frames, max_labels) in run.items():
        table, hist = K.restate(labels, frames, max_labels)
        got = ops.RegionIntensity(table, hist)
        mean, var, std, wc = got.mean, got.var, got.std, got.weighted_centroid
        pct = {q: got.percentile(q) for q in (0, 10, 50, 90.5, 100)}
        assert got.count.shape == table.shape[:2] and mean.shape == table.shape[:3] and wc.shape == table.shape[:3] + (2,), name
        assert got.min.dtype == got.max.dtype == pct[50].dtype == np.int64 and np.array_equal(got.median, pct[50]), name
        lists = K.pixel_lists(labels, frames, max_labels)
        hw = max(labels.shape[1:])
        for f in range(table.shape[0]):
            for l in range(1, max_labels + 1):
                for k in range(table.shape[2]):
                    at = (f, l - 1, k)
                    if (f, l, k) not in lists:
                        assert got.count[f, l - 1] == 0 and got.min[at] == got.max[at] == -1, (name, at)
                        assert all(p[at] == -1 for p in pct.values()), (name, at)
                        assert np.isnan(mean[at]) and np.isnan(var[at]) and np.isnan(std[at]) and np.isnan(wc[at]).all(), (name, at)
                        continue
                    v, xs, ys = lists[(f, l, k)]
                    regions += 1
                    assert got.count[f, l - 1] == len(v) and got.min[at] == v.min() and got.max[at] == v.max(), (name, at)
                    for q, p in pct.items():
                        assert p[at] == K.nearest_rank(v, q), (name, at, q)
                    assert abs(mean[at] - np.mean(v)) <= 255 * 2.0 ** -52, (name, at)
                    tol = (10 + math.log2(len(v))) * 255.0 ** 2 * 2.0 ** -53
                    assert abs(var[at] - np.var(v)) <= tol and var[at] >= 0 and std[at] == np.sqrt(var[at]), (name, at)
                    if v.sum() == 0:
                        assert np.isnan(wc[at]).all(), (name, at)
                    else:
                        want = ((v.astype(np.float64) * xs).sum() / v.sum(), (v.astype(np.float64) * ys).sum() / v.sum())
                        assert np.abs(wc[at] - want).max() <= hw * 2.0 ** -52, (name, at)
    assert regions > 2000
    with pytest.raises(ValueError):
        ops.RegionIntensity(table).percentile(50)               # no histograms
    with pytest.raises(ValueError):
        ops.RegionIntensity(table, hist).percentile(101)
    one = ops.RegionIntensity(table, hist).frame(0, 1)
    assert one.raw.shape == (1,) + table.shape[2:] and one.hist.shape == (1, table.shape[2], 256)
    assert np.array_equal(one.mean, got.mean[0, :1], equal_nan=True)


def test_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    exe = K.compile_shim(tmp_path)
    run = {name: case[:3] for name, case in cases.items()}
    run.update(("content_" + name, case) for name, case in K.content_cases().items())
    run.update(("shape_" + name, case) for name, case in K.shape_cases().items() if name.startswith(("1x", "3x")))
    run["bands"] = K.band_case(3)
    for name, (labels, frames, max_labels) in run.items():
        table, hist, pct = K.run_shim(exe, labels, frames, max_labels)
        want_table, want_hist = K.restate(labels, frames, max_labels)
        assert np.array_equal(table, want_table) and np.array_equal(hist, want_hist), name
        from video import ops
        done = ops.RegionIntensity(want_table, want_hist)
        for i, q in enumerate(K.QS):
            assert np.array_equal(pct[..., i], done.percentile(q)), (name, q)
    table, hist, pct = K.run_shim(exe, np.zeros((0, 3, 4), np.int32), np.zeros((0, 3, 4, 3), np.uint8), 2)
    assert table.shape == (0, 2, 3, 8) and hist.size == 0 and pct.size == 0
