"""CPU: the region links of DESIGN.md §9, "Region links".  The restatement of tests/region_links_checks.py equals the
fixture that two other restatements agreed on (tests/golden/make_golden_region_links.py) and conserves pixels;
va_links_math.h, compiled with the host compiler under sanitizers into a stand-alone program, gives the same links
and the candidate bound; the entry points are declared and bound and fail loudly without a GPU; RegionTracker on
hand-made links.  Comparisons are exact."""
import numpy as np
import pytest

import region_links_checks as K


@pytest.fixture(scope="module")
def cases():
    fix = K.fixture()
    assert len(fix) >= 60
    return fix


def test_restatement_equals_the_fixture(cases):
    busy = 0
    for name, (labels, prev, want) in cases.items():
        rows, per = K.restate(labels, prev)
        assert rows.dtype == want.dtype and np.array_equal(rows, want), name
        assert np.array_equal(per, np.bincount(want[:, 0], minlength=len(labels))), name
        busy += len(want) >= 40
    assert busy >= 5
    assert len(cases["background"][2]) == 0
    assert cases["one_label"][2].tolist() == [[0, 3, 7, 37 * 53], [1, 7, 7, 37 * 53]]
    assert len(cases["stripes"][2]) == 3 * 37 * 53 and (cases["stripes"][2][:, 3] == 1).all()
    assert cases["wide_labels"][2][:, 1:3].max() == K.I32_MAX and cases["wide_labels"][2][:, 1:3].min() >= 1


def test_conservation(cases):
    for name, (labels, prev, rows) in cases.items():
        for t in range(len(labels)):
            E = labels[t - 1] if t else prev
            mine = rows[rows[:, 0] == t]
            if E is None:
                assert len(mine) == 0, name
                continue
            assert mine[:, 3].sum() == np.count_nonzero((E >= 1) & (labels[t] >= 1)), name
            assert len({(a, b) for a, b in mine[:, 1:3].tolist()}) == len(mine), name
            for a in np.unique(mine[:, 1]):
                assert mine[mine[:, 1] == a, 3].sum() <= np.count_nonzero(E == a), (name, a)
        total, need = len(rows), K.need_of(labels, prev)
        both = sum(np.count_nonzero(((labels[t - 1] if t else prev) >= 1) & (labels[t] >= 1))
                   for t in range(len(labels)) if t or prev is not None)
        assert total <= need <= both, name


def test_math_header_on_the_host_under_sanitizers(cases, tmp_path):
    exe = K.compile_shim(tmp_path)
    run = dict(cases)
    for name, (labels, prev) in K.content_cases().items():
        run["content_" + name] = (labels, prev, K.restate(labels, prev)[0])
    for name, (labels, prev, want) in run.items():
        rows, per, need = K.run_shim(exe, labels, prev)
        assert np.array_equal(rows, want), name
        assert np.array_equal(per, np.bincount(want[:, 0], minlength=len(labels))), name
        assert need == K.need_of(labels, prev), name
    rows, per, need = K.run_shim(exe, np.zeros((0, 3, 4), np.int32))
    assert len(rows) == 0 and len(per) == 0 and need == 0


def test_entry_points_are_declared_bound_and_need_a_gpu():
    from video import _hip, ops
    lib = _hip.load_library()
    assert "va_region_links" in _hip.SIGNATURES and "va_region_links_workspace_bytes" in _hip.SIGNATURES
    assert lib.va_region_links_workspace_bytes(0, 4, 4, 10) == 256 and lib.va_region_links_workspace_bytes(2, 4, 4, -1) == 256
    # never less than room for one pair of any content (2 px + 1 slots of 16 bytes), then 32 bytes a link of capacity
    small, roomy = lib.va_region_links_workspace_bytes(3, 37, 53, 0), lib.va_region_links_workspace_bytes(3, 37, 53, 5000)
    assert small >= (2 * 37 * 53 + 1) * 16 and small == lib.va_region_links_workspace_bytes(3, 37, 53, 1000)
    assert roomy - small >= (2 * 5000 + 3 - 2 * 37 * 53 - 1) * 16 - 256
    # no call needs more than one candidate per pixel: a capacity beyond the pixels adds nothing
    assert (lib.va_region_links_workspace_bytes(3, 37, 53, 3 * 37 * 53)
            == lib.va_region_links_workspace_bytes(3, 37, 53, 2 ** 40))
    if not _hip.gpu_available():
        with pytest.raises(_hip.HipUnavailableError):
            ops.region_links(np.ones((2, 4, 4), np.int32))
        with pytest.raises(_hip.HipUnavailableError):
            ops.region_links(np.ones((0, 4, 4), np.int32))


# ------------------------------------------------------------------------------------------------ the tracker
def _links(pairs):
    """RegionLinks-shaped tuple from one list of (a, b, count) per frame"""
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pairs])]).astype(np.int64)
    flat = np.array([row for p in pairs for row in p], np.int32).reshape(-1, 3)
    return offsets, flat[:, 0], flat[:, 1], flat[:, 2]


def _update(tracker, pairs, counts):
    ids, lin, lout = tracker.update(_links(pairs), np.array(counts, np.int32))
    return [v.tolist() for v in ids], [v.tolist() for v in lin], [v.tolist() for v in lout]


def test_tracker_continuation_birth_and_death():
    from video.analysis.tracking import RegionTracker
    tr = RegionTracker()
    ids, lin, lout = _update(tr, [[], [(1, 2, 10), (2, 1, 8)], [(1, 1, 5)]], [2, 3, 2])
    assert ids == [[0, 1], [1, 0, 2], [1, 3]]           # labels swap, label 3 is born; then 2 and 3 die, 2 is born
    assert lin == [[0, 0], [1, 1, 0], [1, 0]]
    assert lout == [[], [1, 1], [1, 0, 0]]
    assert ids[0] + ids[1] + ids[2] and tr.next_id == 4 and tr.last_ids.tolist() == [1, 3]


def test_tracker_split_and_merge():
    from video.analysis.tracking import RegionTracker
    tr = RegionTracker()
    ids, lin, lout = _update(tr, [[], [(1, 1, 30), (1, 2, 20)], [(1, 1, 30), (2, 1, 20)]], [1, 2, 1])
    assert ids == [[0], [0, 1], [0]]                    # the larger part keeps the id; the merge goes on with it
    assert lout[1] == [2] and lin[1] == [1, 1]          # a split
    assert lin[2] == [2] and lout[2] == [1, 1]          # a merge
    # b = succ(a) is not enough: a must be pred(b) too
    tr = RegionTracker()
    ids, _, _ = _update(tr, [[], [(1, 1, 5), (2, 1, 9)]], [2, 1])
    assert ids == [[0, 1], [1]]
    tr = RegionTracker()
    ids, _, _ = _update(tr, [[], [(1, 1, 9), (1, 2, 5), (2, 2, 1)]], [2, 2])
    assert ids == [[0, 1], [0, 2]]                      # pred(2) = 1 but succ(1) = 1; succ(2) = 2 but pred(2) = 1


def test_tracker_ties_go_to_the_smallest_label():
    from video.analysis.tracking import RegionTracker
    tr = RegionTracker()
    ids, _, _ = _update(tr, [[], [(1, 2, 7), (1, 1, 7)]], [1, 2])           # succ(1): 1 and 2 tie -> 1
    assert ids == [[0], [0, 1]]
    tr = RegionTracker()
    ids, _, _ = _update(tr, [[], [(2, 1, 7), (1, 1, 7)]], [2, 1])           # pred(1): 1 and 2 tie -> 1
    assert ids == [[0, 1], [0]]


def test_tracker_min_overlap():
    from video.analysis.tracking import RegionTracker
    tr = RegionTracker(min_overlap=5)
    ids, lin, lout = _update(tr, [[], [(1, 1, 4), (2, 2, 5)]], [2, 2])
    assert ids == [[0, 1], [2, 1]] and lin[1] == [0, 1] and lout[1] == [0, 1]


def test_tracker_errors():
    from video.analysis.tracking import RegionTracker
    with pytest.raises(ValueError):
        RegionTracker().update(_links([[(1, 1, 3)]]), [1])          # links into nothing
    tr = RegionTracker()
    tr.update(_links([[]]), [2])
    with pytest.raises(ValueError):
        tr.update(_links([[(3, 1, 3)]]), [1])                       # the earlier frame has two regions
    with pytest.raises(ValueError):
        tr.update(_links([[(1, 2, 3)]]), [1])
    with pytest.raises(ValueError):
        tr.update(_links([[], []]), [1])


def test_tracker_one_update_equals_two():
    from video.analysis.tracking import RegionTracker
    rng = np.random.default_rng(12)
    counts = rng.integers(0, 6, 12)
    pairs = [[]]
    for t in range(1, 12):
        keys = sorted({(int(rng.integers(1, counts[t - 1] + 1)), int(rng.integers(1, counts[t] + 1)))
                       for _ in range(8)} if counts[t - 1] and counts[t] else ())
        pairs.append([(a, b, int(rng.integers(1, 4))) for a, b in keys])
    assert sum(len(p) for p in pairs) > 20
    whole = _update(RegionTracker(), pairs, counts)
    tr = RegionTracker()
    head, tail = _update(tr, pairs[:5], counts[:5]), _update(tr, pairs[5:], counts[5:])
    assert all(h + t == w for h, t, w in zip(head, tail, whole))
    flat = [i for frame in whole[0] for i in frame]
    assert sorted(set(flat)) == list(range(max(flat) + 1))          # consecutive ids from 0
