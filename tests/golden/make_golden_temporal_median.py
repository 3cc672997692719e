"""Writes tests/golden/temporal_median_v1.npz: uint8 stacks with their rank planes over time ("Temporal
median"): out[j, p] = sort(frames[:, p])[ranks[j]].

The definition is restated twice here, independently of each other and of the package: np.sort(axis=0)[rank], and a
Python `sorted` list per pixel.  The script asserts that the two agree on every case while it writes the fixture.
Per case `name` = t<t>_px<px>_<content>: frames_<name> (t, px) uint8 (planes back to back: an odd px makes every
second plane start on an odd byte) and want_<name> (r, px) uint8, the planes of the ranks rank_sets(t) lists, all its
sets one after the other; ranksets_t<t> (sets, 8) int32 holds those sets, each padded with -1.  The depths sit on both sides of every switch of the kernels (8 | 9, 16 | 17, 32 | 33 between
the sorting networks, 64 | 65 between sorting and counting) and at 1, 254 and 255; every depth comes with a px that is
a multiple of four and with one that is not.  Run: python tests/golden/make_golden_temporal_median.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255)
ALIGNED_PX = (4, 16, 64, 256)
ODD_PX = (1, 3, 5, 7, 15, 17, 63, 65, 255, 257, 1027)
CONTENTS = ("noise", "zeros", "full", "ties", "middle", "ascending", "descending", "outlier")
ALL_CONTENTS_AT = (5, 64, 65, 255)          # depths that get every content, at px = 16 and px = 17
MORE_THAN_A_WORKGROUP = ((64, 1027, "ties"), (65, 1027, "noise"))    # beside t32_px1027: 1024 pixels a workgroup
HALF_A_DWORD = ((3, 2, "noise"), (65, 2, "ties"))                    # px = 2: every plane starts on an even byte


def rank_sets(t):
    """the rank sets of depth t: the medians, the minimum, the maximum, both, eight ranks in descending order with a
    repeat, and from t = 8 on eight ranks spread over the depth"""
    sets = [sorted({(t - 1) // 2, t // 2}), [0], [t - 1], [0, t - 1]]
    down = [max(t - 1 - (j * t) // 9, 0) for j in range(7)]
    sets.append(down[:3] + [down[2]] + down[3:])
    if t >= 8:
        sets.append([(j * (t - 1)) // 7 for j in range(8)])
    return sets


def content(kind, t, px, rng):
    noise = rng.integers(0, 256, (t, px), dtype=np.uint8)
    if kind == "noise":
        return noise
    if kind == "zeros":
        return np.zeros((t, px), np.uint8)
    if kind == "full":
        return np.full((t, px), 255, np.uint8)
    if kind == "ties":
        return (rng.integers(0, 2, (t, px)) * 255).astype(np.uint8)
    if kind == "middle":
        return (127 + rng.integers(0, 2, (t, px))).astype(np.uint8)
    if kind == "ascending":
        return np.sort(noise, axis=0)
    if kind == "descending":
        return np.sort(noise, axis=0)[::-1].copy()
    quiet = (100 + rng.integers(0, 4, (t, px))).astype(np.uint8)      # "outlier": one plane far above the others
    quiet[t // 3] = 255
    return quiet


def ranks_numpy(frames, ranks):
    return np.sort(frames, axis=0)[np.asarray(ranks)]


def ranks_lists(frames, ranks):
    out = np.empty((len(ranks), frames.shape[1]), np.uint8)
    for p in range(frames.shape[1]):
        column = sorted(frames[:, p].tolist())
        for j, r in enumerate(ranks):
            out[j, p] = column[r]
    return out


def cases():
    """(t, px, content) of every case"""
    out = []
    for i, t in enumerate(DEPTHS):
        out.append((t, ALIGNED_PX[i % len(ALIGNED_PX)], CONTENTS[(2 * i) % len(CONTENTS)]))
        out.append((t, ODD_PX[i % len(ODD_PX)], CONTENTS[(2 * i + 1) % len(CONTENTS)]))
    for t in ALL_CONTENTS_AT:
        for kind in CONTENTS:
            out += [(t, 16, kind), (t, 17, kind)]
    out += MORE_THAN_A_WORKGROUP + HALF_A_DWORD
    return sorted(set(out))


def main():
    rng = np.random.default_rng(20261020)
    data = {}
    for t, px, kind in cases():
        frames = content(kind, t, px, rng)
        ranks = [r for rs in rank_sets(t) for r in rs]
        assert all(0 <= r < t for r in ranks) and all(1 <= len(rs) <= 8 for rs in rank_sets(t))
        want = ranks_numpy(frames, ranks)
        assert np.array_equal(want, ranks_lists(frames, ranks)), (t, px, kind)
        name = "t%d_px%d_%s" % (t, px, kind)
        data["frames_" + name], data["want_" + name] = frames, want
    for t in DEPTHS:
        data["ranksets_t%d" % t] = np.array([rs + [-1] * (8 - len(rs)) for rs in rank_sets(t)], np.int32)
    assert {t for t, _, _ in cases()} == set(DEPTHS)
    assert {px for _, px, _ in cases()} >= set(ALIGNED_PX) | set(ODD_PX) | {2}
    path = os.path.join(HERE, "temporal_median_v1.npz")
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d bytes" % (path, len(cases()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
