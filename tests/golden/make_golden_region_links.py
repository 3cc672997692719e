"""Writes tests/golden/region_links_v1.npz: label stacks with the region links of DESIGN.md §9, "Region links".

The definition is restated twice here, independently of each other and of the package: with np.unique on the packed
keys, and with a plain dict filled pixel by pixel.  The script asserts that the two agree on every case while it
writes the fixture.  Per case `name`: labels_<name> (n, h, w) int32, prev_<name> (h, w) int32 where the case has
one, links_<name> (k, 4) int32 rows (frame, a, b, count).  Run: python tests/golden/make_golden_region_links.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def links_unique(E, L):
    """(a, b, count) rows of one pair in the order of the first pixel: np.unique on key = a << 32 | b"""
    E, L = E.ravel().astype(np.int64), L.ravel().astype(np.int64)
    key = ((E << 32) | L)[(E >= 1) & (L >= 1)]
    keys, first, count = np.unique(key, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return np.stack([keys[order] >> 32, keys[order] & 0xffffffff, count[order]], 1).reshape(-1, 3)


def links_dict(E, L):
    """the same with a dict over the pixels in raster order (dicts keep the order of first insertion)"""
    seen = {}
    for a, b in zip(E.ravel().tolist(), L.ravel().tolist()):
        if a >= 1 and b >= 1:
            seen[(a, b)] = seen.get((a, b), 0) + 1
    return np.array([(a, b, c) for (a, b), c in seen.items()], np.int64).reshape(-1, 3)


def batch_links(labels, prev, one_pair):
    rows = []
    for t in range(len(labels)):
        E = labels[t - 1] if t else prev
        if E is None:
            continue
        for a, b, c in one_pair(E, labels[t]):
            rows.append((t, a, b, c))
    return np.array(rows, np.int64).reshape(-1, 4).astype(np.int32)


def cases():
    rng = np.random.default_rng(20250)
    out = {}
    for h, w in ((1, 1), (1, 7), (7, 1), (2, 3), (64, 2), (37, 53), (16, 129)):
        for n in (1, 2, 3, 5):
            stack = rng.integers(-1, 5, (n, h, w)).astype(np.int32)
            out["random_%dx%dx%d" % (n, h, w)] = (stack, None)
            out["random_prev_%dx%dx%d" % (n, h, w)] = (stack, rng.integers(-1, 5, (h, w)).astype(np.int32))
    h, w = 37, 53
    yy, xx = np.mgrid[:h, :w]
    out["background"] = (np.zeros((3, h, w), np.int32), np.zeros((h, w), np.int32))
    out["one_label"] = (np.full((2, h, w), 7, np.int32), np.full((h, w), 3, np.int32))
    stripes = np.stack([xx + 1, yy + 1, xx + 1]).astype(np.int32)
    out["stripes"] = (stripes, (yy + 1).astype(np.int32))
    big = 2 ** 31 - 1
    wide = np.choose(rng.integers(0, 5, (3, h, w)), [0, -1, big, big - 65536, 65536 + 3]).astype(np.int32)
    wide[:, ::5, ::3] = -2 ** 31
    out["wide_labels"] = (wide, wide[2])
    ends = np.zeros((2, h, w), np.int32)
    ends[0, 0, 5], ends[0, h - 1, 9], ends[0, 10:20, 10:20] = 4, 4, 9
    ends[1, 0, 5], ends[1, h - 1, 9], ends[1, 12:22, 8:18] = 6, 6, 2
    out["first_and_last_row"] = (ends, None)
    gap = rng.integers(1, 4, (4, h, w)).astype(np.int32)
    gap[2] = 0
    out["empty_pair_between"] = (gap, gap[0])
    return out


def main():
    arrays = {}
    for name, (labels, prev) in cases().items():
        fast, slow = batch_links(labels, prev, links_unique), batch_links(labels, prev, links_dict)
        assert fast.dtype == slow.dtype == np.int32 and np.array_equal(fast, slow), name
        arrays["labels_" + name] = labels
        if prev is not None:
            arrays["prev_" + name] = prev
        arrays["links_" + name] = fast
    path = os.path.join(HERE, "region_links_v1.npz")
    np.savez_compressed(path, **arrays)
    links = [v for k, v in arrays.items() if k.startswith("links_")]
    print("%s: %d cases, %d links, %d bytes" % (path, len(links), sum(len(v) for v in links), os.path.getsize(path)))

if __name__ == "__main__":
    main()
