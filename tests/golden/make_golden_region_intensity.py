"""Writes tests/golden/region_intensity_v1.npz: label stacks and frames with the region intensity of DESIGN.md §9,
"Region intensity".

The definition is restated twice here, independently of each other and of the package: with np.bincount /
np.minimum.at over flattened keys, and with a plain dict of Python ints filled pixel by pixel.  The script asserts that
the two agree on every case while it writes the fixture.  Per case `name`: labels_<name> (n, h, w) int32,
frames_<name> (n, h, w) or (n, h, w, 3) uint8, max_labels_<name>, table_<name> (n, max_labels, c, 8) int64, and for a
handful of cases hist_<name> (n, max_labels, c, 256) uint32.  Run: python tests/golden/make_golden_region_intensity.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WITH_HIST = ("random_2x7x9x3", "random_3x5x16x1", "blobs_1", "blobs_3", "garbage_3", "one_label_full_1")


def intensity_bincount(labels, frames, max_labels):
    """table and histograms with np.bincount over key = ((frame * max_labels + label - 1) * c + channel)"""
    n, h, w, c = frames.shape
    entries = n * max_labels * c
    f, y, x = np.nonzero((labels >= 1) & (labels <= max_labels))
    table = np.zeros((entries, 8), np.int64)
    table[:, 4], table[:, 5] = 256, -1
    hist = np.zeros((entries, 256), np.int64)
    for k in range(c):
        key = ((f * max_labels + labels[f, y, x].astype(np.int64) - 1) * c + k).astype(np.int64)
        v = frames[f, y, x, k].astype(np.int64)
        for slot, weight in ((0, v), (1, v * v), (2, v * x), (3, v * y), (6, np.ones_like(v))):
            # (float64 weights: every sum of a fixture case stays far below 2^53)
            table[:, slot] += np.bincount(key, weights=weight, minlength=entries).astype(np.int64)
        np.minimum.at(table[:, 4], key, v)
        np.maximum.at(table[:, 5], key, v)
        hist += np.bincount(key * 256 + v, minlength=entries * 256).reshape(entries, 256)
    return table.reshape(n, max_labels, c, 8), hist.astype(np.uint32).reshape(n, max_labels, c, 256)


def intensity_dict(labels, frames, max_labels):
    """the same pixel by pixel, with Python ints in dicts"""
    n, h, w, c = frames.shape
    table = np.zeros((n, max_labels, c, 8), np.int64)
    table[..., 4], table[..., 5] = 256, -1
    hist = np.zeros((n, max_labels, c, 256), np.uint32)
    recs, bins = {}, {}
    lab, pix = labels.tolist(), frames.tolist()
    for f in range(n):
        for y in range(h):
            for x in range(w):
                l = lab[f][y][x]
                if not 1 <= l <= max_labels:
                    continue
                for k in range(c):
                    v = pix[f][y][x][k]
                    r = recs.setdefault((f, l, k), [0, 0, 0, 0, 256, -1, 0, 0])
                    r[0] += v
                    r[1] += v * v
                    r[2] += v * x
                    r[3] += v * y
                    r[4] = min(r[4], v)
                    r[5] = max(r[5], v)
                    r[6] += 1
                    bins[(f, l, k, v)] = bins.get((f, l, k, v), 0) + 1
    for (f, l, k), r in recs.items():
        table[f, l - 1, k] = r
    for (f, l, k, v), count in bins.items():
        hist[f, l - 1, k, v] = count
    return table, hist


def cases():
    """{name: (labels, frames (n, h, w[, 3]), max_labels)}"""
    rng = np.random.default_rng(20251)
    out = {}

    def noise(shape, c):
        return rng.integers(0, 256, shape + ((3,) if c == 3 else ()), dtype=np.uint8)
    for n, h, w in ((1, 1, 1), (2, 1, 7), (2, 7, 1), (3, 2, 3), (2, 7, 9), (3, 5, 16), (1, 9, 21), (2, 3, 40), (1, 2, 260)):
        for c in (1, 3):
            out["random_%dx%dx%dx%d" % (n, h, w, c)] = (rng.integers(-1, 8, (n, h, w)).astype(np.int32), noise((n, h, w), c), 6)
    h, w = 9, 14
    yy, xx = np.mgrid[:h, :w]
    for c in (1, 3):
        pix = noise((2, h, w), c)
        out["background_%d" % c] = (np.zeros((2, h, w), np.int32), pix, 3)
        out["one_label_%d" % c] = (np.full((2, h, w), 2, np.int32), pix, 2)
        out["one_label_zeros_%d" % c] = (np.full((2, h, w), 2, np.int32), np.zeros_like(pix), 2)
        out["one_label_full_%d" % c] = (np.full((2, h, w), 1, np.int32), np.full_like(pix, 255), 1)
        own = np.stack([np.arange(1, h * w + 1).reshape(h, w)] * 2).astype(np.int32)
        out["own_label_%d" % c] = (own, pix, h * w - 30)
        out["stripes_%d" % c] = (np.stack([xx + 1, yy + 1]).astype(np.int32), pix, w)
        alt = ((xx // 3) % 2 + 1).astype(np.int32)
        out["alternating_3_%d" % c] = (np.stack([alt, alt[:, ::-1]]), pix, 2)
        big = 2 ** 31 - 1
        wide = np.choose(rng.integers(0, 6, (2, h, w)), [0, -1, big, -2 ** 31, 65536 + 3, 3]).astype(np.int32)
        out["garbage_%d" % c] = (wide, pix, 4)
        out["max_labels_1_%d" % c] = (rng.integers(0, 4, (2, h, w)).astype(np.int32), pix, 1)
        blobs = np.zeros((2, h, w), np.int32)
        for t in range(2):
            for k, (cx, cy, r) in enumerate(((5 + 2 * t, 3, 3), (w - 6, h // 2, 4))):
                blobs[t][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = k + 1
        out["blobs_%d" % c] = (blobs, pix, 5)
    return out


def main():
    arrays, with_hist = {}, 0
    for name, (labels, frames, max_labels) in cases().items():
        nhwc = frames[..., None] if frames.ndim == 3 else frames
        fast, slow = intensity_bincount(labels, nhwc, max_labels), intensity_dict(labels, nhwc, max_labels)
        for a, b in zip(fast, slow):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
        arrays["labels_" + name], arrays["frames_" + name] = labels, frames
        arrays["max_labels_" + name], arrays["table_" + name] = np.int32(max_labels), fast[0]
        if name in WITH_HIST:
            arrays["hist_" + name] = fast[1]
            with_hist += 1
    assert with_hist == len(WITH_HIST)
    path = os.path.join(HERE, "region_intensity_v1.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d cases, %d with histograms, %d bytes" % (path, len(cases()), with_hist, os.path.getsize(path)))


if __name__ == "__main__":
    main()
