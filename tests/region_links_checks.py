"""Shared by tests/test_region_links_host.py and tests/test_gpu_region_links.py: the NumPy restatement of the region
links ("Region links"), the fixture, the label stacks the tests run, and the stand-alone host program
around va_links_math.h."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "region_links_v1.npz")
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (64, 2), (37, 53), (16, 129))
COUNTS = (1, 2, 3, 5)
I32_MAX = 2 ** 31 - 1


def pair_links(E, L):
    """the (a, b, count) rows of one pair, in the order of the first pixel"""
    E, L = np.asarray(E).ravel().astype(np.int64), np.asarray(L).ravel().astype(np.int64)
    keys, first, count = np.unique(((E << 32) | L)[(E >= 1) & (L >= 1)], return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return np.stack([keys[order] >> 32, keys[order] & 0xffffffff, count[order]], 1).reshape(-1, 3)


def restate(labels, prev=None):
    """(rows (k, 4) int32 of (frame, a, b, count), links per pair (n,) int32) of a stack"""
    rows, per = [np.zeros((0, 4), np.int64)], np.zeros(len(labels), np.int32)
    for t in range(len(labels)):
        E = labels[t - 1] if t else prev
        if E is not None:
            got = pair_links(E, labels[t])
            rows.append(np.concatenate([np.full((len(got), 1), t), got], 1))
            per[t] = len(got)
    return np.concatenate(rows).astype(np.int32), per


def need_of(labels, prev=None):
    """the candidates of a stack: pixels with a key whose left and upper neighbours carry another key or none"""
    need = 0
    for t in range(len(labels)):
        E = labels[t - 1] if t else prev
        if E is None:
            continue
        E, L = np.asarray(E).astype(np.int64), np.asarray(labels[t]).astype(np.int64)
        key = np.where((E >= 1) & (L >= 1), (E << 32) | L, 0)
        cand = key != 0
        cand[:, 1:] &= key[:, 1:] != key[:, :-1]
        cand[1:, :] &= key[1:, :] != key[:-1, :]
        need += int(cand.sum())
    return need


def as_rows(links):
    """an ops.RegionLinks as (k, 4) int32 rows of (frame, a, b, count)"""
    offsets = np.asarray(links.offsets)
    frame = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return np.stack([frame, links.a, links.b, links.count], 1).astype(np.int32).reshape(-1, 4)


def fixture():
    """{name: (labels, prev or None, rows)}"""
    data = np.load(FIXTURE)
    names = sorted(k[len("labels_"):] for k in data.files if k.startswith("labels_"))
    return {n: (data["labels_" + n], data["prev_" + n] if "prev_" + n in data.files else None, data["links_" + n])
            for n in names}


def content_cases():
    """{name: (labels, prev or None)}: the label contents the GPU test runs, small"""
    rng = np.random.default_rng(4711)
    h, w = 37, 53
    yy, xx = np.mgrid[:h, :w]
    out = {}
    out["background"] = (np.zeros((3, h, w), np.int32), np.zeros((h, w), np.int32))
    out["one_label"] = (np.full((2, h, w), 7, np.int32), np.full((h, w), 3, np.int32))
    blobs = rng.integers(0, 6, (4, h, w)).astype(np.int32)
    out["identical"] = (np.stack([blobs[0]] * 4), blobs[0])
    shifted = np.zeros((4, h, w), np.int32)
    for t in range(4):
        shifted[t, :, t:] = blobs[0][:, :w - t]
    out["shifted"] = (shifted, None)
    out["stripes"] = (np.stack([xx + 1, yy + 1, xx + 1, yy + 1]).astype(np.int32), (yy + 1).astype(np.int32))
    giant = np.ones((2, 40, 50), np.int32)
    giant[1] = 0
    spots = rng.permutation(40 * 50)[:500]
    giant[1].ravel()[spots] = np.arange(1, 501)
    out["giant_vs_500_singles"] = (np.stack([giant[0], giant[1], giant[0]]), giant[1])
    ends = np.zeros((2, h, w), np.int32)
    ends[0, 0, 5], ends[0, h - 1, 9], ends[0, 10:20, 10:20] = 4, 4, 9
    ends[1, 0, 5], ends[1, h - 1, 9], ends[1, 12:22, 8:18] = 6, 6, 2
    out["first_and_last_row"] = (ends, None)
    wide = np.choose(rng.integers(0, 6, (3, h, w)), [0, -1, I32_MAX, I32_MAX - 65536, 65536 + 3, 3]).astype(np.int32)
    wide[:, ::5, ::3] = -2 ** 31
    out["wide_labels"] = (wide, wide[2])
    gap = rng.integers(1, 4, (5, h, w)).astype(np.int32)
    gap[2] = rng.integers(-3, 1, (h, w))
    out["empty_pairs_between"] = (gap, gap[0])
    return out


def shape_cases():
    """{name: (labels, prev or None)}: every frame shape x every n, with and without prev, random labels -1 .. 4"""
    rng = np.random.default_rng(815)
    out = {}
    for h, w in SHAPES:
        for n in COUNTS:
            stack = rng.integers(-1, 5, (n, h, w)).astype(np.int32)
            out["%dx%dx%d" % (n, h, w)] = (stack, None)
            out["%dx%dx%d_prev" % (n, h, w)] = (stack, rng.integers(-1, 5, (h, w)).astype(np.int32))
    return out


def blob_clip(n=12, h=48, w=64, seed=3):
    """(n, h, w) uint8 frames of bright discs that move, meet and part on a dark noisy ground"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    clip = np.empty((n, h, w), np.uint8)
    for t in range(n):
        f = 20 + rng.normal(0, 2, (h, w))
        for cx, cy, r in ((8 + 3 * t, 12, 5), (56 - 3 * t, 14, 5), (20, 36 - t, 4), (44, 30, 3 + (t % 5))):
            f[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 200
        if t in (4, 5, 9):
            f[40:44, 50:56] = 220
        clip[t] = np.clip(f, 0, 255).astype(np.uint8)
    return clip


def host_compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)


def compile_shim(directory):
    """tests/region_links_shim.cpp with -fsanitize=address,undefined: the path of the program"""
    cxx = host_compiler()
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(directory), "region_links_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "region_links_shim.cpp"), "-o", exe])
    return exe


def run_shim(exe, labels, prev=None):
    """(rows, links per pair, need) as the program computes them"""
    labels = np.ascontiguousarray(labels, np.int32)
    n, h, w = labels.shape
    blob = np.array([n, h, w, prev is not None], np.int32).tobytes()
    if prev is not None:
        blob += np.ascontiguousarray(prev, np.int32).tobytes()
    done = subprocess.run([exe], input=blob + labels.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr.decode("utf-8", "replace")[-2000:]
    total, need = np.frombuffer(done.stdout, np.int64, 2)
    per = np.frombuffer(done.stdout, np.int32, n, 16)
    rows = np.frombuffer(done.stdout, np.int32, 4 * int(total), 16 + 4 * n).reshape(-1, 4)
    assert len(done.stdout) == 16 + 4 * n + 16 * int(total)
    return rows, per, int(need)
