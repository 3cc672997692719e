"""Shared by tests/test_temporal_median_host.py and tests/test_gpu_temporal_median.py: the fixture of the temporal rank
planes ("Temporal median"), its rank sets, and the stand-alone host program around va_median_math.h."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "temporal_median_v1.npz")
PERCENTILES = (0, 1, 10, 25, 50, 75, 90, 99, 100)
METHODS = ("lower", "higher", "nearest")


def fixture():
    """{name: (frames (t, px) uint8, [(ranks, planes (k, px) uint8) of every rank set of the depth])}"""
    data = np.load(FIXTURE)
    out = {}
    for key in data.files:
        if not key.startswith("frames_"):
            continue
        name = key[len("frames_"):]
        frames, want = data[key], data["want_" + name]
        sets, at = [], 0
        for row in data["ranksets_t%d" % len(frames)]:
            ranks = [int(r) for r in row if r >= 0]
            sets.append((ranks, want[at:at + len(ranks)]))
            at += len(ranks)
        assert at == len(want)
        out[name] = (frames, sets)
    return out


def stepped(frames, step, filler):
    """a stack whose planes 0, step, 2 step, ... are `frames` and whose other planes hold the byte `filler`"""
    t, px = frames.shape
    out = np.full(((t - 1) * step + 1, px), filler, np.uint8)
    out[::step] = frames
    return out


def host_compiler():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (
        rocm_clang if os.path.exists(rocm_clang) else None)


def compile_shim(directory):
    """tests/median_shim.cpp with -fsanitize=address,undefined: the path of the program"""
    cxx = host_compiler()
    assert cxx is not None, "no host C++ compiler"
    exe = os.path.join(str(directory), "median_shim")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "video-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "median_shim.cpp"), "-o", exe])
    return exe


def run_shim(exe, calls):
    """calls: [(frames (t, px) uint8, ranks, stride)] -> the planes (k, px) of each, as the program computes them in
    one run; the frames go in as (t - 1) * stride + px bytes"""
    blob = []
    for frames, ranks, stride in calls:
        t, px = frames.shape
        flat = np.zeros((t - 1) * stride + px, np.uint8)
        for i in range(t):
            flat[i * stride:i * stride + px] = frames[i]
        blob += [np.array([t, px, stride, len(ranks)] + list(ranks), np.int64).tobytes(), flat.tobytes()]
    done = subprocess.run([exe], input=b"".join(blob), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr.decode("utf-8", "replace")[-2000:]
    out, at = [], 0
    for frames, ranks, _ in calls:
        size = len(ranks) * frames.shape[1]
        out.append(np.frombuffer(done.stdout, np.uint8, size, at).reshape(len(ranks), -1))
        at += size
    assert at == len(done.stdout)
    return out
