#!/usr/bin/env python3
"""Time of the outline queries on the GPU (va_ray_hits, va_points_in_outlines, va_outline.hip):
  stars      about 2000 seeded star rings of 20 .. 300 points, 36 rays from the centre of each
  long       16 rings of 5000 points, 1000 rays each
  triangles  100 000 rays onto 3-point rings (1000 triangles, 100 rays each)
  contains   10^6 points in the rings of the first set
  sweep      rings of one size each, 3 .. 1024 points, 36 rays a ring and about 72 000 rays a size: where the
             8-lane and the 64-lane kernel cross (the rule of lanes = 0 and of implementation=None is set from it)
Every leg runs with 8 and with 64 lanes a query on resident data, HIP events around the call; the first four also
run through video.ops with its copies (wall clock, implementation None, 'lanes8', 'lanes64'); --legs picks among
the resident kernels, the ops, the sweep and the restatement.  The NumPy
restatement of tests/golden/make_golden_outline.py on one core runs a subsample for context.  Times are the median
of the repetitions.  One JSON line per leg, appended to profiles/outline_bench.jsonl (or --out); a leg that did not
run is written "not measured".
Run on an MI355X:
    python tools/bench_outline.py [--reps 15]"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--rings", type=int, default=2000)
ap.add_argument("--points", type=int, default=1000000)
ap.add_argument("--cpu", type=int, default=200, help="queries of the restatement legs (0: not measured)")
ap.add_argument("--legs", default="kernels,ops,sweep,cpu", help="which of kernels, ops, sweep and cpu run")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outline_bench.jsonl"))
args = ap.parse_args()
LEGS = set(args.legs.split(","))
SWEEP = (3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 512, 1024)
LANES = (8, 64)


def generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_outline", os.path.join(ROOT, "tests", "golden", "make_golden_outline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = generator()


def fan_batch(rng, sizes, rays):
    """rings of the given sizes about (50, 50) and `rays` rays from the centre of each: (rings, anchors, fars,
    index)"""
    rings = [G.star_ring(rng, int(n)) for n in sizes]
    ang = rng.uniform(0, 2 * np.pi, (len(rings), 1)) + np.arange(rays) * (2 * np.pi / rays)
    anchors = np.full((len(rings) * rays, 2), 50.0)
    fars = anchors + 1000 * np.stack([np.cos(ang).ravel(), np.sin(ang).ravel()], 1)
    return rings, anchors, fars, np.repeat(np.arange(len(rings)), rays).astype(np.int32)


def timed(call, torch):
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(args.reps):
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def wall(call):
    call()
    ms = []
    for _ in range(max(3, args.reps // 3)):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return min(ms), float(np.median(ms))


class Resident(object):
    """a batch in HBM as torch tensors"""

    def __init__(self, torch, dev, rings, queries, fars, index):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.m, self.q = len(rings), len(index)
        counts = np.array([len(r) for r in rings], np.int64)
        self.npoints, self.edges = int(counts.sum()), int(counts[index].sum())
        self.points, self.off = up(np.concatenate(rings)), up(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        self.closed = up(np.ones(self.m, np.uint8))
        self.queries, self.fars, self.index = up(queries), None if fars is None else up(fars), up(index)
        self.t, self.hits = torch.empty(self.q, dtype=torch.float64, device=dev), torch.empty(
            (self.q, 2), dtype=torch.float64, device=dev)
        self.edge, self.count = (torch.empty(self.q, dtype=torch.int32, device=dev) for _ in range(2))
        self.inside = torch.empty(self.q, dtype=torch.uint8, device=dev)

    def rays(self, L, check, lanes, S):
        check(L.va_ray_hits(self.points.data_ptr(), self.off.data_ptr(), self.closed.data_ptr(), self.npoints, self.m,
                            self.queries.data_ptr(), self.fars.data_ptr(), self.index.data_ptr(), self.q, lanes,
                            self.t.data_ptr(), self.hits.data_ptr(), self.edge.data_ptr(), self.count.data_ptr(), S))

    def contains(self, L, check, lanes, S):
        check(L.va_points_in_outlines(self.points.data_ptr(), self.off.data_ptr(), self.npoints, self.m,
                                      self.queries.data_ptr(), self.index.data_ptr(), self.q, lanes,
                                      self.inside.data_ptr(), S))


def kernel_rows(name, res, run, torch, extra=None):
    rows, outs = [], []
    for lanes in LANES:
        best, med = timed(lambda: run(lanes), torch)
        outs.append(torch.cat([res.t.view(torch.uint8), res.hits.view(torch.uint8).reshape(-1),
                               res.edge.view(torch.uint8), res.count.view(torch.uint8), res.inside]).cpu())
        row = {"leg": "%s/lanes%d" % (name, lanes), "outlines": res.m, "points": res.npoints, "queries": res.q,
               "edge_tests": res.edges, "ms_per_call_min": round(best, 4), "ms_per_call_median": round(med, 4),
               "queries_per_s": round(res.q / med * 1e3, 1), "edge_tests_per_s": round(res.edges / med * 1e3, 1)}
        row.update(extra or {})
        rows.append(row)
    rows[-1]["same_bytes_as_lanes8"] = bool(torch.equal(outs[0], outs[1]))
    return rows


def ops_rows(name, call):
    rows = []
    for impl in (None, "lanes8", "lanes64"):
        best, med = wall(lambda: call(impl))
        rows.append({"leg": "%s/ops/%s" % (name, impl or "rule"), "ms_per_call_min": round(best, 3),
                     "ms_per_call_median": round(med, 3), "note": "wall clock with packing, copies and the download"})
    return rows


def main():
    import torch
    dev = torch.device("cuda", 0)
    S = torch.cuda.current_stream(dev).cuda_stream
    from video import _hip, ops
    L, check = _hip.lib(), _hip.check
    rng = np.random.default_rng(31)
    rows, cpu = [], []

    def emit(new):
        for row in new:
            print(json.dumps(row), flush=True)
        rows.extend(new)

    legs = {"stars": fan_batch(rng, rng.integers(20, 301, args.rings), 36),
            "long": fan_batch(rng, [5000] * 16, 1000),
            "triangles": fan_batch(rng, [3] * 1000, 100)}
    for name, (rings, a, f, index) in legs.items():
        if "kernels" in LEGS:
            res = Resident(torch, dev, rings, a, f, index)
            emit(kernel_rows(name, res, lambda lanes: res.rays(L, check, lanes, S), torch))
        if "ops" in LEGS:
            closed = [True] * len(rings)
            emit(ops_rows(name, lambda impl: ops.ray_hits(rings, closed, a, f, index, implementation=impl)))
        cpu.append((name, "rays", rings, a, f, index))
    rings = legs["stars"][0]
    p = 50.0 + rng.uniform(-45, 45, (args.points, 2))
    pidx = rng.integers(0, len(rings), args.points).astype(np.int32)
    if "kernels" in LEGS:
        res = Resident(torch, dev, rings, p, None, pidx)
        emit(kernel_rows("contains", res, lambda lanes: res.contains(L, check, lanes, S), torch))
    if "ops" in LEGS:
        emit(ops_rows("contains", lambda impl: ops.points_in_outlines(rings, p, pidx, implementation=impl)))
    cpu.append(("contains", "points", rings, p, None, pidx))
    for n in SWEEP if "sweep" in LEGS else ():
        rings, a, f, index = fan_batch(rng, [n] * 2000, 36)
        res = Resident(torch, dev, rings, a, f, index)
        emit(kernel_rows("sweep_rays_%d" % n, res, lambda lanes: res.rays(L, check, lanes, S), torch,
                         {"ring_points": n}))
        res = Resident(torch, dev, rings, 50.0 + rng.uniform(-45, 45, (len(index), 2)), None, index)
        emit(kernel_rows("sweep_contains_%d" % n, res, lambda lanes: res.contains(L, check, lanes, S), torch,
                         {"ring_points": n}))
    for name, kind, rings, a, f, index in cpu:
        if not args.cpu or "cpu" not in LEGS:
            emit([{"leg": name + "/numpy_restatement_one_core", "ms_per_query": "not measured"}])
            continue
        pick = rng.choice(len(index), min(args.cpu, len(index)), replace=False)
        t0 = time.perf_counter()
        if kind == "rays":
            G.ray_hits(rings, [True] * len(rings), a[pick], f[pick], index[pick])
        else:
            G.contains_points(rings, a[pick], index[pick])
        ms = (time.perf_counter() - t0) * 1e3
        emit([{"leg": name + "/numpy_restatement_one_core", "queries": len(pick), "ms_per_query": round(ms / len(pick), 4),
               "ms_for_the_whole_leg_extrapolated": round(ms / len(pick) * len(index), 1)}])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


main()
