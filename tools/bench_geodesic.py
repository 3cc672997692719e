#!/usr/bin/env python3
"""Device time of the geodesic entry points (va_geodesic.hip) on 64 x 1080p masks, HIP events around
each call, inputs resident in HBM.  Three cases: the disc masks of tools/bench_next_tier.py, a
serpentine corridor, and a spiral (the worst case: a sweep pair per turn of the geodesic).  One JSON
line per op: ms per call, and the maps built and sweeps per frame.  For comparison, the CPU time of
scipy.sparse.csgraph.dijkstra for one distance map of one frame.  Run on an MI355X:
    python tools/bench_geodesic.py [--frames 64] [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np
import torch
from video import _hip

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

L = _hip.lib()
dev = torch.device("cuda", 0)
S = torch.cuda.current_stream(dev).cuda_stream
n, h, w = args.frames, 1080, 1920


def discs():
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), np.uint8)
    for k in range(30):
        cx, cy, r = (97 * k * 7) % w, (61 * k * 5) % h, 15 + 3 * k
        m |= (((xx - cx) ** 2 + (yy - cy) ** 2) <= r * r).astype(np.uint8)
    return m


def snake(corridor=24, wall=8):
    m = np.zeros((h, w), np.uint8)
    y, k = 0, 0
    while y + corridor <= h:
        m[y:y + corridor, :] = 1
        if y + corridor + wall + corridor <= h:
            xs = slice(w - corridor, w) if k % 2 == 0 else slice(0, corridor)
            m[y + corridor:y + corridor + wall, xs] = 1
        y += corridor + wall
        k += 1
    return m


def spiral(scale=4):
    """a rectangular spiral corridor (1-pixel corridors and walls on a coarse grid, scaled up)"""
    hc, wc = h // scale, w // scale
    m = np.zeros((hc, wc), np.uint8)
    x0, y0, x1, y1 = 0, 0, wc - 1, hc - 1
    while x0 <= x1 and y0 <= y1:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 - y0 >= 2:
            m[y1, x0 + 2:x1 + 1] = 1
        if x1 - x0 >= 2:
            m[y0 + 2:y1 + 1, x0 + 2] = 1
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
    return np.kron(m, np.ones((scale, scale), np.uint8))


def csgraph_ms(m, p1):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    fill = m != 0
    ys, xs = np.nonzero(fill)
    idx = -np.ones((h, w), np.int64)
    idx[ys, xs] = np.arange(len(ys))
    rows, cols, wts = [], [], []
    for dy, dx, c in ((0, 1, 1.0), (1, 0, 1.0), (1, 1, np.sqrt(2)), (1, -1, np.sqrt(2))):
        ny, nx = ys + dy, xs + dx
        ok = (ny < h) & (nx >= 0) & (nx < w)
        ok[ok] &= fill[ny[ok], nx[ok]]
        rows.append(idx[ys[ok], xs[ok]]); cols.append(idx[ny[ok], nx[ok]]); wts.append(np.full(ok.sum(), c))
    g = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(len(ys),) * 2).tocsr()
    t = time.perf_counter()
    dijkstra(g, directed=False, indices=idx[p1[1], p1[0]])
    return (time.perf_counter() - t) * 1e3


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for name, m in (("discs", discs()), ("snake", snake()), ("spiral", spiral())):
    masks = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m, (n, h, w)))).to(dev)
    ys, xs = np.nonzero(m)
    p1 = (int(xs[0]), int(ys[0]))
    p1s = torch.tensor([p1] * n, dtype=torch.int32, device=dev)
    wsb = L.va_geodesic_workspace_bytes(n, h, w)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    p1o = torch.empty((n, 2), dtype=torch.int32, device=dev); p2o = torch.empty_like(p1o)
    dist = torch.empty((n,), dtype=torch.int32, device=dev); rounds = torch.empty((n, 2), dtype=torch.int32, device=dev)
    cap = 1 << 16
    path = torch.empty((n, cap, 2), dtype=torch.int32, device=dev); npath = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n, h, w), dtype=torch.int32, device=dev)
    nst = torch.ones((n,), dtype=torch.int32, device=dev)
    dm = timed(lambda: _hip.check(L.va_distance_map_i32(masks.data_ptr(), n, h, w, p1s.data_ptr(), nst.data_ptr(), 1,
                                                        None, None, 0, out.data_ptr(), ws.data_ptr(), wsb, S)),
               args.reps)
    fp = timed(lambda: _hip.check(L.va_farthest_points(masks.data_ptr(), n, h, w, p1s.data_ptr(), p1o.data_ptr(),
                                                       p2o.data_ptr(), dist.data_ptr(), rounds.data_ptr(), path.data_ptr(),
                                                       cap, npath.data_ptr(), ws.data_ptr(), wsb, S)), args.reps)
    r = rounds.cpu().numpy()
    fd = timed(lambda: _hip.check(L.va_farthest_points(masks.data_ptr(), n, h, w, None, p1o.data_ptr(),
                                                       p2o.data_ptr(), dist.data_ptr(), rounds.data_ptr(), None,
                                                       0, None, ws.data_ptr(), wsb, S)), args.reps)
    row = {"case": name, "frames": n, "fg_fraction": round(float(m.mean()), 3),
           "distance_map_ms": round(dm, 3), "farthest_points_path_ms": round(fp, 3),
           "farthest_points_default_p1_ms": round(fd, 3),
           "maps_per_frame": int(r[0, 0]), "sweeps_per_frame": int(r[0, 1]),
           "max_dist": int(dist.max().item()), "path_points": int(npath[0].item()),
           "csgraph_dijkstra_1_frame_ms": round(csgraph_ms(m, p1), 1)}
    print(json.dumps(row), flush=True)
