#!/usr/bin/env python3
"""va_label_i32 on 64 x 1080p masks of known span occupancy, through the per-frame kernel with its span list
(hook path 2) and with the dense link sweep forced (path 5): the measurement behind kListPercent in va_ccl.hip.
Masks: all foreground, and one pixel in a share p of the (row, 256-pixel span) pairs.
    python tools/span_list_crossover.py [library under video-analysis_amd/csrc/build/dbg]
Build the library with -DVA_CCL_LIST_PERCENT=100 (tools/debug/build_variant.sh) to time the list at every
share; a library from before the span list has no path 5 and reports path 2 only.  Run on an MI355X."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-analysis_amd"))
import numpy as np, torch
from video import _hip
if len(sys.argv) > 1:
    _hip.LIB_PATH = os.path.join(ROOT, "video-analysis_amd/csrc/build/dbg", sys.argv[1])
L = _hip.lib()
dev = torch.device("cuda", 0)
n, h, w = 64, 1080, 1920
rng = np.random.default_rng(5)


def spans(share):
    m = np.zeros((n, h, w), np.uint8)
    g = (w + 255) // 256
    pick = rng.random((n, h, g)) < share
    x = rng.integers(0, 256, (n, h, g))
    f, y, s = np.nonzero(pick)
    xs = np.minimum(s * 256 + x[f, y, s], w - 1)
    m[f, y, xs] = 1
    return m


masks = [("ones", np.ones((n, h, w), np.uint8))] + [("spans %3d %%" % p, spans(p / 100.0)) for p in (10, 25, 50, 75, 100)]
ws_bytes = L.va_label_workspace_bytes(n, h, w)
ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
lab = torch.empty((n, h, w), dtype=torch.int32, device=dev)
cnt = torch.empty((n,), dtype=torch.int32, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream
for name, m in masks:
    src = torch.from_numpy(m).to(dev)
    line = []
    for path in (2, 5):
        if L.va_test_hook_labelling(path, 0) != 0:
            line.append("path %d: not in this library" % path)
            continue
        ts = []
        for rep in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.check(L.va_label_i32(src.data_ptr(), lab.data_ptr(), cnt.data_ptr(), n, h, w, 4, ws.data_ptr(), ws_bytes, st))
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts = sorted(ts[5:])
        line.append("path %d: median %.1f us (min %.1f)" % (path, ts[len(ts) // 2], ts[0]))
    _hip.check(L.va_test_hook_labelling(0, 0))
    print("%-12s labels %8d   %s" % (name, int(cnt.sum()), "   ".join(line)), flush=True)
