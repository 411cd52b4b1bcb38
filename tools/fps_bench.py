"""Timing of fgoicp_farthest_point_sample for the table of DESIGN.md section 16:  python tools/fps_bench.py [runs]
Targets of the synth workloads bunny (40k points) and dragon (437k) at m = 1 000, 4 096 and 16 384, and synthetic1m (1M) at m = 4 096.
Per case the median of `runs` (5) whole calls in one process after one warm-up call — host array in, host arrays out: the host's
validation pass, the copies, the allocation, the m step launches and the finish — with every array asked for and with the points only.
The time per step is derived from two whole calls on the same cloud, (t(m_large) - t(m_small)) / (m_large - m_small): what one more
dependent step costs, launch and kernel boundary included; for the single 1M case it is the whole call over m (an upper bound).  The
numpy restatement of the definition is timed once on the 40k cloud at m = 1 000 as the CPU comparison.  One JSON line per case."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402


def median_seconds(f, runs):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def numpy_fps(p, m, start=0):
    """the definition (include/fgoicp_amd.h) in numpy; the unfused fp32 sum stands in for the fma: a timing, not a check"""
    D = np.full(len(p), np.inf, np.float32)
    low = np.int64(0xFFFFFFFF) - np.arange(len(p), dtype=np.int64)
    picked = np.zeros(len(p), bool)
    idx = np.empty(m, np.uint32)
    c = start
    for t in range(m):
        idx[t] = c
        d = p - p[c]
        D = np.minimum(D, d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]))
        picked[c] = True
        c = int(np.argmax(np.where(picked, np.int64(-1) << np.int64(62), D.view(np.int32).astype(np.int64) << np.int64(32)) | low))
    return idx


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
for wl, ms in (("bunny", (1000, 4096, 16384)), ("dragon", (1000, 4096, 16384)), ("synthetic1m", (4096,))):
    p = fg.synth.workload(wl)[0]
    call_ms = {}
    for m in ms:
        out, idx, pick, mind, owner, info = fg.farthest_point_sample(p, m, return_map=True)  # warm-up, and the answer
        call_ms[m] = 1e3 * median_seconds(lambda: fg.farthest_point_sample(p, m, return_map=True), runs)
        print(json.dumps({"workload": wl, "points": len(p), "m": m, "cover_radius": float(np.sqrt(np.float64(info["cover_dist2"]))),
                          "consistent": bool(np.array_equal(out, p[idx]) and len(np.unique(idx)) == m and np.all(pick[:-1] >= pick[1:]) and mind.max() == info["cover_dist2"]),
                          "call_ms": call_ms[m], "call_points_only_ms": 1e3 * median_seconds(lambda: fg.farthest_point_sample(p, m), runs)}), flush=True)
    lo, hi = min(ms), max(ms)
    step_us = 1e3 * (call_ms[hi] - call_ms[lo]) / (hi - lo) if hi > lo else 1e3 * call_ms[hi] / hi
    print(json.dumps({"workload": wl, "points": len(p), "step_us": step_us, "derived_from": [lo, hi] if hi > lo else "whole call / m"}), flush=True)
    if wl == "bunny":
        t0 = time.perf_counter()
        ref = numpy_fps(p, 1000)
        print(json.dumps({"workload": wl, "points": len(p), "m": 1000, "numpy_ms": 1e3 * (time.perf_counter() - t0),
                          "numpy_picks_equal": int((ref == fg.farthest_point_sample(p, 1000, return_map=True)[1]).sum())}), flush=True)
