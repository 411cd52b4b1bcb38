"""Timing of fgoicp_remove_outliers for the table of DESIGN.md section 14:  python tools/outlier_bench.py [runs]
Targets of the synth workloads bunny (40k points), dragon (437k) and synthetic1m (1M) at k = 16 and k = 32, statistical mode (std ratio 2)
and radius mode (the radius that keeps about half of the cloud).  Per case the median of `runs` (7) whole calls in one process after one
warm-up call — host array in, host arrays out: the host's validation pass, the tree build, the copies, the allocation and the kernels —
with every array asked for and with the kept points only.  One JSON line per case.  The neighbour kernel alone is not timed here: no entry
point exposes it; a kernel trace of this script (outlier_knn_kernel) gives it."""
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


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
for wl in ("bunny", "dragon", "synthetic1m"):
    p = fg.synth.workload(wl)[0]
    for k in (16, 32):
        kept, keep, idx, m, kth, info = fg.remove_statistical_outliers(p, k=k, std_ratio=2.0, return_map=True)  # warm-up, and the answer
        r = float(np.sqrt(np.float64(np.median(kth))))
        rinfo = fg.remove_radius_outliers(p, k, r, return_map=True)[5]
        print(json.dumps({"workload": wl, "points": len(p), "k": k, "kept_statistical": info["kept"], "threshold": info["threshold"], "radius": r,
                          "kept_radius": rinfo["kept"], "consistent": bool(np.array_equal(keep, m <= info["threshold"]) and np.array_equal(kept, p[keep])),
                          "statistical_call_ms": 1e3 * median_seconds(lambda: fg.remove_statistical_outliers(p, k=k, std_ratio=2.0, return_map=True), runs),
                          "statistical_call_points_only_ms": 1e3 * median_seconds(lambda: fg.remove_statistical_outliers(p, k=k, std_ratio=2.0), runs),
                          "radius_call_ms": 1e3 * median_seconds(lambda: fg.remove_radius_outliers(p, k, r, return_map=True), runs)}), flush=True)
