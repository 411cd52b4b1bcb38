"""Timing of fgoicp_cluster_dbscan for the table of DESIGN.md section 17:  python tools/cluster_bench.py [runs] [workload ...]
Targets of the synth workloads bunny (40k points), dragon (437k) and synthetic1m (1M); eps = 2, 3 and 4 times the median nearest-neighbour
spacing of the cloud (fgoicp_remove_outliers at k = 2 gives it), min_points = 10, the largest cluster kept.  Per case the median of `runs` (5)
whole calls in one process after one warm-up call — host array in, host arrays out: the host's validation pass, the tree build, the copies,
the allocation, the kernels and one host round trip per round — with every array asked for, and the rounds the call reports.  The yardstick
is fgoicp_remove_outliers at k = 20 on the same cloud: the same tree and the same walk with a shrinking bound in place of a constant one.
One JSON line per case.  The kernels alone are not timed here: no entry point exposes them; a kernel trace of this script (cluster_count_kernel,
cluster_hook_kernel, cluster_compress_kernel, cluster_border_kernel) gives them."""
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


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
for wl in sys.argv[2:] or ("bunny", "dragon", "synthetic1m"):
    p = fg.synth.workload(wl)[0]
    spacing = float(np.sqrt(np.float64(np.median(fg.remove_statistical_outliers(p, k=2, return_map=True)[4]))))
    fg.remove_statistical_outliers(p, k=20)  # warm-up
    print(json.dumps({"workload": wl, "points": len(p), "nearest_neighbour_spacing": spacing,
                      "outlier_k20_call_ms": 1e3 * median_seconds(lambda: fg.remove_statistical_outliers(p, k=20, return_map=True), runs)}), flush=True)
    for mult in (2.0, 3.0, 4.0):
        eps = mult * spacing
        kept, label, nbr, size, idx, info = fg.cluster_dbscan(p, eps, min_points=10, return_map=True)  # warm-up, and the answer
        again = fg.cluster_dbscan(p, eps, min_points=10, return_map=True)
        print(json.dumps({"workload": wl, "points": len(p), "eps": eps, "eps_over_spacing": mult, "mean_neighbours": float(nbr.mean()), "clusters": info["clusters"],
                          "core_points": info["core_points"], "border_points": info["border_points"], "noise_points": info["noise_points"], "kept": info["kept"],
                          "rounds": info["rounds"], "rounds_again": again[5]["rounds"],
                          "consistent": bool(np.array_equal(kept, p[label == info["largest_label"]]) and int(size.sum()) == int((label >= 0).sum())
                                             and all(x.tobytes() == y.tobytes() for x, y in zip(again[:5], (kept, label, nbr, size, idx)))),
                          "call_ms": 1e3 * median_seconds(lambda: fg.cluster_dbscan(p, eps, min_points=10, return_map=True), runs),
                          "call_points_only_ms": 1e3 * median_seconds(lambda: fg.cluster_dbscan(p, eps, min_points=10), runs)}), flush=True)
