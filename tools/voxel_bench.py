"""Timing of fgoicp_voxel_downsample for the table of DESIGN.md section 13:  python tools/voxel_bench.py [runs]
Targets of the synth workloads bunny (40k points), dragon (437k) and synthetic1m (1M), each at a sparse voxel size (about 2 points per
occupied cell) and a dense one (about 100), found by bisection on the numpy cell count.  Per case the median of `runs` (7) whole calls
in one process after one warm-up call — host array in, host arrays out: the host's validation pass, both copies, the allocation and the
kernels — and next to it the time of the numpy restatement of the definition on the same machine (median of 3).  One JSON line per case."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402


def keys_of(p, v):
    c = np.floor((p.astype(np.float64) - p.min(0).astype(np.float64)) / np.float64(np.float32(v))).astype(np.int64)
    return (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]


def restate(p, v):
    uk, inv, cnt = np.unique(keys_of(p, v), return_inverse=True, return_counts=True)
    sums = np.zeros((len(uk), 3), np.float64)
    np.add.at(sums, inv.reshape(-1), p.astype(np.float64))
    return (sums / cnt[:, None]).astype(np.float32), inv, cnt


def voxel_for(p, per_cell):
    lo, hi = 1e-5, float((p.max(0) - p.min(0)).max())
    for _ in range(30):
        mid = (lo * hi) ** 0.5
        if len(p) / len(np.unique(keys_of(p, mid))) < per_cell:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


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
    for per_cell in (2, 100):
        v = voxel_for(p, per_cell)
        out, vop, cnt, info = fg.voxel_downsample(p, v, return_map=True)  # warm-up, and the answer
        ref, rinv, rcnt = restate(p, v)
        same = bool(np.array_equal(cnt, rcnt) and np.array_equal(vop, rinv) and np.abs(out - ref).max() <= np.spacing(np.abs(ref).max()))
        print(json.dumps({"workload": wl, "points": len(p), "voxel": v, "voxels": info["voxels"], "points_per_voxel": len(p) / info["voxels"],
                          "max_points_per_voxel": info["max_points_per_voxel"], "matches_numpy": same,
                          "gpu_call_ms": 1e3 * median_seconds(lambda: fg.voxel_downsample(p, v, return_map=True), runs),
                          "gpu_call_points_only_ms": 1e3 * median_seconds(lambda: fg.voxel_downsample(p, v), runs),
                          "numpy_ms": 1e3 * median_seconds(lambda: restate(p, v), 3)}), flush=True)
