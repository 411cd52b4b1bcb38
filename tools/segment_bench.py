"""Timing of fgoicp_segment_planes for the table of DESIGN.md section 18:  python tools/segment_bench.py [runs]
Whole calls — host array in, host arrays out: the host's validation pass, the hypothesis tables, the copies, the allocation, the kernels and
the host round trips of every peel — as the median of `runs` (5) calls in one process after one warm-up call, on the planted scene of the
README (5060 points, 256 and 1000 hypotheses), on a room of 300 000 points (two planes, 512 hypotheses) and on 1 M uniform points with 1000
hypotheses.  The scoring kernel alone is timed by tools/calib/segment_score.hip with HIP events at the same sizes: the script builds that
program next to its source when it is not there and runs it.  One JSON line per case."""
import json
import os
import subprocess
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


def planted():
    rng = np.random.default_rng(1)
    s = rng.normal(size=(2000, 3))
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    tab = np.stack([rng.uniform(-2, 2, 3000), rng.uniform(-2, 2, 3000), -1 + rng.normal(size=3000) * 0.002], 1)
    cl = np.array([1.5, 1.2, -0.9]) + rng.normal(size=(60, 3)) * 0.04
    P = np.concatenate([s, tab, cl]).astype(np.float32)
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def room(n):
    rng = np.random.default_rng(9)
    a, b = 2 * n // 5, n // 5
    floor = np.stack([rng.uniform(-4, 4, a), rng.uniform(-4, 4, a), 0.004 * rng.normal(size=a)], 1)
    wall = np.stack([rng.uniform(-4, 4, b), 4 + 0.004 * rng.normal(size=b), rng.uniform(0, 3, b)], 1)
    rest = rng.uniform([-4, -4, 0.3], [4, 4, 3], (n - a - b, 3))
    P = np.concatenate([floor, wall, rest]).astype(np.float32)
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def score_kernel(points, hypotheses):
    src = os.path.join(REPO, "tools", "calib", "segment_score.hip")
    exe = src[:-4]
    if not os.path.exists(exe):
        subprocess.run([fg.build._hipcc(), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-o", exe, src], check=True)
    return json.loads(subprocess.run([exe, str(points), str(hypotheses)], check=True, capture_output=True, text=True, timeout=300).stdout)


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CASES = (("planted", planted(), 0.02, 256, 1, 506), ("planted", planted(), 0.02, 1000, 1, 506), ("room300k", room(300000), 0.02, 512, 2, 30000),
         ("uniform1m", np.ascontiguousarray(np.random.default_rng(2).uniform(-1, 1, (1000000, 3)).astype(np.float32)), 0.02, 1000, 1, 0))
for name, P, T, K, planes, min_inliers in CASES:
    call = lambda return_map: fg.segment_planes(P, T, iterations=K, seed=3, max_planes=planes, min_inliers=min_inliers, return_map=return_map)
    kept, label, idx, models, info = call(True)  # warm-up, and the answer
    again = call(True)
    print(json.dumps({"case": name, "points": len(P), "hypotheses": K, "max_planes": planes, "planes": info["planes"], "inliers": [m["inliers"] for m in models],
                      "kept": info["kept"], "consistent": bool(kept.tobytes() == P[label < 0].tobytes() and label.tobytes() == again[1].tobytes()),
                      "call_ms": 1e3 * median_seconds(lambda: call(True), runs), "call_points_only_ms": 1e3 * median_seconds(lambda: call(False), runs),
                      "score_kernel": score_kernel(len(P), K)}), flush=True)
