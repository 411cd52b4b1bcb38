"""Timing of fgoicp_mesh_refine for the table of DESIGN.md section 23:  python tools/mesh_refine_bench.py [runs]
The meshes and points of tools/mesh_distance_bench.py at its two smaller sizes: height fields of about 2 000 and 200 000 faces against
the 40 097 and 437 645 source points of the bunny and dragon shapes scaled onto the mesh's box, from the identity pose.  Three columns,
all host clocks around whole calls (host arrays in, results out; every call ends in a device synchronise), taken in one process after a
warm-up of each, alternating within each of `runs` (9) rounds so that a drift of the machine meets all three alike:

  evaluation   one evaluation INSIDE fgoicp_mesh_refine: (seconds at max_iter = N0 + K) - (seconds at max_iter = N0), over K, with
               conv_thr = 0 (no step is short enough to stop), N0 = 4, K = 16 — the set-up (tree, uploads, sort) is in both and cancels
  moments      a whole fgoicp_mesh_moments call without per-point outputs: the set-up and one evaluation
  distance     a whole fgoicp_mesh_distance call with dist2 only: what a caller looping over the deviation map pays per evaluation

Per column the median over the rounds and the lowest and highest round.  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402
from tools.mesh_distance_bench import height_field, queries  # noqa: E402

N0, K = 4, 16


def seconds(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


if __name__ == "__main__":
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for nf, shape in ((2_000, "bunny"), (200_000, "dragon")):
        V, T = height_field(nf)
        P = queries(shape, V)
        short = lambda: fg.refine_to_mesh(V, T, P, eye, zero, max_iter=N0, conv_thr=0.0)
        long = lambda: fg.refine_to_mesh(V, T, P, eye, zero, max_iter=N0 + K, conv_thr=0.0)
        moments = lambda: fg.mesh_moments(V, T, P, eye, zero)
        distance = lambda: fg.mesh_distance(V, T, P)
        for f in (short, long, moments, distance):  # warm-up: code objects, rocPRIM's choices, the allocator
            f()
        cols = {"evaluation_ms": [], "moments_ms": [], "distance_ms": [], "refine_short_ms": []}
        for _ in range(runs):
            ts, a = seconds(short)
            tl, b = seconds(long)
            assert a.iterations == N0 and b.iterations == N0 + K, (a.iterations, b.iterations)
            cols["evaluation_ms"].append(1e3 * (tl - ts) / K)
            cols["refine_short_ms"].append(1e3 * ts)
            cols["moments_ms"].append(1e3 * seconds(moments)[0])
            cols["distance_ms"].append(1e3 * seconds(distance)[0])
        row = {"faces": len(T), "points": len(P), "runs": runs, "rms_distance_start": moments().rms_distance, "rms_distance_end": b.rms_distance}
        row.update({k: stats(v) for k, v in cols.items()})
        print(json.dumps(row), flush=True)
