"""Timing of fgoicp_mesh_distance for the table of DESIGN.md section 22:  python tools/mesh_distance_bench.py [runs] [brute_pairs]
Height-field meshes of about 2 000, 200 000 and 2 000 000 faces against 40 097, 437 645 and 1 000 000 queries: the
source clouds of the bunny, dragon and synthetic1m shapes (fg.synth) scaled onto the mesh's box.  Per case the median of `runs` (7) whole
calls in one process after one warm-up call — host arrays in, host arrays out: the host's validation pass and tree, the copies, the
allocation, the sort and the walk — with every array asked for; and the same with the flag that walks no tree wherever faces x queries
stays at or below `brute_pairs` (1e11), with its result compared byte for byte.  One JSON line per case."""
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


def height_field(nf):
    """about nf triangles: a grid of c x c cells, c = floor(sqrt(nf / 2)) (the mesh of tools/mesh_bench.py)"""
    c = int(np.sqrt(nf / 2))
    g = np.linspace(-1.0, 1.0, c + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 0.2 * np.sin(5.0 * x) * np.cos(3.0 * y) + 0.05 * np.random.default_rng(1).normal(size=x.shape)
    V = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(c)[:, None] * (c + 1) + np.arange(c)[None, :]).reshape(-1)
    T = np.concatenate([np.stack([i, i + 1, i + c + 2], 1), np.stack([i, i + c + 2, i + c + 1], 1)]).astype(np.uint32)
    return V, T


def queries(shape, V):
    src = fg.synth.workload(shape)[1].astype(np.float64)
    lo, hi = src.min(0), src.max(0)
    vlo, vhi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    return (vlo + (src - lo) / (hi - lo) * (vhi - vlo)).astype(np.float32)


if __name__ == "__main__":
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    brute_pairs = float(sys.argv[2]) if len(sys.argv) > 2 else 1e11
    for nf, shape in ((2_000, "bunny"), (200_000, "dragon"), (2_000_000, "synthetic1m")):
        V, T = height_field(nf)
        Q = queries(shape, V)
        tree = fg.mesh_distance(V, T, Q, return_map=True)  # warm-up, and the answer
        row = {"faces": len(T), "vertices": len(V), "queries": len(Q), "tree_depth": tree[5]["tree_depth"], "max_dist": float(np.sqrt(tree[5]["max_dist2"])),
               "rms_dist": float(np.sqrt(tree[5]["dist2"].mean())), "tree_ms": 1e3 * median_seconds(lambda: fg.mesh_distance(V, T, Q, return_map=True), runs)}
        if float(len(T)) * float(len(Q)) <= brute_pairs:
            brute = fg.mesh_distance(V, T, Q, return_map=True, brute=True)
            row["brute_equal"] = all(a.tobytes() == b.tobytes() for a, b in zip(tree[:5], brute[:5]))
            row["brute_ms"] = 1e3 * median_seconds(lambda: fg.mesh_distance(V, T, Q, return_map=True, brute=True), max(1, runs if nf <= 2_000 else 3))
        print(json.dumps(row), flush=True)
