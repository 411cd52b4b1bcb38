"""Timing of fgoicp_mesh_sample for the table of DESIGN.md section 21:  python tools/mesh_bench.py [runs]
Meshes of nf = 10 000 and 1 000 000 faces (a bumpy height field over a square grid, two triangles per cell) at m = 100 000 and 1 000 000
samples.  Per case the median of `runs` (7) whole calls in one process after one warm-up call — host arrays in, host arrays out: the
host's validation pass, the copies, the allocation, the three kernels and the scan — with every array asked for and with the points
only.  One JSON line per case."""
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
    """about nf triangles: a grid of c x c cells, c = floor(sqrt(nf / 2))"""
    c = int(np.sqrt(nf / 2))
    g = np.linspace(-1.0, 1.0, c + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 0.2 * np.sin(5.0 * x) * np.cos(3.0 * y) + 0.05 * np.random.default_rng(1).normal(size=x.shape)
    V = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(c)[:, None] * (c + 1) + np.arange(c)[None, :]).reshape(-1)
    T = np.concatenate([np.stack([i, i + 1, i + c + 2], 1), np.stack([i, i + c + 2, i + c + 1], 1)]).astype(np.uint32)
    return V, T


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
for nf in (10_000, 1_000_000):
    V, T = height_field(nf)
    for m in (100_000, 1_000_000):
        pts, nrm, face, uv, area, info = fg.sample_mesh(V, T, m, seed=1, return_map=True)  # warm-up, and the answer
        print(json.dumps({"faces": len(T), "vertices": len(V), "m": m, "area": info["area"], "unweighted": info["unweighted"],
                          "consistent": bool(face.max() < len(T) and (uv >= 0).all() and (uv.sum(1) <= 1).all() and np.isfinite(pts).all()),
                          "call_ms": 1e3 * median_seconds(lambda: fg.sample_mesh(V, T, m, seed=1, return_map=True), runs),
                          "call_points_only_ms": 1e3 * median_seconds(lambda: fg.sample_mesh(V, T, m, seed=1), runs)}), flush=True)
