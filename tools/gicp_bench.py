"""Timing of the Generalized-ICP refinement for the table of DESIGN.md section 15:  python tools/gicp_bench.py [runs]
The synth workloads bunny (40k points), dragon (437k) and synthetic1m (1M), pre-processed as the solver does, at the true pose.  Per case
the median of `runs` (7) whole calls in one process after one warm-up call: fgoicp_gicp_moments, fgoicp_plane_moments and
fgoicp_alignment with the summary only (every array NULL) — the three share the report's device half, so the differences are the
reductions — and fgoicp_ctx_set_source_normals at k = 16 (the download of the source, the tree build on the host, the upload, the
neighbour kernel, the move into slot order).  One JSON line per workload."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402


def median_seconds(f, runs):
    f()  # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
for wl in ("bunny", "dragon", "synthetic1m"):
    tgt, src, R_gt, t_gt = fg.synth.workload(wl, angle_deg=20.0)
    pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
    t_s = (np.float64(scale) * (t_gt + off_t.astype(np.float64) - R_gt @ off_s.astype(np.float64))).astype(np.float32)
    R = R_gt.astype(np.float32)
    reg = fg.Registration(pct, pcs, bounds, 0.005)
    reg.set_target_normals(k=16)
    normals_ms = 1e3 * median_seconds(lambda: reg.set_source_normals(k=16), runs)
    Rg = fg.to_glm(R)
    fp = fg._lib.c_float_p
    sm = fg._lib.AlignmentSummary()

    def summary_only():
        fg._lib.check(reg._lib.fgoicp_alignment(reg._h, Rg.ctypes.data_as(fp), t_s.ctypes.data_as(fp), None, None, None, None, C.byref(sm)), "fgoicp_alignment")

    g = reg.gicp_moments(R, t_s)
    print(json.dumps({"workload": wl, "nt": len(pct), "ns": len(pcs), "counted": g.correspondences,
                      "gicp_moments_ms": 1e3 * median_seconds(lambda: reg.gicp_moments(R, t_s), runs),
                      "plane_moments_ms": 1e3 * median_seconds(lambda: reg.plane_moments(R, t_s), runs),
                      "alignment_summary_ms": 1e3 * median_seconds(summary_only, runs),
                      "source_normals_k16_ms": normals_ms}), flush=True)
    reg.close()
