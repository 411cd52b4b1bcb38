"""Timing of the robustly weighted normal equations for the table of DESIGN.md section 19:  python tools/robust_bench.py [runs] [rounds]
The synth workloads bunny (40k points) and dragon (437k), pre-processed as the solver does, at the true pose, normals at k = 16.  Per
workload and model, whole calls in one process (each ends in a device synchronise and the read-back of the sums): fgoicp_plane_moments /
fgoicp_gicp_moments, then fgoicp_robust_moments with every loss at the automatic scale, and fgoicp_robust_residuals (the instantiation
with the per-point stores, plus their read-back).  After one warm-up call of each, `rounds` (5) rounds visit the calls in turn, `runs`
(9) timed calls each, so that a drift of the machine falls on all of them alike; reported are the median over all timed calls of a
call and the spread of its per-round medians.  One JSON line per workload and model."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LOSSES = ("none", "huber", "cauchy", "geman_mcclure", "tukey")
for wl in ("bunny", "dragon"):
    tgt, src, R_gt, t_gt = fg.synth.workload(wl, angle_deg=20.0)
    pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
    t_s = (np.float64(scale) * (t_gt + off_t.astype(np.float64) - R_gt @ off_s.astype(np.float64))).astype(np.float32)
    R = R_gt.astype(np.float32)
    reg = fg.Registration(pct, pcs, bounds, 0.005)
    reg.set_target_normals(k=16)
    reg.set_source_normals(k=16)
    for model in ("plane", "gicp"):
        c = reg.robust_scale(R, t_s, model)
        calls = {"plain": (lambda: reg.plane_moments(R, t_s)) if model == "plane" else (lambda: reg.gicp_moments(R, t_s))}
        for loss in LOSSES:
            calls["robust_" + loss] = lambda loss=loss: reg.robust_moments(R, t_s, model, loss, c)
        calls["residuals_tukey"] = lambda: reg.robust_residuals(R, t_s, model, "tukey", c)
        times = {name: [] for name in calls}
        for f in calls.values():
            f()  # warm-up
        for _ in range(rounds):
            for name, f in calls.items():
                ts = []
                for _ in range(runs):
                    t0 = time.perf_counter()
                    f()
                    ts.append(time.perf_counter() - t0)
                times[name].append(ts)
        rec = {"workload": wl, "model": model, "nt": len(pct), "ns": len(pcs), "counted": reg.robust_moments(R, t_s, model, "tukey", c).correspondences, "scale": c,
               "runs": runs, "rounds": rounds}
        for name, ts in times.items():
            per_round = [float(np.median(r)) for r in ts]
            rec[name + "_ms"] = round(1e3 * float(np.median(np.concatenate(ts))), 4)
            rec[name + "_round_medians_ms"] = [round(1e3 * min(per_round), 4), round(1e3 * max(per_round), 4)]
        print(json.dumps(rec), flush=True)
    reg.close()
