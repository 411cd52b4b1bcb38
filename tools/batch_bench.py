"""Batched Go-ICP against a loop of solo runs (fgoicp_batch vs FastGoICP), same pairs, same process, one GPU.

    python tools/batch_bench.py --workload a      # 64 pairs of ~1k source / 2k target points, lut_resolution 0.01, mse_threshold 1e-3
    python tools/batch_bench.py --workload b      # 16 pairs of the size of the reference's test/bunny.toml (~3k / 18k points)
    python tools/batch_bench.py --trim 0.2        # every pair trimmed (trim_fraction 0.2; a tenth of each source replaced by outliers)
    python tools/batch_bench.py --refine gicp:tukey --pairs 16 --rounds 2
                                                  # every pair refined (MODEL[:LOSS]): a batch with refine= against a loop of solo solvers that
                                                  # run and refine, the two sides alternating, --rounds runs each; its own JSON line

Prints one JSON line: wall time of the batch and of the loop (the loop split into context creation = LUT builds, and runs), the
ratio, whether every pair of the batch is bit-equal to its solo run (R, t, best error, counters), and the fused bounds launches of
the batch against the bounds launches of the solo runs summed (a profiled second loop: FGOICP_FLAG_PROFILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgoicp_amd as fg  # noqa: E402

CONTRACT = ("trans_cubes", "rot_cubes", "inner_bnb", "icp_runs", "icp_iters", "rounds", "initial_icp_sse")
WORKLOADS = {"a": dict(n=64, ns=1000, nt=2000, lut=0.01, mse=1e-3), "b": dict(n=16, ns=3000, nt=18000, lut=0.005, mse=1e-3)}


def make_pairs(w, seed, trim=0.0):
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(w["n"]):
        tgt, src, _, _ = fg.synth.make_pair(w["nt"], w["ns"], (1.0, 0.8, 0.6), seed=seed * 1000 + i, angle_deg=float(rng.uniform(10, 90)), outlier_frac=trim / 2)
        pairs.append((tgt, src, w["lut"], w["mse"]))
    return pairs


def refine_bench(a, w, pairs, kw):
    """--refine: a batch with refine= against a loop of solo solvers that run and refine, alternating; every pair's refinement compared byte
    for byte."""
    model, _, loss = a.refine.partition(":")
    spec = {"model": model, "loss": loss or None}
    loop_s, batch_s, equal, launches = [], [], [], (0, 0)
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        solo = []
        for p in pairs:
            s = fg.FastGoICP(*p, **kw)
            s.run()
            solo.append((s.refine_gicp if model == "gicp" else s.refine_plane)(loss=spec["loss"]).raw)
            s.close()
        loop_s.append(time.perf_counter() - t0)
        b = fg.FastGoICPBatch(pairs, max_live=a.max_live, refine=spec, **kw)
        t0 = time.perf_counter()
        out = b.run()
        batch_s.append(time.perf_counter() - t0)
        equal = [out[i] is not None and b.refined(i).raw == solo[i] for i in range(len(pairs))]
        launches = b.refine_launches()
        b.close()
    print(json.dumps({
        "workload": a.workload, "pairs": len(pairs), "ns": w["ns"], "nt": w["nt"], "lut_resolution": w["lut"], "mse_threshold": w["mse"], "schedule": a.schedule,
        "refine": a.refine, "rounds": a.rounds, "batch_s": [round(t, 4) for t in batch_s], "loop_run_and_refine_s": [round(t, 4) for t in loop_s],
        "speedup_vs_loop": round(min(loop_s) / min(batch_s), 3), "refined_byte_equal": all(equal),
        "fused_refine_launches": launches[0], "refine_evaluations": launches[1]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="a")
    ap.add_argument("--schedule", choices=["serial", "round"], default="serial")
    ap.add_argument("--max-live", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trim", type=float, default=0.0, help="trim_fraction of every pair (0: untrimmed)")
    ap.add_argument("--alignment", action="store_true", help="the batch keeps every pair's alignment report (fgoicp_batch_opts.alignment)")
    ap.add_argument("--information", action="store_true", help="the batch keeps every pair's information matrix (fgoicp_batch_opts.information)")
    ap.add_argument("--refine", default="", help="MODEL[:LOSS], e.g. plane or gicp:tukey: every pair refined after its search; times the batch against a loop that runs and refines")
    ap.add_argument("--pairs", type=int, default=0, help="pairs of the workload (0: its own count)")
    ap.add_argument("--rounds", type=int, default=2, help="--refine: runs of each side, alternating")
    a = ap.parse_args()
    w = dict(WORKLOADS[a.workload])
    if a.pairs > 0:
        w["n"] = a.pairs
    sched = fg.SCHEDULE_ROUND if a.schedule == "round" else fg.SCHEDULE_SERIAL
    rw = 0 if sched == fg.SCHEDULE_ROUND else 1
    pairs = make_pairs(w, a.seed, a.trim)
    kw = dict(schedule=sched, round_width=rw, trim_fraction=a.trim)
    import torch
    torch.cuda.init()

    # warm-up: one solo run (module load, first allocations)
    s = fg.FastGoICP(*pairs[0], **kw)
    s.run()
    s.close()
    if a.refine:
        return refine_bench(a, w, pairs, kw)

    solo, t_create, t_run = [], 0.0, 0.0
    for p in pairs:
        t0 = time.perf_counter()
        s = fg.FastGoICP(*p, **kw)
        t1 = time.perf_counter()
        R, t = s.run()
        t2 = time.perf_counter()
        t_create += t1 - t0
        t_run += t2 - t1
        solo.append((R, t, s.get_best_error(), s.stats()))
        s.close()

    b = fg.FastGoICPBatch(pairs, max_live=a.max_live, alignment=a.alignment, information=a.information, **kw)
    t0 = time.perf_counter()
    out = b.run()
    t_batch = time.perf_counter() - t0
    equal = []
    for i, (R, t, e, st) in enumerate(solo):
        ok = out[i] is not None and np.array_equal(out[i][0].view(np.uint32), R.view(np.uint32)) and np.array_equal(out[i][1].view(np.uint32), t.view(np.uint32))
        ok = ok and np.float32(b.get_best_error(i)).view(np.uint32) == np.float32(e).view(np.uint32)
        ok = ok and all(b.stats(i)[k] == st[k] for k in CONTRACT)
        equal.append(bool(ok))
    bounds_launches, icp_steps = b.launches()
    b.close()

    solo_launches = 0
    for p in pairs:
        s = fg.FastGoICP(*p, **kw, flags=fg.FLAG_PROFILE)
        s.run()
        solo_launches += s.registration.profile()["launches"]
        s.close()

    loop = t_create + t_run
    print(json.dumps({
        "workload": a.workload, "pairs": w["n"], "ns": w["ns"], "nt": w["nt"], "lut_resolution": w["lut"], "mse_threshold": w["mse"], "schedule": a.schedule, "trim_fraction": a.trim, "alignment": bool(a.alignment), "information": bool(a.information),
        "batch_s": round(t_batch, 4), "loop_s": round(loop, 4), "loop_lut_build_s": round(t_create, 4), "loop_run_s": round(t_run, 4),
        "speedup_vs_loop": round(loop / t_batch, 3), "speedup_vs_loop_runs_only": round(t_run / t_batch, 3),
        "bit_equal": equal, "all_bit_equal": all(equal),
        "fused_bounds_launches": bounds_launches, "solo_bounds_launches_summed": solo_launches, "icp_lockstep_iterations": icp_steps}))


if __name__ == "__main__":
    main()
