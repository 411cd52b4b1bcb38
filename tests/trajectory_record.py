"""The recorded trajectories of the host driver over the oracle's operators (tests/golden/driver_trajectory.json).

The driver is deterministic on the CPU: a run's seven counters and the bits of its (R, t, sse) depend on the clouds, the schedule
and the knobs only — not on the thread counts (the record was taken under two settings of OMP_NUM_THREADS and FGOICP_HOST_THREADS).
The ROUND tests compare every run they make anyway with its record, so that a change to the driver which is meant to leave the
trajectory alone is held to that.  A change that is meant to move it re-records: FGOICP_TRAJECTORY_RECORD=<file> makes check()
write the entries into <file> instead of comparing them."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_trajectory.json")
COUNTERS = ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb", "rounds")
_record = None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).tobytes().hex()


def entry(stats, R, t, sse, exchange_calls=None):
    e = {"counters": [int(stats[k]) for k in COUNTERS], "R": _bits(R), "t": _bits(t), "sse": _bits(sse)}
    if exchange_calls is not None:
        e["exchange_calls"] = int(exchange_calls)
    return e


def check(name, stats, R, t, sse, exchange_calls=None):
    global _record
    got = entry(stats, R, t, sse, exchange_calls)
    out = os.environ.get("FGOICP_TRAJECTORY_RECORD")
    if out:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec[name] = got
        with open(out, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if _record is None:
        with open(PATH) as f:
            _record = json.load(f)
    assert got == _record[name], (name, got, _record[name])


def check_run(name, r):
    """r: what tests.host_harness.HostDriver.run() returns"""
    check(name, r["stats"], r["R"], r["t"], r["best_sse"])
