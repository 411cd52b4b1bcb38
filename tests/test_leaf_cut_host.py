"""Terminal rows of the early exit (fgoicp_bounds_submit_leaf) and the host driver, without a GPU: tests/host_harness/leaf_harness.cpp runs
the product's driver template over the oracle's operators plus the optional operator entry Ops::bounds_submit_leaf, which answers by the
device's contract — a leaf of the inner BnB (translation span < 0.1, never split) comes back as {T, T} once its UPPER bound is >= T,
every other row once its lower bound is.  The driver must not be able to tell: same counters, same bits as with exact answers
(driver.hpp InnerTask::cut_above / leaf_below carry the proof)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import host_harness as hh

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")
_REPO = os.path.dirname(os.path.dirname(_DIR))
_SO = os.path.join(_DIR, "libleaf_harness.so")
_fp = C.POINTER(C.c_float)
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goicp_golden.npz"))
KEYS = ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb")
NAMES = KEYS + ("rounds",)


@pytest.fixture(scope="module")
def leaf_lib():
    hh.build()  # the oracle library
    deps = [os.path.join(_DIR, "leaf_harness.cpp"), os.path.join(_DIR, "oracle_ops.hpp"), os.path.join(_REPO, "oracle/libgoicp_oracle.so")]
    deps += [os.path.join(_REPO, "fast-go-icp_amd/csrc", f) for f in ("host/driver.hpp", "host/math3.hpp", "host/knobs.hpp", "device/morton.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        tmp = f"{_SO}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fopenmp", "-shared", "-o", tmp, os.path.join(_DIR, "leaf_harness.cpp"),
                        "-L" + os.path.join(_REPO, "oracle"), "-lgoicp_oracle", "-Wl,-rpath," + os.path.join(_REPO, "oracle")], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.leaf_harness_create.argtypes = [_fp, C.c_size_t, _fp, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    L.leaf_harness_create.restype = C.c_void_p
    L.leaf_harness_destroy.argtypes = [C.c_void_p]
    L.leaf_harness_run.argtypes = [C.c_void_p, _fp, _fp, _fp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    return L


def _run(L, mse, sched, K, thresholds, pre="runsyn_"):
    tgt = np.ascontiguousarray(G[pre + "tgt"], np.float32); src = np.ascontiguousarray(G[pre + "src"], np.float32)
    h = C.c_void_p(L.leaf_harness_create(tgt.ctypes.data_as(_fp), len(tgt), src.ctypes.data_as(_fp), len(src), float(G[pre + "res"]), float(mse), sched, K, int(thresholds)))
    try:
        R = np.empty(9, np.float32); t = np.empty(3, np.float32); sse = C.c_float()
        st = (C.c_ulonglong * 7)(); rows = (C.c_ulonglong * 3)()
        assert L.leaf_harness_run(h, R.ctypes.data_as(_fp), t.ctypes.data_as(_fp), C.byref(sse), st, rows) == 0
    finally:
        L.leaf_harness_destroy(h)
    return dict(R=R.reshape(3, 3).T.copy(), t=t, best_sse=np.float32(sse.value), stats={n: int(st[i]) for i, n in enumerate(NAMES)},
                rows=int(rows[0]), cut_lb=int(rows[1]), cut_leaf=int(rows[2]))


def _same(a, b):
    return (a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes() and a["best_sse"].tobytes() == b["best_sse"].tobytes()
            and a["stats"] == b["stats"])


@pytest.mark.parametrize("sched,K", [(0, 1), (3, 1), (5, 1), (1, 3), (2, 4), (4, 0)])
def test_leaf_answers_change_nothing_the_search_can_see(leaf_lib, sched, K):
    """The golden pair under every schedule (0 / 1: the synchronous task loop, which stays on the lower-bound rule; 2 - 5: the pipelined one,
    which submits through bounds_submit_leaf): the run with the new answers is the run with exact answers, and SERIAL is moreover the golden
    record of the oracle's literal restatement of fgoicp.cpp."""
    pre = "runsyn_"
    exact = _run(leaf_lib, float(G[pre + "mse"]), sched, K, False)
    leaf = _run(leaf_lib, float(G[pre + "mse"]), sched, K, True)
    assert exact["rows"] == 0
    assert _same(exact, leaf)
    if sched >= 2:
        assert leaf["rows"] > 0 and leaf["cut_leaf"] > 0  # the new entry was detected, and its rule decided rows
    if sched in (0, 3, 5):
        assert [leaf["stats"][k] for k in KEYS] == list(G[pre + "stats"])
        assert np.array_equal(leaf["R"], G[pre + "R"]) and np.array_equal(leaf["t"], G[pre + "t"]) and leaf["best_sse"] == G[pre + "sse"]


def test_leaf_rule_is_not_vacuous_on_a_longer_search(leaf_lib):
    """The same pair at mse_threshold 0.004, ROUND with the adaptive width over the pipelined task loop with the memo (as on the GPU): about
    100 000 subcubes.  Equal to the exact run — and more than a quarter of all rows are terminal rows answered {T, T} although their
    lower bound was below T, i.e. rows only the new rule decides.  (Counted at the operator, against the threshold of the submission:
    26 378 of 105 112 rows, next to 52 921 with lb >= T; counted in the driver's consume, against the running threshold: 33 626 of 89 919.)"""
    exact = _run(leaf_lib, 0.004, 4, 0, False)
    leaf = _run(leaf_lib, 0.004, 4, 0, True)
    assert _same(exact, leaf)
    print(f"rows {leaf['rows']}, lb >= T {leaf['cut_lb']}, leaves with ub >= T > lb {leaf['cut_leaf']}, subcubes {leaf['stats']['trans_cubes']}")
    assert leaf["cut_leaf"] > leaf["rows"] / 4
