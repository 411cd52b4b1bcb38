"""CPU: fgoicp_batch without a GPU — the scheduler of csrc/host/batch.hpp (window, rendezvous, launcher, one driver thread per pair)
over the oracle's operators with the grouping of requests into launches varied at random: every pair must end with the incumbent
bits and counters of its own solo driver run, under both schedules; and the refusals of fgoicp_batch_create, which needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")
SRC = os.path.join(HERE, "batch_sched.cpp")
ORACLE = os.path.join(HERE, "..", "..", "oracle", "goicp_oracle.cpp")
DEPS = [SRC, os.path.join(HERE, "oracle_ops.hpp"), ORACLE, os.path.join(HERE, "..", "..", "fast-go-icp_amd", "csrc", "host", "batch.hpp"),
        os.path.join(HERE, "..", "..", "fast-go-icp_amd", "csrc", "host", "driver.hpp")]


def _build(exe, flags):
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in DEPS):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"  # built aside and renamed: an interrupted build never leaves a newer, broken binary behind
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-fopenmp", "-pthread", "-o", tmp, SRC, ORACLE], check=True, cwd=HERE)
    os.replace(tmp, exe)
    return exe


def _run(exe, args, env=None):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="2", **(env or {})))
    assert p.returncode == 0, p.stderr[-4000:]
    assert "all runs matched" in p.stderr
    return p.stderr


def test_scheduler_gives_every_pair_its_solo_run_under_random_grouping():
    exe = _build(os.path.join(HERE, "batch_sched"), ["-O2"])
    err = _run(exe, ["3", "3", "1"])
    assert "SERIAL: 3 pairs x 3 runs checked" in err and "ROUND: 3 pairs x 3 runs checked" in err


def _opts(fg, **kw):
    o = fg._lib.BatchOpts(C.sizeof(fg._lib.BatchOpts), fg._lib.SolverOpts(0, 1, 0, 0, 0.0), 0)
    for k, v in kw.items():
        if k == "trim_fraction":
            o.solver.trim_fraction = v
        else:
            setattr(o, k, v)
    return o


def _create(fg, pairs, opts, n=None):
    arr = (fg._lib.BatchPair * max(1, len(pairs)))(*pairs)
    h = C.c_void_p()
    rc = fg._lib.load().fgoicp_batch_create(arr, len(pairs) if n is None else n, C.byref(opts) if opts is not None else None, C.byref(h))
    if h.value:
        fg._lib.load().fgoicp_batch_destroy(h)
    return rc


def test_create_refusals(fg):
    pts = np.random.default_rng(0).uniform(-1, 1, (64, 3)).astype(np.float32)
    fp = pts.ctypes.data_as(C.POINTER(C.c_float))
    good = fg._lib.BatchPair(fp, 64, fp, 64, 0.05, 1e-3)
    assert _create(fg, [good, good], _opts(fg)) == 0  # host pre-processing only: no device needed
    assert _create(fg, [good], _opts(fg, trim_fraction=0.1)) == 1
    assert _create(fg, [good], _opts(fg), n=0) == 1
    assert _create(fg, [good], _opts(fg), n=-3) == 1
    assert _create(fg, [fg._lib.BatchPair(None, 64, fp, 64, 0.05, 1e-3)], _opts(fg)) == 1
    assert _create(fg, [fg._lib.BatchPair(fp, 64, None, 64, 0.05, 1e-3)], _opts(fg)) == 1
    assert _create(fg, [fg._lib.BatchPair(fp, 0, fp, 64, 0.05, 1e-3)], _opts(fg)) == 1
    assert _create(fg, [good], _opts(fg, struct_size=8)) == 1
    assert _create(fg, [good], None) == 1
    with pytest.raises(fg.FgoicpError):
        fg.FastGoICPBatch([])
