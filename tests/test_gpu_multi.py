"""GPU: the multi-GPU path inside the library (include/fgoicp_amd.h, fgoicp_rccl_* / fgoicp_multi_*) on the one GPU a test box has:
several ranks on device 0 over the in-process transport, the RCCL transport with one rank, record / replay, and the CLI's --gpus.
The exchange logic itself (uneven shards, ties between ranks, 8 ranks) is covered on CPU by tests/test_dist_gloo.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "goicp_golden.npz"))


def same(a, b, tol=1e-5):
    (Ra, ta, ea), (Rb, tb, eb) = a, b
    return abs(float(ea) - float(eb)) <= tol * float(eb) and np.allclose(Ra, Rb, atol=max(tol, 1e-5) * 10 if tol > 1e-5 else 1e-5) and \
        np.allclose(ta, tb, atol=(max(tol, 1e-5) * 10 if tol > 1e-5 else 1e-5) * max(1.0, float(np.abs(tb).max())))


@pytest.mark.parametrize("world,late", [(2, "0"), (3, "0"), (5, "0"), (2, "1"), (3, "1"), (5, "1")])
def test_ranks_on_one_gpu_reach_the_single_gpu_optimum(fg, gpu_required, monkeypatch, world, late):
    """late = "1" (FGOICP_LATE_ICP, a knob: measured slower on the 8-rank replay, off by default): a round's triggered ICP runs overlap the next round's bounds work on an ICP lane of
    their own and join the exchange one round late — the same optimum through another sequence of incumbents, so the final
    refinement (stops when an iteration improves the error by < 0.05 %, fgoicp.cpp:22-23) may end a hair elsewhere: compared at 2e-3."""
    monkeypatch.setenv("FGOICP_LATE_ICP", late)
    tgt, src, R_gt, t_gt = fg.synth.workload("small", angle_deg=150.0, min_angle_deg=110.0)
    mse = 2e-4  # ns * mse = 1.0: below the residual, the search has to certify
    one = fg.FastGoICP(tgt, src, 0.01, mse, schedule=fg.SCHEDULE_ROUND, round_width=0)
    R1, t1 = one.run()
    ref = (R1, t1, one.get_best_error())
    sub1 = one.stats()["trans_cubes"]
    one.close()
    m = fg.MultiGoICP(tgt, src, 0.01, mse, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS)
    m.set_record(True)
    R, t = m.run()
    assert same((R, t, m.get_best_error()), ref, 1e-5 if late == "0" else 2e-3)
    subs = [m.stats(r)["trans_cubes"] for r in range(world)]
    assert min(subs) > 0 and 0.5 * sub1 < sum(subs) < 2.5 * sub1  # every rank worked; the total stays in the single-GPU ballpark
    for r in range(world):
        assert m.get_best_error(r) == m.get_best_error(0)  # identical incumbents by construction
    # one rank alone against the recorded exchange: same share of the work, same end state
    secs = m.replay_rank(world - 1)
    assert secs > 0 and m.stats(world - 1)["trans_cubes"] == subs[world - 1]
    assert m.get_best_error(world - 1) == m.get_best_error(0)
    m.close()


@pytest.mark.parametrize("world", [2, 3, 5])
def test_cooperative_icp_returns_the_single_gpu_bits(fg, gpu_required, monkeypatch, world):
    """fgoicp_multi_icp: ONE ICP run executed by `world` ranks together (each scans 1/world of the source per pass, the per-query
    results are all-gathered on device memory, sums and SVD replicated) == fgoicp_icp on one context, bit for bit: sse, R, t and the
    iteration count — from a far start (many iterations), from the optimum (the loop ends at once) and with max_iter reached.  A
    cloud whose size is not a multiple of the ranks' 256-query blocks, and more ranks than the smallest share needs.
    FGOICP_COOP_SPLIT_MIN=0: by default the scans are not split (the loop runs replicated on every rank: measured no slower at 437k
    points on 8 ranks) — the last case checks that default against the same bits."""
    monkeypatch.setenv("FGOICP_COOP_SPLIT_MIN", "0")
    tgt, src, R_gt, t_gt = fg.synth.workload("small", angle_deg=25.0)
    src = src[:len(src) - 37]
    m = fg.MultiGoICP(tgt, src, 0.01, 1e-3, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS)
    reg = m.registration(0)
    rng = np.random.default_rng(3)
    starts = [(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 100), (fg.synth.random_rotation(rng, 12.0).astype(np.float32), rng.uniform(-0.05, 0.05, 3).astype(np.float32), 100),
              (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 3)]
    for R0, t0, mi in starts:
        icp = fg.IterativeClosestPoint3D(reg, None, None, mi, 0.005, R0, t0)
        e1, R1, t1 = icp.run()
        e, R, t, it = m.icp(R0, t0, mi, 0.005)
        assert np.float32(e).view(np.uint32) == np.float32(e1).view(np.uint32) and np.array_equal(R, R1) and np.array_equal(t, t1) and it == icp.iterations, (world, mi, e, e1)
    m.close()
    monkeypatch.delenv("FGOICP_COOP_SPLIT_MIN")
    m = fg.MultiGoICP(tgt, src, 0.01, 1e-3, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS)
    e, R, t, it = m.icp(*starts[1][:2], 100, 0.005)
    icp = fg.IterativeClosestPoint3D(m.registration(0), None, None, 100, 0.005, *starts[1][:2])
    e1, R1, t1 = icp.run()
    assert np.float32(e).view(np.uint32) == np.float32(e1).view(np.uint32) and np.array_equal(R, R1) and np.array_equal(t, t1) and it == icp.iterations
    m.close()


def test_cooperative_trimmed_icp_returns_the_single_gpu_bits(fg, gpu_required, monkeypatch):
    """The trimmed loop split the same way (brackets, cuts and the inlier selection over the whole cloud on every rank, the dual walk
    on the rank's share, skipped queries included): == the one-context trimmed ICP, bit for bit, with and without the skip lists."""
    monkeypatch.setenv("FGOICP_COOP_SPLIT_MIN", "0")
    tgt, src, R_gt, t_gt = fg.synth.workload("small", angle_deg=25.0, outlier_frac=0.2)
    for skip in ("1", "0"):
        monkeypatch.setenv("FGOICP_TRIM_SKIP", skip)
        m = fg.MultiGoICP(tgt, src, 0.01, 1e-3, devices=[0] * 3, transport=fg.TRANSPORT_IN_PROCESS, trim_fraction=0.2)
        reg = m.registration(0)
        rng = np.random.default_rng(4)
        for R0, t0, mi in ((np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 100), (fg.synth.random_rotation(rng, 10.0).astype(np.float32), rng.uniform(-0.05, 0.05, 3).astype(np.float32), 100),
                           (np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 2)):
            icp = fg.IterativeClosestPoint3D(reg, None, None, mi, 0.005, R0, t0)
            e1, R1, t1 = icp.run()
            e, R, t, it = m.icp(R0, t0, mi, 0.005)
            assert np.float32(e).view(np.uint32) == np.float32(e1).view(np.uint32) and np.array_equal(R, R1) and np.array_equal(t, t1) and it == icp.iterations, (skip, mi, e, e1, it, icp.iterations)
        m.close()


@pytest.mark.parametrize("max_iter", [0, 1])
def test_cooperative_icp_without_a_riding_pass_returns_the_single_gpu_bits(fg, gpu_required, max_iter):
    """The two shortest cooperative runs, scans split over three ranks (fgoicp_ctx_set_coop_split), untrimmed and trimmed: max_iter = 0, the
    loop's body never runs and nothing is enqueued behind the working cloud; max_iter = 1, pass 1 and one iteration whose scan has no
    pass of a next iteration riding along.  == fgoicp_icp on one context, bit for bit."""
    tgt, src, R_gt, t_gt = fg.synth.workload("tiny", angle_deg=25.0, outlier_frac=0.2)
    R0, t0 = fg.synth.random_rotation(np.random.default_rng(5), 12.0).astype(np.float32), np.array([0.01, -0.02, 0.005], np.float32)
    for trim in (0.0, 0.2):
        m = fg.MultiGoICP(tgt, src, 0.05, 1e-3, devices=[0] * 3, transport=fg.TRANSPORT_IN_PROCESS, trim_fraction=trim)
        for r in range(3):
            m.registration(r).set_coop_split(0, 0)
        m.set_record(True)
        icp = fg.IterativeClosestPoint3D(m.registration(0), None, None, max_iter, 0.005, R0, t0)
        e1, R1, t1 = icp.run()
        e, R, t, it = m.icp(R0, t0, max_iter, 0.005)
        assert it == icp.iterations == max_iter
        assert m.recorded(0)[1] == 2 * max_iter  # the scans were split: pass 1's correspondences and the iteration's minima were gathered
        assert np.float32(e).view(np.uint32) == np.float32(e1).view(np.uint32) and np.array_equal(R, R1) and np.array_equal(t, t1), (trim, e, e1)
        m.close()


@pytest.mark.parametrize("world", [2, 3])
def test_cooperative_rounds_are_the_single_gpu_run(fg, gpu_required, monkeypatch, world):
    """The multi-rank run with cooperative refinements (the default for clouds of at least 131072 source points when the exchange can
    all-gather device memory; forced here) against ONE GPU:
    bounds exchanged first, triggers on every rank in the single-GPU child order, each ICP run by all ranks together.  With a fixed
    round width and the tail-batch rule off (a task's batches then do not depend on which tasks share its rank) the N-rank run IS
    the one-GPU ROUND run: same (R, t, sse) bit for bit, same rounds, ICP runs and iterations, the rotation cubes split between
    the ranks.  FGOICP_COOP_ICP=0 (round 2's flow: a rank refines its own children alone) reaches the same optimum to 1e-5."""
    monkeypatch.setenv("FGOICP_TAIL_BATCH", "0")
    monkeypatch.setenv("FGOICP_COOP_ICP", "1")        # by default the flow is chosen by cloud size (cooperative from 131072 source points)
    monkeypatch.setenv("FGOICP_COOP_SPLIT_MIN", "0")  # and split the scans of every ICP over the ranks (default: replicated runs)
    tgt, src, R_gt, t_gt = fg.synth.workload("small", angle_deg=150.0, min_angle_deg=110.0)
    mse = 2e-4
    one = fg.FastGoICP(tgt, src, 0.01, mse, schedule=fg.SCHEDULE_ROUND, round_width=6)
    R1, t1 = one.run()
    e1, st1 = one.get_best_error(), one.stats()
    one.close()
    m = fg.MultiGoICP(tgt, src, 0.01, mse, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS, round_width=6)
    m.set_record(True)
    R, t = m.run()
    st = [m.stats(r) for r in range(world)]
    assert np.array_equal(R, R1) and np.array_equal(t, t1) and np.float32(m.get_best_error()).view(np.uint32) == np.float32(e1).view(np.uint32)
    for s in st:
        assert (s["rounds"], s["icp_runs"], s["icp_iters"]) == (st1["rounds"], st1["icp_runs"], st1["icp_iters"])
    assert sum(s["rot_cubes"] for s in st) == st1["rot_cubes"] and min(s["rot_cubes"] for s in st) > 0
    assert sum(s["trans_cubes"] for s in st) == st1["trans_cubes"]
    # one rank alone against the recording (bounds exchanges and device all-gathers): same share, same end state
    secs = m.replay_rank(world - 1)
    assert secs > 0 and m.stats(world - 1)["trans_cubes"] == st[world - 1]["trans_cubes"] and m.get_best_error(world - 1) == m.get_best_error(0)
    m.close()
    monkeypatch.setenv("FGOICP_COOP_ICP", "0")
    m = fg.MultiGoICP(tgt, src, 0.01, mse, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS, round_width=6)
    R, t = m.run()
    assert same((R, t, m.get_best_error()), (R1, t1, e1), 1e-5)
    m.close()


@pytest.mark.parametrize("world,split", [(2, "0"), (3, None), (5, "0")])
def test_sharded_serial_schedule_is_the_single_gpu_serial_run(fg, gpu_required, monkeypatch, world, split):
    """SERIAL — the reference's exact trajectory (fgoicp.cpp:32-100) — on N ranks: the inner BnBs of every speculative evaluation are
    dealt over the ranks, everything else is replicated (driver.hpp run_task_list_sharded).  EVERY rank must end with the one-GPU
    SERIAL run's counters (subcubes, operator calls, rotation cubes, inner BnBs, ICP runs and iterations, pops) and its (R, t, sse),
    bit for bit — with the refinements split over the ranks (FGOICP_COOP_ICP=1, FGOICP_COOP_SPLIT_MIN=0) or replicated (the default).
    Replaying one rank alone against the recording ends in the same state."""
    if split is not None:
        monkeypatch.setenv("FGOICP_COOP_ICP", "1")
        monkeypatch.setenv("FGOICP_COOP_SPLIT_MIN", split)
    tgt, src, R_gt, t_gt = fg.synth.workload("small", angle_deg=150.0, min_angle_deg=110.0)
    mse = 2e-4
    one = fg.FastGoICP(tgt, src, 0.01, mse, schedule=fg.SCHEDULE_SERIAL)
    R1, t1 = one.run()
    e1, st1 = one.get_best_error(), one.stats()
    one.close()
    keys = ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb", "rounds")
    m = fg.MultiGoICP(tgt, src, 0.01, mse, devices=[0] * world, transport=fg.TRANSPORT_IN_PROCESS, schedule=fg.SCHEDULE_SERIAL)
    m.set_record(True)
    R, t = m.run()
    assert np.array_equal(R, R1) and np.array_equal(t, t1) and np.float32(m.get_best_error()).view(np.uint32) == np.float32(e1).view(np.uint32)
    for r in range(world):
        st = m.stats(r)
        assert [st[k] for k in keys] == [st1[k] for k in keys], (r, st, st1)
    secs = m.replay_rank(world - 1)
    st = m.stats(world - 1)
    assert secs > 0 and [st[k] for k in keys] == [st1[k] for k in keys] and m.get_best_error(world - 1) == m.get_best_error(0)
    m.close()


def test_recorded_eight_rank_serial_run_replays_and_tears_down(fg, gpu_required):
    """The sequence of tools/scale_replay.py whose teardown aborted once in round 3 (`double free or corruption` after the
    8-rank SERIAL replay), as a test: create an 8-rank in-process fgoicp_multi, record a SERIAL run, replay EVERY rank alone against the
    recording (twice for rank 0), form and destroy a one-rank RCCL communicator next to it as the script does, destroy the object —
    and once more from the start (a teardown that corrupted the heap would take the second round or the process down).  The same
    sequence runs under AddressSanitizer on the CPU (tests/test_multi_asan.py)."""
    tgt, src, _, _ = fg.synth.workload("small", angle_deg=150.0, min_angle_deg=110.0)
    keys = ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb", "rounds")
    one = fg.FastGoICP(tgt, src, 0.01, 2e-4, schedule=fg.SCHEDULE_SERIAL)
    one.run()
    e1, st1 = one.get_best_error(), one.stats()
    one.close()
    for _ in range(2):
        m = fg.MultiGoICP(tgt, src, 0.01, 2e-4, devices=[0] * 8, transport=fg.TRANSPORT_IN_PROCESS, schedule=fg.SCHEDULE_SERIAL)
        m.set_record(True)
        m.run()
        assert np.float32(m.get_best_error()).view(np.uint32) == np.float32(e1).view(np.uint32)
        for r in list(range(8)) + [0]:
            assert m.replay_rank(r) > 0
            st = m.stats(r)
            assert [st[k] for k in keys] == [st1[k] for k in keys] and m.get_best_error(r) == m.get_best_error(0)
        ex = fg.RcclExchange(0, 1, fg.rccl_unique_id(), 0)
        assert ex.warmup()
        ex.close()
        m.close()


def test_a_failing_rank_ends_the_run_for_all_ranks(fg, gpu_required):
    """One rank's exchange fails mid-run (fgoicp_multi_test_fault, a test hook of the ABI): the others must not wait for it in
    their next collective; the call returns that rank's error and THE SAME OBJECT runs cleanly afterwards (the rendezvous is
    reset, stale generations and accumulators do not leak into the next run)."""
    tgt, src, _, _ = fg.synth.workload("small", angle_deg=150.0, min_angle_deg=110.0)
    m = fg.MultiGoICP(tgt, src, 0.01, 2e-4, devices=[0, 0, 0], transport=fg.TRANSPORT_IN_PROCESS)
    for rank, call in ((1, 3), (2, 0), (0, 5)):
        m.test_fault(rank, call)
        with pytest.raises(fg.FgoicpError, match=rf"rank {rank}: .*exchange callback failed"):
            m.run()
    m.run()  # the same object, after three aborted runs
    e = m.get_best_error()
    assert all(m.get_best_error(r) == e for r in range(3))
    m.close()
    one = fg.FastGoICP(tgt, src, 0.01, 2e-4, schedule=fg.SCHEDULE_ROUND, round_width=0)
    one.run()
    assert abs(one.get_best_error() - e) <= 1e-5 * e
    one.close()


def test_rccl_abort_fails_later_collectives(fg, gpu_required):
    ex = fg.RcclExchange(0, 1, fg.rccl_unique_id(), 0)
    assert ex.warmup()
    ex.abort(); ex.abort()  # idempotent
    buf = (C.c_float * 1)(1.0)
    assert ex.struct.allreduce_min(buf, 1, ex.struct.user) != 0
    assert b"aborted" in fg._lib.load().fgoicp_last_error()
    ex.close()


def test_rccl_nonblocking_communicator_settles_every_collective(fg, gpu_required):
    """fgoicp_multi_create forms its communicators with ncclConfig_t.blocking = 0, and on such a communicator every collective may
    return ncclInProgress (round 3 treated that as a failure).  The same kind of communicator with the one rank a test box
    can form: the three collectives of the exchange return the right data, also when they are made to report ncclInProgress first
    (fgoicp_rccl_test_inprogress, a test hook of the ABI) — the transport then polls ncclCommGetAsyncError before it enqueues the copy
    back — and a whole run goes through it."""
    import torch
    ex = fg.RcclExchange(0, 1, fg.rccl_unique_id(), 0, nonblocking=True)
    assert ex.comm_count == 1
    for forced in (0, 3):
        before = ex.test_inprogress(forced)
        buf = (C.c_float * 3)(3.0, -1.0, 2.5)
        assert ex.struct.allreduce_min(buf, 3, ex.struct.user) == 0 and list(buf) == [3.0, -1.0, 2.5]
        send = (C.c_float * 70)(*range(70))
        recv = (C.c_float * 70)()
        assert ex.struct.allgather(send, recv, 70, ex.struct.user) == 0 and list(recv) == list(map(float, range(70)))
        dev = torch.arange(4096, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert ex.struct.allgather_device(dev.data_ptr(), 4096, ex.struct.user) == 0
        assert torch.equal(dev.cpu(), torch.arange(4096, dtype=torch.uint8))
        if forced:
            assert ex.test_inprogress(0) >= before + forced  # the polling path ran once per forced collective
    s = fg.FastGoICP(G["runsyn_tgt"], G["runsyn_src"], float(G["runsyn_res"]), float(G["runsyn_mse"]), schedule=fg.SCHEDULE_ROUND, round_width=2)
    s.set_exchange(ex)
    ex.test_inprogress(1000)
    R, t = s.run()
    assert np.allclose(R, G["runsyn_R"], atol=1e-5)
    s.close()
    ex.close()


@pytest.mark.parametrize("torch_first", [True, False])
def test_process_exit_is_clean_with_torch_and_rccl_in_one_process(fg, gpu_required, torch_first):
    """The recorded heap abort of rounds 3 and 4 (`double free or corruption (!prev)` AFTER main() had returned): PyTorch-ROCm bundles its own
    librccl.so + librocm_smi64.so; the library used to dlopen the system's librccl.so.1 RTLD_GLOBAL next to them, two librocm_smi64 then
    destroyed the same C++ globals in the exit handlers (profiles/r04_exit_abort_rocm_smi.txt).  Now the transport uses the librccl the process
    already has, or loads the system one RTLD_LOCAL | RTLD_DEEPBIND: a child process that uses torch on the GPU AND the library's RCCL
    transport, in either order, must exit with status 0 and an empty heap-checker."""
    import subprocess
    import sys
    code = f"""
import sys
sys.path.insert(0, {REPO!r})
import fgoicp_amd as fg
def use_torch():
    import torch
    t = torch.arange(1024, device="cuda:0", dtype=torch.float32)
    assert float(t.sum()) == 523776.0
def use_rccl():
    ex = fg.RcclExchange(0, 1, fg.rccl_unique_id(), 0)
    assert ex.warmup()
    print("rccl:", fg._lib.load().fgoicp_rccl_library().decode())
    ex.close()
for f in ({'use_torch, use_rccl' if torch_first else 'use_rccl, use_torch'}):
    f()
print("done", flush=True)
"""
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-1500:])
    assert "done" in p.stdout and "double free" not in p.stderr and "corruption" not in p.stderr
    if torch_first:
        assert "already in the process" in p.stdout  # torch's own librccl was reused: one RCCL, one SMI library


def test_rccl_transport_with_one_rank(fg, gpu_required):
    """ncclCommInitRank + all-reduce(min) + all-gather on device buffers (world size 1 is all a one-GPU box can form)."""
    ident = fg.rccl_unique_id()
    assert len(ident) == 128
    ex = fg.RcclExchange(0, 1, ident, 0)
    buf = (C.c_float * 3)(3.0, -1.0, 2.5)
    assert ex.struct.allreduce_min(buf, 3, ex.struct.user) == 0 and list(buf) == [3.0, -1.0, 2.5]
    send = (C.c_float * 200)(*range(200))  # beyond the initial buffer: the transport re-allocates
    recv = (C.c_float * 200)()
    assert ex.struct.allgather(send, recv, 200, ex.struct.user) == 0 and list(recv) == list(map(float, range(200)))
    assert ex.calls == 2 and ex.warmup() and ex.calls == 4
    s = fg.FastGoICP(G["runsyn_tgt"], G["runsyn_src"], float(G["runsyn_res"]), float(G["runsyn_mse"]), schedule=fg.SCHEDULE_ROUND, round_width=2)
    s.set_exchange(ex)
    R, t = s.run()
    assert np.allclose(R, G["runsyn_R"], atol=1e-5)
    s.close()
    ex.close()
    m = fg.MultiGoICP(G["runsyn_tgt"], G["runsyn_src"], float(G["runsyn_res"]), float(G["runsyn_mse"]), devices=[0], transport=fg.TRANSPORT_RCCL, round_width=2)
    R2, t2 = m.run()
    assert np.allclose(R2, G["runsyn_R"], atol=1e-5)
    m.close()
    with pytest.raises(fg.FgoicpError):  # two ranks on one device cannot form an RCCL communicator: refused up front
        fg.MultiGoICP(G["runsyn_tgt"], G["runsyn_src"], float(G["runsyn_res"]), float(G["runsyn_mse"]), devices=[0, 0], transport=fg.TRANSPORT_RCCL)


def test_cli_gpus_flag(fg, gpu_required, tmp_path):
    from tests.test_gpu_cli_dist import write_txt
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    write_txt(tmp_path / "tgt.txt", G["runsyn_tgt"])
    write_txt(tmp_path / "src.txt", G["runsyn_src"][:250])
    out = {}
    for name, extra, env in (("one", [], {}), ("two", ["--gpus", "2"], {"FGOICP_MULTI_DEVICES": "0,0", "FGOICP_LATE_ICP": "0"})):
        cfg = tmp_path / f"{name}.toml"
        cfg.write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{name}_out.toml"\n'
                       f'[params]\nsource_subsample = 1.0\nschedule = "round"\nround_width = 4\nlut_resolution = {float(G["runsyn_res"])}\nmse_threshold = {float(G["runsyn_mse"])}\nseed = 3\n')
        p = subprocess.run([exe, "-c", str(cfg), *extra], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        if extra:
            assert "Sharding the search over 2 GPUs" in p.stdout
        txt = (tmp_path / f"{name}_out.toml").read_text()
        out[name] = float(re.search(r"^sse = (.*)$", txt, re.M).group(1))
    assert out["two"] == pytest.approx(out["one"], rel=1e-5)
    # the default schedule ("serial": the reference's order) with --gpus 2: the one-GPU record, counter for counter
    rec = {}
    for name, extra, env in (("s_one", [], {}), ("s_two", ["--gpus", "2"], {"FGOICP_MULTI_DEVICES": "0,0"})):
        cfg = tmp_path / f"{name}.toml"
        cfg.write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{name}_out.toml"\n'
                       f'[params]\nsource_subsample = 1.0\nlut_resolution = {float(G["runsyn_res"])}\nmse_threshold = {float(G["runsyn_mse"])}\nseed = 3\n')
        p = subprocess.run([exe, "-c", str(cfg), *extra], capture_output=True, text=True, timeout=300, env={**os.environ, **env})
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        if extra:
            assert "the reference's order, evaluations sharded" in p.stdout
        txt = (tmp_path / f"{name}_out.toml").read_text()
        rec[name] = re.sub(r"^seconds = .*$", "", txt, flags=re.M)  # R, t, sse, mse, subcubes, rotation cubes, ICP runs and iterations, pops
    assert rec["s_two"] == rec["s_one"]
