"""CPU: the batch scheduler (csrc/host/batch.hpp: window, rendezvous, launcher, driver threads woken by the launcher) under
ThreadSanitizer — tests/host_harness/batch_sched.cpp over the oracle's operators, requests grouped at random, every window size.
The oracle's own OpenMP loops run on one thread (OMP_NUM_THREADS=1): libgomp is not instrumented, the scheduler's threads are."""
import os
import subprocess

from tests.test_batch_host import HERE, _build


def test_batch_scheduler_is_clean_under_thread_sanitizer():
    exe = _build(os.path.join(HERE, "batch_sched_tsan"), ["-O1", "-g", "-fsanitize=thread"])
    env = dict(os.environ, OMP_NUM_THREADS="1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    p = subprocess.run([exe, "3", "3", "5", "0.05"], capture_output=True, text=True, timeout=1200, env=env)
    assert "ThreadSanitizer" not in p.stderr, p.stderr[-6000:]
    assert p.returncode == 0, p.stderr[-4000:]
    assert "all runs matched" in p.stderr
