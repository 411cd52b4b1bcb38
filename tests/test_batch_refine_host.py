"""CPU: refinement inside a batch without a GPU — what fgoicp_batch_create refuses of fgoicp_batch_opts_refine.refine (each refusal names its pair),
the getters' refusals, the Python refine= mapping, the REFINING state of the scheduler (csrc/host/batch.hpp) over a fake backend with the
launcher's random grouping on, and the hoisted information-pose helper against the expression it replaced."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_harness")
REPO = os.path.join(HERE, "..", "..")
HOST = os.path.join(REPO, "fast-go-icp_amd", "csrc", "host")
ORACLE = os.path.join(REPO, "oracle", "goicp_oracle.cpp")


def _build(exe, srcs, deps, flags):
    deps = [*srcs, *deps]
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in deps):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"  # built aside and renamed: an interrupted build never leaves a newer, broken binary behind
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-o", tmp, *srcs], check=True, cwd=HERE)
    os.replace(tmp, exe)
    return exe


def test_scheduler_keeps_refining_pairs_live_until_their_last_step():
    src = os.path.join(HERE, "batch_refine_sched.cpp")
    exe = _build(os.path.join(HERE, "batch_refine_sched"), [src, ORACLE],
                 [os.path.join(HERE, "oracle_ops.hpp"), os.path.join(HOST, "batch.hpp"), os.path.join(HOST, "driver.hpp")], ["-O2", "-fopenmp", "-pthread"])
    p = subprocess.run([exe, "6", "4", "1"], capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert p.returncode == 0, p.stderr[-4000:]
    assert "6 pairs x 4 runs checked" in p.stderr and "all runs matched" in p.stderr


def test_information_pose_helper_has_the_bits_of_the_expression_it_replaced():
    src = os.path.join(HERE, "refined_pose_check.cpp")
    exe = _build(os.path.join(HERE, "refined_pose_check"), [src], [os.path.join(HOST, "refined_pose.hpp"), os.path.join(REPO, "include", "fgoicp_amd.h")], ["-O2"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "96 cases matched" in p.stderr


def _pair(fg, n=64):
    pts = np.random.default_rng(0).uniform(-1, 1, (n, 3)).astype(np.float32)
    fp = pts.ctypes.data_as(C.POINTER(C.c_float))
    return pts, fg._lib.BatchPair(fp, n, fp, n, 0.05, 1e-3)


def _entry(fg, **kw):
    e = dict(struct_size=C.sizeof(fg._lib.BatchRefine), model=fg._lib.MODEL_PLANE, k=16, max_iter=30, conv_thr=1e-6, max_distance=math.inf, epsilon=1e-3,
             loss=fg._lib.LOSS_NONE, loss_scale=0.0)
    e.update(kw)
    r = fg._lib.BatchRefine()
    for k, v in e.items():
        setattr(r, k, v)
    return r


def _create(fg, pairs, entries, struct_size=None):
    """-> (status, message, handle or None)"""
    lib = fg._lib.load()
    arr = (fg._lib.BatchPair * len(pairs))(*pairs)
    o = fg._lib.BatchOptsRefine(C.sizeof(fg._lib.BatchOptsRefine) if struct_size is None else struct_size, fg._lib.SolverOpts(0, 1, 0, 0, 0.0), 0)
    rarr = (fg._lib.BatchRefine * len(entries))(*entries)
    o.refine = rarr
    h = C.c_void_p()
    rc = lib.fgoicp_batch_create(arr, len(pairs), C.byref(o), C.byref(h))
    return rc, lib.fgoicp_last_error().decode(), (h if h.value else None)


BAD_ENTRIES = [
    (dict(k=3), "k must lie in [4, 32]"),
    (dict(k=33), "k must lie in [4, 32]"),
    (dict(max_distance=-1.0), "max_distance must be >= 0"),
    (dict(max_distance=math.nan), "max_distance must be >= 0"),
    (dict(model=2), "unknown model 2"),
    (dict(model=-2), "unknown model -2"),
    (dict(loss=5), "unknown loss 5"),
    (dict(loss=-1), "unknown loss -1"),
    (dict(model=1, epsilon=0.0), "epsilon must be finite and lie in (0, 1]"),
    (dict(model=1, epsilon=1.5), "epsilon must be finite and lie in (0, 1]"),
    (dict(model=1, epsilon=math.nan), "epsilon must be finite and lie in (0, 1]"),
    (dict(loss=1, loss_scale=math.inf), "loss_scale must be finite"),
    (dict(loss=4, loss_scale=math.nan), "loss_scale must be finite"),
    (dict(struct_size=0), "struct_size"),
]


@pytest.mark.parametrize("bad,text", BAD_ENTRIES, ids=[f"{sorted(b.items())}" for b, _ in BAD_ENTRIES])
def test_create_refuses_a_bad_refine_entry_and_names_the_pair(fg, bad, text):
    pts, good = _pair(fg)
    for at in (0, 2):
        entries = [_entry(fg), _entry(fg, model=-1), _entry(fg, model=fg._lib.MODEL_GICP, loss=fg._lib.LOSS_TUKEY)]
        entries[at] = _entry(fg, **bad)
        rc, msg, h = _create(fg, [good] * 3, entries)
        assert rc == 1 and h is None, (rc, msg)
        assert text in msg and f"pair {at}" in msg and msg.startswith("fgoicp_batch_create"), msg


def test_create_takes_good_entries_and_a_short_struct_means_no_refinement(fg):
    lib = fg._lib.load()
    pts, good = _pair(fg)
    entries = [_entry(fg), _entry(fg, model=-1), _entry(fg, model=1, loss=4, loss_scale=-3.0, epsilon=1.0, k=4), _entry(fg, k=32, max_distance=0.0, max_iter=0)]
    rc, msg, h = _create(fg, [good] * 4, entries)
    assert rc == 0 and h is not None, msg
    out = fg._lib.PlaneResult()
    rob = fg._lib.RobustResult()
    # before a run; the wrong kind; a pair without an entry; an index out of range
    assert lib.fgoicp_batch_refined_plane(h, 0, C.byref(out)) == 1 and "has not run yet" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_robust(h, 2, C.byref(rob)) == 1 and "has not run yet" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_robust(h, 0, C.byref(rob)) == 1 and "fgoicp_batch_refined_plane serves it" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_plane(h, 2, C.byref(out)) == 1 and "fgoicp_batch_refined_robust serves it" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_plane(h, 1, C.byref(out)) == 1 and "pair 1 has no refinement" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_plane(h, 4, C.byref(out)) == 1 and "out of range" in lib.fgoicp_last_error().decode()
    assert lib.fgoicp_batch_refined_plane(h, 0, None) == 1
    inf = fg._lib.Information()
    assert lib.fgoicp_batch_refined_information(h, 0, C.byref(inf)) == 1 and "information = 0" in lib.fgoicp_last_error().decode()
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert lib.fgoicp_batch_refine_launches(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    lib.fgoicp_batch_destroy(h)
    # a struct_size that ends before the member: the entries are not read (a bad one is not refused), no pair has a refinement
    rc, msg, h = _create(fg, [good], [_entry(fg, k=99)], struct_size=C.sizeof(fg._lib.BatchOptsInformation))
    assert rc == 0 and h is not None, msg
    assert lib.fgoicp_batch_refined_plane(h, 0, C.byref(out)) == 1 and "pair 0 has no refinement" in lib.fgoicp_last_error().decode()
    lib.fgoicp_batch_destroy(h)
    assert C.sizeof(fg._lib.BatchOptsRefine) == C.sizeof(fg._lib.BatchOptsInformation) + C.sizeof(C.c_void_p)


def test_ctypes_layouts_match_the_header_and_the_published_options_keep_their_size(fg, tmp_path):
    """the layouts as a C compiler sees the header: fgoicp_batch_opts keeps the 56 bytes it was published with, the refine table lies right
    behind it in fgoicp_batch_opts_refine, and the ctypes mirrors have the same offsets"""
    R, B = fg._lib.BatchRefine, fg._lib.BatchOptsRefine
    names = [n for n, _ in R._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fgoicp_amd.h"\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", offsetof(fgoicp_batch_refine_t, {n}));\n' for n in names)
                   + '  printf("refine_t.sizeof %zu\\n", sizeof(fgoicp_batch_refine_t));\n'
                   '  printf("opts.sizeof %zu\\n", sizeof(fgoicp_batch_opts));\n'
                   '  printf("opts_refine.opts %zu\\n", offsetof(fgoicp_batch_opts_refine, opts));\n'
                   '  printf("opts_refine.refine %zu\\n", offsetof(fgoicp_batch_opts_refine, refine));\n'
                   '  printf("opts_refine.sizeof %zu\\n", sizeof(fgoicp_batch_opts_refine));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], check=True)  # the header is C
    c = {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())}
    for n in names:
        assert c[n] == getattr(R, n).offset, n
    assert c["refine_t.sizeof"] == C.sizeof(R)
    assert c["opts.sizeof"] == C.sizeof(fg._lib.BatchOptsInformation) == 56
    assert c["opts_refine.opts"] == 0 and c["opts_refine.refine"] == B.refine.offset == 56
    assert c["opts_refine.sizeof"] == C.sizeof(B) == 64


def test_python_refine_mapping(fg):
    pts = np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(np.float32)
    pairs = [(pts, pts)] * 3
    lib = fg._lib.load()
    # one dict serves every pair; the defaults are refine_plane's
    b = fg.FastGoICPBatch(pairs, refine={"model": "gicp", "loss": "huber"})
    assert [r["model"] for r in b._refine] == ["gicp"] * 3 and b._refine[0]["k"] == 16 and b._refine[0]["max_iter"] == 30 and b._refine[0]["conv_thr"] == 1e-6
    assert b._refine[0]["max_distance"] is None and b._refine[0]["epsilon"] == 1e-3 and b._refine[0]["loss_scale"] is None
    with pytest.raises(fg.FgoicpError, match="has not run yet"):
        b.refined(0)
    assert b.refine_launches() == (0, 0)
    b.close()
    # a list with None entries: those pairs have no refinement, and loss None / "none" is the plain kind
    b = fg.FastGoICPBatch(pairs, refine=[None, {"loss": "none", "max_distance": 0.5}, {"model": "plane", "loss": "tukey", "loss_scale": 0.1, "k": 8}])
    with pytest.raises(fg.FgoicpError, match="pair 0 has no refinement"):
        b.refined(0)
    with pytest.raises(fg.FgoicpError, match="has not run yet"):
        b.refined(1)
    rob = fg._lib.RobustResult()
    assert lib.fgoicp_batch_refined_robust(b._h, 1, C.byref(rob)) == 1 and "serves it" in lib.fgoicp_last_error().decode()
    with pytest.raises(fg.FgoicpError, match="has not run yet"):
        b.refined(2)
    b.close()
    arr = fg.batch._refine_array(fg.batch._refine_entries([None, {"model": "gicp", "loss": "cauchy", "loss_scale": 2.0, "max_distance": 0.25, "epsilon": 0.5, "k": 5, "max_iter": 7}], 2))
    assert arr[0].model == -1 and arr[0].struct_size == C.sizeof(fg._lib.BatchRefine)
    assert (arr[1].model, arr[1].k, arr[1].max_iter, arr[1].loss, arr[1].loss_scale, arr[1].max_distance, arr[1].epsilon) == (1, 5, 7, fg._lib.LOSS_CAUCHY, 2.0, 0.25, 0.5)
    # without refine= nothing is passed
    b = fg.FastGoICPBatch(pairs)
    with pytest.raises(fg.FgoicpError, match="pair 0 has no refinement"):
        b.refined(0)
    b.close()
    with pytest.raises(ValueError, match="2 entries for 3 pairs"):
        fg.FastGoICPBatch(pairs, refine=[None, None])
    with pytest.raises(ValueError, match="unknown keys"):
        fg.FastGoICPBatch(pairs, refine={"modle": "plane"})
    with pytest.raises(fg.FgoicpError, match=r"pair 1\).*k must lie in \[4, 32\]"):
        fg.FastGoICPBatch(pairs, refine=[None, {"k": 2}, None])
