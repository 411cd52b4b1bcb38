"""The alignment report (fgoicp_alignment, fgoicp_solver_alignment, fgoicp_batch_alignment) as far as it goes without a GPU: the
ctypes table against the header, the refusals of the three calls (status 1 with a message, no device touched), the batch options'
struct_size guard with the appended member, the CLI's io.alignment key and the file it writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "host_harness")
INVALID_ARG = 1


def _pairs(fg, n=2):
    pts = np.random.default_rng(3).uniform(-1, 1, (32, 3)).astype(np.float32)
    arr = (fg._lib.BatchPair * n)()
    for i in range(n):
        arr[i] = fg._lib.BatchPair(pts.ctypes.data_as(fg._lib.c_float_p), 32, pts.ctypes.data_as(fg._lib.c_float_p), 32, 0.1, 1e-3)
    return pts, arr


def _msg(lib):
    return lib.fgoicp_last_error().decode()


def test_ctypes_table_covers_the_alignment_calls_and_the_summary_layout(fg):
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fgoicp_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fgoicp_[a-z_0-9]+)\s*\(", txt)))
    for name in ("fgoicp_alignment", "fgoicp_solver_alignment", "fgoicp_batch_alignment"):
        assert name in declared and name in fg._lib.exported_symbols()
    assert sorted(fg._lib.exported_symbols()) == declared
    S = fg._lib.AlignmentSummary
    # uint32 struct_size, three uint64, three floats (include/fgoicp_amd.h)
    assert (S.struct_size.offset, S.points.offset, S.inliers.offset, S.targets_hit.offset) == (0, 8, 16, 24)
    assert (S.sse.offset, S.max_inlier_dist2.offset, S.scaling_factor.offset) == (32, 36, 40) and C.sizeof(S) == 48
    assert S().struct_size == 48
    assert fg._lib.load().fgoicp_abi_version() == 2


def test_alignment_calls_refuse_null_handles_with_a_message(fg):
    lib = fg._lib.load()
    sm = fg._lib.AlignmentSummary()
    R = np.eye(3, dtype=np.float32).reshape(9)
    t = np.zeros(3, np.float32)
    fp = fg._lib.c_float_p
    assert lib.fgoicp_alignment(None, R.ctypes.data_as(fp), t.ctypes.data_as(fp), None, None, None, None, C.byref(sm)) == INVALID_ARG
    assert "fgoicp_alignment" in _msg(lib)
    assert lib.fgoicp_solver_alignment(None, None, None, None, None, C.byref(sm)) == INVALID_ARG
    assert "fgoicp_solver_alignment" in _msg(lib)
    assert lib.fgoicp_batch_alignment(None, 0, None, None, None, None, C.byref(sm)) == INVALID_ARG
    assert "fgoicp_batch_alignment" in _msg(lib)
    assert (sm.points, sm.inliers, sm.targets_hit, sm.sse) == (0, 0, 0, 0.0)  # nothing written on refusal


def test_batch_alignment_refuses_option_off_and_not_yet_run(fg):
    """fgoicp_batch_create makes no device state, so these run anywhere: the option off, the option on before run(), a pair index out of
    range — FGOICP_ERR_INVALID_ARG each, the reason in fgoicp_last_error."""
    lib = fg._lib.load()
    L = fg._lib
    pts, arr = _pairs(fg)
    sm = L.AlignmentSummary()
    for on in (0, 1):
        o = L.BatchOpts(C.sizeof(L.BatchOpts), L.SolverOpts(0, 1, 0, 0, 0.0), 0, None, on)
        h = C.c_void_p()
        assert lib.fgoicp_batch_create(arr, 2, C.byref(o), C.byref(h)) == 0 and h.value
        assert lib.fgoicp_batch_alignment(h, 0, None, None, None, None, C.byref(sm)) == INVALID_ARG
        assert ("alignment = 0" in _msg(lib)) if not on else ("has not run" in _msg(lib)), _msg(lib)
        assert lib.fgoicp_batch_alignment(h, 7, None, None, None, None, None) == INVALID_ARG
        lib.fgoicp_batch_destroy(h)
    # the Python wrapper raises the same refusal
    b = fg.FastGoICPBatch([(pts, pts)], lut_resolution=0.1, alignment=True)
    with pytest.raises(fg.FgoicpError) as e:
        b.alignment(0)
    assert e.value.status == INVALID_ARG and "has not run" in str(e.value)
    b.close()
    b = fg.FastGoICPBatch([(pts, pts)], lut_resolution=0.1)
    with pytest.raises(fg.FgoicpError) as e:
        b.alignment(0)
    assert e.value.status == INVALID_ARG and "alignment = 0" in str(e.value)
    b.close()


def test_batch_create_accepts_the_shorter_options_struct(fg):
    """a caller built before `alignment` was appended hands over 40 bytes: accepted, and the member it does not know reads as 0 (the
    garbage behind its struct is not read as the option)"""
    lib = fg._lib.load()
    L = fg._lib
    _, arr = _pairs(fg)
    end = L.BatchOpts.alignment.offset
    assert end == 40 and C.sizeof(L.BatchOpts) == 48
    o = L.BatchOpts(end, L.SolverOpts(0, 1, 0, 0, 0.0), 0, None, 0x5A5A5A5A)  # what lies behind an old caller's struct
    h = C.c_void_p()
    assert lib.fgoicp_batch_create(arr, 2, C.byref(o), C.byref(h)) == 0 and h.value
    assert lib.fgoicp_batch_alignment(h, 0, None, None, None, None, None) == INVALID_ARG
    assert "alignment = 0" in _msg(lib), _msg(lib)
    lib.fgoicp_batch_destroy(h)


class AlignConfigOut(C.Structure):
    _fields_ = [(k, C.c_char * 512) for k in ("target", "source", "output", "visualization", "alignment")]


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HERE, "libalign_harness.so")
    src = os.path.join(HERE, "align_harness.cpp")
    deps = [src, os.path.join(REPO, "fast-go-icp_amd/csrc/cli/config.hpp"), os.path.join(REPO, "include/fgoicp/common.hpp"), os.path.join(REPO, "include/fgoicp_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.align_parse_config.argtypes = [C.c_char_p, C.POINTER(AlignConfigOut)]
    L.align_write.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_ulonglong,
                              C.c_ulonglong, C.c_float, C.c_float, C.c_float]
    return L


def test_cli_parser_reads_io_alignment_and_leaves_other_configs_alone(harness, tmp_path):
    base = '[io]\ntarget = "t.txt"\nsource = "s.txt"\noutput = "out.toml"\nvisualization = "viz.ply"\n{extra}[params]\nlut_resolution = 0.01\n'
    out = AlignConfigOut()
    (tmp_path / "a.toml").write_text(base.format(extra='alignment = "pairs/align.txt"   # the report\n'))
    assert harness.align_parse_config(str(tmp_path / "a.toml").encode(), C.byref(out)) == 0
    assert out.alignment == b"pairs/align.txt"
    assert (out.target, out.source, out.output, out.visualization) == (b"t.txt", b"s.txt", b"out.toml", b"viz.ply")
    out2 = AlignConfigOut()
    (tmp_path / "b.toml").write_text(base.format(extra=""))
    assert harness.align_parse_config(str(tmp_path / "b.toml").encode(), C.byref(out2)) == 0
    assert out2.alignment == b""
    assert (out2.target, out2.source, out2.output, out2.visualization) == (b"t.txt", b"s.txt", b"out.toml", b"viz.ply")


def test_alignment_file_has_the_documented_lines(harness, tmp_path):
    """two '#' lines (summary, column names), then per source point: x y z as loaded, target index, distance in the files' units
    (sqrt(dist2) / scaling_factor), inlier flag"""
    src = np.array([[0.5, -1.25, 3.0], [1e-3, 2.0, -7.5], [10.0, 20.0, 30.0]], np.float32)
    idx = np.array([7, 0, 123456], np.uint32)
    d2 = np.array([4.0, 0.0, 2.25], np.float32)
    inl = np.array([1, 1, 0], np.uint8)
    path = tmp_path / "align.txt"
    fp = C.POINTER(C.c_float)
    assert harness.align_write(str(path).encode(), src.ctypes.data_as(fp), 3, idx.ctypes.data_as(C.POINTER(C.c_uint32)), d2.ctypes.data_as(fp),
                               inl.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2, 4.0, 4.0, 0.5) == 0
    lines = path.read_text().splitlines()
    assert len(lines) == 5
    assert lines[0] == ("# alignment: points = 3, inliers = 2, targets_hit = 2, sse = 4, max_inlier_dist2 = 4, scaling_factor = 0.5, "
                        "fitness = 0.666666667, inlier_rmse = 2.82842712")
    assert lines[1] == "# x y z target_index distance inlier"
    assert lines[2] == "0.5 -1.25 3 7 4 1"  # sqrt(4) / 0.5
    assert lines[3] == "0.00100000005 2 -7.5 0 0 1"  # 9 significant digits: the float as loaded
    assert lines[4] == "10 20 30 123456 3 0"
    rows = np.loadtxt(path)  # '#' lines are comments to every reader of such files
    assert rows.shape == (3, 6) and np.array_equal(rows[:, :3].astype(np.float32), src)
    assert harness.align_write(str(tmp_path / "no" / "such" / "dir.txt").encode(), src.ctypes.data_as(fp), 3, idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                               d2.ctypes.data_as(fp), inl.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 2, 4.0, 4.0, 0.5) == 1


def test_alignment_facade_compiles_against_the_c_abi_alone(fg, tmp_path):
    """icp::Registration::alignment / icp::FastGoICP::alignment (include/fgoicp/*.hpp) build with a plain C++17 compiler; without a GPU
    the solver's constructor throws before anything is computed."""
    fg.build.build()
    exe = str(tmp_path / "facade_alignment_check")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(HERE, "facade_alignment_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    import torch
    if torch.cuda.is_available():
        return  # the run itself: tests/test_gpu_alignment.py
    (tmp_path / "pc.txt").write_text("2\n0 0 0\n1 1 1\n")
    p = subprocess.run([exe, str(tmp_path / "pc.txt"), str(tmp_path / "pc.txt"), "0.05", "0"], capture_output=True, text=True)
    assert p.returncode != 0 and "no HIP device" in (p.stderr + p.stdout)
