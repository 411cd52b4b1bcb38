"""The information matrix (fgoicp_information, fgoicp_solver_information, fgoicp_batch_information, fgoicp_information_from_moments) as
far as it goes without a GPU: the host half against numpy, the ctypes table and the struct layout against the header, the struct_size
guard, the refusals (status 1 with a message, no device touched), the batch options with the appended members, the CLI's keys and the
file it writes, the C++ facade.  (The refusal for a FAILED pair needs a batch that ran: tests/test_gpu_information.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "host_harness")
INVALID_ARG = 1
EPS = 2.0 ** -52


def _msg(lib):
    return lib.fgoicp_last_error().decode()


def direct_information(q):
    """sum G_i^T G_i with G_i = [-[q_i]x | I3], in float64"""
    q = np.asarray(q, np.float64)
    info = np.zeros((6, 6))
    for x, y, z in q:
        G = np.array([[0.0, z, -y, 1, 0, 0], [-z, 0.0, x, 0, 1, 0], [y, -x, 0.0, 0, 0, 1]])
        info += G.T @ G
    return info


def moments(q):
    q = np.asarray(q, np.float64)
    return q.sum(0), np.array([(q[:, a] * q[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])


# ---- 1. the host half against numpy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300, 517])
def test_from_moments_matches_the_direct_sum(fg, n):
    """tolerance per entry: 8 N 2^-52 sum |q|^2 in the callers' frame — the fp64 operations on the path times the unit round-off"""
    rng = np.random.default_rng(40 + n)
    q = (rng.normal(size=(n, 3)) * [1.0, 3.0, 0.5] + [2.0, -1.0, 0.25]).astype(np.float32)
    want = direct_information(q)
    tol = 8 * n * EPS * float((q.astype(np.float64) ** 2).sum())
    sq, sqq = moments(q)
    info, q_out, qq_out = fg.information_from_moments(n, sq, sqq)
    assert np.array_equal(q_out, sq) and np.array_equal(qq_out, sqq)  # no change of frame: the moments as given
    print(f"n {n}: largest deviation {np.abs(info - want).max():.3g}, tolerance {tol:.3g}")
    assert np.abs(info - want).max() <= tol
    assert np.array_equal(info, info.T) and np.all(np.diag(info)[3:] == n)
    # with (offset, scale): the context's frame is q_s = (q - c) * s
    c = np.array([1.75, -0.5, 0.125], np.float32)
    s = np.float32(0.37)
    qs = (q.astype(np.float64) - c.astype(np.float64)) * np.float64(s)
    sq_s, sqq_s = moments(qs)
    info2, q2, qq2 = fg.information_from_moments(n, sq_s, sqq_s, offset=c, scale=s)
    print(f"n {n} (offset, scale): largest deviation {np.abs(info2 - want).max():.3g}, tolerance {tol:.3g}")
    assert np.abs(info2 - want).max() <= tol
    assert np.abs(q2 - sq).max() <= tol and np.abs(qq2 - sqq).max() <= tol


def test_from_moments_of_nothing_is_the_zero_matrix_and_bad_arguments_are_refused(fg):
    lib = fg._lib.load()
    info, q, qq = fg.information_from_moments(0, np.zeros(3), np.zeros(6), offset=np.array([1, 2, 3], np.float32), scale=0.5)
    assert not info.any() and not np.signbit(info).any() and not q.any() and not qq.any()
    info, _, _ = fg.information_from_moments(0, np.zeros(3), np.zeros(6))
    assert not info.any() and not np.signbit(info).any()
    z3, z6, out = (C.c_double * 3)(), (C.c_double * 6)(), (C.c_double * 36)()
    assert lib.fgoicp_information_from_moments(1, None, z6, None, 1.0, out, None, None) == INVALID_ARG
    assert "fgoicp_information_from_moments" in _msg(lib)
    assert lib.fgoicp_information_from_moments(1, z3, None, None, 1.0, out, None, None) == INVALID_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.fgoicp_information_from_moments(1, z3, z6, None, bad, out, None, None) == INVALID_ARG, bad
    assert lib.fgoicp_information_from_moments(1, z3, z6, None, 1.0, None, None, None) == 0  # every output is optional
    # one point at (1, 2, 3), worked by hand
    info, _, _ = fg.information_from_moments(1, [1, 2, 3], [1, 2, 3, 4, 6, 9])
    assert np.array_equal(info, [[13, -2, -3, 0, -3, 2], [-2, 10, -6, 3, 0, -1], [-3, -6, 5, -2, 1, 0], [0, 3, -2, 1, 0, 0], [-3, 0, 1, 0, 1, 0], [2, -1, 0, 0, 0, 1]])


# ---- 2. table and struct ------------------------------------------------------------------------------------------------------------
def test_ctypes_table_and_struct_layouts_match_the_header(fg, tmp_path):
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fgoicp_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fgoicp_[a-z_0-9]+)\s*\(", txt)))
    for name in ("fgoicp_information", "fgoicp_solver_information", "fgoicp_batch_information", "fgoicp_information_from_moments"):
        assert name in declared and name in fg._lib.exported_symbols()
    assert sorted(fg._lib.exported_symbols()) == declared
    assert fg._lib.load().fgoicp_abi_version() == 2  # additions only
    # the layouts as a C compiler sees the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fgoicp_amd.h"\n'
                   '#define O(T, m) printf("%s.%s %zu\\n", #T, #m, offsetof(T, m))\n'
                   'int main(void) {\n'
                   '  O(fgoicp_information_t, struct_size); O(fgoicp_information_t, points); O(fgoicp_information_t, correspondences); O(fgoicp_information_t, sum_dist2);\n'
                   '  O(fgoicp_information_t, sum_q); O(fgoicp_information_t, sum_qq); O(fgoicp_information_t, info); O(fgoicp_information_t, max_dist2);\n'
                   '  O(fgoicp_information_t, scaling_factor); printf("fgoicp_information_t.sizeof %zu\\n", sizeof(fgoicp_information_t));\n'
                   '  O(fgoicp_batch_opts, alignment); O(fgoicp_batch_opts, information); O(fgoicp_batch_opts, information_max_distance);\n'
                   '  printf("fgoicp_batch_opts.sizeof %zu\\n", sizeof(fgoicp_batch_opts));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], check=True)  # the header is C
    c_layout = dict(ln.rsplit(" ", 1) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    S, B = fg._lib.Information, fg._lib.BatchOptsInformation
    for name, _ in S._fields_:
        assert int(c_layout[f"fgoicp_information_t.{name}"]) == getattr(S, name).offset, name
    assert int(c_layout["fgoicp_information_t.sizeof"]) == C.sizeof(S) == S().struct_size == 400
    for name in ("alignment", "information", "information_max_distance"):
        assert int(c_layout[f"fgoicp_batch_opts.{name}"]) == getattr(B, name).offset, name
    assert int(c_layout["fgoicp_batch_opts.sizeof"]) == C.sizeof(B) == 56
    assert B.information.offset == 48 == C.sizeof(fg._lib.BatchOpts)  # behind the tail padding of the struct as first published


# ---- 3. struct_size, 4. null handles ------------------------------------------------------------------------------------------------
def test_information_calls_refuse_null_handles_and_a_zero_struct_size_with_a_message(fg):
    lib = fg._lib.load()
    fp = fg._lib.c_float_p
    R = np.eye(3, dtype=np.float32).reshape(9)
    t = np.zeros(3, np.float32)
    out = fg._lib.Information()
    assert lib.fgoicp_information(None, R.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), C.byref(out)) == INVALID_ARG
    assert "fgoicp_information" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_solver_information(None, float("inf"), C.byref(out)) == INVALID_ARG
    assert "fgoicp_solver_information" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_batch_information(None, 0, C.byref(out)) == INVALID_ARG
    assert "fgoicp_batch_information" in _msg(lib) and "null" in _msg(lib)
    assert (out.points, out.correspondences, out.sum_dist2, out.struct_size) == (0, 0, 0.0, 400) and not any(out.info)  # nothing written on refusal
    # struct_size 0 and a null `out` on a batch that exists (fgoicp_batch_create makes no device state)
    pts = np.random.default_rng(3).uniform(-1, 1, (32, 3)).astype(np.float32)
    b = fg.FastGoICPBatch([(pts, pts)], lut_resolution=0.1, information=True)
    zero = fg._lib.Information()
    zero.struct_size = 0
    for o in (C.byref(zero), None):
        assert lib.fgoicp_batch_information(b._h, 0, o) == INVALID_ARG
    b.close()


def test_a_refused_call_writes_nothing_into_the_callers_struct(fg):
    """struct_size 0 is refused and no byte is written (that a shorter struct is not overrun by an ANSWER needs a device:
    tests/test_gpu_information.py)"""
    lib = fg._lib.load()
    buf = (C.c_ubyte * 512)(*([0xA5] * 512))
    out = C.cast(buf, C.POINTER(fg._lib.Information))
    out.contents.struct_size = 0
    fp = fg._lib.c_float_p
    R = np.eye(3, dtype=np.float32).reshape(9)
    t = np.zeros(3, np.float32)
    fake = C.c_void_p(1)  # never looked at: the struct is checked first
    assert lib.fgoicp_information(fake, R.ctypes.data_as(fp), t.ctypes.data_as(fp), 1.0, out) == INVALID_ARG and "struct_size" in _msg(lib)
    assert lib.fgoicp_solver_information(None, 1.0, out) == INVALID_ARG
    assert bytes(buf)[4:] == bytes([0xA5] * 508) and out.contents.struct_size == 0


# ---- 5. batch refusals --------------------------------------------------------------------------------------------------------------
def _pairs(fg, n=2):
    pts = np.random.default_rng(3).uniform(-1, 1, (32, 3)).astype(np.float32)
    arr = (fg._lib.BatchPair * n)()
    for i in range(n):
        arr[i] = fg._lib.BatchPair(pts.ctypes.data_as(fg._lib.c_float_p), 32, pts.ctypes.data_as(fg._lib.c_float_p), 32, 0.1, 1e-3)
    return pts, arr


def test_batch_information_refuses_option_off_and_not_yet_run(fg):
    lib = fg._lib.load()
    L = fg._lib
    pts, arr = _pairs(fg)
    out = L.Information()
    for on in (0, 1):
        o = L.BatchOptsInformation(C.sizeof(L.BatchOptsInformation), L.SolverOpts(0, 1, 0, 0, 0.0), 0, None, 0, on, 0.25)
        h = C.c_void_p()
        assert lib.fgoicp_batch_create(arr, 2, C.byref(o), C.byref(h)) == 0 and h.value
        assert lib.fgoicp_batch_information(h, 0, C.byref(out)) == INVALID_ARG
        assert ("information = 0" in _msg(lib)) if not on else ("has not run" in _msg(lib)), _msg(lib)
        assert lib.fgoicp_batch_information(h, 7, C.byref(out)) == INVALID_ARG
        assert lib.fgoicp_batch_alignment(h, 0, None, None, None, None, None) == INVALID_ARG and "alignment = 0" in _msg(lib)  # the other option is its own
        lib.fgoicp_batch_destroy(h)
    # a NaN distance is refused at create
    o = L.BatchOptsInformation(C.sizeof(L.BatchOptsInformation), L.SolverOpts(0, 1, 0, 0, 0.0), 0, None, 0, 1, float("nan"))
    h = C.c_void_p()
    assert lib.fgoicp_batch_create(arr, 2, C.byref(o), C.byref(h)) == INVALID_ARG and not h.value and "information_max_distance" in _msg(lib)
    # the Python wrapper raises the same refusals
    for kw, text in ((dict(information=True), "has not run"), (dict(information=0.5), "has not run"), (dict(), "information = 0"), (dict(alignment=True), "information = 0")):
        b = fg.FastGoICPBatch([(pts, pts)], lut_resolution=0.1, **kw)
        with pytest.raises(fg.FgoicpError) as e:
            b.information(0)
        assert e.value.status == INVALID_ARG and text in str(e.value)
        b.close()


def test_batch_create_accepts_the_shorter_options_structs(fg):
    """callers built before the members were appended hand over 40 bytes (before `alignment`) or 48 (with it, tail padding included):
    accepted, and what lies behind their struct is not read as the option"""
    lib = fg._lib.load()
    L = fg._lib
    _, arr = _pairs(fg)
    for size in (L.BatchOpts.alignment.offset, C.sizeof(L.BatchOpts), L.BatchOptsInformation.information_max_distance.offset):
        o = L.BatchOptsInformation(size, L.SolverOpts(0, 1, 0, 0, 0.0), 0, None, 0, 0x5A5A5A5A, float("nan"))
        if size >= 52:
            o.information = 1  # a struct that ends behind `information`: the option is read, the distance is not (NaN would be refused)
        raw = (C.c_ubyte * C.sizeof(o)).from_buffer(o)
        if size <= 48:
            raw[44:48] = [0x5A] * 4  # an old caller's tail padding holds anything
        h = C.c_void_p()
        assert lib.fgoicp_batch_create(arr, 2, C.byref(o), C.byref(h)) == 0 and h.value, (size, _msg(lib))
        out = L.Information()
        assert lib.fgoicp_batch_information(h, 0, C.byref(out)) == INVALID_ARG
        assert ("information = 0" if size <= 48 else "has not run") in _msg(lib), (size, _msg(lib))
        lib.fgoicp_batch_destroy(h)


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------------
class InfoConfigOut(C.Structure):
    _fields_ = [(k, C.c_char * 512) for k in ("target", "source", "output", "visualization", "alignment", "information")] + [("printed", C.c_char * 2048),
                                                                                                                            ("information_distance", C.c_float)]


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HERE, "libinformation_harness.so")
    src = os.path.join(HERE, "information_harness.cpp")
    deps = [src, os.path.join(REPO, "fast-go-icp_amd/csrc/cli/config.hpp"), os.path.join(REPO, "include/fgoicp/common.hpp"), os.path.join(REPO, "include/fgoicp_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.info_parse_config.argtypes = [C.c_char_p, C.POINTER(InfoConfigOut)]
    L.info_write.argtypes = [C.c_char_p, C.c_ulonglong, C.c_ulonglong, C.c_double, C.POINTER(C.c_double), C.c_float, C.c_float]
    return L


def test_cli_parser_reads_the_two_keys_and_leaves_other_configs_alone(harness, tmp_path):
    base = '[io]\ntarget = "t.txt"\nsource = "s.txt"\noutput = "out.toml"\n{io}[params]\nlut_resolution = 0.01\nmse_threshold = 0.002\n{params}'
    out = InfoConfigOut()
    (tmp_path / "a.toml").write_text(base.format(io='information = "pairs/info.txt"   # the matrix\n', params="information_distance = 0.125\n"))
    assert harness.info_parse_config(str(tmp_path / "a.toml").encode(), C.byref(out)) == 0
    assert out.information == b"pairs/info.txt" and out.information_distance == 0.125
    plain = InfoConfigOut()
    (tmp_path / "b.toml").write_text(base.format(io="", params=""))
    assert harness.info_parse_config(str(tmp_path / "b.toml").encode(), C.byref(plain)) == 0
    assert plain.information == b"" and plain.information_distance == 0.0
    for o in (out, plain):
        assert (o.target, o.source, o.output, o.visualization, o.alignment) == (b"t.txt", b"s.txt", b"out.toml", b"", b"")
    # the printed summary does not know the keys: the two configs print the same lines, the ones the reference prints
    assert out.printed == plain.printed and b"nformation" not in plain.printed
    assert plain.printed.decode().splitlines()[0] == "Fast Go-ICP Configurations" and b"MSE Threshold: 0.002" in plain.printed
    # a key without a file name, a zero and a negative distance: none
    for params in ("information_distance = 0\n", "information_distance = -3\n"):
        o = InfoConfigOut()
        (tmp_path / "c.toml").write_text(base.format(io='information = "i.txt"\n', params=params))
        assert harness.info_parse_config(str(tmp_path / "c.toml").encode(), C.byref(o)) == 0
        assert o.information == b"i.txt" and o.information_distance == 0.0


def test_information_file_has_the_documented_lines(harness, tmp_path):
    """one '#' line (correspondences, fitness, inlier_rmse in the files' units, the distance used), then six lines of six numbers at
    precision 17: the doubles read back are the doubles written"""
    rng = np.random.default_rng(9)
    info = rng.normal(size=36) * 10.0 ** rng.integers(-3, 9, 36)
    info[7] = 0.0
    info[8] = 1.0 / 3.0
    path = tmp_path / "info.txt"
    dp = C.POINTER(C.c_double)
    assert harness.info_write(str(path).encode(), 4, 3, 12.0, info.ctypes.data_as(dp), 0.5, 0.25) == 0
    lines = path.read_text().splitlines()
    assert len(lines) == 7
    assert lines[0] == "# information: correspondences = 3, fitness = 0.75, inlier_rmse = 4, distance = 0.25"  # sqrt(12 / 3) / 0.5
    assert all(len(ln.split()) == 6 for ln in lines[1:])
    assert lines[2].split()[1:3] == ["0", "0.33333333333333331"]
    back = np.loadtxt(path)  # the '#' line is a comment to every reader of such files
    assert back.shape == (6, 6) and np.array_equal(back.reshape(36), info)
    assert harness.info_write(str(path).encode(), 4, 0, 0.0, info.ctypes.data_as(dp), 0.5, 0.0) == 0  # nothing counted, no threshold
    assert path.read_text().splitlines()[0] == "# information: correspondences = 0, fitness = 0, inlier_rmse = 0, distance = inf"
    assert harness.info_write(str(tmp_path / "no" / "such" / "dir.txt").encode(), 4, 3, 12.0, info.ctypes.data_as(dp), 0.5, 0.25) == 1


# ---- 7. the facade ------------------------------------------------------------------------------------------------------------------
def test_information_facade_compiles_against_the_c_abi_alone(fg, tmp_path):
    """icp::Registration::information / icp::FastGoICP::information (include/fgoicp/*.hpp) build with a plain C++17 compiler; without a
    GPU the host half still answers and the solver's constructor throws before anything is computed."""
    fg.build.build()
    exe = str(tmp_path / "facade_information_check")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(HERE, "facade_information_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    import torch
    if torch.cuda.is_available():
        return  # the run itself: tests/test_gpu_information.py
    (tmp_path / "pc.txt").write_text("2\n0 0 0\n1 1 1\n")
    p = subprocess.run([exe, str(tmp_path / "pc.txt"), str(tmp_path / "pc.txt"), "0.05", "0"], capture_output=True, text=True)
    assert p.returncode not in (0, 2, 3) and "no HIP device" in (p.stderr + p.stdout)
