"""The point-to-plane refinement (fgoicp_plane_step_from_moments, fgoicp_plane_apply_step, fgoicp_plane_moments, fgoicp_icp_plane,
fgoicp_solver_refine_plane, fgoicp_ctx_set_target_normals, fgoicp_target_normals, fgoicp_target_knn) as far as it goes without a GPU: the
host half against numpy, the refusals, the ctypes table and the struct layouts against the header, the CLI's keys and the table it
writes, the C++ facade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "host_harness")
INVALID_ARG = 1
f32, f64 = np.float32, np.float64
NEW = ("fgoicp_ctx_set_target_normals", "fgoicp_target_normals", "fgoicp_target_knn", "fgoicp_plane_moments", "fgoicp_plane_step_from_moments",
       "fgoicp_plane_apply_step", "fgoicp_icp_plane", "fgoicp_solver_refine_plane")


def _msg(lib):
    return lib.fgoicp_last_error().decode()


def moments(x, n, r):
    """the 28 sums in float64: the upper triangle of sum J^T J row by row, sum J^T r, sum r^2"""
    J = np.hstack([np.cross(x, n), n])
    A, g = J.T @ J, J.T @ r
    return np.concatenate([A[np.triu_indices(6)], g, [r @ r]]), A, g


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- 1. the step against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 50, 1000])
def test_step_matches_lstsq_on_a_generic_set(fg, n):
    rng = np.random.default_rng(n)
    x, nn, r = rng.normal(size=(n, 3)), unit(rng.normal(size=(n, 3))), rng.normal(size=n) * 0.01
    m, A, g = moments(x, nn, r)
    xi, rank = fg.plane_step_from_moments(n, m)
    want = np.linalg.lstsq(A, -g, rcond=None)[0]
    print(f"n {n}: rank {rank}, largest deviation / largest entry {np.abs(xi - want).max() / np.abs(want).max():.3g}")
    assert rank == 6
    assert np.abs(xi - want).max() <= 1e-10 * np.abs(want).max()


def test_rank_of_degenerate_sets(fg):
    """equal normals (a plane): 3 — the two tilts and the offset; normals all perpendicular to one axis, generic points (a prism): 5 — the
    slide along the axis is free; the same normals with the points ON the axis: the rotation about it is free too, the matrix has rank 4
    (numpy.linalg.matrix_rank agrees) — J = (-z n_y, z n_x, 0, n_x, n_y, 0) has two zero columns; a sphere: 3 in rotation, the step moves
    the centre only"""
    rng = np.random.default_rng(1)
    n = 200
    x, r = rng.normal(size=(n, 3)), rng.normal(size=n) * 0.01
    m, A, g = moments(x, np.tile([0.0, 0.0, 1.0], (n, 1)), r)
    xi, rank = fg.plane_step_from_moments(n, m)
    assert rank == 3 and not xi[[2, 3, 4]].any()
    want = np.linalg.lstsq(A, -g, rcond=1e-9)[0]
    assert np.abs(xi - want).max() <= 1e-10 * np.abs(want).max()
    perp = rng.normal(size=(n, 3))
    perp[:, 2] = 0
    perp = unit(perp)
    m, A, g = moments(x, perp, r)
    xi, rank = fg.plane_step_from_moments(n, m)
    assert rank == 5 == np.linalg.matrix_rank(A, tol=1e-9 * np.linalg.eigvalsh(A).max()) and xi[5] == 0
    on_axis = np.zeros((n, 3))
    on_axis[:, 2] = rng.normal(size=n)
    m, A, g = moments(on_axis, perp, r)
    xi, rank = fg.plane_step_from_moments(n, m)
    assert rank == 4 == np.linalg.matrix_rank(A, tol=1e-9 * np.linalg.eigvalsh(A).max()) and not xi[[2, 5]].any()
    sph = unit(rng.normal(size=(n, 3)))
    m, A, g = moments(2.0 * sph, sph, r)  # x cross n = 0
    xi, rank = fg.plane_step_from_moments(n, m)
    assert rank == 3 and not xi[:3].any() and np.abs(xi[3:] - np.linalg.lstsq(A[3:, 3:], -g[3:], rcond=None)[0]).max() <= 1e-12
    # nothing but zeros: rank 0, no step
    xi, rank = fg.plane_step_from_moments(5, np.zeros(28))
    assert rank == 0 and not xi.any()


# ---- 2. the pose update --------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)
    return np.eye(3) + (np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K) if th > 0 else K)


@pytest.mark.parametrize("scale", [0.0, 1e-9, 1e-3, 0.3, 2.5])
def test_pose_update_is_rodrigues_in_float64_rounded_once(fg, scale):
    """R' within 4 float32 ulps of Rod(w) R (one rounding, then the nearest rotation of a matrix 1 ulp from one), t' the float32 of
    Rod(w) t + v"""
    rng = np.random.default_rng(7)
    R = fg.synth.random_rotation(rng).astype(f32)
    R, _ = fg.plane_apply_step(R, np.zeros(3), np.zeros(6))  # the float32 rotation nearest to it
    t = rng.normal(size=3).astype(f32)
    xi = np.concatenate([unit(rng.normal(size=3)) * scale, rng.normal(size=3) * 0.1])
    R1, t1 = fg.plane_apply_step(R, t, xi)
    Q = rodrigues(xi[:3])
    assert R1.dtype == np.float32 and np.abs(R1.astype(f64) - Q @ R.astype(f64)).max() <= 4 * 2.0 ** -24
    assert np.abs(R1.astype(f64).T @ R1.astype(f64) - np.eye(3)).max() <= 4 * 2.0 ** -24 and np.linalg.det(R1.astype(f64)) > 0.999
    assert np.abs(t1.astype(f64) - (Q @ t.astype(f64) + xi[3:])).max() <= 2.0 ** -24 * max(1.0, np.abs(t1).max())
    if scale == 0.0:
        assert np.array_equal(R1, R) and np.array_equal(t1, (t.astype(f64) + xi[3:]).astype(f32))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_host_calls_refuse_null_nothing_counted_and_non_finite_moments(fg):
    lib = fg._lib.load()
    dp = C.POINTER(C.c_double)
    m, xi, rank = (C.c_double * 28)(), (C.c_double * 6)(), C.c_int(7)
    m[0] = m[6] = 1.0
    assert lib.fgoicp_plane_step_from_moments(1, m, xi, C.byref(rank)) == 0 and rank.value == 2
    for args in ((1, None, xi, C.byref(rank)), (1, m, None, C.byref(rank)), (1, m, xi, None)):
        assert lib.fgoicp_plane_step_from_moments(*args) == INVALID_ARG and "fgoicp_plane_step_from_moments" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_plane_step_from_moments(0, m, xi, C.byref(rank)) == INVALID_ARG and "n = 0" in _msg(lib)
    for k, bad in ((0, float("nan")), (13, float("inf")), (27, float("-inf"))):
        spoiled = (C.c_double * 28)(*m)
        spoiled[k] = bad
        assert lib.fgoicp_plane_step_from_moments(1, spoiled, xi, C.byref(rank)) == INVALID_ARG and "finite" in _msg(lib)
    R, t = np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32)
    fp = fg._lib.c_float_p
    good = np.zeros(6)
    assert lib.fgoicp_plane_apply_step(None, t.ctypes.data_as(fp), good.ctypes.data_as(dp), R.ctypes.data_as(fp), t.ctypes.data_as(fp)) == INVALID_ARG
    bad = np.array([0, 0, np.nan, 0, 0, 0.0])
    assert lib.fgoicp_plane_apply_step(R.ctypes.data_as(fp), t.ctypes.data_as(fp), bad.ctypes.data_as(dp), R.ctypes.data_as(fp), t.ctypes.data_as(fp)) == INVALID_ARG
    with pytest.raises(fg.FgoicpError):
        fg.plane_step_from_moments(0, np.zeros(28))


def test_device_calls_refuse_null_handles_and_a_zero_struct_size_before_any_device_work(fg):
    lib = fg._lib.load()
    fp = fg._lib.c_float_p
    R, t = np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32)
    Rp, tp = R.ctypes.data_as(fp), t.ctypes.data_as(fp)
    pm, pr = fg._lib.PlaneMoments(), fg._lib.PlaneResult()
    assert lib.fgoicp_ctx_set_target_normals(None, None, 16) == INVALID_ARG and "fgoicp_ctx_set_target_normals" in _msg(lib)
    assert lib.fgoicp_target_normals(None, Rp) == INVALID_ARG and "fgoicp_target_normals" in _msg(lib)
    assert lib.fgoicp_target_knn(None, 8, None, None) == INVALID_ARG and "fgoicp_target_knn" in _msg(lib)
    assert lib.fgoicp_plane_moments(None, Rp, tp, float("inf"), C.byref(pm)) == INVALID_ARG and "fgoicp_plane_moments" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_icp_plane(None, Rp, tp, 30, 1e-6, float("inf"), C.byref(pr)) == INVALID_ARG and "fgoicp_icp_plane" in _msg(lib) and "null" in _msg(lib)
    assert lib.fgoicp_solver_refine_plane(None, 16, 30, 1e-6, float("inf"), C.byref(pr)) == INVALID_ARG and "fgoicp_solver_refine_plane" in _msg(lib)
    assert (pm.points, pm.correspondences, pr.iterations, pr.rank) == (0, 0, 0, 0)
    # struct_size 0, a null struct, a NaN or negative threshold: refused before the context is looked at (the handle is never followed)
    fake = C.c_void_p(1)
    for cls, call in ((fg._lib.PlaneMoments, lambda o, d=float("inf"): lib.fgoicp_plane_moments(fake, Rp, tp, d, o)),
                      (fg._lib.PlaneResult, lambda o, d=float("inf"): lib.fgoicp_icp_plane(fake, Rp, tp, 30, 1e-6, d, o))):
        buf = (C.c_ubyte * 512)(*([0xA5] * 512))
        out = C.cast(buf, C.POINTER(cls))
        out.contents.struct_size = 0
        assert call(out) == INVALID_ARG and "struct_size" in _msg(lib)
        assert bytes(buf)[4:] == bytes([0xA5] * 508) and out.contents.struct_size == 0
        assert call(None) == INVALID_ARG
        ok = cls()
        for d in (float("nan"), -1.0):
            assert call(C.byref(ok), d) == INVALID_ARG and "max_dist2" in _msg(lib)


# ---- 4. table and structs ------------------------------------------------------------------------------------------------------------
def test_ctypes_table_and_struct_layouts_match_the_header(fg, tmp_path):
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "fgoicp_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fgoicp_[a-z_0-9]+)\s*\(", txt)))
    for name in NEW:
        assert name in declared and name in fg._lib.exported_symbols() and hasattr(fg._lib.load(), name)
    assert sorted(fg._lib.exported_symbols()) == declared
    assert fg._lib.load().fgoicp_abi_version() == 2  # additions only
    src = tmp_path / "layout.c"
    members = {"fgoicp_plane_moments_t": ("struct_size", "points", "correspondences", "m", "max_dist2"),
               "fgoicp_plane_result_t": ("struct_size", "R", "t", "iterations", "rank", "correspondences", "plane_rmse", "sse", "scaling_factor")}
    body = "".join(f'  printf("{T}.{m} %zu\\n", offsetof({T}, {m}));\n' for T, ms in members.items() for m in ms)
    body += "".join(f'  printf("{T}.sizeof %zu\\n", sizeof({T}));\n' for T in members)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fgoicp_amd.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", exe], check=True)  # the header is C
    c_layout = dict(ln.rsplit(" ", 1) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for T, S in (("fgoicp_plane_moments_t", fg._lib.PlaneMoments), ("fgoicp_plane_result_t", fg._lib.PlaneResult)):
        for name, _ in S._fields_:
            assert int(c_layout[f"{T}.{name}"]) == getattr(S, name).offset, (T, name)
        assert int(c_layout[f"{T}.sizeof"]) == C.sizeof(S) == S().struct_size
    assert C.sizeof(fg._lib.PlaneMoments) == 256 and C.sizeof(fg._lib.PlaneResult) == 88


# ---- 5. the CLI ----------------------------------------------------------------------------------------------------------------------
class PlaneConfigOut(C.Structure):
    _fields_ = [("refine", C.c_char * 64), ("printed", C.c_char * 2048), ("error", C.c_char * 512), ("refine_knn", C.c_int), ("refine_max_iter", C.c_int),
                ("refine_distance", C.c_float)]


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(HERE, "libplane_harness.so")
    src = os.path.join(HERE, "plane_harness.cpp")
    deps = [src, os.path.join(REPO, "fast-go-icp_amd/csrc/cli/config.hpp"), os.path.join(REPO, "include/fgoicp/common.hpp"), os.path.join(REPO, "include/fgoicp_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.plane_parse_config.argtypes = [C.c_char_p, C.POINTER(PlaneConfigOut)]
    L.plane_write_result.argtypes = [C.c_char_p, C.c_void_p]
    return L


def test_cli_parser_reads_the_refine_keys_and_refuses_another_refinement(harness, tmp_path):
    base = '[io]\ntarget = "t.txt"\nsource = "s.txt"\noutput = "out.toml"\n[params]\nlut_resolution = 0.01\nmse_threshold = 0.002\n{params}'
    out = PlaneConfigOut()
    (tmp_path / "a.toml").write_text(base.format(params='refine = "plane"   # after the search\nrefine_knn = 12\nrefine_max_iter = 7\nrefine_distance = 0.125\n'))
    assert harness.plane_parse_config(str(tmp_path / "a.toml").encode(), C.byref(out)) == 0
    assert (out.refine, out.refine_knn, out.refine_max_iter, out.refine_distance) == (b"plane", 12, 7, 0.125)
    dflt = PlaneConfigOut()
    (tmp_path / "b.toml").write_text(base.format(params='refine = "plane"\nrefine_distance = -2\n'))
    assert harness.plane_parse_config(str(tmp_path / "b.toml").encode(), C.byref(dflt)) == 0
    assert (dflt.refine, dflt.refine_knn, dflt.refine_max_iter, dflt.refine_distance) == (b"plane", 16, 30, 0.0)
    plain = PlaneConfigOut()
    (tmp_path / "c.toml").write_text(base.format(params=""))
    assert harness.plane_parse_config(str(tmp_path / "c.toml").encode(), C.byref(plain)) == 0
    assert (plain.refine, plain.refine_knn, plain.refine_max_iter, plain.refine_distance) == (b"", 16, 30, 0.0)
    assert out.printed == plain.printed and b"efine" not in plain.printed  # the printed summary is the reference's
    for params, text in (('refine = "other"\n', b'"other"'), ('refine = "point"\n', b'"point"'), ('refine = "plane"\nrefine_knn = 3\n', b"refine_knn"),
                         ('refine = "plane"\nrefine_knn = 33\n', b"refine_knn")):
        bad = PlaneConfigOut()
        (tmp_path / "d.toml").write_text(base.format(params=params))
        assert harness.plane_parse_config(str(tmp_path / "d.toml").encode(), C.byref(bad)) == 2 and text in bad.error, params


def test_result_file_gets_a_refined_table_behind_the_unchanged_keys(fg, harness, tmp_path):
    raw = fg._lib.PlaneResult()
    raw.R[:] = [0, 1, 0, -1, 0, 0, 0, 0, 1]  # glm order: the columns (0, 1, 0), (-1, 0, 0), (0, 0, 1)
    raw.t[:] = [0.5, -0.25, 4]
    raw.iterations, raw.rank, raw.correspondences, raw.plane_rmse, raw.scaling_factor = 9, 6, 123, 0.5, 4.0
    assert harness.plane_write_result(str(tmp_path / "plain.toml").encode(), None) == 0
    assert harness.plane_write_result(str(tmp_path / "with.toml").encode(), C.cast(C.byref(raw), C.c_void_p)) == 0
    plain, with_ = (tmp_path / "plain.toml").read_text(), (tmp_path / "with.toml").read_text()
    assert with_.startswith(plain) and "[refined]" not in plain
    tail = with_[len(plain):].splitlines()
    assert tail == ["", "[refined]", "rotation = [", "  [0, -1, 0],", "  [1, 0, 0],", "  [0, 0, 1],", "]", "translation = [0.5, -0.25, 4]", "plane_rmse = 0.125", "iterations = 9",
                    "rank = 6", "correspondences = 123"]


# ---- 6. the facade -------------------------------------------------------------------------------------------------------------------
def test_plane_facade_compiles_against_the_c_abi_alone(fg, tmp_path):
    """the new members of icp::Registration and icp::FastGoICP build with a plain C++17 compiler; without a GPU the host half still
    answers and the solver's constructor throws before anything is computed"""
    fg.build.build()
    exe = str(tmp_path / "facade_plane_check")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(HERE, "facade_plane_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    import torch
    if torch.cuda.is_available():
        return  # the run itself: tests/test_gpu_plane.py
    (tmp_path / "pc.txt").write_text("2\n0 0 0\n1 1 1\n")
    p = subprocess.run([exe, str(tmp_path / "pc.txt"), str(tmp_path / "pc.txt"), "0.05"], capture_output=True, text=True)
    assert p.returncode not in (0, 2, 3) and "no HIP device" in (p.stderr + p.stdout)
