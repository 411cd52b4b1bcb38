"""Mesh sampling (fgoicp_mesh_sample, fgoicp_solver_set_target_normals / _source_normals, params.*_mesh_points) as far as it goes without a
GPU: the numpy restatement of the definition itself (tests/mesh_restatement.py) on the planted mesh, the struct layout against the header,
every refusal that needs no device (status 1 with a message), the ctypes table, the PLY mesh reader and the two configuration keys.  The
device's results are checked in tests/test_gpu_mesh.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_restatement as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
PREFIX = "fgoicp_mesh_sample: "


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    return mr.planted_mesh()


def test_the_planted_mesh_is_what_it_says(planted):
    V, T = planted
    area = mr.face_area(V, T)
    q, Q, amax = mr.weights(area)
    assert len(T) == 15 and amax == 3.0
    assert int((area == 0.0).sum()) == 1 and int((q == 0).sum()) == 2
    assert area[14] > 0.0 and area[14] * 2.0 ** 32 < amax  # the tiny face: more than 2^32 times smaller than the largest
    assert int(q.max()) == 2 ** 32 and int(Q[-1]) == int(q.astype(object).sum())
    info = mr.info(V, T, 7, area)
    assert info["zero_area"] == 1 and info["unweighted"] == 2 and info["area"] == pytest.approx(22.002, rel=1e-9)


@pytest.mark.parametrize("m", [257, 20000])
def test_the_restatement_spreads_the_samples_by_area(planted, m):
    """the counts per face against their expectation m * q_f / weight_total, over the faces that expect at least 5 samples: the largest
    |count - expected| / sqrt(expected) must be <= 4 (a 4-sigma bound on a Poisson-like count; with seed 12345 and this face order the restatement gives 1.46 at m = 20000 and 2.14
    at m = 257)"""
    V, T = planted
    pts, nrm, face, uv, area, info = mr.sample(V, T, m, seed=12345)
    q, Q, _ = mr.weights(area)
    expected = m * q.astype(np.float64) / float(Q[-1])
    count = np.bincount(face, minlength=len(T))
    big = expected >= 5.0
    z = np.abs(count[big] - expected[big]) / np.sqrt(expected[big])
    print(f"m = {m}: {int(big.sum())} faces expect >= 5 samples, largest |count - expected| / sqrt(expected) = {z.max():.3f}")
    assert big.sum() >= 12 and z.max() <= 4.0
    assert count[q == 0].sum() == 0  # the unweighted faces get no sample
    assert (uv >= 0.0).all() and (uv.sum(1) <= 1.0).all()
    a, e1, e2, n, n2 = mr.faces(V, T)
    dist = ((pts.astype(np.float64) - a[face]) * n[face]).sum(1)  # axis-aligned faces: one non-zero term, exact
    assert (dist == 0.0).all()
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-7)
    assert pts.dtype == np.float32 and face.dtype == np.uint32 and uv.dtype == np.float64


def test_the_restatement_is_counter_based(planted):
    V, T = planted
    a = mr.sample(V, T, 257, seed=3)
    b = mr.sample(V, T, 64, seed=3)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x[:64], y)
    assert not np.array_equal(a[2], mr.sample(V, T, 257, seed=4)[2])
    assert mr.mulhi64(np.array([2 ** 64 - 1, 2 ** 63, 12345], np.uint64), 2 ** 36 + 5).tolist() == [2 ** 36 + 4, 2 ** 35 + 2, (12345 * (2 ** 36 + 5)) >> 64]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_calls_and_the_struct_is_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    new = ("fgoicp_mesh_sample", "fgoicp_solver_set_target_normals", "fgoicp_solver_set_source_normals")
    header = open(os.path.join(REPO, "include", "fgoicp_amd.h")).read()
    for name in new:
        assert hasattr(lib, name) and name in fg._lib.exported_symbols() and name + "(" in header
    for path in (fg.build.DEFAULT_LIB, fg.build.DEV_LIB):  # built into both libraries
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        for name in new:
            assert f" T {name}\n" in syms, (path, name)
    assert callable(fg.sample_mesh) and callable(fg.sample_mesh_even) and callable(fg.FastGoICP.set_target_normals) and callable(fg.FastGoICP.set_source_normals)
    fields = ["struct_size", "vertices", "triangles", "samples", "zero_area", "unweighted", "weight_total", "max_area", "area"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(fgoicp_mesh_info_t), '
                   + ", ".join(f"offsetof(fgoicp_mesh_info_t, {f})" for f in fields) + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    M = fg._lib.MeshInfo
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert got == [72, 0, 8, 16, 24, 32, 40, 48, 56, 64]


def _call(fg, V, T, nv=None, nf=None, m=10, seed=0, info="full", want_points=True):
    """the raw call: returns (status, message)"""
    L = fg._lib
    lib = L.load()
    mi = L.MeshInfo()
    if isinstance(info, int):
        mi.struct_size = info
    out = np.empty((max(min(m, 1 << 16), 1), 3), np.float32) if want_points else None  # (a refused m never writes a row)
    rc = lib.fgoicp_mesh_sample(None if V is None else V.ctypes.data_as(L.c_float_p), len(V) if nv is None else nv, None if T is None else T.ctypes.data_as(L.c_uint32_p),
                                len(T) if nf is None else nf, m, seed, 0, None if out is None else out.ctypes.data_as(L.c_float_p), None, None, None, None,
                                None if info is None else C.byref(mi))
    return rc, lib.fgoicp_last_error().decode()


def _with(a, i, j, value):
    b = a.copy()
    b[i, j] = value
    return b


REFUSALS = {
    "null vertices": (lambda V, T: dict(V=None, T=T, nv=5), "the vertices must not be null or empty"),
    "no vertices": (lambda V, T: dict(V=V, T=T, nv=0), "the vertices must not be null or empty"),
    "null triangles": (lambda V, T: dict(V=V, T=None, nf=5), "the triangles must not be null or empty"),
    "no triangles": (lambda V, T: dict(V=V, T=T, nf=0), "the triangles must not be null or empty"),
    "2^31 vertices": (lambda V, T: dict(V=V, T=T, nv=2 ** 31), "more than 2^31 - 1 vertices"),  # refused on the count alone: the array is not read
    "2^31 triangles": (lambda V, T: dict(V=V, T=T, nf=2 ** 31), "more than 2^31 - 1 triangles"),
    "m = 0": (lambda V, T: dict(V=V, T=T, m=0), "the sample count must lie in [1, 2^31 - 1]"),
    "m = 2^31": (lambda V, T: dict(V=V, T=T, m=2 ** 31), "the sample count must lie in [1, 2^31 - 1]"),
    "null points": (lambda V, T: dict(V=V, T=T, want_points=False), "points_m3 must not be null"),
    "nan vertex": (lambda V, T: dict(V=_with(V, 9, 1, np.nan), T=T), "vertex 9 has a non-finite coordinate"),
    "infinite vertex": (lambda V, T: dict(V=_with(V, 13, 2, -np.inf), T=T), "vertex 13 has a non-finite coordinate"),
    "index = nv": (lambda V, T: dict(V=V, T=_with(T, 6, 2, len(V))), "face 6 has vertex index 14: the mesh has 14 vertices"),
    "index far above nv": (lambda V, T: dict(V=V, T=_with(T, 14, 0, 2 ** 32 - 1)), "face 14 has vertex index 4294967295: the mesh has 14 vertices"),
    "null info": (lambda V, T: dict(V=V, T=T, info=None), "out must not be null and out->struct_size = sizeof(fgoicp_mesh_info_t)"),
    "struct_size 0": (lambda V, T: dict(V=V, T=T, info=0), "out must not be null and out->struct_size = sizeof(fgoicp_mesh_info_t)"),
    "struct_size short": (lambda V, T: dict(V=V, T=T, info=64), "out must not be null and out->struct_size = sizeof(fgoicp_mesh_info_t)"),  # ends before `area` ends
    "struct_size above 4096": (lambda V, T: dict(V=V, T=T, info=4097), "out must not be null and out->struct_size = sizeof(fgoicp_mesh_info_t)"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, planted, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    make, message = REFUSALS[case]
    rc, msg = _call(fg, **make(*planted))
    assert rc == INVALID_ARG and msg == PREFIX + message, (case, rc, msg)


def test_a_valid_call_without_a_device_reports_no_device(fg, planted):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_mesh.py)"""
    V, T = planted
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(m=1), dict(info=72), dict(info=4096), dict(seed=2 ** 64 - 1)):
        rc, msg = _call(fg, V, T, **kw)
        assert rc == want and (msg.startswith(PREFIX) or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.sample_mesh(V, T, 10)
        assert e.value.status == NO_DEVICE


def test_the_python_wrappers_check_shapes_and_types_first(fg, planted):
    V, T = planted
    for bad_v in (V[:, :2], V.reshape(-1)):
        with pytest.raises(ValueError):
            fg.sample_mesh(bad_v, T, 1)
    for bad_t in (T[:, :2], T.reshape(-1), T.astype(np.float32), T.astype(np.int64) - 1):
        with pytest.raises(ValueError):
            fg.sample_mesh(V, bad_t, 1)
    for m in (0, -1):
        with pytest.raises(ValueError):
            fg.sample_mesh(V, T, m)
        with pytest.raises(ValueError):
            fg.sample_mesh_even(V, T, m)
    with pytest.raises(ValueError):
        fg.sample_mesh_even(V, T, 5, init_factor=0)
    for m in (2.5, True, "3"):
        with pytest.raises(TypeError):
            fg.sample_mesh(V, T, m)
        with pytest.raises(TypeError):
            fg.sample_mesh_even(V, T, m)
    with pytest.raises(TypeError):
        fg.sample_mesh(V, T, 5, seed=1.5)
    with pytest.raises(fg.FgoicpError) as e:  # what the wrapper does not check itself, the call refuses
        fg.sample_mesh(V, _with(T, 3, 1, 99), 10)
    assert e.value.status == INVALID_ARG and "face 3 has vertex index 99" in str(e.value)


def test_the_solver_normal_setters_refuse_a_null_solver_and_null_normals(fg):
    lib = fg._lib.load()
    buf = np.zeros((4, 3), np.float32).ctypes.data_as(fg._lib.c_float_p)
    fake = C.c_void_p(8)  # never dereferenced: the null pointer is refused first
    for name in ("fgoicp_solver_set_target_normals", "fgoicp_solver_set_source_normals"):
        fn = getattr(lib, name)
        assert fn(None, buf) == INVALID_ARG and lib.fgoicp_last_error().decode() == name + ": the solver must not be null"
        assert fn(fake, None) == INVALID_ARG and lib.fgoicp_last_error().decode() == name + ": the normals must not be null"


def test_the_facade_with_the_normal_setters_compiles_against_the_c_abi_alone(fg, tmp_path):
    src = tmp_path / "facade_normals.cpp"
    src.write_text('#include "fgoicp/fgoicp.hpp"\n'
                   "int main() {\n"
                   "    void (icp::FastGoICP::*t)(const std::vector<icp::vec3>&) = &icp::FastGoICP::set_target_normals;\n"
                   "    void (icp::FastGoICP::*s)(const std::vector<icp::vec3>&) = &icp::FastGoICP::set_source_normals;\n"
                   "    return t && s ? 0 : 1;\n}\n")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "facade_normals"),
                    "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    assert subprocess.run([str(tmp_path / "facade_normals")]).returncode == 0


# ---- the PLY mesh reader and the configuration keys ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mesh_config") / "mesh_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "mesh_config_check.cpp")], check=True)

    def run(mode, path):
        p = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True, timeout=60)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith(("MESH", "V ", "T ", "REFUSED "))]
        return p.returncode, lines
    return run


# 8 vertices, 4 quads and 4 triangles: a cube whose top and bottom are split already
CUBE_V = np.array([(x, y, z) for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)], np.float32) * np.float32(1.25) + np.float32(0.1)
CUBE_POLYGONS = [[0, 1, 5, 4], [2, 6, 7, 3], [0, 4, 6, 2], [1, 3, 7, 5], [0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6]]
CUBE_TRIANGLES = [(0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5), (0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6)]


def _parse(lines):
    head = [int(x) for x in lines[0].split()[1:]]
    V = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("V ")], np.float32).reshape(-1, 3)
    T = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("T ")]
    return head, V, T


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_the_mesh_reader_fan_triangulates_in_every_format(check, tmp_path, fmt):
    for kw in (dict(), dict(list_name="vertex_index", count_type="ushort", index_type="uint"), dict(count_type="int", index_type="short")):
        path = tmp_path / "cube.ply"
        mr.write_ply(path, CUBE_V, CUBE_POLYGONS, fmt=fmt, **kw)
        rc, lines = check("mesh", path)
        assert rc == 0, lines
        head, V, T = _parse(lines)
        assert head == [8, 12, 0] and np.array_equal(V, CUBE_V) and T == CUBE_TRIANGLES, (fmt, kw)
        rc, lines = check("cloud", path)  # the cloud loader still sees the vertices alone
        head, V, T = _parse(lines)
        assert rc == 0 and head == [8, 0, 0] and np.array_equal(V, CUBE_V)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_the_mesh_reader_drops_short_faces_and_passes_over_other_lists(check, tmp_path, fmt):
    path = tmp_path / "short.ply"
    mr.write_ply(path, CUBE_V, [[0, 1], [0, 1, 2, 3, 4], [], [5], [7, 6, 5]], fmt=fmt, extra_list=("range_grid", "vertex_indices", [[0], [], [1, 2]]))
    rc, lines = check("mesh", path)
    head, V, T = _parse(lines)
    assert rc == 0 and head == [8, 4, 3] and T == [(0, 1, 2), (0, 2, 3), (0, 3, 4), (7, 6, 5)]  # range_grid's list is no face
    path = tmp_path / "scan.ply"  # a Stanford scan: a range_grid list and no faces
    mr.write_ply(path, CUBE_V, None, fmt=fmt, extra_list=("range_grid", "vertex_indices", [[0], [], [1], [2, 3]]))
    for mode in ("mesh", "cloud"):
        rc, lines = check(mode, path)
        head, V, T = _parse(lines)
        assert rc == 0 and head == [8, 0, 0] and np.array_equal(V, CUBE_V) and T == [], mode


def test_the_mesh_reader_refuses_a_negative_index(check, tmp_path):
    path = tmp_path / "neg.ply"
    mr.write_ply(path, CUBE_V, [[0, 1, 2], [3, -1, 2]])
    rc, lines = check("mesh", path)
    assert rc == 2 and lines[-1] == "REFUSED Error reading PLY file: face 1 has a vertex index outside [0, 2^32)"


def test_the_config_parser_reads_the_two_keys(check, tmp_path):
    def config(params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.ply"\nsource = "s.ply"\n[params]\nseed = 1\n{params}')
        rc, lines = check("config", tmp_path / "c.toml")
        return rc, lines[-1]
    assert config("") == (0, "MESH_POINTS 0 0")  # absent: off
    assert config("target_mesh_points = 20000\nsource_mesh_points = 500\n") == (0, "MESH_POINTS 20000 500")
    assert config("source_mesh_points = 300\n") == (0, "MESH_POINTS 0 300")
    assert config("target_mesh_points = 0\nsource_mesh_points = -7\n") == (0, "MESH_POINTS 0 0")
    assert config("target_mesh_points = 2000.0\n") == (0, "MESH_POINTS 2000 0")  # an integer however it is written
    for key in ("target_mesh_points", "source_mesh_points"):
        assert config(f"{key} = 2.5\n") == (2, f"REFUSED params.{key} must be an integer")
        for value in ('"many"', "true"):
            assert config(f"{key} = {value}\n") == (2, f"REFUSED params.{key} must be a number")
        rc, line = config(f"{key} = nan\n")
        assert rc == 2 and f"params.{key} must not be NaN" in line


def test_cli_refuses_a_mesh_key_on_a_file_that_holds_no_mesh(fg, tmp_path):
    """a TXT file and a PLY without faces end the run with exit code 1 and the key's name, before any device is asked for"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))
    mr.write_ply(tmp_path / "cloud.ply", pts, None)
    mr.write_ply(tmp_path / "cube.ply", CUBE_V, CUBE_POLYGONS)

    def run(target, source, extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/{target}"\nsource = "{tmp_path}/{source}"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    rc, log = run("c.txt", "c.txt", "target_mesh_points = 100\n")
    assert rc == 1 and "params.target_mesh_points = 100" in log and "is not a PLY file" in log
    rc, log = run("c.txt", "cloud.ply", "source_mesh_points = 100\n")
    assert rc == 1 and "params.source_mesh_points = 100" in log and "has no faces" in log
    rc, log = run("c.txt", "c.txt", "source_mesh_points = 2.5\n")
    assert rc == 1 and "params.source_mesh_points must be an integer" in log
    if not _has_gpu():
        rc, log = run("cube.ply", "c.txt", "target_mesh_points = 100\n")
        assert rc == 1 and "params.target_mesh_points = 100: status 2" in log and "no HIP device" in log
