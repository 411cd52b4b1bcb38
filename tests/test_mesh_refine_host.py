"""CPU: the host half of the point-to-mesh refinement — fgoicp_mesh_pair_terms against the numpy restatement of the
definition (tests/mesh_refine_restatement.py), bit for bit; the layout of the two structs from C; every refusal of the three calls that
needs no device; the CLI's parse of params.refine = "mesh"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_refine_restatement as rr
from tests import mesh_restatement as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
f32, f64 = np.float32, np.float64
LOSSES = (None, "huber", "cauchy", "geman_mcclure", "tukey")
GENERIC = np.array([[0.25, -0.5, 1.0], [2.0, 0.125, 1.5], [0.5, 1.75, 0.75]], f32)
EXACT = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]], f32)  # (1, 1, 0), (2, 0, 0) and a are closest points without rounding
MOMENTS_FIELDS = ["struct_size", "flags", "points", "correspondences", "m", "weight_sum", "sum_dist2", "max_dist2", "loss", "scale", "vertices", "triangles", "faces", "zero_area",
                  "tree_depth", "leaf_faces"]
RESULT_FIELDS = ["struct_size", "R", "t", "iterations", "rank", "points", "correspondences", "weight_sum", "mesh_rmse", "rms_distance", "loss", "scale_estimated", "loss_scale",
                 "triangles", "faces", "zero_area"]


def _bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def _same(got, want, label):
    for key in ("closest", "dist2", "g", "s", "w", "v"):
        assert np.array_equal(_bits(got[key]), _bits(np.asarray(want[key])[0])), (label, key, got[key], want[key])
    assert got["region"] == int(want["region"][0]), label


def seven_regions():
    """points over every region of GENERIC's plane — (u, v) of a + u ab + v ac — on the plane, above and below it"""
    a, b, c = GENERIC.astype(f64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    uv = [(0.3, 0.3), (0.5, -0.4), (0.8, 0.8), (-0.4, 0.5), (-0.5, -0.5), (1.6, -0.3), (-0.3, 1.6)]
    return np.array([a + u * (b - a) + v * (c - a) + h * n for u, v in uv for h in (0.0, 0.7, -1.3)]).astype(f32)


@pytest.mark.parametrize("loss", LOSSES)
def test_pair_terms_are_the_restatement_bit_for_bit(fg, loss):
    scale = None if loss is None else 0.4
    seen = set()
    for i, x in enumerate(seven_regions()):
        got = fg.mesh_pair_terms(x, *GENERIC, loss=loss, scale=scale)
        _same(got, rr.pair_terms(x, *GENERIC, loss=loss, scale=scale), (loss, i))
        seen.add(got["region"])
        if got["region"] != 0 and got["dist2"] > 0.0:  # the unit vector towards the point: s = |d| up to rounding
            assert abs(got["s"] - np.sqrt(got["dist2"])) <= 4 * np.spacing(np.sqrt(got["dist2"]))
        if loss is None:
            assert got["w"] == 1.0
    assert seen == set(range(7))


@pytest.mark.parametrize("loss", LOSSES)
def test_points_on_the_face_on_an_edge_and_on_a_vertex(fg, loss):
    """dist2 == 0: there is no direction to the point, the face normal serves in every region, and the residual is 0"""
    scale = None if loss is None else 0.4
    for x, region in (((1.0, 1.0, 0.0), 0), ((2.0, 0.0, 0.0), 1), ((0.0, 0.0, 0.0), 4), ((4.0, 0.0, 0.0), 5), ((0.0, 4.0, 0.0), 6), ((2.0, 2.0, 0.0), 2), ((0.0, 1.0, 0.0), 3)):
        got = fg.mesh_pair_terms(np.array(x, f32), *EXACT, loss=loss, scale=scale)
        _same(got, rr.pair_terms(np.array(x, f32), *EXACT, loss=loss, scale=scale), (loss, x))
        assert got["region"] == region and got["dist2"] == 0.0 and got["s"] == 0.0 and got["w"] == 1.0, x
        assert np.array_equal(got["g"], [0.0, 0.0, 1.0]) and np.array_equal(got["closest"], np.array(x, f64))
        assert np.array_equal(got["v"][21:], np.zeros(7))  # J^T s and s s
    above = fg.mesh_pair_terms(np.array((2.0, -3.0, 4.0), f32), *EXACT)  # off the edge ab: the direction is d / |d| = (0, -3, 4) / 5
    assert above["region"] == 1 and above["dist2"] == 25.0 and np.array_equal(above["g"], np.array([0.0, -3.0, 4.0]) / 5.0) and above["s"] == (-0.6 * -3.0 + 0.0) + 0.8 * 4.0


def test_the_terms_are_the_layout_of_the_plane_moments(fg):
    """v = the upper triangle of J J^T row by row, J s, s s, with J = [x cross g, g]: rebuilt here from the outputs g and s alone"""
    x = seven_regions()[4]
    got = fg.mesh_pair_terms(x, *GENERIC)
    X = x.astype(f64)
    J = np.concatenate([np.cross(X, got["g"]), got["g"]])
    want = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * got["s"] for a in range(6)] + [got["s"] * got["s"]]
    assert np.allclose(got["v"], want, rtol=1e-15, atol=0.0)
    weighted = fg.mesh_pair_terms(x, *GENERIC, loss="cauchy", scale=0.3)
    assert np.array_equal(_bits(weighted["v"]), _bits(got["v"] * weighted["w"])) and 0.0 < weighted["w"] < 1.0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_calls_and_the_structs_are_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    new = ("fgoicp_mesh_pair_terms", "fgoicp_mesh_moments", "fgoicp_mesh_refine")
    header = open(os.path.join(REPO, "include", "fgoicp_amd.h")).read()
    for name in new:
        assert hasattr(lib, name) and name in fg._lib.exported_symbols() and name + "(" in header
    for path in (fg.build.DEFAULT_LIB, fg.build.DEV_LIB):  # built into both libraries
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        for name in new:
            assert f" T {name}\n" in syms, (path, name)
    assert callable(fg.mesh_pair_terms) and callable(fg.mesh_moments) and callable(fg.refine_to_mesh)
    src = tmp_path / "layout.c"
    types = (("fgoicp_mesh_moments_t", MOMENTS_FIELDS), ("fgoicp_mesh_refine_result_t", RESULT_FIELDS))
    args = ", ".join(f"sizeof({t})" for t, _ in types) + ", " + ", ".join(f"offsetof({t}, {f})" for t, fields in types for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("' + "%zu " * (2 + len(MOMENTS_FIELDS) + len(RESULT_FIELDS))
                   + '\\n", ' + args + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    M, R = fg._lib.MeshMoments, fg._lib.MeshRefineResult
    assert got == [C.sizeof(M), C.sizeof(R)] + [getattr(M, f).offset for f in MOMENTS_FIELDS] + [getattr(R, f).offset for f in RESULT_FIELDS]
    assert lib.fgoicp_abi_version() == 2  # additions only


# ---- the refusals: all of these need no device ---------------------------------------------------------------------------------------------------
V0, T0 = mr.planted_mesh()
P0 = np.array([[0.5, 1.0, 1.5], [0.2, 0.3, 3.5], [2.0, 1.0, 1.0]], f32)
EYE = np.eye(3, dtype=f32).reshape(9)
ZERO = np.zeros(3, f32)


def _raw(fg, call, V=V0, T=T0, P=P0, R=EYE, t=ZERO, nv=None, nf=None, ns=None, max_distance=0.0, loss=0, scale=0.0, flags=0, out="full", conv_thr=1e-6):
    """(status, message) of fgoicp_mesh_moments / fgoicp_mesh_refine"""
    L = fg._lib
    lib = L.load()
    keep = [np.ascontiguousarray(a, f32) if a is not None else None for a in (V, P, R, t)]
    tri = None if T is None else np.ascontiguousarray(T, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(L.c_float_p)
    res = L.MeshMoments() if call == "fgoicp_mesh_moments" else L.MeshRefineResult()
    if isinstance(out, int):
        res.struct_size = out
    o = None if out is None else C.byref(res)
    head = (ptr(keep[0]), len(V) if nv is None else nv, None if tri is None else tri.ctypes.data_as(L.c_uint32_p), len(T) if nf is None else nf, ptr(keep[1]),
            len(P) if ns is None else ns, ptr(keep[2]), ptr(keep[3]))
    if call == "fgoicp_mesh_moments":
        rc = lib.fgoicp_mesh_moments(*head, max_distance, loss, scale, flags, 0, None, None, None, None, None, None, None, None, None, o)
    else:
        rc = lib.fgoicp_mesh_refine(*head, 3, conv_thr, max_distance, loss, scale, flags, 0, o)
    return rc, lib.fgoicp_last_error().decode()


def _bad(a, at, value):
    a = np.array(a, f32)
    a.reshape(-1)[at] = value
    return a


@pytest.mark.parametrize("call", ["fgoicp_mesh_moments", "fgoicp_mesh_refine"])
def test_every_refusal_names_its_call_and_needs_no_device(fg, call):
    big = 1 << 31
    bad_face = T0.copy()
    bad_face[3, 1] = len(V0)
    cases = [
        (dict(V=None, nv=1), "the vertices must not be null or empty"), (dict(nv=0), "the vertices must not be null or empty"),
        (dict(T=None, nf=1), "the triangles must not be null or empty"), (dict(nf=0), "the triangles must not be null or empty"),
        (dict(P=None, ns=1), "the points must not be null or empty"), (dict(ns=0), "the points must not be null or empty"),
        (dict(nv=big), "more than 2^31 - 1 vertices"), (dict(nf=big), "more than 2^31 - 1 triangles"), (dict(ns=big), "more than 2^31 - 1 points"),
        (dict(out=None), "out must not be null and out->struct_size = sizeof("), (dict(out=0), "out must not be null and out->struct_size = sizeof("),
        (dict(out=64), "out must not be null and out->struct_size = sizeof("), (dict(out=4097), "out must not be null and out->struct_size = sizeof("),
        (dict(flags=2), "unknown flag bits 2"), (dict(flags=5), "unknown flag bits 4"),
        (dict(R=None), "R9 and t3 must not be null"), (dict(t=None), "R9 and t3 must not be null"),
        (dict(R=_bad(EYE, 4, np.nan)), "the pose must be finite"), (dict(t=_bad(ZERO, 2, np.inf)), "the pose must be finite"),
        (dict(max_distance=float("nan")), "max_distance must be finite"), (dict(max_distance=float("inf")), "max_distance must be finite"),
        (dict(loss=-1), "unknown loss -1"), (dict(loss=5), "unknown loss 5"),
        (dict(loss=1, scale=float("nan")), "the scale must be finite"), (dict(loss=0, scale=float("inf")), "the scale must be finite"),
        (dict(V=_bad(V0, 3 * 7 + 1, np.nan)), "vertex 7 has a non-finite coordinate"), (dict(P=_bad(P0, 3 * 2, -np.inf)), "point 2 has a non-finite coordinate"),
        (dict(T=bad_face), f"face 3 has vertex index {len(V0)}: the mesh has {len(V0)} vertices"),
        (dict(R=EYE * f32(3e38), P=_bad(P0, 0, 3e38)), "the pose moves a point beyond the fp32 range"),
    ]
    if call == "fgoicp_mesh_moments":  # a loss needs its scale; the loop estimates one instead
        cases += [(dict(loss=4, scale=0.0), "the scale must be finite and > 0"), (dict(loss=2, scale=-1.0), "the scale must be finite and > 0")]
    else:
        cases += [(dict(conv_thr=float("nan")), "conv_thr must be finite"), (dict(conv_thr=float("inf")), "conv_thr must be finite")]
    for kwargs, message in cases:
        rc, text = _raw(fg, call, **kwargs)
        assert rc == INVALID_ARG and text.startswith(f"{call}: {message}"), (kwargs.keys(), rc, text)


def test_pair_terms_refusals(fg):
    L = fg._lib
    lib = L.load()
    x = np.array([0.1, 0.2, 0.3], f32)
    a, b, c = (np.ascontiguousarray(r) for r in GENERIC)
    p = lambda v: None if v is None else v.ctypes.data_as(L.c_float_p)
    w = C.c_double(-7.0)

    def call(x=x, a=a, b=b, c=c, loss=0, scale=0.0):
        rc = lib.fgoicp_mesh_pair_terms(p(x), p(a), p(b), p(c), loss, scale, None, None, None, None, None, C.byref(w), None)
        return rc, lib.fgoicp_last_error().decode()

    assert call()[0] == 0 and w.value == 1.0  # every other output NULL
    w.value = -7.0
    for kwargs, message in ((dict(x=None), "x3, a3, b3 and c3 must not be null"), (dict(c=None), "x3, a3, b3 and c3 must not be null"),
                            (dict(x=_bad(x, 1, np.nan)), "a coordinate is not finite"), (dict(b=_bad(b, 0, np.inf)), "a coordinate is not finite"),
                            (dict(loss=9), "unknown loss 9"), (dict(loss=1, scale=0.0), "the scale must be finite and > 0"),
                            (dict(loss=3, scale=float("inf")), "the scale must be finite and > 0"), (dict(b=a), "the triangle has no area")):
        rc, text = call(**kwargs)
        assert rc == INVALID_ARG and text == f"fgoicp_mesh_pair_terms: {message}", (kwargs.keys(), rc, text)
        assert w.value == -7.0  # a refusal writes nothing
    with pytest.raises(ValueError):
        fg.mesh_pair_terms(x, a, b, c, loss="l2")


# ---- params.refine = "mesh": the configuration key, the [refined] table, the fatal errors that need no device -------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mesh_refine_config") / "mesh_refine_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"), "-o", str(exe),
                    os.path.join(REPO, "tests", "host_harness", "mesh_refine_config_check.cpp")], check=True)

    def run(mode, path):
        p = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True, timeout=60)
        return p.returncode, [ln for ln in p.stdout.splitlines() if ln.startswith(("REFINE", "WRITTEN", "REFUSED"))]
    return run


def test_the_config_parser_reads_refine_mesh_and_ignores_the_normal_keys(harness, tmp_path):
    def config(params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.ply"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        rc, lines = harness("config", tmp_path / "c.toml")
        return rc, lines[-1]
    assert config('refine = "mesh"\n') == (0, "REFINE [mesh] KNN 16 MAX_ITER 30 DISTANCE 0 EPSILON 0.001 LOSS [none] 0 SCALE 0 DEVIATION []")
    # refine_knn and refine_epsilon are read and not checked: no normal is estimated ("plane" refuses the first, "gicp" both)
    assert config('refine = "mesh"\nrefine_knn = 2\nrefine_epsilon = 7.0\n') == (0, "REFINE [mesh] KNN 2 MAX_ITER 30 DISTANCE 0 EPSILON 7 LOSS [none] 0 SCALE 0 DEVIATION []")
    assert config('refine = "plane"\nrefine_knn = 2\n') == (2, "REFUSED params.refine_knn must lie in [4, 32]")
    assert config('refine = "mesh"\nrefine_max_iter = 5\nrefine_distance = 0.25\nrefine_loss = "tukey"\nrefine_loss_scale = 0.5\n') == (
        0, "REFINE [mesh] KNN 16 MAX_ITER 5 DISTANCE 0.25 EPSILON 0.001 LOSS [tukey] 4 SCALE 0.5 DEVIATION []")
    rc, line = config('refine = "meshes"\n')
    assert rc == 2 and line.startswith("REFUSED") and '"mesh"' in line and '"plane"' in line and '"gicp"' in line
    rc, line = config('refine_loss = "huber"\n')
    assert rc == 2 and line.startswith("REFUSED") and "params.refine" in line and '"mesh"' in line


def test_the_refined_table_of_a_mesh_refinement(harness, tmp_path):
    rc, lines = harness("write", tmp_path / "out.toml")
    assert (rc, lines) == (0, ["WRITTEN"])
    refined = (tmp_path / "out.toml").read_text().split("[refined]\n")[1].splitlines()
    assert refined[5:] == ["translation = [0.5, -0.25, 2]", "mesh_rmse = 0.125", "rms_distance = 0.25", "iterations = 4", "rank = 6", "correspondences = 600", 'loss = "tukey"',
                           "loss_scale = 0.75", "weight_sum = 480.5"]


def test_cli_refuses_refine_mesh_on_a_target_that_holds_no_mesh(fg, tmp_path):
    """a TXT target and a PLY without faces end the run with exit code 1 and the key's name, before any device is asked for; a mesh without
    area is refused by the call itself once a device is there (tests/test_gpu_mesh_refine.py)"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(f32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))
    mr.write_ply(tmp_path / "cloud.ply", pts, None)

    def run(target, batch=False):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/{target}"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\nrefine = "mesh"\n')
        (tmp_path / "list.txt").write_text("c.toml\n")
        args = ["--batch", str(tmp_path / "list.txt")] if batch else ["-c", str(tmp_path / "c.toml")]
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    for batch in (False, True):
        rc, log = run("c.txt", batch=batch)
        assert rc == 1 and 'params.refine = "mesh": the target' in log and "is not a PLY file" in log, log[-1000:]
        rc, log = run("cloud.ply", batch=batch)
        assert rc == 1 and 'params.refine = "mesh": the target' in log and "has no faces" in log, log[-1000:]
