"""Plane segmentation (fgoicp_segment_planes, fgoicp_segment_hypotheses, fgoicp_segment_fit_from_moments) as far as it goes without a GPU:
the symbols, both struct layouts against the header, every refusal of the definition (status 1 with a message: the checks run on the host,
before any device work), a valid call, which on a machine without a device returns FGOICP_ERR_NO_DEVICE (there is no CPU path), the Python
wrapper's own checks, the two host halves — the hypothesis table against the numpy restatement of tests/segment_restatement.py to the bit,
the refit against numpy.linalg.eigh within the derived bound — the eight keys of the CLI's configuration and the CLI's refusals.  The device
half is checked in tests/test_gpu_segment.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import segment_restatement as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
f32, f64 = np.float32, np.float64
INFO_FIELDS = ["struct_size", "points", "planes", "on_planes", "kept", "iterations", "max_planes", "refit", "keep_planes", "min_inliers", "seed", "distance_threshold"]
MODEL_FIELDS = ["candidates", "sample", "hypothesis", "hypothesis_inliers", "inliers", "hypothesis_plane", "plane", "pivot", "sum_u", "sum_uu"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _call(fg, xyz, n, distance=0.05, iterations=64, seed=0, max_planes=1, min_inliers=0, refit=1, keep_planes=0, device=0, info="full", want_out=True, models=None,
          model_size=None):
    """the raw call: returns (status, message, SegmentInfo)"""
    lib = fg._lib.load()
    L = fg._lib
    si = L.SegmentInfo()
    if isinstance(info, int):
        si.struct_size = info
    cap = 0 if xyz is None else len(xyz)
    out = np.empty((max(cap, 1), 3), f32) if want_out else None
    mod = (L.SegmentModel * 16)() if models else None
    rc = lib.fgoicp_segment_planes(None if xyz is None else xyz.ctypes.data_as(L.c_float_p), n, C.c_float(distance), iterations, seed, max_planes, min_inliers, refit, keep_planes,
                                   device, None if out is None else out.ctypes.data_as(L.c_float_p), cap, None, None, mod, 16 if models else 0,
                                   C.sizeof(L.SegmentModel) if model_size is None else model_size, None if info is None else C.byref(si))
    return rc, lib.fgoicp_last_error().decode(), si


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.random.default_rng(5).uniform(-1.0, 1.0, (200, 3)).astype(f32))


def test_the_library_exports_the_calls_and_the_structs_are_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    for name in ("fgoicp_segment_planes", "fgoicp_segment_hypotheses", "fgoicp_segment_fit_from_moments"):
        assert hasattr(lib, name) and name in fg._lib.exported_symbols()
    assert lib.fgoicp_abi_version() == 2
    assert callable(fg.segment_planes) and callable(fg.segment_hypotheses) and callable(fg.segment_fit_from_moments)
    args = ", ".join(["sizeof(fgoicp_segment_info_t)"] + [f"offsetof(fgoicp_segment_info_t, {f})" for f in INFO_FIELDS] + ["sizeof(fgoicp_segment_model_t)"]
                     + [f"offsetof(fgoicp_segment_model_t, {f})" for f in MODEL_FIELDS])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu' + " %zu" * (len(INFO_FIELDS) + len(MODEL_FIELDS) + 1)
                   + '\\n", ' + args + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    V, M = fg._lib.SegmentInfo, fg._lib.SegmentModel
    assert [name for name, _ in V._fields_] == INFO_FIELDS and [name for name, _ in M._fields_] == MODEL_FIELDS
    assert got == [C.sizeof(V)] + [getattr(V, f).offset for f in INFO_FIELDS] + [C.sizeof(M)] + [getattr(M, f).offset for f in MODEL_FIELDS]
    assert got[0] == 80 and got[len(INFO_FIELDS)] == 72 and got[len(INFO_FIELDS) + 1] == 200 and got[-1] == 152


def _with(p, i, a, value):
    q = p.copy()
    q[i, a] = value
    return q


REFUSALS = {
    "null cloud": lambda p: dict(xyz=None, n=5),
    "no points": lambda p: dict(xyz=p, n=0),
    "2^31 points": lambda p: dict(xyz=p, n=2 ** 31),  # refused on the count alone: the array is not read
    "nan coordinate": lambda p: dict(xyz=_with(p, 17, 1, np.nan), n=len(p)),
    "infinite coordinate": lambda p: dict(xyz=_with(p, 199, 2, -np.inf), n=len(p)),
    "zero threshold": lambda p: dict(xyz=p, n=len(p), distance=0.0),
    "negative threshold": lambda p: dict(xyz=p, n=len(p), distance=-0.5),
    "nan threshold": lambda p: dict(xyz=p, n=len(p), distance=float("nan")),
    "infinite threshold": lambda p: dict(xyz=p, n=len(p), distance=float("inf")),
    "iterations 0": lambda p: dict(xyz=p, n=len(p), iterations=0),
    "iterations negative": lambda p: dict(xyz=p, n=len(p), iterations=-1),
    "iterations 65537": lambda p: dict(xyz=p, n=len(p), iterations=65537),
    "max_planes 0": lambda p: dict(xyz=p, n=len(p), max_planes=0),
    "max_planes negative": lambda p: dict(xyz=p, n=len(p), max_planes=-2),
    "max_planes 17": lambda p: dict(xyz=p, n=len(p), max_planes=17),
    "null info": lambda p: dict(xyz=p, n=len(p), info=None),
    "struct_size 0": lambda p: dict(xyz=p, n=len(p), info=0),
    "struct_size short": lambda p: dict(xyz=p, n=len(p), info=79),  # ends inside distance_threshold, the last member
    "struct_size 4097": lambda p: dict(xyz=p, n=len(p), info=4097),
    "model_size 0": lambda p: dict(xyz=p, n=len(p), models=True, model_size=0),
    "negative device": lambda p: dict(xyz=p, n=len(p), device=-1),  # (an ordinal above the device count needs the count: tests/test_gpu_segment.py)
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, cloud, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    rc, msg, _ = _call(fg, **REFUSALS[case](cloud))
    assert rc == INVALID_ARG and msg.startswith("fgoicp_segment_planes: "), (case, rc, msg)
    if case == "nan coordinate":
        assert "point 17 " in msg
    if case == "infinite coordinate":
        assert "point 199 " in msg


def test_a_valid_call_without_a_device_reports_no_device(fg, cloud):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_segment.py)"""
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(want_out=False), dict(iterations=1), dict(iterations=65536), dict(max_planes=16), dict(min_inliers=10 ** 9), dict(refit=0), dict(keep_planes=1),
               dict(seed=2 ** 64 - 1), dict(info=84), dict(info=4096), dict(models=True), dict(models=True, model_size=8), dict(distance=1e-30), dict(n=1), dict(n=2)):
        rc, msg, _ = _call(fg, cloud, **{"n": len(cloud), **kw})
        assert rc == want and (msg.startswith("fgoicp_segment_planes: ") or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.segment_planes(cloud, 0.05)
        assert e.value.status == NO_DEVICE and "no CPU path" in str(e.value)
    for bad in (lambda: fg.segment_planes(cloud, 0.0), lambda: fg.segment_planes(cloud, 0.05, iterations=0), lambda: fg.segment_planes(cloud, 0.05, max_planes=17)):
        with pytest.raises(fg.FgoicpError) as e:  # the Python entry point passes the refusals on
            bad()
        assert e.value.status == INVALID_ARG


def test_the_python_wrapper_checks_shapes_and_types_first(fg, cloud):
    with pytest.raises(ValueError):
        fg.segment_planes(cloud[:, :2], 0.05)
    with pytest.raises(ValueError):
        fg.segment_planes(cloud.reshape(-1), 0.05)
    with pytest.raises(ValueError):
        fg.segment_planes(np.array([["a", "b", "c"]]), 0.05)
    for name in ("iterations", "max_planes", "seed", "min_inliers"):
        for bad in (2.5, True, "4", None):
            with pytest.raises(TypeError):
                fg.segment_planes(cloud, 0.05, **{name: bad})
    for bad in ("all", "", None, 1):
        with pytest.raises(ValueError):
            fg.segment_planes(cloud, 0.05, keep=bad)
    with pytest.raises(ValueError):
        fg.segment_planes(cloud, 0.05, seed=-1)
    with pytest.raises(ValueError):
        fg.segment_planes(cloud, 0.05, min_inliers=-1)
    with pytest.raises(TypeError):
        fg.segment_hypotheses(cloud, 2.5)
    with pytest.raises(ValueError):
        fg.segment_hypotheses(cloud[:, :2], 4)


# ---- fgoicp_segment_hypotheses against the restatement ----

def _uniform(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(f32))


def _same_table(fg, P, K, seed=0, peel=0, cand=None):
    sample, plane, deg = fg.segment_hypotheses(P, K, seed=seed, peel=peel, candidates=cand)
    rs, rp, rd = sr.hypotheses(P, K, seed, peel, cand)
    assert sample.dtype == np.uint32 and plane.dtype == f64 and deg.dtype == bool
    assert np.array_equal(sample.astype(np.int64), rs)
    assert np.array_equal(deg, rd)
    assert plane.tobytes() == rp.tobytes()
    return rs, rp, rd


@pytest.mark.parametrize("n", [3, 4, 1000])
@pytest.mark.parametrize("peel", [0, 5])
@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1])
def test_hypotheses_equal_the_restatement(fg, n, peel, seed):
    P = _uniform(n, 11 + n)
    idx, plane, deg = _same_table(fg, P, 64, seed, peel)
    assert idx.min() >= 0 and idx.max() < n
    if n == 1000:
        assert not deg.all() and np.allclose(np.linalg.norm(plane[~deg, :3], axis=1), 1.0, atol=1e-15)


def test_hypotheses_of_a_proper_subset_draw_from_it_alone(fg):
    P = _uniform(1000, 3)
    cand = np.flatnonzero(np.random.default_rng(4).uniform(size=1000) < 0.3).astype(np.uint32)
    assert 3 < len(cand) < 1000
    for peel in (0, 5):
        idx, _, _ = _same_table(fg, P, 500, 9, peel, cand)
        assert np.isin(idx, cand).all()
    first, _, _ = sr.hypotheses(P, 500, 9, 0, cand)
    assert not np.array_equal(first, idx)  # another peel, other draws


def test_hypotheses_at_the_ends_of_the_iteration_range(fg):
    P = _uniform(1000, 8)
    _same_table(fg, P, 1, 5, 0)
    idx, _, deg = _same_table(fg, P, 65536, 5, 5)  # peel 5 of 65536: the counter passes 3 * 2^18
    assert len(np.unique(idx)) == 1000 and deg.mean() < 0.01


def test_hypotheses_of_degenerate_clouds_are_all_degenerate(fg):
    equal = np.ascontiguousarray(np.tile(np.array([[0.25, -1.5, 3.0]], f32), (50, 1)))
    _, plane, deg = _same_table(fg, equal, 64, 1, 0)
    assert deg.all() and not plane.any() and not np.signbit(plane).any()
    t = np.arange(50, dtype=f32)[:, None]
    line = np.ascontiguousarray(t * np.array([[1.0, 2.0, -0.5]], f32) + np.array([[4.0, 0.0, 1.0]], f32))  # exact in fp32: the cross products vanish exactly
    _, plane, deg = _same_table(fg, line, 64, 1, 0)
    assert deg.all() and not plane.any()


def test_three_points_give_degenerate_and_valid_hypotheses(fg):
    P = _uniform(3, 14)
    idx, _, deg = sr.hypotheses(P, 64, 0, 0)
    distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    assert 0 < distinct.sum() < 64 and np.array_equal(deg, ~distinct)  # (2/9 of the draws are three distinct indices; seed 0 gives 21 of 64)
    _same_table(fg, P, 64, 0, 0)


def test_hypotheses_refusals(fg, cloud):
    lib, L = fg._lib.load(), fg._lib
    fp = cloud.ctypes.data_as(L.c_float_p)
    cand = np.array([5, 3, 9], np.uint32)
    bad_cloud = _with(cloud, 17, 0, np.nan)
    for args in ((None, 200, None, 200, 4, 0, 0), (fp, 0, None, 0, 4, 0, 0), (fp, 200, None, 100, 4, 0, 0), (fp, 200, None, 200, 0, 0, 0), (fp, 200, None, 200, 65537, 0, 0),
                 (fp, 200, None, 200, 4, 0, -1), (fp, 200, None, 200, 4, 0, 16), (fp, 200, cand.ctypes.data_as(L.c_uint32_p), 3, 4, 0, 0),
                 (bad_cloud.ctypes.data_as(L.c_float_p), 200, None, 200, 4, 0, 0)):
        assert lib.fgoicp_segment_hypotheses(*args, None, None, None) == INVALID_ARG, args
        assert lib.fgoicp_last_error().decode().startswith("fgoicp_segment_hypotheses: ")
    assert lib.fgoicp_segment_hypotheses(fp, 200, None, 200, 4, 0, 0, None, None, None) == OK  # every output is optional


# ---- fgoicp_segment_fit_from_moments against numpy.linalg.eigh ----

def _patch(seed, normal, noise, n=600):
    """a noisy square patch with the given normal, somewhere off the origin"""
    rng = np.random.default_rng(seed)
    nv = np.asarray(normal, f64) / np.linalg.norm(normal)
    a = np.cross(nv, [0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    b = np.cross(nv, a)
    uv = rng.uniform(-1.0, 1.0, (n, 2))
    return np.ascontiguousarray((uv[:, :1] * a + uv[:, 1:] * b + noise * rng.normal(size=(n, 1)) * nv + [2.0, -1.0, 0.5]).astype(f32))


@pytest.mark.parametrize("case", [(1, (0, 0, 1), 0.002), (2, (1, 2, -3), 0.01), (3, (-1, 0.1, 0.2), 0.05), (4, (0, 1, 0), 0.0)])
def test_fit_from_moments_agrees_with_eigh(fg, case):
    seed, normal, noise = case
    P = _patch(seed, normal, noise)
    pivot = P[7].astype(f64)
    sum_u, sum_uu = sr.moments(P, np.ones(len(P), bool), pivot)
    for toward in (np.array([*normal, 0.0]), -np.array([*normal, 0.0]), None):
        ref, w = sr.fit_eigh(len(P), pivot, sum_u, sum_uu, toward)
        assert w[1] - w[0] >= 0.01 * w[2]  # the gap the bound needs: a square patch has two equal large eigenvalues and a small one
        bound = sr.fit_bound(w)
        assert bound < 1e-10
        got = fg.segment_fit_from_moments(len(P), pivot, sum_u, sum_uu, toward)
        assert got.dtype == f64 and abs(np.linalg.norm(got[:3]) - 1.0) < 1e-15
        if toward is None:
            ref = ref if ref[:3] @ got[:3] >= 0 else -ref
        else:
            assert got[:3] @ toward[:3] >= 0  # the sign follows toward
        err_n, err_d = 1.0 - abs(got[:3] @ ref[:3]), abs(got[3] - ref[3])
        print(f"case {seed}: 1 - |n.n_ref| = {err_n:.3e}, |d - d_ref| = {err_d:.3e}, bound {bound:.3e}")
        assert err_n <= bound and err_d <= bound
        assert np.abs(sr.residual(P, got)).max() <= 6.0 * noise + 1e-6  # and it is the patch's plane


def test_fit_from_moments_refusals(fg):
    lib = fg._lib.load()
    dp = lambda a: a.ctypes.data_as(fg._lib.c_double_p)
    piv, su, suu, out = np.zeros(3), np.array([1.0, 2.0, 0.0]), np.array([3.0, 0.5, 0.0, 4.0, 0.0, 0.0]), np.full(4, 7.0)
    msg = lambda: lib.fgoicp_last_error().decode()
    assert lib.fgoicp_segment_fit_from_moments(5, dp(piv), dp(su), dp(suu), None, dp(out)) == OK and out[2] != 7.0
    out[:] = 7.0
    for count in (0, 1, 2):
        assert lib.fgoicp_segment_fit_from_moments(count, dp(piv), dp(su), dp(suu), None, dp(out)) == INVALID_ARG and msg().startswith("fgoicp_segment_fit_from_moments: ")
    for bad in (np.nan, np.inf, -np.inf):
        for which, at in ((su, 1), (suu, 4), (piv, 0)):
            v = which.copy()
            v[at] = bad
            args = [dp(v) if x is which else dp(x) for x in (piv, su, suu)]
            assert lib.fgoicp_segment_fit_from_moments(5, *args, None, dp(out)) == INVALID_ARG and "finite" in msg()
    for args in ((None, dp(su), dp(suu), None, dp(out)), (dp(piv), None, dp(suu), None, dp(out)), (dp(piv), dp(su), None, None, dp(out)), (dp(piv), dp(su), dp(suu), None, None)):
        assert lib.fgoicp_segment_fit_from_moments(5, *args) == INVALID_ARG and "null" in msg()
    assert (out == 7.0).all()  # nothing written on refusal
    with pytest.raises(fg.FgoicpError):
        fg.segment_fit_from_moments(2, piv, su, suu)


# ---- the CLI ----

@pytest.fixture(scope="module")
def config_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("segment_config") / "segment_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "segment_config_check.cpp")], check=True)

    def run(tmp_path, params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.txt"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        p = subprocess.run([str(exe), str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=60)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(("SEGMENT ", "REFUSED "))]
        return p.returncode, line[-1] if line else p.stdout + p.stderr
    return run


KEYS = ("target_plane_distance", "source_plane_distance", "target_plane_min_fraction", "source_plane_min_fraction", "target_plane_iterations", "source_plane_iterations",
        "target_plane_count", "source_plane_count")


def test_the_config_parser_reads_the_eight_keys(config_check, tmp_path):
    assert config_check(tmp_path, "") == (0, "SEGMENT 0 0 1000 1000 1 1 0.10000000000000001 0.10000000000000001")  # absent: off, 1000 hypotheses, one plane, a tenth
    assert config_check(tmp_path, "target_plane_distance = 0.02\nsource_plane_distance = 0.5\ntarget_plane_iterations = 256\nsource_plane_iterations = 1\n"
                        "target_plane_count = 3\nsource_plane_count = 16\ntarget_plane_min_fraction = 0.25\nsource_plane_min_fraction = 0\n") == \
        (0, "SEGMENT 0.0199999996 0.5 256 1 3 16 0.25 0")
    # a distance <= 0 is "off" where the filter is applied; iterations and count are handed to the call as they stand (the call judges their range)
    assert config_check(tmp_path, "target_plane_distance = -1\ntarget_plane_iterations = 0\nsource_plane_count = -4\nsource_plane_min_fraction = -0.5\n") == \
        (0, "SEGMENT -1 0 0 1000 1 -4 0.10000000000000001 -0.5")
    for key in KEYS:
        for value in ('"many"', "true"):
            rc, line = config_check(tmp_path, f"{key} = {value}\n")
            assert rc == 2 and line == f"REFUSED params.{key} must be a number", (key, value, line)
        rc, line = config_check(tmp_path, f"{key} = nan\n")
        assert rc == 2 and f"params.{key} must not be NaN" in line
    for key in KEYS[4:]:
        rc, line = config_check(tmp_path, f"{key} = 2.5\n")
        assert rc == 2 and line == f"REFUSED params.{key} must be an integer"
    for key in KEYS[:4]:
        rc, line = config_check(tmp_path, f"{key} = 2.5\n")
        assert rc == 0


def test_cli_reports_a_refused_filter(fg, tmp_path):
    """a value that is not a number is refused when the config is read, a parameter the call refuses when the cloud is filtered — after
    loading, before any solver exists — each with exit code 1 and a message naming the key"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(f32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))

    def run(extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/c.txt"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, p.stdout + p.stderr
    rc, log = run('target_plane_distance = "0.02"\n')
    assert rc == 1 and "params.target_plane_distance must be a number" in log
    rc, log = run("source_plane_iterations = true\n")
    assert rc == 1 and "params.source_plane_iterations must be a number" in log
    rc, log = run("target_plane_distance = inf\n")
    assert rc == 1 and "params.target_plane_distance = inf: status 1" in log and "distance_threshold must be a positive finite number" in log
    rc, log = run("source_plane_distance = 0.02\nsource_plane_count = 0\n")
    assert rc == 1 and "params.source_plane_distance = 0.02: status 1" in log and "max_planes must lie in [1, 16]" in log
    if not _has_gpu():
        rc, log = run("source_plane_distance = 0.02\n")
        assert rc == 1 and "params.source_plane_distance" in log and "no HIP device" in log
        rc, log = run("source_plane_distance = -1\ntarget_plane_distance = 0\ntarget_plane_count = 0\n")
        assert "Plane filter" not in log and "_plane_" not in log
