"""Outlier removal (fgoicp_remove_outliers) as far as it goes without a GPU: the symbol, the struct layout against the header, every refusal
of the definition (status 1 with a message: the checks run on the host, before any device work), a valid call, which on a machine without a
device returns FGOICP_ERR_NO_DEVICE (there is no CPU path), the six keys of the CLI's configuration and the Python wrappers' own checks.
The results are checked in tests/test_gpu_outlier.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
STATISTICAL, RADIUS = 0, 1


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _call(fg, xyz, n, mode=STATISTICAL, k=8, param=2.0, info="full", want_out=True):
    """the raw call: returns (status, message, OutlierInfo)"""
    lib = fg._lib.load()
    L = fg._lib
    oi = L.OutlierInfo()
    if isinstance(info, int):
        oi.struct_size = info
    cap = 0 if xyz is None else len(xyz)
    out = np.empty((max(cap, 1), 3), np.float32) if want_out else None
    rc = lib.fgoicp_remove_outliers(None if xyz is None else xyz.ctypes.data_as(L.c_float_p), n, mode, k, C.c_float(param), 0,
                                    None if out is None else out.ctypes.data_as(L.c_float_p), cap, None, None, None, None, None if info is None else C.byref(oi))
    return rc, lib.fgoicp_last_error().decode(), oi


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.random.default_rng(5).uniform(-1.0, 1.0, (200, 3)).astype(np.float32))


def test_the_library_exports_the_call_and_the_struct_is_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    assert hasattr(lib, "fgoicp_remove_outliers") and "fgoicp_remove_outliers" in fg._lib.exported_symbols()
    assert lib.fgoicp_abi_version() == 2
    assert callable(fg.remove_statistical_outliers) and callable(fg.remove_radius_outliers)
    fields = ["struct_size", "points", "kept", "mode", "k", "mean", "stddev", "threshold", "radius2"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + ' %d %d\\n", sizeof(fgoicp_outlier_info_t), '
                   + ", ".join(f"offsetof(fgoicp_outlier_info_t, {f})" for f in fields) + ", (int)FGOICP_OUTLIER_STATISTICAL, (int)FGOICP_OUTLIER_RADIUS); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    V = fg._lib.OutlierInfo
    assert got == [C.sizeof(V)] + [getattr(V, f).offset for f in fields] + [fg._lib.OUTLIER_STATISTICAL, fg._lib.OUTLIER_RADIUS]
    assert got[:1] + got[-3:] == [64, 56, 0, 1]


def _with(p, i, a, value):
    q = p.copy()
    q[i, a] = value
    return q


REFUSALS = {
    "null cloud": lambda p: dict(xyz=None, n=5),
    "no points": lambda p: dict(xyz=p, n=0),
    "2^31 points": lambda p: dict(xyz=p, n=2 ** 31),  # refused on the count alone: the array is not read
    "unknown mode": lambda p: dict(xyz=p, n=len(p), mode=2),
    "negative mode": lambda p: dict(xyz=p, n=len(p), mode=-1),
    "k = 1": lambda p: dict(xyz=p, n=len(p), k=1),
    "k = 0": lambda p: dict(xyz=p, n=len(p), k=0),
    "k = 33": lambda p: dict(xyz=p, n=len(p), k=33),
    "k above n": lambda p: dict(xyz=p, n=7, k=8),
    "one point": lambda p: dict(xyz=p, n=1, k=2),
    "negative std_ratio": lambda p: dict(xyz=p, n=len(p), param=-0.5),
    "nan std_ratio": lambda p: dict(xyz=p, n=len(p), param=float("nan")),
    "infinite std_ratio": lambda p: dict(xyz=p, n=len(p), param=float("inf")),
    "zero radius": lambda p: dict(xyz=p, n=len(p), mode=RADIUS, param=0.0),
    "negative radius": lambda p: dict(xyz=p, n=len(p), mode=RADIUS, param=-1.0),
    "nan radius": lambda p: dict(xyz=p, n=len(p), mode=RADIUS, param=float("nan")),
    "infinite radius": lambda p: dict(xyz=p, n=len(p), mode=RADIUS, param=float("inf")),
    "nan coordinate": lambda p: dict(xyz=_with(p, 17, 1, np.nan), n=len(p)),
    "infinite coordinate": lambda p: dict(xyz=_with(p, 199, 2, -np.inf), n=len(p)),
    "null info": lambda p: dict(xyz=p, n=len(p), info=None),
    "struct_size 0": lambda p: dict(xyz=p, n=len(p), info=0),
    "struct_size short": lambda p: dict(xyz=p, n=len(p), info=48),  # ends before radius2
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, cloud, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    rc, msg, _ = _call(fg, **REFUSALS[case](cloud))
    assert rc == INVALID_ARG and msg.startswith("fgoicp_remove_outliers: "), (case, rc, msg)


def test_a_valid_call_without_a_device_reports_no_device(fg, cloud):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_outlier.py)"""
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(want_out=False), dict(mode=RADIUS, param=0.3), dict(param=0.0), dict(k=2), dict(k=32), dict(info=60)):
        rc, msg, _ = _call(fg, cloud, len(cloud), **kw)
        assert rc == want and (msg or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.remove_statistical_outliers(cloud)
        assert e.value.status == NO_DEVICE
    for bad in (lambda: fg.remove_statistical_outliers(cloud, k=1), lambda: fg.remove_radius_outliers(cloud, 8, 0.0)):  # the Python entry points pass the refusals on
        with pytest.raises(fg.FgoicpError) as e:
            bad()
        assert e.value.status == INVALID_ARG


def test_the_python_wrappers_check_shapes_and_types_first(fg, cloud):
    for call in (lambda p, k: fg.remove_statistical_outliers(p, k=k), lambda p, k: fg.remove_radius_outliers(p, k, 0.1)):
        with pytest.raises(ValueError):
            call(cloud[:, :2], 8)
        with pytest.raises(ValueError):
            call(cloud.reshape(-1), 8)
        with pytest.raises(ValueError):
            call(np.array([["a", "b", "c"]]), 8)
        with pytest.raises(TypeError):
            call(cloud, 2.5)
        with pytest.raises(TypeError):
            call(cloud, True)


@pytest.fixture(scope="module")
def config_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("outlier_config") / "outlier_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "outlier_config_check.cpp")], check=True)

    def run(tmp_path, params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.txt"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        p = subprocess.run([str(exe), str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=60)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(("OUTLIER ", "REFUSED "))]
        return p.returncode, line[-1] if line else p.stdout + p.stderr
    return run


def test_the_config_parser_reads_the_six_keys(config_check, tmp_path):
    assert config_check(tmp_path, "") == (0, "OUTLIER 0 0 2 2 0 0")  # absent: off, std ratio 2, no radius
    assert config_check(tmp_path, "target_outlier_knn = 16\nsource_outlier_knn = 20\ntarget_outlier_std = 1.5\nsource_outlier_std = 3\n"
                        "target_outlier_radius = 0.05\nsource_outlier_radius = 0.25\n") == (0, "OUTLIER 16 20 1.5 3 0.0500000007 0.25")
    assert config_check(tmp_path, "target_outlier_knn = -3\nsource_outlier_knn = 0\n") == (0, "OUTLIER 0 0 2 2 0 0")
    for key in ("target_outlier_knn", "source_outlier_knn", "target_outlier_std", "source_outlier_std", "target_outlier_radius", "source_outlier_radius"):
        for value in ('"many"', "true"):
            rc, line = config_check(tmp_path, f"{key} = {value}\n")
            assert rc == 2 and line == f"REFUSED params.{key} must be a number", (key, value, line)
        rc, line = config_check(tmp_path, f"{key} = nan\n")
        assert rc == 2 and f"params.{key} must not be NaN" in line


def test_cli_reports_a_refused_filter(fg, tmp_path):
    """a value that is not a number is refused when the config is read, a parameter the call refuses when the cloud is filtered — after
    loading, before any solver exists — each with exit code 1 and a message"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))

    def run(extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/c.txt"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, p.stdout + p.stderr
    rc, log = run('target_outlier_knn = "16"\n')
    assert rc == 1 and "params.target_outlier_knn must be a number" in log
    rc, log = run("target_outlier_knn = 40\n")
    assert rc == 1 and "params.target_outlier_knn = 40: status 1" in log and "k must lie in [2, 32]" in log
    rc, log = run("source_outlier_knn = 8\nsource_outlier_std = -1.0\n")
    assert rc == 1 and "params.source_outlier_knn = 8: status 1" in log and "std_ratio" in log
    if not _has_gpu():
        rc, log = run("source_outlier_knn = 8\n")
        assert rc == 1 and "params.source_outlier_knn" in log and "no HIP device" in log
        rc, log = run("source_outlier_knn = -1\ntarget_outlier_knn = 0\ntarget_outlier_radius = 0.5\n")
        assert "Outlier filter" not in log and "_outlier_" not in log
