"""Density clustering (fgoicp_cluster_dbscan) as far as it goes without a GPU: the symbol, the struct layout against the header, every refusal
of the definition (status 1 with a message: the checks run on the host, before any device work), a valid call, which on a machine without a
device returns FGOICP_ERR_NO_DEVICE (there is no CPU path), the six keys of the CLI's configuration, the CLI's refusals and the Python
wrapper's own checks.  The results are checked in tests/test_gpu_cluster.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
FIELDS = ["struct_size", "points", "core_points", "border_points", "noise_points", "clusters", "largest_label", "largest_size", "kept", "keep_min_size", "min_points",
          "eps2", "rounds"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _call(fg, xyz, n, eps=0.3, min_points=4, keep_min_size=0, device=0, info="full", want_out=True):
    """the raw call: returns (status, message, ClusterInfo)"""
    lib = fg._lib.load()
    L = fg._lib
    ci = L.ClusterInfo()
    if isinstance(info, int):
        ci.struct_size = info
    cap = 0 if xyz is None else len(xyz)
    out = np.empty((max(cap, 1), 3), np.float32) if want_out else None
    rc = lib.fgoicp_cluster_dbscan(None if xyz is None else xyz.ctypes.data_as(L.c_float_p), n, C.c_float(eps), min_points, keep_min_size, device,
                                   None if out is None else out.ctypes.data_as(L.c_float_p), cap, None, None, None, None, 0, None if info is None else C.byref(ci))
    return rc, lib.fgoicp_last_error().decode(), ci


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.random.default_rng(5).uniform(-1.0, 1.0, (200, 3)).astype(np.float32))


def test_the_library_exports_the_call_and_the_struct_is_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    assert hasattr(lib, "fgoicp_cluster_dbscan") and "fgoicp_cluster_dbscan" in fg._lib.exported_symbols()
    assert lib.fgoicp_abi_version() == 2
    assert callable(fg.cluster_dbscan)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu' + " %zu" * len(FIELDS)
                   + '\\n", sizeof(fgoicp_cluster_info_t), ' + ", ".join(f"offsetof(fgoicp_cluster_info_t, {f})" for f in FIELDS) + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    V = fg._lib.ClusterInfo
    assert [name for name, _ in V._fields_] == FIELDS
    assert got == [C.sizeof(V)] + [getattr(V, f).offset for f in FIELDS]
    assert got[0] == 96 and got[-1] == 88


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
    "zero eps": lambda p: dict(xyz=p, n=len(p), eps=0.0),
    "negative eps": lambda p: dict(xyz=p, n=len(p), eps=-0.5),
    "nan eps": lambda p: dict(xyz=p, n=len(p), eps=float("nan")),
    "infinite eps": lambda p: dict(xyz=p, n=len(p), eps=float("inf")),
    "min_points 0": lambda p: dict(xyz=p, n=len(p), min_points=0),
    "min_points negative": lambda p: dict(xyz=p, n=len(p), min_points=-3),
    "null info": lambda p: dict(xyz=p, n=len(p), info=None),
    "struct_size 0": lambda p: dict(xyz=p, n=len(p), info=0),
    "struct_size short": lambda p: dict(xyz=p, n=len(p), info=88),  # ends before rounds
    "struct_size 4097": lambda p: dict(xyz=p, n=len(p), info=4097),
    "negative device": lambda p: dict(xyz=p, n=len(p), device=-1),  # (an ordinal above the device count needs the count: tests/test_gpu_cluster.py)
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, cloud, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    rc, msg, _ = _call(fg, **REFUSALS[case](cloud))
    assert rc == INVALID_ARG and msg.startswith("fgoicp_cluster_dbscan: "), (case, rc, msg)
    if case == "nan coordinate":
        assert "point 17 " in msg
    if case == "infinite coordinate":
        assert "point 199 " in msg


def test_a_valid_call_without_a_device_reports_no_device(fg, cloud):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_cluster.py)"""
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(want_out=False), dict(min_points=1), dict(min_points=10 ** 6), dict(keep_min_size=50), dict(info=92), dict(info=4096), dict(eps=1e-30)):
        rc, msg, _ = _call(fg, cloud, len(cloud), **kw)
        assert rc == want and (msg.startswith("fgoicp_cluster_dbscan: ") or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.cluster_dbscan(cloud, 0.3)
        assert e.value.status == NO_DEVICE and "no CPU path" in str(e.value)
    for bad in (lambda: fg.cluster_dbscan(cloud, 0.0), lambda: fg.cluster_dbscan(cloud, 0.3, min_points=0)):  # the Python entry point passes the refusals on
        with pytest.raises(fg.FgoicpError) as e:
            bad()
        assert e.value.status == INVALID_ARG


def test_the_python_wrapper_checks_shapes_and_types_first(fg, cloud):
    with pytest.raises(ValueError):
        fg.cluster_dbscan(cloud[:, :2], 0.3)
    with pytest.raises(ValueError):
        fg.cluster_dbscan(cloud.reshape(-1), 0.3)
    with pytest.raises(ValueError):
        fg.cluster_dbscan(np.array([["a", "b", "c"]]), 0.3)
    for bad in (2.5, True, "4", None):
        with pytest.raises(TypeError):
            fg.cluster_dbscan(cloud, 0.3, min_points=bad)
    for bad in (2.5, False):
        with pytest.raises(TypeError):
            fg.cluster_dbscan(cloud, 0.3, keep_min_size=bad)
    with pytest.raises(ValueError):
        fg.cluster_dbscan(cloud, 0.3, keep_min_size=-1)


@pytest.fixture(scope="module")
def config_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cluster_config") / "cluster_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "cluster_config_check.cpp")], check=True)

    def run(tmp_path, params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.txt"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        p = subprocess.run([str(exe), str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=60)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(("CLUSTER ", "REFUSED "))]
        return p.returncode, line[-1] if line else p.stdout + p.stderr
    return run


KEYS = ("target_cluster_eps", "source_cluster_eps", "target_cluster_min_points", "source_cluster_min_points", "target_cluster_min_size", "source_cluster_min_size")


def test_the_config_parser_reads_the_six_keys(config_check, tmp_path):
    assert config_check(tmp_path, "") == (0, "CLUSTER 0 0 10 10 0 0")  # absent: off, 10 neighbours, the largest cluster
    assert config_check(tmp_path, "target_cluster_eps = 0.2\nsource_cluster_eps = 0.05\ntarget_cluster_min_points = 5\nsource_cluster_min_points = 1\n"
                        "target_cluster_min_size = 50\nsource_cluster_min_size = 1\n") == (0, "CLUSTER 0.200000003 0.0500000007 5 1 50 1")
    # eps <= 0 is "off" where the filter is applied; min_points is handed to the call as it stands (the call refuses < 1); a size <= 0 is 0
    assert config_check(tmp_path, "target_cluster_eps = -1\ntarget_cluster_min_points = 0\nsource_cluster_min_points = -4\ntarget_cluster_min_size = -2\n") == \
        (0, "CLUSTER -1 0 0 -4 0 0")
    for key in KEYS:
        for value in ('"many"', "true"):
            rc, line = config_check(tmp_path, f"{key} = {value}\n")
            assert rc == 2 and line == f"REFUSED params.{key} must be a number", (key, value, line)
        rc, line = config_check(tmp_path, f"{key} = nan\n")
        assert rc == 2 and f"params.{key} must not be NaN" in line
    for key in KEYS[2:]:
        rc, line = config_check(tmp_path, f"{key} = 2.5\n")
        assert rc == 2 and line == f"REFUSED params.{key} must be an integer"


def test_cli_reports_a_refused_filter(fg, tmp_path):
    """a value that is not a number is refused when the config is read, a parameter the call refuses when the cloud is filtered — after
    loading, before any solver exists — each with exit code 1 and a message naming the key"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))

    def run(extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/c.txt"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, p.stdout + p.stderr
    rc, log = run('target_cluster_eps = "0.2"\n')
    assert rc == 1 and "params.target_cluster_eps must be a number" in log
    rc, log = run("source_cluster_min_points = true\n")
    assert rc == 1 and "params.source_cluster_min_points must be a number" in log
    rc, log = run("target_cluster_eps = 0.2\ntarget_cluster_min_points = 0\n")
    assert rc == 1 and "params.target_cluster_eps = 0.2: status 1" in log and "min_points must be at least 1" in log
    rc, log = run("source_cluster_eps = inf\n")
    assert rc == 1 and "params.source_cluster_eps = inf: status 1" in log and "eps must be a positive finite number" in log
    if not _has_gpu():
        rc, log = run("source_cluster_eps = 0.2\n")
        assert rc == 1 and "params.source_cluster_eps" in log and "no HIP device" in log
        rc, log = run("source_cluster_eps = -1\ntarget_cluster_eps = 0\ntarget_cluster_min_points = 0\n")
        assert "Cluster filter" not in log and "_cluster_" not in log
