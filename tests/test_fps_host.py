"""Farthest-point sampling (fgoicp_farthest_point_sample) as far as it goes without a GPU: the symbol, the struct layout against the header,
every refusal of the definition (status 1 with a message: the checks run on the host, before any device work), a valid call, which on a
machine without a device returns FGOICP_ERR_NO_DEVICE (there is no CPU path), the two keys of the CLI's configuration and the Python
wrapper's own checks.  The results are checked in tests/test_gpu_fps.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
PREFIX = "fgoicp_farthest_point_sample: "


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _call(fg, xyz, n, m=10, start=0, info="full", want_out=True):
    """the raw call: returns (status, message, FpsInfo)"""
    lib = fg._lib.load()
    L = fg._lib
    fi = L.FpsInfo()
    if isinstance(info, int):
        fi.struct_size = info
    out = np.empty((max(min(m, 1 << 16), 1), 3), np.float32) if want_out else None  # (a refused m never writes a row)
    rc = lib.fgoicp_farthest_point_sample(None if xyz is None else xyz.ctypes.data_as(L.c_float_p), n, m, start, 0, None if out is None else out.ctypes.data_as(L.c_float_p),
                                          None, None, None, None, None if info is None else C.byref(fi))
    return rc, lib.fgoicp_last_error().decode(), fi


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.random.default_rng(5).uniform(-1.0, 1.0, (200, 3)).astype(np.float32))


def test_the_library_exports_the_call_and_the_struct_is_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    assert hasattr(lib, "fgoicp_farthest_point_sample") and "fgoicp_farthest_point_sample" in fg._lib.exported_symbols()
    assert "fgoicp_farthest_point_sample(" in open(os.path.join(REPO, "include", "fgoicp_amd.h")).read()
    for path in (fg.build.DEFAULT_LIB, fg.build.DEV_LIB):  # built into both libraries
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        assert " T fgoicp_farthest_point_sample\n" in syms, path
    assert lib.fgoicp_abi_version() == 2
    assert callable(fg.farthest_point_sample)
    fields = ["struct_size", "points", "samples", "start_index", "next_index", "cover_dist2"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(fgoicp_fps_info_t), '
                   + ", ".join(f"offsetof(fgoicp_fps_info_t, {f})" for f in fields) + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    V = fg._lib.FpsInfo
    assert got == [C.sizeof(V)] + [getattr(V, f).offset for f in fields]
    assert got == [48, 0, 8, 16, 24, 32, 40]


def _with(p, i, a, value):
    q = p.copy()
    q[i, a] = value
    return q


REFUSALS = {
    "null cloud": lambda p: dict(xyz=None, n=5, m=1),
    "no points": lambda p: dict(xyz=p, n=0, m=1),
    "2^31 points": lambda p: dict(xyz=p, n=2 ** 31, m=10),  # refused on the count alone: the array is not read
    "m = 0": lambda p: dict(xyz=p, n=len(p), m=0),
    "m above n": lambda p: dict(xyz=p, n=len(p), m=len(p) + 1),
    "m far above n": lambda p: dict(xyz=p, n=len(p), m=2 ** 40),
    "start_index = n": lambda p: dict(xyz=p, n=len(p), start=len(p)),
    "start_index far above n": lambda p: dict(xyz=p, n=len(p), start=2 ** 40),
    "nan coordinate": lambda p: dict(xyz=_with(p, 17, 1, np.nan), n=len(p)),
    "infinite coordinate": lambda p: dict(xyz=_with(p, 199, 2, -np.inf), n=len(p)),
    "null info": lambda p: dict(xyz=p, n=len(p), info=None),
    "struct_size 0": lambda p: dict(xyz=p, n=len(p), info=0),
    "struct_size short": lambda p: dict(xyz=p, n=len(p), info=32),  # ends before cover_dist2
    "struct_size above 4096": lambda p: dict(xyz=p, n=len(p), info=4097),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, cloud, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    rc, msg, _ = _call(fg, **REFUSALS[case](cloud))
    assert rc == INVALID_ARG and msg.startswith(PREFIX), (case, rc, msg)
    if case == "nan coordinate":
        assert "point 17 " in msg
    if case == "infinite coordinate":
        assert "point 199 " in msg


def test_a_valid_call_without_a_device_reports_no_device(fg, cloud):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_fps.py)"""
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(want_out=False), dict(m=1), dict(m=len(cloud)), dict(start=len(cloud) - 1), dict(info=40), dict(info=4096)):
        rc, msg, _ = _call(fg, cloud, len(cloud), **kw)
        assert rc == want and (msg.startswith(PREFIX) or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.farthest_point_sample(cloud, 10)
        assert e.value.status == NO_DEVICE


def test_the_python_wrapper_checks_shapes_types_and_ranges_first(fg, cloud):
    for bad in (cloud[:, :2], cloud.reshape(-1), np.array([["a", "b", "c"]])):
        with pytest.raises(ValueError):
            fg.farthest_point_sample(bad, 1)
    for m in (0, -1, len(cloud) + 1):
        with pytest.raises(ValueError):
            fg.farthest_point_sample(cloud, m)
    for s in (-1, len(cloud), 2 ** 40):
        with pytest.raises(ValueError):
            fg.farthest_point_sample(cloud, 10, start_index=s)
    with pytest.raises(ValueError):
        fg.farthest_point_sample(np.empty((0, 3), np.float32), 1)
    for m in (2.5, True, "3"):
        with pytest.raises(TypeError):
            fg.farthest_point_sample(cloud, m)
    with pytest.raises(TypeError):
        fg.farthest_point_sample(cloud, 10, start_index=1.0)
    with pytest.raises(fg.FgoicpError) as e:  # what the wrapper does not check itself, the call refuses
        fg.farthest_point_sample(_with(cloud, 3, 0, np.inf), 10)
    assert e.value.status == INVALID_ARG and "point 3 " in str(e.value)


@pytest.fixture(scope="module")
def config_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fps_config") / "fps_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "fps_config_check.cpp")], check=True)

    def run(tmp_path, params):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.txt"\nsource = "s.txt"\n[params]\nseed = 1\n{params}')
        p = subprocess.run([str(exe), str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=60)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(("POINTS ", "REFUSED "))]
        return p.returncode, line[-1] if line else p.stdout + p.stderr
    return run


def test_the_config_parser_reads_the_two_keys(config_check, tmp_path):
    assert config_check(tmp_path, "") == (0, "POINTS 0 0")  # absent: off
    assert config_check(tmp_path, "target_points = 5000\nsource_points = 1000\n") == (0, "POINTS 5000 1000")
    assert config_check(tmp_path, "source_points = 300\n") == (0, "POINTS 0 300")
    assert config_check(tmp_path, "target_points = 0\nsource_points = -7\n") == (0, "POINTS 0 0")
    assert config_check(tmp_path, "target_points = 2000.0\n") == (0, "POINTS 2000 0")  # an integer however it is written
    for key in ("target_points", "source_points"):
        rc, line = config_check(tmp_path, f"{key} = 2.5\n")
        assert rc == 2 and line == f"REFUSED params.{key} must be an integer", (key, line)
        for value in ('"many"', "true"):
            rc, line = config_check(tmp_path, f"{key} = {value}\n")
            assert rc == 2 and line == f"REFUSED params.{key} must be a number", (key, value, line)
        rc, line = config_check(tmp_path, f"{key} = nan\n")
        assert rc == 2 and f"params.{key} must not be NaN" in line


def test_cli_reports_a_refused_key_and_leaves_small_clouds_alone(fg, tmp_path):
    """a value that is not an integer is refused when the config is read, with exit code 1 and a message; a request at or above the cloud's
    size makes no call (without a device the run then gets as far as the solver)"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))

    def run(extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/c.txt"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    rc, log = run("source_points = 2.5\n")
    assert rc == 1 and "params.source_points must be an integer" in log
    rc, log = run('target_points = "100"\n')
    assert rc == 1 and "params.target_points must be a number" in log
    if not _has_gpu():
        rc, log = run("target_points = 20\n")
        assert rc == 1 and "params.target_points = 20: status 2" in log and "no HIP device" in log
        rc, log = run("target_points = 50\nsource_points = 1000\n")  # the target has 50 points, the loaded source fewer: neither call is made
        assert "params.target_points" not in log and "params.source_points" not in log and "fgoicp_solver_create" in log
