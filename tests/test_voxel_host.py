"""Voxel-grid downsampling (fgoicp_voxel_downsample) as far as it goes without a GPU: the symbol, the struct layout against the header, every
refusal of the definition (status 1 with a message: the checks run on the host, before any device work), and a valid call, which on a
machine without a device returns FGOICP_ERR_NO_DEVICE (there is no CPU path).  The results are checked in tests/test_gpu_voxel.py."""
import ctypes as C

import numpy as np
import pytest

OK, INVALID_ARG, NO_DEVICE = 0, 1, 2


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _call(fg, xyz, n, v, origin=None, info="full", capacity=None, want_out=True):
    """the raw call: returns (status, message, VoxelInfo)"""
    lib = fg._lib.load()
    f32 = lambda a: None if a is None else a.ctypes.data_as(fg._lib.c_float_p)
    vi = fg._lib.VoxelInfo()
    if isinstance(info, int):
        vi.struct_size = info
    cap = (0 if xyz is None else len(xyz)) if capacity is None else capacity
    out = np.empty((max(cap, 1), 3), np.float32) if want_out else None
    rc = lib.fgoicp_voxel_downsample(f32(xyz), n, C.c_float(v), f32(origin), 0, f32(out), cap, None, None, None if info is None else C.byref(vi))
    return rc, lib.fgoicp_last_error().decode(), vi


@pytest.fixture(scope="module")
def cloud():
    return np.ascontiguousarray(np.random.default_rng(5).uniform(-1.0, 1.0, (200, 3)).astype(np.float32))


def test_the_library_exports_the_call_and_the_abi_revision_stays(fg):
    lib = fg._lib.load()
    assert hasattr(lib, "fgoicp_voxel_downsample") and "fgoicp_voxel_downsample" in fg._lib.exported_symbols()
    assert lib.fgoicp_abi_version() == 2
    assert callable(fg.voxel_downsample)
    # the struct as the header lays it out (x86-64): uint32 + padding, three uint64, four floats
    V = fg._lib.VoxelInfo
    assert (V.points.offset, V.voxels.offset, V.max_points_per_voxel.offset, V.origin.offset, V.voxel_size.offset, C.sizeof(V)) == (8, 16, 24, 32, 44, 48)


REFUSALS = {
    "null cloud": lambda p: dict(xyz=None, n=5, v=0.1),
    "no points": lambda p: dict(xyz=p, n=0, v=0.1),
    "2^31 points": lambda p: dict(xyz=p, n=2 ** 31, v=0.1),  # refused on the count alone: the array is not read
    "zero voxel": lambda p: dict(xyz=p, n=len(p), v=0.0),
    "negative voxel": lambda p: dict(xyz=p, n=len(p), v=-0.5),
    "nan voxel": lambda p: dict(xyz=p, n=len(p), v=float("nan")),
    "infinite voxel": lambda p: dict(xyz=p, n=len(p), v=float("inf")),
    "nan coordinate": lambda p: dict(xyz=_with(p, 17, 1, np.nan), n=len(p), v=0.1),
    "infinite coordinate": lambda p: dict(xyz=_with(p, 199, 2, -np.inf), n=len(p), v=0.1),
    "nan origin": lambda p: dict(xyz=p, n=len(p), v=0.1, origin=np.array([0, np.nan, 0], np.float32)),
    "infinite origin": lambda p: dict(xyz=p, n=len(p), v=0.1, origin=np.array([np.inf, 0, 0], np.float32)),
    "null info": lambda p: dict(xyz=p, n=len(p), v=0.1, info=None),
    "struct_size 0": lambda p: dict(xyz=p, n=len(p), v=0.1, info=0),
    "struct_size short": lambda p: dict(xyz=p, n=len(p), v=0.1, info=8),
    "point below the origin": lambda p: dict(xyz=p, n=len(p), v=0.1, origin=np.array([-1.0, -1.0, 0.5], np.float32)),
    "extent above 2^21 cells": lambda p: dict(xyz=p, n=len(p), v=1e-7),
}


def _with(p, i, a, value):
    q = p.copy()
    q[i, a] = value
    return q


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, cloud, case):
    rc, msg, _ = _call(fg, **REFUSALS[case](cloud))
    assert rc == INVALID_ARG and msg, (case, rc, msg)
    if case in ("point below the origin", "extent above 2^21 cells"):
        assert "voxel size is too small for the extent" in msg


def test_the_last_cell_of_an_axis_is_accepted_and_the_next_refused(fg):
    """c = 2^21 - 1 passes the host check (the call then goes to the device, or reports that there is none); c = 2^21 does not"""
    p = np.array([[0, 0, 0], [2.0 ** 21 - 1, 0, 0]], np.float32)
    rc, msg, _ = _call(fg, p, 2, 1.0)
    assert rc == (OK if _has_gpu() else NO_DEVICE), msg
    p[1, 0] = 2.0 ** 21
    rc, msg, _ = _call(fg, p, 2, 1.0)
    assert rc == INVALID_ARG and "voxel size is too small for the extent" in msg


def test_a_valid_call_without_a_device_reports_no_device(fg, cloud):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_voxel.py)"""
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(want_out=False), dict(origin=np.array([-1, -1, -1], np.float32))):
        rc, msg, _ = _call(fg, cloud, len(cloud), 0.1, **kw)
        assert rc == want and (msg or want == OK)
    if want == NO_DEVICE:
        with pytest.raises(fg.FgoicpError) as e:
            fg.voxel_downsample(cloud, 0.1)
        assert e.value.status == NO_DEVICE
    with pytest.raises(fg.FgoicpError) as e:  # the Python entry point passes the refusals on
        fg.voxel_downsample(cloud, -1.0)
    assert e.value.status == INVALID_ARG


def test_cli_reports_a_refused_voxel_size(fg, tmp_path):
    """params.source_voxel / params.target_voxel: NaN is refused when the config is read, a size the call refuses when the cloud is thinned —
    after loading, before any solver exists — each with exit code 1 and a message; absent or <= 0 the key is off (the run then goes on to
    the solver, which on a machine without a device fails there, not in the thinning)"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(np.float32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))

    def run(extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/c.txt"\nsource = "{tmp_path}/c.txt"\n[params]\nseed = 1\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=120)
        return p.returncode, p.stdout + p.stderr
    rc, log = run("source_voxel = nan\n")
    assert rc == 1 and "must not be NaN" in log
    rc, log = run("target_voxel = 1e-7\n")
    assert rc == 1 and "params.target_voxel" in log and "voxel size is too small for the extent" in log
    rc, log = run("source_voxel = inf\n")
    assert rc == 1 and "params.source_voxel" in log
    if not _has_gpu():
        rc, log = run("source_voxel = 0.5\n")
        assert rc == 1 and "params.source_voxel" in log and "no HIP device" in log
        rc, log = run("source_voxel = -1.0\ntarget_voxel = 0\n")
        assert "Voxel grid" not in log and "_voxel" not in log
