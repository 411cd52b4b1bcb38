"""Voxel-grid downsampling on the device (fgoicp_voxel_downsample, fg.voxel_downsample, params.source_voxel / params.target_voxel) against
the numpy restatement of its definition (include/fgoicp_amd.h): cells by the fp64 formula, rows in ascending key order, fp64 sums, one
rounding to fp32.

Rows, their order, counts and voxel_of_point must be EQUAL.  A centroid coordinate may differ from the restatement's by
    ulp32(ref) + count * 2^-52 * max|x|
(max|x| over the cell's members): the two sides add the same fp64 terms in different orders — each side's mean is within
(count - 1) * 2^-53 * max|x| of the exact one — and round to fp32 once, which moves a value by at most one fp32 step when the two fp64
means straddle a rounding boundary.

The segment paths by run length L (csrc/device/voxel.hip): L <= 64 one thread; 64 < L <= 4096 one wave; L > 4096 tiles of 4096 members,
one wave each, folded in tile order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, TOO_LARGE = 0, 5
THREAD_MAX, TILE = 64, 4096  # kVoxThreadMax, kVoxTile


def restate(p, v, origin=None):
    """(keys, voxel_of_point, counts, centroids fp32, per-row tolerance) of the definition, in numpy"""
    p = np.ascontiguousarray(p, np.float32)
    p64 = p.astype(np.float64)
    o = (p.min(0) if origin is None else np.asarray(origin, np.float32)).astype(np.float64)
    c = np.floor((p64 - o) / np.float64(np.float32(v))).astype(np.int64)
    assert c.min() >= 0 and c.max() < 2 ** 21
    keys = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(uk), 3), np.float64)
    np.add.at(sums, inv, p64)
    cen = (sums / cnt[:, None]).astype(np.float32)
    big = np.zeros(len(uk), np.float64)
    np.maximum.at(big, inv, np.abs(p64).max(1))
    tol = np.spacing(np.abs(cen)).astype(np.float64) + (cnt * 2.0 ** -52 * big)[:, None]
    return uk, inv.astype(np.uint32), cnt.astype(np.uint32), cen, tol


def check(fg, p, v, origin=None, label=""):
    """the call against the restatement; returns (out, voxel_of_point, counts, info, restatement)"""
    out, vop, cnt, info = fg.voxel_downsample(p, v, origin=origin, return_map=True)
    ref = restate(p, v, origin)
    uk, rvop, rcnt, rcen, tol = ref
    assert out.dtype == np.float32 and out.shape == (len(uk), 3), (label, out.shape, len(uk))
    assert info["points"] == len(p) and info["voxels"] == len(uk) and info["max_points_per_voxel"] == int(rcnt.max())
    assert np.array_equal(cnt, rcnt), label
    assert np.array_equal(vop, rvop), label
    dev = np.abs(out.astype(np.float64) - rcen.astype(np.float64))
    print(f"{label}: n {len(p)}, rows {len(uk)}, longest {int(rcnt.max())}, largest deviation / tolerance {float((dev / tol).max()):.3g}")
    assert np.all(dev <= tol), label
    want_o = np.asarray(p, np.float32).min(0) if origin is None else np.asarray(origin, np.float32)
    assert np.array_equal(info["origin"], want_o) and info["voxel_size"] == float(np.float32(v))
    return out, vop, cnt, info, ref


def cloud(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def voxel_for(n, per_cell):
    """edge of a grid over [-1, 1]^3 with about per_cell points per cell"""
    return 2.0 / max(n / per_cell, 1.0) ** (1.0 / 3.0) * 1.0001


# ---- equality with the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cell", [2, 100], ids=["sparse", "dense"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 20000])
def test_random_clouds_match_the_restatement(fg, gpu_required, n, per_cell):
    """sparse: thread rows; dense: n <= 64 one thread row, 65 one wave row, 1000 and 20 000 wave rows (up to about 130 points) next to thread rows"""
    check(fg, cloud(n, 100 + n), voxel_for(n, per_cell), label=f"n {n}, {per_cell} per cell")


def test_200k_points_cross_the_block_boundaries_of_sort_and_scan(fg, gpu_required):
    p = cloud(200_000, 9)
    check(fg, p, voxel_for(len(p), 2), label="200k sparse")
    check(fg, p, voxel_for(len(p), 100), origin=(-1.25, -1.5, -1.0), label="200k dense, given origin")


# ---- boundaries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["cloud minimum", "given origin"])
def test_points_on_cell_faces_land_in_the_cell_the_formula_names(fg, gpu_required, given):
    """v = 0.25; points exactly on o + j v fall into cell j, points one fp32 step below into cell j - 1.  (The origins are odd multiples
    of 0.125, so no face lies at 0, where one fp32 step below is a denormal that the fp64 subtraction rounds away: everywhere else p - o
    is exact in fp64.)"""
    v, o = 0.25, np.array([-2.125, -1.375, -3.125] if given else [-1.625, -1.625, -1.625], np.float32)
    rng = np.random.default_rng(3)
    j = rng.integers(1, 14, (400, 3))
    on = (o + j * np.float32(v)).astype(np.float32)
    assert np.array_equal(on.astype(np.float64), o.astype(np.float64) + j * 0.25) and np.all(on != 0)
    below = on.copy()
    pick = rng.integers(0, 3, len(on))
    below[np.arange(len(on)), pick] = np.nextafter(on[np.arange(len(on)), pick], np.float32(-np.inf))
    jb = j.copy()
    jb[np.arange(len(on)), pick] -= 1
    p = np.concatenate([o[None, :], on, below]).astype(np.float32)  # the first point is the origin itself: the cloud's minimum
    cells = np.concatenate([np.zeros((1, 3), np.int64), j, jb])
    out, vop, cnt, info, (uk, *_rest) = check(fg, p, v, origin=o if given else None, label=f"faces, given {given}")
    want = (cells[:, 2] << 42) | (cells[:, 1] << 21) | cells[:, 0]
    assert np.array_equal(uk[vop], want)


# ---- population extremes -------------------------------------------------------------------------------------------------------------
def one_cell(n, seed, lo=0.25, hi=0.5):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def test_5000_points_in_a_single_cell(fg, gpu_required):
    """L = 5000 > 4096: the tile path, two tiles (4096 + 904) and the fold; the whole cloud in one cell also sorts over a single bit"""
    p = one_cell(5000, 1)
    out, _, cnt, _, _ = check(fg, p, 1.0, origin=(0, 0, 0), label="5000 in one cell")
    assert len(out) == 1 and cnt[0] == 5000 > TILE


def test_55000_points_in_a_single_cell_next_to_shorter_rows(fg, gpu_required):
    """the 5000 plus 50 000 more in the same cell: 14 tiles (more than one block of the tile kernel, a last tile of 1752), next to a wave
    row of 700 points and thread rows"""
    p = np.concatenate([one_cell(5000, 1), one_cell(50_000, 2), one_cell(700, 3, 1.25, 1.5), cloud(300, 4) * 3.0 + 4.0]).astype(np.float32)
    p = p[np.random.default_rng(5).permutation(len(p))]
    _, _, cnt, _, _ = check(fg, p, 1.0, origin=(0, 0, 0), label="55000 in one cell")
    assert cnt.max() == 55_000 and np.any((cnt > THREAD_MAX) & (cnt <= TILE)) and np.any(cnt <= THREAD_MAX)


def test_rows_at_the_thresholds_between_the_paths(fg, gpu_required):
    """cells of 64 (the last thread row), 65 (the first wave row), 4096 (the last wave row), 4097 (two tiles, the second of one point)
    and 8192 (two full tiles)"""
    sizes = [THREAD_MAX, THREAD_MAX + 1, TILE, TILE + 1, 2 * TILE]
    p = np.concatenate([one_cell(m, 10 + k) + np.float32(k) for k, m in enumerate(sizes)]).astype(np.float32)
    p = p[np.random.default_rng(6).permutation(len(p))]
    _, _, cnt, _, _ = check(fg, p, 1.0, origin=(0, 0, 0), label="threshold rows")
    assert sorted(cnt.tolist()) == sizes


def test_every_point_in_a_cell_of_its_own(fg, gpu_required):
    """L = 1 everywhere: thread rows; a centroid of one point is that point"""
    g = np.stack(np.meshgrid(np.arange(17), np.arange(13), np.arange(11), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(8)
    p = ((g + rng.uniform(0.1, 0.9, g.shape)) * 0.5 - 3.0).astype(np.float32)
    p = p[rng.permutation(len(p))]
    out, vop, cnt, _, _ = check(fg, p, 0.5, origin=(-3, -3, -3), label="one point per cell")
    assert len(out) == len(p) and np.all(cnt == 1) and np.array_equal(out[vop], p)


def test_300_duplicates_of_a_point_have_that_point_as_centroid(fg, gpu_required):
    """a wave row (64 < 300 <= 4096) among thread rows: every partial sum k x, k <= 300, is exact in fp64 and 300 x / 300 = x, bit for bit"""
    x = np.array([0.3337, -0.7219, 0.1113], np.float32)
    others = cloud(900, 12)
    c = np.floor((others.astype(np.float64) + 1.0) / 0.125)
    cx = np.floor((x.astype(np.float64) + 1.0) / 0.125)
    others = others[np.any(c != cx, axis=1)]  # nobody else in the duplicates' cell
    p = np.concatenate([others, np.repeat(x[None, :], 300, 0)]).astype(np.float32)
    p = p[np.random.default_rng(13).permutation(len(p))]
    out, vop, cnt, _, _ = check(fg, p, 0.125, origin=(-1, -1, -1), label="300 duplicates")
    row = vop[np.flatnonzero(np.all(p == x, axis=1))[0]]
    assert cnt[row] == 300 and out[row].tobytes() == x.tobytes()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes_and_a_shuffled_cloud_the_same_rows(fg, gpu_required):
    p = np.concatenate([cloud(30_000, 21), one_cell(6000, 22), cloud(40, 23) + np.float32(5)]).astype(np.float32)  # wave rows, a tiled row, thread rows
    v = 0.5
    a = fg.voxel_downsample(p, v, return_map=True)
    b = fg.voxel_downsample(p, v, return_map=True)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[2].max() > TILE and np.any((a[2] > THREAD_MAX) & (a[2] <= TILE)) and np.any(a[2] <= THREAD_MAX)  # all three paths
    perm = np.random.default_rng(24).permutation(len(p))
    out2, vop2, cnt2, _ = fg.voxel_downsample(p[perm], v, return_map=True)
    *_, tol = restate(p, v)
    assert out2.shape == a[0].shape and np.array_equal(cnt2, a[2]) and np.array_equal(vop2, a[1][perm])
    assert np.all(np.abs(out2.astype(np.float64) - a[0].astype(np.float64)) <= tol)


# ---- capacity and struct_size --------------------------------------------------------------------------------------------------------
def test_capacity_count_only_and_a_short_struct(fg, gpu_required):
    lib = fg._lib.load()
    p = cloud(5000, 31)
    v = voxel_for(len(p), 2)
    voxels = len(restate(p, v)[0])
    f32 = lambda a: a.ctypes.data_as(fg._lib.c_float_p)
    u32 = lambda a: a.ctypes.data_as(fg._lib.c_uint32_p)
    # one row short: refused, the count reported, the arrays untouched
    out = np.full((voxels - 1, 3), 777.0, np.float32); vop = np.full(len(p), 0xDEADBEEF, np.uint32); cnt = np.full(voxels - 1, 0xDEADBEEF, np.uint32)
    vi = fg._lib.VoxelInfo()
    rc = lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, f32(out), voxels - 1, u32(vop), u32(cnt), C.byref(vi))
    assert rc == TOO_LARGE and lib.fgoicp_last_error() and vi.voxels == voxels and vi.points == len(p)
    assert np.all(out == 777.0) and np.all(vop == 0xDEADBEEF) and np.all(cnt == 0xDEADBEEF)
    rc = lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, None, voxels - 1, None, u32(cnt), C.byref(vi))  # the counts alone are sized too
    assert rc == TOO_LARGE and np.all(cnt == 0xDEADBEEF)
    # count only: no array at all, capacity 0
    vi = fg._lib.VoxelInfo()
    assert lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, None, 0, None, None, C.byref(vi)) == OK
    assert vi.voxels == voxels and vi.max_points_per_voxel == int(restate(p, v)[2].max())
    # ... and the map alone needs no capacity
    assert lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, None, 0, u32(vop), None, C.byref(vi)) == OK
    assert np.array_equal(vop, restate(p, v)[1])
    # exactly enough
    out = np.full((voxels, 3), 777.0, np.float32)
    assert lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, f32(out), voxels, None, None, C.byref(vi)) == OK
    assert np.array_equal(out, fg.voxel_downsample(p, v))
    # a struct_size that ends before `origin`: the members before it are filled, no byte behind it is written
    vi = fg._lib.VoxelInfo()
    vi.struct_size = fg._lib.VoxelInfo.origin.offset
    vi.origin[:] = [777.0, 777.0, 777.0]; vi.voxel_size = 777.0
    assert lib.fgoicp_voxel_downsample(f32(p), len(p), v, None, 0, None, 0, None, None, C.byref(vi)) == OK
    assert vi.struct_size == fg._lib.VoxelInfo.origin.offset and vi.voxels == voxels and vi.points == len(p) and vi.max_points_per_voxel > 0
    assert list(vi.origin) == [777.0] * 3 and vi.voxel_size == 777.0


# ---- independence --------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_an_open_registration_alone(fg, gpu_required, tiny_case):
    reg = fg.Registration(tiny_case["pct"], tiny_case["pcs"], tiny_case["bounds"], tiny_case["res"], device=0)
    rng = np.random.default_rng(0)
    tn = np.concatenate([rng.uniform(-0.5, 0.5, (32, 3)), np.full((32, 1), 0.25)], axis=1).astype(np.float32)
    rn = fg.RotNode(0.25, -0.125, 0.375, 0.125)
    lb, ub = reg.compute_sse_error(rn, tn, False)
    check(fg, cloud(20_000, 41), 0.2, label="next to a registration")
    lb2, ub2 = reg.compute_sse_error(rn, tn, False)
    assert lb.tobytes() == lb2.tobytes() and ub.tobytes() == ub2.tobytes()
    reg.close()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def test_cli_registers_the_thinned_clouds(fg, gpu_required, tmp_path):
    # The loader thins first: the reference caps params.source_subsample at 0.5, so with the default the CLI keeps half of the source file
    # (seeded, hence the same half in both runs), and the grid is laid over the cloud as loaded. The run without the keys goes first: its
    # alignment file holds the loaded source, which is what the run with the keys has to thin.
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    src = src[:600]
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    v = 0.01
    thin_tgt = fg.voxel_downsample(tgt, v)  # target_subsample is 1: the whole file is loaded
    assert 1 < len(thin_tgt) < len(tgt)
    loaded = thin_src = None
    for tag, extra in (("plain", ""), ("with", f"source_voxel = {v}\ntarget_voxel = {v}\n")):
        (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\nalignment = "{tmp_path}/{tag}_align.txt"\n'
                                              f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}.toml")], capture_output=True, text=True, timeout=300)
        log = p.stdout + p.stderr
        assert p.returncode == 0, log[-2000:]
        lines = (tmp_path / f"{tag}_align.txt").read_text().splitlines()
        points = int(lines[0].split("points = ")[1].split(",")[0])
        rows = np.loadtxt(lines[2:], ndmin=2)
        xyz = rows[:, :3].astype(np.float32)  # written at precision 9: the float32 reads back exactly
        assert points == len(rows)
        if tag == "plain":  # without the keys: no grid, the source as the loader leaves it, as today
            assert "Voxel grid" not in log, log[-2000:]
            assert f"Source point cloud ({points}) loaded" in log and f"Target point cloud ({len(tgt)}) loaded" in log, log[-2000:]
            assert points == len(src) // 2
            where = [int(np.flatnonzero(np.all(src == q, axis=1))[0]) for q in xyz]  # every row is a point of the file, in file order
            assert np.all(np.diff(where) > 0)
            assert np.all(rows[:, 3] < len(tgt))
            loaded = xyz
            thin_src = fg.voxel_downsample(loaded, v)
            assert 1 < len(thin_src) < len(loaded)
        else:
            assert f"Voxel grid (source): {len(loaded)} -> {len(thin_src)} points, voxel {v}" in log, log[-2000:]
            assert f"Voxel grid (target): {len(tgt)} -> {len(thin_tgt)} points, voxel {v}" in log, log[-2000:]
            assert points == len(thin_src)
            assert np.array_equal(xyz, thin_src)
            assert np.all(rows[:, 3] < len(thin_tgt)) and np.all(rows[:, 3] >= 0)
