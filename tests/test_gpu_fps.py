"""Farthest-point sampling on the device (fgoicp_farthest_point_sample, fg.farthest_point_sample, params.source_points / params.target_points)
against the numpy restatement of its definition (include/fgoicp_amd.h): an explicit loop over the m steps, the next pick by the largest
64-bit key (bits(D) << 32) | (0xFFFFFFFF - i), a picked point below everything.

Every comparison is EXACT: the outputs contain no sum.  To keep rounding out of it the clouds lie on the 2^-10 grid in [-1, 1] or are small
integers: dx, dy, dz are multiples of 2^-10 of magnitude <= 2, their squares multiples of 2^-20, and dx^2 + dy^2 + dz^2 <= 12 has at most
24 significant bits — every d2 is exact in fp32 whatever the order of operations (d2_grid asserts it against fp64), and ties are plentiful.
One case uses unrestricted floats and restates fma(dz, dz, fma(dy, dy, dx * dx)) with exact rationals, rounded once per operation.

The step kernel (csrc/device/fps.hip): blocks of 256 points, at most 1024 blocks — above 262 144 points a block loops over its slice."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
BLOCK, MAX_BLOCKS = 256, 1024  # kFpsBlock, kFpsMaxBlocks
PICKED = np.int64(np.float32(-1.0).view(np.int32)) << np.int64(32)  # the high word of a picked point's key


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def d2_grid(p, c):
    """dist_sq(p_i, p_c) for clouds whose every d2 is exact in fp32: the fp32 arithmetic, checked against fp64"""
    d = p - p[c]
    r = d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])
    d64 = p.astype(np.float64) - p[c].astype(np.float64)
    assert r.dtype == np.float32 and np.array_equal(r.astype(np.float64), (d64 * d64).sum(1))
    return r


def _round_f32(q):
    """the fp32 nearest to the non-negative rational q, ties to even (no overflow: the inputs are small)"""
    if q == 0:
        return np.float32(0.0)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1  # 2^e <= q < 2^(e + 1)
    e = max(e, -126)
    s = q / Fraction(2) ** (e - 23)
    k = s.numerator // s.denominator
    rem = s - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (k & 1)):
        k += 1
    return np.float32(math.ldexp(k, e - 23))


def d2_fma(p, c):
    """dist_sq for any floats: the differences in fp32 (one IEEE subtraction each), then dx * dx and the two fmas in exact rationals,
    each rounded to fp32 once"""
    d = p - p[c]
    out = np.empty(len(p), np.float32)
    for i, (dx, dy, dz) in enumerate(d):
        dx, dy, dz = Fraction(float(dx)), Fraction(float(dy)), Fraction(float(dz))
        a = Fraction(float(_round_f32(dx * dx)))
        a = Fraction(float(_round_f32(dy * dy + a)))
        out[i] = _round_f32(dz * dz + a)
    return out


def restate(p, m, start=0, d2=d2_grid):
    """(sample_index, pick_dist2, min_dist2, owner, next_index, cover_dist2) of the definition"""
    p = np.ascontiguousarray(p, np.float32)
    n = len(p)
    D = np.full(n, np.inf, np.float32)
    owner = np.zeros(n, np.uint32)
    picked = np.zeros(n, bool)
    idx, pick = np.empty(m, np.uint32), np.empty(m, np.float32)
    low = np.int64(0xFFFFFFFF) - np.arange(n, dtype=np.int64)
    c, dc = start, np.float32(np.inf)
    for t in range(m):
        idx[t], pick[t] = c, dc
        d = d2(p, c)
        lower = d < D
        D[lower] = d[lower]
        owner[lower] = t
        picked[c] = True
        key = np.where(picked, PICKED, D.view(np.int32).astype(np.int64) << np.int64(32)) | low
        w = int(np.argmax(key))  # the keys are distinct
        assert int(low[w]) == 0xFFFFFFFF - w
        if picked[w]:  # nothing is left
            assert t == n - 1
            c, dc = n, np.float32(0.0)
        else:
            c, dc = w, D[w]
    assert np.all(D[idx.astype(np.int64)] == 0)  # a sample's own distance
    return idx, pick, D, owner, c, dc


def grid_cloud(n, seed):
    return (np.random.default_rng(seed).integers(-1024, 1025, (n, 3)) / 1024.0).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(fg, p, m, start=0, d2=d2_grid, label=""):
    """the call against the restatement; returns the call's outputs"""
    p = np.ascontiguousarray(p, np.float32)
    out = fg.farthest_point_sample(p, m, start_index=start, return_map=True)
    xyz, idx, pick, mind, owner, info = out
    r_idx, r_pick, r_min, r_owner, r_next, r_cover = restate(p, m, start, d2)
    print(f"{label}: n {len(p)}, m {m}, start {start}, next {info['next_index']}, cover_dist2 {float(info['cover_dist2']):.9g}, "
          f"equal picks {int((idx == r_idx).sum())} / {m}")
    assert xyz.dtype == np.float32 and xyz.shape == (m, 3) and idx.dtype == np.uint32 and owner.dtype == np.uint32
    assert np.array_equal(idx, r_idx), label
    assert xyz.tobytes() == p[idx].tobytes(), label
    assert len(np.unique(idx)) == m and idx[0] == start
    assert np.array_equal(_bits(pick), _bits(r_pick)), label
    assert np.isposinf(pick[0]) and np.all(pick[:-1] >= pick[1:]) and np.all(pick >= 0), label  # non-increasing
    assert np.array_equal(_bits(mind), _bits(r_min)), label
    assert np.array_equal(owner, r_owner), label
    assert np.all(owner < m) and np.all(_bits(mind[idx]) == 0)  # +0.0 for a sample itself
    if d2 is d2_grid:  # the owner is a nearest sample: its distance is the minimum (every d2 of these clouds is exact)
        d = (p - p[idx[owner]]).astype(np.float64)
        assert np.array_equal((d * d).sum(1), mind.astype(np.float64)), label
    assert info["points"] == len(p) and info["samples"] == m and info["start_index"] == start
    assert info["next_index"] == r_next and _bits(info["cover_dist2"]) == _bits(r_cover), label
    assert _bits(info["cover_dist2"]) == _bits(mind.max())
    if m == len(p):
        assert info["next_index"] == len(p) and _bits(info["cover_dist2"]) == 0 and np.array_equal(np.sort(idx), np.arange(len(p)))
    else:
        nxt = info["next_index"]
        assert nxt not in set(idx.tolist()) and nxt == np.flatnonzero((mind == mind.max()) & ~np.isin(np.arange(len(p)), idx))[0]
    return out


# ---- equality with the restatement ---------------------------------------------------------------------------------------------------
def test_one_point_and_two_points(fg, gpu_required):
    check(fg, grid_cloud(1, 1), 1, label="n = m = 1")
    p = grid_cloud(2, 2)
    check(fg, p, 2, label="n = m = 2")
    check(fg, p, 2, start=1, label="n = m = 2 from the second")
    check(fg, p, 1, start=1, label="n = 2, m = 1")
    check(fg, np.repeat(p[:1], 2, 0), 2, label="two copies of a point")


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_the_full_permutation_at_the_block_edge(fg, gpu_required, n):
    """m = n: every point is picked, the last steps run over a cloud that is picked nearly everywhere"""
    check(fg, grid_cloud(n, 10 + n), n, label=f"permutation of {n}")


def test_copies_are_picked_last_in_ascending_index_order(fg, gpu_required):
    """2 500 points of which 64 are copies of others, m = n: once every distinct position holds a sample, D = 0 everywhere and the picks
    go on through the copies by index — none twice"""
    rng = np.random.default_rng(20)
    base = np.unique(rng.integers(-1024, 1025, (2600, 3)), axis=0)
    base = base[rng.permutation(len(base))[:2436]]
    p = np.concatenate([base, base[rng.choice(len(base), 64, replace=False)]])
    p = (p[rng.permutation(len(p))] / 1024.0).astype(np.float32)
    assert len(p) == 2500 and len(np.unique(p, axis=0)) == 2436
    xyz, idx, pick, *_ = check(fg, p, len(p), label="2500 with 64 copies")
    assert np.all(pick[:2436] > 0) and np.all(_bits(pick[2436:]) == 0)
    assert np.all(np.diff(idx[2436:].astype(np.int64)) > 0)
    assert len(np.unique(xyz[:2436], axis=0)) == 2436  # the copies' positions were all picked before


def test_the_integer_lattice_where_nearly_every_pick_is_a_tie(fg, gpu_required):
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    _, _, pick, *_ = check(fg, g, 200, label="12 x 12 x 12 lattice")
    assert len(np.unique(pick)) < len(pick)  # squared distances of a lattice are integers: picks share them, the index rule decides


@pytest.fixture(scope="module")
def cloud6000():
    return grid_cloud(6000, 30)


@pytest.mark.parametrize("start", [0, 2999, 5999])
def test_6000_points_from_three_start_indices(fg, gpu_required, cloud6000, start):
    check(fg, cloud6000, 500, start=start, label="6000 points")


def test_a_block_loops_over_its_slice_above_the_block_cap(fg, gpu_required):
    n = 300_000
    assert n > BLOCK * MAX_BLOCKS
    check(fg, grid_cloud(n, 40), 64, start=n - 1, label="300k points")


def test_unrestricted_floats_against_a_correctly_rounded_fma(fg, gpu_required):
    p = np.random.default_rng(50).uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    check(fg, p, 60, d2=d2_fma, label="uniform floats")


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_every_prefix_is_the_sampling_of_that_size(fg, gpu_required, cloud6000):
    long = fg.farthest_point_sample(cloud6000, 500, return_map=True)
    short = fg.farthest_point_sample(cloud6000, 100, return_map=True)
    assert short[0].tobytes() == long[0][:100].tobytes() and np.array_equal(short[1], long[1][:100]) and short[2].tobytes() == long[2][:100].tobytes()
    assert short[5]["next_index"] == long[1][100] and _bits(short[5]["cover_dist2"]) == _bits(long[2][100])
    assert fg.farthest_point_sample(cloud6000, 100).tobytes() == short[0].tobytes()  # without the maps


def test_two_calls_return_the_same_bytes(fg, gpu_required, cloud6000):
    a = fg.farthest_point_sample(cloud6000, 300, start_index=17, return_map=True)
    b = fg.farthest_point_sample(cloud6000, 300, start_index=17, return_map=True)
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()
    assert a[5]["next_index"] == b[5]["next_index"] and _bits(a[5]["cover_dist2"]) == _bits(b[5]["cover_dist2"])


def test_every_combination_of_null_outputs(fg, gpu_required):
    """the arrays that are given hold the same values whichever others are NULL (owner_n selects another instance of the step kernel);
    all NULL fills `out` alone; a struct_size that ends before cover_dist2 leaves it untouched"""
    lib, L = fg._lib.load(), fg._lib
    p = grid_cloud(1000, 60)
    m = 50
    full = fg.farthest_point_sample(p, m, start_index=3, return_map=True)
    types = (L.c_float_p, L.c_uint32_p, L.c_float_p, L.c_float_p, L.c_uint32_p)
    for given in itertools.product((False, True), repeat=5):
        arrs = [np.full_like(a, 7) if g else None for a, g in zip(full[:5], given)]
        fi = L.FpsInfo()
        rc = lib.fgoicp_farthest_point_sample(p.ctypes.data_as(L.c_float_p), len(p), m, 3, 0, *[None if a is None else a.ctypes.data_as(t) for a, t in zip(arrs, types)],
                                              C.byref(fi))
        assert rc == OK, (given, lib.fgoicp_last_error())
        for a, want in zip(arrs, full[:5]):
            assert a is None or a.tobytes() == want.tobytes(), given
        assert (fi.points, fi.samples, fi.start_index, fi.next_index) == (len(p), m, 3, full[5]["next_index"]) and _bits(fi.cover_dist2) == _bits(full[5]["cover_dist2"])
    fi = L.FpsInfo()
    fi.struct_size = L.FpsInfo.cover_dist2.offset
    fi.cover_dist2 = 777.0
    assert lib.fgoicp_farthest_point_sample(p.ctypes.data_as(L.c_float_p), len(p), m, 3, 0, None, None, None, None, None, C.byref(fi)) == OK
    assert fi.struct_size == L.FpsInfo.cover_dist2.offset and fi.next_index == full[5]["next_index"] and fi.cover_dist2 == 777.0


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def _config(tmp_path, tag, extra):
    path = tmp_path / f"{tag}.toml"
    path.write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\nalignment = "{tmp_path}/{tag}_align.txt"\noutput = "{tmp_path}/{tag}_out.toml"\n'
                    f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
    return str(path)


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    assert p.returncode == 0, log[-2000:]
    return log


def _align_rows(tmp_path, tag):
    rows = np.loadtxt((tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:], ndmin=2)
    return rows[:, :3].astype(np.float32), rows[:, 3].astype(np.int64)  # written at precision 9: the float32 reads back exactly


def _result(tmp_path, tag):
    """(R (3, 3), t (3,), sse) of io.output, float32 (written at precision 9)"""
    text = (tmp_path / f"{tag}_out.toml").read_text().split("[stats]")[0]
    nums = [np.float32(x) for x in re.findall(r"-?\d+\.?\d*(?:e[-+]?\d+)?", text.split("rotation = ")[1])]
    return np.array(nums[:9], np.float32).reshape(3, 3), np.array(nums[9:12], np.float32), nums[12]


def test_cli_registers_the_sampled_clouds(fg, gpu_required, tmp_path):
    # The loader thins first: the reference caps params.source_subsample at 0.5, so the CLI keeps half of the source file (seeded, hence the
    # same half in every run).  The run without the keys goes first: its alignment file holds the loaded source, which is what the run with
    # the keys has to sample.
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    log = _run(exe, "-c", _config(tmp_path, "plain", ""))
    assert "Farthest-point sampling" not in log, log[-2000:]
    loaded, _ = _align_rows(tmp_path, "plain")
    assert 300 < len(loaded) < len(src)  # (each point of the file is kept with probability 0.5)
    want, _, _, _, _, info = fg.farthest_point_sample(loaded, 300, return_map=True)
    log = _run(exe, "-c", _config(tmp_path, "with", f"source_points = 300\ntarget_points = {len(tgt) + 5}\n"))
    lines = [ln.split("Farthest-point sampling ")[1] for ln in log.splitlines() if "Farthest-point sampling" in ln]
    assert len(lines) == 2, log[-2000:]
    assert lines[0] == f"(target): {len(tgt)} points, at most {len(tgt) + 5} asked: unchanged"
    assert lines[1].startswith(f"(source): {len(loaded)} -> 300 points, cover radius ")
    radius = math.sqrt(float(info["cover_dist2"]))
    assert abs(float(lines[1].split("cover radius ")[1]) - radius) <= 1e-5 * radius  # (printed at the stream's 6 digits)
    xyz, corr = _align_rows(tmp_path, "with")
    assert xyz.tobytes() == want.tobytes()  # the sampled cloud in pick order
    # the library on the same clouds: the same registration and the same report
    s = fg.FastGoICP(tgt, want, 0.05, 0.001)
    R, t = s.run()
    a = s.alignment()
    Rc, tc, ec = _result(tmp_path, "with")
    assert np.array_equal(_bits(Rc), _bits(R)) and np.array_equal(_bits(tc), _bits(t)) and _bits(ec) == _bits(s.get_best_error())
    assert np.array_equal(corr, a.indices.astype(np.int64))
    s.close()
    # a request of exactly the cloud's size changes nothing either
    log = _run(exe, "-c", _config(tmp_path, "same", f"source_points = {len(loaded)}\n"))
    assert f"Farthest-point sampling (source): {len(loaded)} points, at most {len(loaded)} asked: unchanged" in log, log[-2000:]
    assert _align_rows(tmp_path, "same")[0].tobytes() == loaded.tobytes()
    # --batch: each config is sampled with its own count
    a = _config(tmp_path, "a", "source_points = 200\n")
    b = _config(tmp_path, "b", "source_points = 120\ntarget_points = 700\n")
    (tmp_path / "list.txt").write_text(f"{os.path.basename(a)}\n{os.path.basename(b)}\n")
    log = _run(exe, "--batch", str(tmp_path / "list.txt"))
    lines = [ln.split("Farthest-point sampling ")[1] for ln in log.splitlines() if "Farthest-point sampling" in ln]
    assert len(lines) == 3, log[-2000:]
    assert lines[0].startswith(f"(source): {len(loaded)} -> 200 points, cover radius ")
    assert lines[1].startswith(f"(target): {len(tgt)} -> 700 points, cover radius ")
    assert lines[2].startswith(f"(source): {len(loaded)} -> 120 points, cover radius ")
    assert _align_rows(tmp_path, "a")[0].tobytes() == want[:200].tobytes()  # a prefix of the longer sampling
    xyz, corr = _align_rows(tmp_path, "b")
    assert xyz.tobytes() == want[:120].tobytes() and np.all(corr < 700) and np.all(corr >= 0)
