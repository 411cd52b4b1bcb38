"""Outlier removal on the device (fgoicp_remove_outliers) against a numpy restatement written from the definition in
include/fgoicp_amd.h: the keys (bits(fp32 dist_sq) << 32) | index by brute force over the whole cloud, mean_dist by an explicit left-to-right
loop over the k columns.  The mask is checked against the values the call itself reports, and those against the restatement: no check
depends on a point sitting near the threshold."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
OK, TOO_LARGE = 0, 5
STATISTICAL, RADIUS = 0, 1
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def brute_lists(pts, k, rows=None):
    """(kth_dist2 fp32, mean_dist fp64) of the definition for the points `rows` (None: all) of the cloud, keys formed in row chunks"""
    key = (pts.tobytes(), k, None if rows is None else rows.tobytes())
    if key not in _CACHE:
        n = len(pts)
        rows_ = np.arange(n) if rows is None else rows
        d2k = np.empty((len(rows_), k), f32)
        col = np.arange(n, dtype=np.uint64)[None, :]
        for a in range(0, len(rows_), 256):
            r = rows_[a:a + 256]
            d2 = npr.dist_sq(pts[r][:, None, :], pts[None, :, :]).astype(f32)
            keys = (_bits(d2).astype(np.uint64) << np.uint64(32)) | col
            keys = np.sort(keys, axis=1)[:, :k]
            d2k[a:a + 256] = (keys >> np.uint64(32)).astype(np.uint32).view(f32)
        root = np.sqrt(d2k.astype(f64))
        s = np.zeros(len(rows_), f64)
        for j in range(k):  # list order, left to right
            s = s + root[:, j]
        _CACHE[key] = (d2k[:, k - 1].copy(), s / f64(k))
    return _CACHE[key]


def uniform(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(f32))


def with_duplicates():
    rng = np.random.default_rng(21)
    p = rng.uniform(-1.0, 1.0, (2500, 3)).astype(f32)
    dst = rng.choice(2500, 64, replace=False)
    rest = np.setdiff1d(np.arange(2500), dst)
    p[dst] = p[rng.choice(rest, 64, replace=False)]
    return np.ascontiguousarray(p)


def lattice():
    g = np.arange(12, dtype=f32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


CLOUDS = {
    "n=k=2": (lambda: uniform(2, 2), 2),
    "n=k=32": (lambda: uniform(32, 3), 32),
    "n=33 k=32": (lambda: uniform(33, 4), 32),
    "n=63 k=8": (lambda: uniform(63, 5), 8),
    "n=64 k=8": (lambda: uniform(64, 6), 8),
    "n=65 k=8": (lambda: uniform(65, 7), 8),
    "n=129 k=8": (lambda: uniform(129, 8), 8),
    "duplicates k=4": (with_duplicates, 4),
    "duplicates k=16": (with_duplicates, 16),
    "duplicates k=32": (with_duplicates, 32),
    "lattice k=7": (lattice, 7),
    "lattice k=27": (lattice, 27),
    "uniform 6000 k=20": (lambda: uniform(6000, 9), 20),
}


def _cloud(name):
    make, k = CLOUDS[name]
    if ("cloud", name) not in _CACHE:
        _CACHE[("cloud", name)] = make()
    return _CACHE[("cloud", name)], k


def check_moments(m, info, n):
    """the reduction against math.fsum of the RETURNED mean_dist"""
    mean_ref = math.fsum(m) / n
    dev_mean = abs(info["mean"] - mean_ref)
    assert dev_mean <= n * 2.0 ** -53 * mean_ref, (dev_mean, mean_ref)
    std_ref = math.sqrt(math.fsum((m - mean_ref) ** 2) / (n - 1)) if n > 1 else 0.0
    dev_std = abs(info["stddev"] - std_ref)
    assert dev_std <= (n + 8) * 2.0 ** -52 * std_ref, (dev_std, std_ref)
    return dev_mean / mean_ref if mean_ref else 0.0, dev_std / std_ref if std_ref else 0.0


def check_statistical(pts, ret, std_ratio):
    kept, keep, idx, m, kth, info = ret
    n = len(pts)
    rel = check_moments(m, info, n)
    want = info["mean"] + float(f32(std_ratio)) * info["stddev"]
    assert abs(info["threshold"] - want) <= 2 * np.spacing(want)
    assert np.array_equal(keep, m <= info["threshold"])
    check_compaction(pts, kept, keep, idx, info)
    assert info["mode"] == STATISTICAL and info["radius2"] == 0.0 and info["points"] == n
    return rel


def check_compaction(pts, kept, keep, idx, info):
    assert kept.dtype == f32 and kept.tobytes() == pts[keep].tobytes()
    assert idx.dtype == np.uint32 and np.array_equal(idx, np.flatnonzero(keep))
    assert info["kept"] == int(keep.sum()) == len(kept)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_per_point_outputs_equal_the_restatement(fg, gpu_required, name):
    pts, k = _cloud(name)
    kth_ref, mean_ref = brute_lists(pts, k)
    _, _, _, m, kth, info = fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True)
    assert info["k"] == k
    assert _bits(kth).tobytes() == _bits(kth_ref).tobytes()
    dev = np.abs(m - mean_ref)
    print(f"{name}: largest |mean_dist - restatement| = {dev.max():.3e} ({(dev / np.spacing(mean_ref)).max():.1f} ulp), {int((dev != 0).sum())} of {len(pts)} differ")
    assert np.all(dev <= 2 * np.spacing(mean_ref))
    if name.startswith("lattice"):  # exact ties at the cut: the k-th distance is still that of the definition, e.g. 1 for an interior point at k = 7
        assert kth_ref[(5 * 12 + 5) * 12 + 5] == (1.0 if k == 7 else 3.0)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_statistical_mode(fg, gpu_required, name):
    pts, k = _cloud(name)
    ret = fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True)
    rel = check_statistical(pts, ret, 1.0)
    print(f"{name}: mean off by {rel[0]:.2e} relative, stddev by {rel[1]:.2e}; kept {ret[5]['kept']} of {len(pts)}")
    assert np.array_equal(fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0), ret[0])


@pytest.mark.parametrize("n", [2, 255, 256, 257, 1025])
def test_statistical_moments_have_the_bits_of_the_fixed_order(fg, gpu_required, n):
    """mean and stddev from the RETURNED mean_dist in the device's fixed order (oracle/np_restatement.py fixed_order_sum), bit for bit.
    n: one lane pair, a block less one lane, a block, a block and one lane, five blocks of which the last holds one point."""
    pts = uniform(n, 40 + n)
    _, _, _, m, _, info = fg.remove_statistical_outliers(pts, k=2, std_ratio=1.0, return_map=True)
    mean = npr.fixed_order_sum(m[:, None])[0] / f64(n)
    stddev = np.sqrt(npr.fixed_order_sum(((m - mean) * (m - mean))[:, None])[0] / f64(n - 1))
    got = np.array([info["mean"], info["stddev"]], f64)
    assert np.array_equal(got.view(np.uint64), np.array([mean, stddev], f64).view(np.uint64)), (got, mean, stddev)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_radius_mode(fg, gpu_required, name):
    pts, k = _cloud(name)
    kth_ref, _ = brute_lists(pts, k)
    r = f32(1.0) if name.startswith("lattice") else f32(np.sqrt(f64(np.median(kth_ref))))
    kept, keep, idx, m, kth, info = fg.remove_radius_outliers(pts, k, float(r), return_map=True)
    r2 = f32(r) * f32(r)
    assert info["mode"] == RADIUS and f32(info["radius2"]) == r2 and info["mean"] == info["stddev"] == info["threshold"] == 0.0
    assert _bits(kth).tobytes() == _bits(kth_ref).tobytes()
    assert np.array_equal(keep, kth_ref <= r2)
    check_compaction(pts, kept, keep, idx, info)
    if name == "lattice k=7":  # r = 1, r * r = 1 = the k-th squared distance of every interior point: <= keeps exactly those
        inner = np.all((pts >= 1) & (pts <= 10), axis=1)
        assert np.all(kth_ref[inner] == 1.0) and np.array_equal(keep, inner) and info["kept"] == 1000
    if name == "lattice k=27":
        assert info["kept"] == 0 and kept.shape == (0, 3)


def planted_cloud():
    if "planted" not in _CACHE:
        rng = np.random.default_rng(1)
        s = rng.normal(size=(2000, 3))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        extra = []
        while len(extra) < 40:
            p = rng.uniform(-3, 3, 3)
            if np.linalg.norm(p) > 1.5:
                extra.append(p)
        pts = np.concatenate([s, np.array(extra)]).astype(f32)
        perm = rng.permutation(len(pts))
        _CACHE["planted"] = (np.ascontiguousarray(pts[perm]), perm >= 2000)
    return _CACHE["planted"]


def test_planted_outliers_are_the_ones_removed(fg, gpu_required):
    pts, planted = planted_cloud()
    assert len(pts) == 2040 and planted.sum() == 40
    kth_ref, mean_ref = brute_lists(pts, 16)
    assert mean_ref[~planted].max() < 0.171 and mean_ref[planted].min() > 0.78  # the restatement: 0.170 and 0.785, threshold 0.644
    ret = fg.remove_statistical_outliers(pts, k=16, std_ratio=2.0, return_map=True)
    check_statistical(pts, ret, 2.0)
    assert abs(ret[5]["threshold"] - 0.644) < 1e-3
    assert np.array_equal(ret[1], ~planted) and ret[5]["kept"] == 2000
    kth8, _ = brute_lists(pts, 8)
    assert np.sqrt(kth8[~planted].max()) < 0.197 and np.sqrt(kth8[planted].min()) > 0.82  # 0.196 and 0.83
    kept, keep, idx, _, _, info = fg.remove_radius_outliers(pts, 8, 0.25, return_map=True)
    assert np.array_equal(keep, ~planted) and info["kept"] == 2000
    check_compaction(pts, kept, keep, idx, info)


def test_scale_without_a_brute_force(fg, gpu_required):
    """300 000 points: a fold over 1172 block rows and a scan over many blocks; the lists of a random sample against the whole cloud"""
    pts = uniform(300_000, 31)
    n, k = len(pts), 8
    ret = fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True)
    rel = check_statistical(pts, ret, 1.0)
    m, kth = ret[3], ret[4]
    assert np.all(m >= 0) and np.all(kth >= 0)
    assert 0 < ret[5]["kept"] < n
    sample = np.sort(np.random.default_rng(32).choice(n, 200, replace=False))
    kth_ref, mean_ref = brute_lists(pts, k, sample)
    assert _bits(kth[sample]).tobytes() == _bits(kth_ref).tobytes()
    dev = np.abs(m[sample] - mean_ref)
    print(f"300k: mean off by {rel[0]:.2e} relative, stddev by {rel[1]:.2e}; sample: largest |mean_dist - restatement| = {dev.max():.3e}")
    assert np.all(dev <= 2 * np.spacing(mean_ref))
    r = f32(np.sqrt(f64(np.median(kth))))
    kept, keep, idx, m2, kth2, info = fg.remove_radius_outliers(pts, k, float(r), return_map=True)
    assert m2.tobytes() == m.tobytes() and kth2.tobytes() == kth.tobytes()
    assert np.array_equal(keep, kth <= f32(r) * f32(r)) and 0 < info["kept"] < n
    check_compaction(pts, kept, keep, idx, info)


def test_two_calls_return_the_same_bytes(fg, gpu_required):
    pts, k = _cloud("uniform 6000 k=20")
    for call in (lambda: fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True),
                 lambda: fg.remove_radius_outliers(pts, k, 0.2, return_map=True)):
        a, b = call(), call()
        for x, y in zip(a[:5], b[:5]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert a[5].keys() == b[5].keys() and all(np.float64(a[5][key]).tobytes() == np.float64(b[5][key]).tobytes() for key in a[5])
        assert 0 < a[5]["kept"] < len(pts)


def _raw(fg, pts, mode, k, param, capacity, arrays=True, fill=0xA5):
    lib = fg._lib.load()
    L = fg._lib
    n = len(pts)
    cap = max(capacity, 1)
    out = np.full((cap, 3), np.nan, f32)
    out.view(np.uint8)[...] = fill
    idx = np.full(cap, fill * 0x01010101, np.uint32)
    keep = np.full(n, fill, np.uint8)
    m = np.full(n, -1.0, f64)
    kth = np.full(n, -1.0, f32)
    info = L.OutlierInfo()
    ptr = lambda a, t: a.ctypes.data_as(t) if arrays else None
    rc = lib.fgoicp_remove_outliers(pts.ctypes.data_as(L.c_float_p), n, mode, k, C.c_float(param), 0, ptr(out, L.c_float_p), capacity, ptr(idx, L.c_uint32_p),
                                    ptr(keep, L.c_uint8_p), ptr(m, L.c_double_p), ptr(kth, L.c_float_p), C.byref(info))
    return rc, info, out, idx, keep, m, kth


def test_capacity_and_count_only(fg, gpu_required):
    pts, k = _cloud("uniform 6000 k=20")
    ref = fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True)
    kept = ref[5]["kept"]
    assert 1 < kept < len(pts)
    rc, info, out, idx, keep, m, kth = _raw(fg, pts, STATISTICAL, k, 1.0, kept - 1)
    assert rc == TOO_LARGE and "capacity_points" in fg._lib.load().fgoicp_last_error().decode()
    assert (info.points, info.kept, info.mode, info.k) == (len(pts), kept, STATISTICAL, k)
    assert (info.mean, info.stddev, info.threshold) == (ref[5]["mean"], ref[5]["stddev"], ref[5]["threshold"])
    assert np.all(out.view(np.uint8) == 0xA5) and np.all(idx == 0xA5A5A5A5)  # untouched
    rc, info, out, idx, keep, m, kth = _raw(fg, pts, STATISTICAL, k, 1.0, kept)  # exactly enough
    assert rc == OK and out[:kept].tobytes() == ref[0].tobytes() and np.array_equal(idx[:kept], ref[2]) and np.array_equal(keep.astype(bool), ref[1])
    assert m.tobytes() == ref[3].tobytes() and kth.tobytes() == ref[4].tobytes()
    rc, info, *_ = _raw(fg, pts, STATISTICAL, k, 1.0, 0, arrays=False)  # all arrays NULL: the count only
    assert rc == OK and info.kept == kept and info.threshold == ref[5]["threshold"]
    rc, info, *_ = _raw(fg, pts, RADIUS, k, 0.2, 0, arrays=False)
    assert rc == OK and info.kept == fg.remove_radius_outliers(pts, k, 0.2, return_map=True)[5]["kept"]


def test_smallest_clouds(fg, gpu_required):
    with pytest.raises(fg.FgoicpError) as e:  # n = 1: k >= 2 > n
        fg.remove_statistical_outliers(np.zeros((1, 3), f32), k=2)
    assert e.value.status == 1
    pts = np.array([[0, 0, 0], [0.3, 0.4, 0]], f32)
    kept, keep, idx, m, kth, info = fg.remove_statistical_outliers(pts, k=2, std_ratio=0.0, return_map=True)
    assert m[0] == m[1] and info["stddev"] == 0.0 and info["mean"] == m[0] == info["threshold"]
    assert np.all(keep) and info["kept"] == 2 and kept.tobytes() == pts.tobytes()
    assert np.array_equal(kth, np.full(2, npr.dist_sq(pts[0], pts[1]), f32))


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def _config(tmp_path, tag, extra):
    (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\nalignment = "{tmp_path}/{tag}_align.txt"\n'
                                          f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.01\nseed = 3\n{extra}')
    return str(tmp_path / f"{tag}.toml")


def test_cli_registers_the_filtered_clouds(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts, planted = planted_cloud()
    _write_txt(tmp_path / "tgt.txt", pts)
    _write_txt(tmp_path / "src.txt", pts[~planted][:600])  # the loader keeps half of it
    thr = fg.remove_statistical_outliers(pts, k=16, std_ratio=2.0, return_map=True)[5]["threshold"]
    for tag, extra in (("plain", ""), ("with", "target_outlier_knn = 16\n")):
        p = subprocess.run([exe, "-c", _config(tmp_path, tag, extra)], capture_output=True, text=True, timeout=300)
        log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
        assert p.returncode == 0, log[-2000:]
        rows = np.loadtxt((tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:], ndmin=2)
        if tag == "plain":
            assert "Outlier filter" not in log, log[-2000:]
            assert np.all(rows[:, 3] < 2040)
        else:
            line = [ln for ln in log.splitlines() if "Outlier filter" in ln]
            assert len(line) == 1 and "Outlier filter (target): 2040 -> 2000 points, 16 neighbours, std ratio 2, threshold " in line[0], log[-2000:]
            assert abs(float(line[0].split("threshold ")[1]) - thr) <= 1e-5 * thr  # (printed at the stream's 6 digits)
            assert np.all(rows[:, 3] < 2000) and np.all(rows[:, 3] >= 0)
    # --batch: each config is filtered with its own parameters
    a = _config(tmp_path, "a", "target_outlier_knn = 16\ntarget_outlier_std = 2.0\n")
    b = _config(tmp_path, "b", "target_outlier_knn = 8\ntarget_outlier_radius = 0.25\nsource_outlier_knn = 4\nsource_outlier_std = 3.0\n")
    (tmp_path / "list.txt").write_text(f"{os.path.basename(a)}\n{os.path.basename(b)}\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    assert p.returncode == 0, log[-2000:]
    lines = [ln.split("Outlier filter ")[1] for ln in log.splitlines() if "Outlier filter" in ln]
    assert len(lines) == 3, log[-2000:]
    assert lines[0].startswith("(target): 2040 -> 2000 points, 16 neighbours, std ratio 2, threshold ")
    assert lines[1] == "(target): 2040 -> 2000 points, 8 neighbours, radius 0.25"
    assert lines[2].startswith("(source): 300 -> ") and ", 4 neighbours, std ratio 3, threshold " in lines[2]
    for tag in ("a", "b"):  # a batch writes each config's report: 2000-point indices only
        rows = np.loadtxt((tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:], ndmin=2)
        assert len(rows) and np.all(rows[:, 3] < 2000)
