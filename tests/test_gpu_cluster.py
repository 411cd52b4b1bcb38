"""Density clustering on the device (fgoicp_cluster_dbscan) against a numpy restatement written from the definition in
include/fgoicp_amd.h: the full fp32 d2 matrix (oracle.np_restatement.dist_sq, in row chunks), the components of the core points by a plain
stack over the boolean adjacency in ascending caller index (so the numbering is the defined one), a border point's cluster by the argmin of
the key (bits(d2) << 32) | index over its core neighbours.  Labels, neighbour counts, cluster sizes and kept indices are compared as
integers, the kept points as bytes, the counts of the info struct one by one.

A cloud of 2 points cannot hold a core, a border and a noise point at once, so the n = 2 wave-boundary case checks equality with the
restatement alone; the assertion that all three kinds occur holds for the clouds of 63 points and more."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
OK, INVALID_ARG, TOO_LARGE = 0, 1, 5
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def d2_rows(pts, rows):
    return npr.dist_sq(pts[rows][:, None, :], pts[None, :, :]).astype(f32)


def restate(pts, eps, min_points):
    """dict(eps2, neighbours, core, label, sizes) of the definition"""
    key = (pts.tobytes(), float(eps), int(min_points))
    if key in _CACHE:
        return _CACHE[key]
    n = len(pts)
    eps2 = f32(eps) * f32(eps)
    adj = np.empty((n, n), bool)
    for a in range(0, n, 256):
        adj[a:a + 256] = d2_rows(pts, np.arange(a, min(a + 256, n))) <= eps2
    neighbours = adj.sum(1).astype(np.uint32)
    core = neighbours >= min_points
    label = np.full(n, -1, np.int32)
    clusters = 0
    for i in range(n):  # ascending caller index: cluster c is the c-th in order of its lowest core index
        if not core[i] or label[i] >= 0:
            continue
        label[i] = clusters
        stack = [i]
        while stack:
            for j in np.flatnonzero(adj[stack.pop()] & core & (label < 0)):
                label[j] = clusters
                stack.append(j)
        clusters += 1
    col = np.arange(n, dtype=np.uint64)
    for i in np.flatnonzero(~core):
        cand = adj[i] & core
        if cand.any():
            keys = (_bits(d2_rows(pts, np.array([i]))[0]).astype(np.uint64) << np.uint64(32)) | col
            label[i] = label[np.flatnonzero(cand)[np.argmin(keys[cand])]]
    sizes = np.bincount(label[label >= 0], minlength=clusters).astype(np.uint64)
    _CACHE[key] = dict(eps2=eps2, neighbours=neighbours, core=core, label=label, sizes=sizes)
    return _CACHE[key]


def keep_mask(label, sizes, keep_min_size):
    if len(sizes) == 0:
        return np.zeros(len(label), bool)
    if keep_min_size == 0:
        return label == int(np.argmax(sizes))  # argmax: the first of equal sizes, the lowest label
    return (label >= 0) & (sizes[np.maximum(label, 0)] >= keep_min_size)


def check(fg, pts, eps, min_points, keep_min_size=0, ref=None):
    """one call against the restatement (or against `ref`, a dict of the same shape); returns the call's outputs"""
    ref = restate(pts, eps, min_points) if ref is None else ref
    kept, label, nbr, size, idx, info = fg.cluster_dbscan(pts, eps, min_points=min_points, keep_min_size=keep_min_size, return_map=True)
    n = len(pts)
    assert label.dtype == np.int32 and nbr.dtype == np.uint32 and size.dtype == np.uint64 and idx.dtype == np.uint32 and kept.dtype == f32
    assert np.array_equal(nbr, ref["neighbours"])
    assert np.array_equal(label, ref["label"])
    assert np.array_equal(size, ref["sizes"])
    keep = keep_mask(ref["label"], ref["sizes"], keep_min_size)
    assert np.array_equal(idx, np.flatnonzero(keep))
    assert kept.tobytes() == pts[keep].tobytes()
    core, lab = ref["core"], ref["label"]
    want = dict(points=n, core_points=int(core.sum()), border_points=int(((lab >= 0) & ~core).sum()), noise_points=int((lab < 0).sum()), clusters=len(ref["sizes"]),
                largest_label=int(np.argmax(ref["sizes"])) if len(ref["sizes"]) else -1, largest_size=int(ref["sizes"].max()) if len(ref["sizes"]) else 0,
                kept=int(keep.sum()), keep_min_size=keep_min_size, min_points=min_points)
    assert {k: info[k] for k in want} == want
    assert _bits(info["eps2"]) == _bits(ref["eps2"])
    assert info["rounds"] >= (1 if want["core_points"] else 0)
    return kept, label, nbr, size, idx, info


def uniform(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(f32))


def lattice():
    g = np.arange(12, dtype=f32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_one_point(fg, gpu_required):
    p = np.array([[0.25, -1.0, 3.0]], f32)
    kept, label, nbr, size, idx, info = check(fg, p, 0.5, 1)
    assert label[0] == 0 and nbr[0] == 1 and list(size) == [1] and info["clusters"] == 1 and info["kept"] == 1 and kept.tobytes() == p.tobytes()
    kept, label, nbr, size, idx, info = check(fg, p, 0.5, 2)
    assert label[0] == -1 and nbr[0] == 1 and len(size) == 0 and info["kept"] == 0 and kept.shape == (0, 3) and info["largest_label"] == -1 and info["rounds"] == 0


@pytest.mark.parametrize("n", [2, 63, 64, 65, 129])
def test_wave_boundaries(fg, gpu_required, n):
    """a partial wave, a full one, one lane over, three leaves.  eps = the square root of the median squared distance to the 4th neighbour (the
    point itself not counted; n = 2: to the only one), min_points = 5 (n = 2: 2): about half of the points are core"""
    pts = uniform(n, 50 + n)
    d2 = np.sort(d2_rows(pts, np.arange(n)), axis=1)
    eps = float(f32(np.sqrt(f64(np.median(d2[:, min(4, n - 1)])))))
    min_points = 5 if n > 2 else 2
    ref = restate(pts, eps, min_points)
    if n > 2:  # the test cannot pass empty (two points cannot be core, border and noise at once)
        assert ref["core"].any() and ((ref["label"] >= 0) & ~ref["core"]).any() and (ref["label"] < 0).any()
    for keep_min_size in (0, 1, 3):
        check(fg, pts, eps, min_points, keep_min_size)


def test_ties_at_eps2_on_the_lattice(fg, gpu_required):
    """d2 == eps2 exactly on every lattice edge: <= counts them"""
    pts = lattice()
    kept, label, nbr, size, idx, info = check(fg, pts, 1.0, 7)
    inner = np.all((pts >= 1) & (pts <= 10), axis=1)
    on_boundary = ((pts == 0) | (pts == 11)).sum(1)
    assert info["clusters"] == 1 and info["core_points"] == 1000 and info["border_points"] == 600 and info["noise_points"] == 128
    assert np.all(nbr[inner] == 7) and np.array_equal(label >= 0, on_boundary <= 1) and np.array_equal(label == -1, on_boundary >= 2)
    assert list(size) == [1600] and info["kept"] == 1600


def test_many_clusters_of_one_point(fg, gpu_required):
    pts = lattice()
    kept, label, nbr, size, idx, info = check(fg, pts, 0.99, 1)
    assert info["clusters"] == 1728 and np.array_equal(label, np.arange(1728)) and np.all(size == 1) and np.all(nbr == 1)
    assert info["largest_label"] == 0 and info["largest_size"] == 1 and info["kept"] == 1 and kept.tobytes() == pts[:1].tobytes()  # the tie goes to the lowest label
    assert check(fg, pts, 0.99, 1, keep_min_size=1)[5]["kept"] == 1728


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_long_chain(fg, gpu_required, order):
    """5000 collinear points one unit apart: the component of greatest diameter for its size"""
    n = 5000
    x = np.arange(n, dtype=f32)
    if order == "descending":
        x = x[::-1]
    if order == "shuffled":
        x = x[np.random.default_rng(7).permutation(n)]
    pts = np.ascontiguousarray(np.stack([x, np.zeros(n, f32), np.zeros(n, f32)], 1))
    ref = dict(eps2=f32(1.0), neighbours=np.where((x == 0) | (x == n - 1), 2, 3).astype(np.uint32), core=np.ones(n, bool), label=np.zeros(n, np.int32),
               sizes=np.array([n], np.uint64))  # (what restate() gives, without its 25 million distances)
    info = check(fg, pts, 1.0, 2, ref=ref)[5]
    print(f"chain of {n}, {order} caller order: {info['rounds']} rounds")
    assert info["clusters"] == 1 and info["kept"] == n


@pytest.mark.parametrize("variant", ["left first", "right first", "duplicates"])
def test_border_tie_between_two_clusters(fg, gpu_required, variant):
    """a dense run in [-1.5, -1], one in [1, 1.5], one point at 0, eps = 1, min_points = 5: the middle point is a border point (3 neighbours)
    with one core neighbour of each cluster at d2 == 1 and joins the cluster of the lower caller index, whichever side that lies on.
    duplicates: every point twice — pairs at d2 == 0 throughout, the middle point's twin a NON-core neighbour at d2 == 0 that must not
    decide, and a four-way tie at d2 == 1 (min_points = 7: the middle points have 6 neighbours)"""
    run = np.linspace(1.0, 1.5, 11).astype(f32)
    first, second = (run, -run) if variant == "right first" else (-run, run)
    x = np.concatenate([first, [0.0], second]).astype(f32)
    min_points, mid, sizes = 5, [11], [12, 11]
    if variant == "duplicates":
        x, min_points, mid, sizes = np.repeat(x, 2), 7, [22, 23], [24, 22]
    pts = np.ascontiguousarray(np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1))
    ref = restate(pts, 1.0, min_points)
    assert not ref["core"][mid].any() and np.all(ref["neighbours"][mid] == 3 * len(mid)) and ref["core"].sum() == len(x) - len(mid)
    assert len(ref["sizes"]) == 2 and np.all(ref["label"][mid] == 0)
    kept, label, nbr, size, idx, info = check(fg, pts, 1.0, min_points)
    assert np.all(label[mid] == 0) and list(size) == sizes and info["border_points"] == len(mid) and info["kept"] == sizes[0]


def planted_clumps():
    """the sphere and the strays of tests/test_gpu_outlier.py's planted cloud (seed 1), with two clumps outside the sphere in place of 25 of the
    40 strays: 2000 + 60 + 25 + 15 points, shuffled.  Returns (points, kind) with kind 0 = sphere, 1 = the 60-point clump, 2 = the 25-point one,
    3 = stray"""
    if "clumps" not in _CACHE:
        rng = np.random.default_rng(1)
        s = rng.normal(size=(2000, 3))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        extra = []
        while len(extra) < 40:
            p = rng.uniform(-3, 3, 3)
            if np.linalg.norm(p) > 1.5:
                extra.append(p)
        strays = np.array(extra)[:15]
        a = np.array([2.2, 0.4, -0.3]) + rng.normal(size=(60, 3)) * 0.06
        b = np.array([-0.5, -2.1, 0.9]) + rng.normal(size=(25, 3)) * 0.05
        pts = np.concatenate([s, a, b, strays]).astype(f32)
        kind = np.repeat([0, 1, 2, 3], [2000, 60, 25, 15])
        perm = rng.permutation(len(pts))
        _CACHE["clumps"] = (np.ascontiguousarray(pts[perm]), kind[perm])
    return _CACHE["clumps"]


def test_planted_clumps_are_removed_where_the_statistical_filter_keeps_them(fg, gpu_required):
    pts, kind = planted_clumps()
    assert len(pts) == 2100
    ref = restate(pts, 0.2, 10)
    assert sorted(ref["sizes"].tolist()) == [25, 60, 2000] and int((ref["label"] < 0).sum()) == 15 and int(((ref["label"] >= 0) & ~ref["core"]).sum()) == 4
    kept, label, nbr, size, idx, info = check(fg, pts, 0.2, 10)
    assert np.array_equal(idx, np.flatnonzero(kind == 0)) and info["kept"] == 2000 and info["clusters"] == 3 and info["noise_points"] == 15 and info["border_points"] == 4
    assert np.array_equal(label == -1, kind == 3)
    assert np.array_equal(check(fg, pts, 0.2, 10, keep_min_size=50)[4], np.flatnonzero(kind <= 1))  # 2060
    assert np.array_equal(check(fg, pts, 0.2, 10, keep_min_size=1)[4], np.flatnonzero(kind <= 2))  # 2085
    assert np.array_equal(fg.cluster_dbscan(pts, 0.2), kept)
    # the reason the feature exists: inside a clump the k nearest neighbours are close
    keep = fg.remove_statistical_outliers(pts, k=16, std_ratio=2.0, return_map=True)[1]
    assert np.all(keep[(kind == 1) | (kind == 2)]) and not np.any(keep[kind == 3]) and np.all(keep[kind == 0])


def blobs():
    if "blobs" not in _CACHE:
        rng = np.random.default_rng(11)
        centres = np.stack(np.meshgrid(np.arange(15.0), np.arange(20.0), np.arange(10.0), indexing="ij"), -1).reshape(-1, 3)
        pts = (np.repeat(centres, 100, axis=0) + rng.uniform(-0.05, 0.05, (300_000, 3))).astype(f32)
        blob = np.repeat(np.arange(3000), 100)
        perm = rng.permutation(len(pts))
        _CACHE["blobs"] = (np.ascontiguousarray(pts[perm]), blob[perm])
    return _CACHE["blobs"]


def test_scale_without_a_brute_force(fg, gpu_required):
    """300 000 points as 3000 blobs of 100 (each within +-0.05 of a centre, the centres one unit apart), shuffled: many waves, block rows of the
    scans, and 3000 roots to number.  The partition is the blob id by construction (a blob's diameter is below eps, the next blob is 0.9 away)."""
    pts, blob = blobs()
    n = len(pts)
    kept, label, nbr, size, idx, info = fg.cluster_dbscan(pts, 0.2, min_points=5, keep_min_size=0, return_map=True)
    assert info["clusters"] == 3000 and info["noise_points"] == 0 and info["border_points"] == 0 and info["core_points"] == n
    first = np.full(3000, n, np.int64)
    np.minimum.at(first, blob, np.arange(n))
    rank = np.empty(3000, np.int32)
    rank[np.argsort(first)] = np.arange(3000, dtype=np.int32)  # the blobs in order of their lowest caller index
    assert np.array_equal(label, rank[blob])
    assert np.all(size == 100) and info["largest_label"] == 0 and info["largest_size"] == 100 and info["kept"] == 100
    assert np.array_equal(idx, np.flatnonzero(label == 0)) and kept.tobytes() == pts[label == 0].tobytes()
    sample = np.sort(np.random.default_rng(12).choice(n, 200, replace=False))
    want = (d2_rows(pts, sample) <= f32(0.2) * f32(0.2)).sum(1)
    assert np.array_equal(nbr[sample], want) and np.all(nbr == 100)
    print(f"300k in 3000 blobs: {info['rounds']} rounds")
    info = fg.cluster_dbscan(pts, 0.2, min_points=5, keep_min_size=100, return_map=True)[5]
    assert info["kept"] == n


def test_two_calls_return_the_same_bytes(fg, gpu_required):
    """every array and every info field.  `rounds` is among them: it is the one field the definition does not fix (it counts passes of the
    device's connected-components loop), and it has been the same in every pair of calls measured; a difference here
    would be a finding about that loop, not about the labels."""
    pts, _ = planted_clumps()
    for keep_min_size in (0, 50):
        a = fg.cluster_dbscan(pts, 0.2, min_points=10, keep_min_size=keep_min_size, return_map=True)
        b = fg.cluster_dbscan(pts, 0.2, min_points=10, keep_min_size=keep_min_size, return_map=True)
        for x, y in zip(a[:5], b[:5]):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert a[5].keys() == b[5].keys() and all(np.float64(a[5][key]).tobytes() == np.float64(b[5][key]).tobytes() for key in a[5]), (a[5], b[5])


def _raw(fg, pts, eps, min_points, keep_min_size, capacity, capacity_clusters, arrays=True, fill=0xA5, device=0):
    lib = fg._lib.load()
    L = fg._lib
    n = len(pts)
    out = np.empty((max(capacity, 1), 3), f32)
    out.view(np.uint8)[...] = fill
    idx = np.full(max(capacity, 1), fill * 0x01010101, np.uint32)
    label = np.full(n, fill * 0x01010101, np.uint32).view(np.int32)
    nbr = np.full(n, fill * 0x01010101, np.uint32)
    size = np.full(max(capacity_clusters, 1), fill * 0x0101010101010101, np.uint64)
    info = L.ClusterInfo()
    ptr = lambda a, t: a.ctypes.data_as(t) if arrays else None
    rc = lib.fgoicp_cluster_dbscan(pts.ctypes.data_as(L.c_float_p), n, C.c_float(eps), min_points, keep_min_size, device, ptr(out, L.c_float_p), capacity, ptr(idx, L.c_uint32_p),
                                   ptr(label, C.POINTER(C.c_int32)), ptr(nbr, L.c_uint32_p), ptr(size, C.POINTER(C.c_uint64)), capacity_clusters, C.byref(info))
    return rc, info, out, idx, label, nbr, size


def test_capacity_and_count_only(fg, gpu_required):
    pts, _ = planted_clumps()
    ref = fg.cluster_dbscan(pts, 0.2, min_points=10, keep_min_size=50, return_map=True)
    kept = ref[5]["kept"]
    assert kept == 2060
    untouched = lambda *arrays: all(np.all(a.view(np.uint8) == 0xA5) for a in arrays)
    rc, info, out, idx, label, nbr, size = _raw(fg, pts, 0.2, 10, 50, kept - 1, 3)
    assert rc == TOO_LARGE and "capacity_points" in fg._lib.load().fgoicp_last_error().decode()
    assert (info.points, info.kept, info.clusters, info.noise_points, info.border_points, info.largest_size, info.largest_label) == (2100, kept, 3, 15, 4, 2000, ref[5]["largest_label"])
    assert (info.core_points, info.keep_min_size, info.min_points, info.rounds > 0) == (ref[5]["core_points"], 50, 10, True)
    assert untouched(out, idx, label, nbr, size)
    rc, info, out, idx, label, nbr, size = _raw(fg, pts, 0.2, 10, 50, kept, 3)  # exactly enough of both
    assert rc == OK and out[:kept].tobytes() == ref[0].tobytes() and np.array_equal(idx[:kept], ref[4])
    assert np.array_equal(label, ref[1]) and np.array_equal(nbr, ref[2]) and np.array_equal(size[:3], ref[3])
    rc, info, out, idx, label, nbr, size = _raw(fg, pts, 0.2, 10, 50, kept, 2)  # one cluster short
    assert rc == TOO_LARGE and "capacity_clusters" in fg._lib.load().fgoicp_last_error().decode() and info.clusters == 3 and info.kept == kept
    assert untouched(out, idx, label, nbr, size)
    rc, info, *_ = _raw(fg, pts, 0.2, 10, 0, 0, 0, arrays=False)  # all arrays NULL: the counts only
    assert rc == OK and (info.kept, info.clusters, info.noise_points) == (2000, 3, 15)
    rc, info, *_ = _raw(fg, pts, 0.2, 10, 0, 2100, 2100, device=99)  # an ordinal above the device count
    assert rc == INVALID_ARG and fg._lib.load().fgoicp_last_error().decode().startswith("fgoicp_cluster_dbscan: device ordinal")


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


def _run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines


def test_cli_registers_the_filtered_clouds(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts, kind = planted_clumps()
    order = np.argsort(kind != 0, kind="stable")  # the sphere first: a kept row's index is below 2000 exactly when the clumps and strays are gone
    pts = np.ascontiguousarray(pts[order])
    _write_txt(tmp_path / "tgt.txt", pts)
    _write_txt(tmp_path / "src.txt", pts[:600])  # the loader keeps about half of it
    want = "2100 -> 2000 points, eps 0.2, 10 neighbours: 3 clusters, 15 noise points, kept the largest"
    for tag, extra in (("plain", ""), ("with", "target_cluster_eps = 0.2\n")):
        rc, log = _run([exe, "-c", _config(tmp_path, tag, extra)])
        assert rc == 0, log[-2000:]
        rows = np.loadtxt((tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:], ndmin=2)
        line = [ln for ln in log.splitlines() if "Cluster filter" in ln]
        if tag == "plain":
            assert not line and np.all(rows[:, 3] < 2100)
        else:
            assert len(line) == 1 and line[0].endswith("Cluster filter (target): " + want), log[-2000:]
            assert len(rows) and np.all(rows[:, 3] < 2000) and np.all(rows[:, 3] >= 0)
    # --batch: each config is filtered with its own keys
    a = _config(tmp_path, "a", "target_cluster_eps = 0.2\n")
    b = _config(tmp_path, "b", "target_cluster_eps = 0.2\ntarget_cluster_min_points = 10\ntarget_cluster_min_size = 50\nsource_cluster_eps = 0.5\nsource_cluster_min_points = 3\n")
    (tmp_path / "list.txt").write_text(f"{os.path.basename(a)}\n{os.path.basename(b)}\n")
    rc, log = _run([exe, "--batch", str(tmp_path / "list.txt")])
    assert rc == 0, log[-2000:]
    lines = [ln.split("Cluster filter ")[1] for ln in log.splitlines() if "Cluster filter" in ln]
    assert len(lines) == 3, log[-2000:]
    assert lines[0] == "(target): " + want
    assert lines[1] == "(target): 2100 -> 2060 points, eps 0.2, 10 neighbours: 3 clusters, 15 noise points, kept 2 clusters of at least 50 points"
    assert lines[2].startswith("(source): ") and ", eps 0.5, 3 neighbours: " in lines[2] and lines[2].endswith("kept the largest")
    # the order against the other filters: the outlier filter first, the cluster filter starts from its count
    rc, log = _run([exe, "-c", _config(tmp_path, "both", "target_outlier_knn = 16\ntarget_cluster_eps = 0.2\n")])
    assert rc == 0, log[-2000:]
    lines = [ln for ln in log.splitlines() if "Outlier filter" in ln or "Cluster filter" in ln]
    assert len(lines) == 2 and "Outlier filter (target): 2100 -> 2085 points" in lines[0], lines
    assert lines[1].endswith("Cluster filter (target): 2085 -> 2000 points, eps 0.2, 10 neighbours: 3 clusters, 0 noise points, kept the largest"), lines
    # a filter that keeps no point ends the run
    rc, log = _run([exe, "-c", _config(tmp_path, "none", "target_cluster_eps = 0.2\ntarget_cluster_min_points = 5000\n")])
    assert rc == 1 and "params.target_cluster_eps = 0.2: the filter keeps no point" in log
