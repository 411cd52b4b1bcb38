"""Plane segmentation on the device (fgoicp_segment_planes) against the numpy restatement of
tests/segment_restatement.py, written from the definition in include/fgoicp_amd.h.  Labels, counts, samples and the winning hypothesis are
compared as integers; hypothesis planes, pivots, sums, kept points and the threshold as bytes.  The refit's eigenvector is the one step
numpy cannot restate to the bit: the final inlier sets are compared against the restatement evaluated with the RETURNED plane doubles, and
the returned plane against the restatement's own numpy.linalg.eigh within the derived bound 1e3 * 2^-52 * lambda_max / (lambda_1 - lambda_0).

The call returns the winner of every peel, not the count of every hypothesis; the restatement forms the whole count vector (every
hypothesis against every candidate, in row chunks) and takes its first maximum, so a wrong count of any hypothesis that would change the
winner, its count or its inlier set fails the comparison."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import segment_restatement as sr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
OK, INVALID_ARG, TOO_LARGE = 0, 1, 5
TILE, CHUNK = 1024, 256  # the scoring kernel's points per block and hypotheses per staged chunk (fg.SEGMENT_TILE, fg.SEGMENT_CHUNK: asserted below)
MODEL_INTS = ("candidates", "hypothesis", "hypothesis_inliers", "inliers")
MODEL_BYTES = ("hypothesis_plane", "pivot", "sum_u", "sum_uu")
_CACHE = {}


def _bytes64(a):
    return np.ascontiguousarray(a, f64).tobytes()


def check(fg, P, T, K, seed=0, max_planes=1, min_inliers=0, refit=True, keep="rest"):
    """one call against the restatement; returns (the call's outputs, the restatement)"""
    kept, label, idx, models, info = fg.segment_planes(P, T, iterations=K, seed=seed, max_planes=max_planes, min_inliers=min_inliers, refit=refit, keep=keep, return_map=True)
    ref = sr.segment(P, T, K, seed, max_planes, min_inliers, refit, final_planes=[m["plane"] for m in models])
    n = len(P)
    assert kept.dtype == f32 and label.dtype == np.int32 and idx.dtype == np.uint32
    assert len(models) == len(ref["models"]), (len(models), len(ref["models"]))
    for j, (m, r) in enumerate(zip(models, ref["models"])):
        for key in MODEL_INTS:
            assert m[key] == r[key], (j, key, m[key], r[key])
        assert np.array_equal(m["sample"], r["sample"]), (j, m["sample"], r["sample"])
        for key in MODEL_BYTES:
            assert _bytes64(m[key]) == _bytes64(r[key]), (j, key, m[key], r[key])
        if refit:
            w = r["eigenvalues"]
            bound = sr.fit_bound(w)
            err_n, err_d = 1.0 - abs(m["plane"][:3] @ r["eigh_plane"][:3]), abs(m["plane"][3] - r["eigh_plane"][3])
            print(f"plane {j}: {m['inliers']} inliers, 1 - |n.n_ref| = {err_n:.3e}, |d - d_ref| = {err_d:.3e}, bound {bound:.3e}, eigenvalues {w}")
            assert m["plane"][:3] @ m["hypothesis_plane"][:3] >= 0.0
            if w[1] - w[0] >= 0.01 * w[2]:  # the gap the bound is derived for; three points, or a thin strip of a cube, may have none
                assert err_n <= bound and err_d <= bound, (j, err_n, err_d, bound)
        else:
            assert _bytes64(m["plane"]) == _bytes64(m["hypothesis_plane"]) and m["inliers"] == m["hypothesis_inliers"]
            assert not m["sum_u"].any() and not m["sum_uu"].any()
    assert np.array_equal(label, ref["label"])
    keep_mask = (ref["label"] >= 0) if keep == "planes" else (ref["label"] < 0)
    assert np.array_equal(idx, np.flatnonzero(keep_mask))
    assert kept.tobytes() == P[keep_mask].tobytes()
    want = dict(points=n, planes=len(ref["models"]), on_planes=int((ref["label"] >= 0).sum()), kept=int(keep_mask.sum()), iterations=K, max_planes=max_planes,
                refit=int(bool(refit)), keep_planes=int(keep == "planes"), min_inliers=min_inliers, seed=seed)
    assert {k: info[k] for k in want} == want
    assert _bytes64(info["distance_threshold"]) == _bytes64(f64(f32(T)))
    return (kept, label, idx, models, info), ref


def uniform(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(f32))


def median_threshold(P, K, seed):
    """T = the median |r| under hypothesis 0 (as the float the call takes): about half of the cloud within it"""
    _, plane, deg = sr.hypotheses(P, K, seed, 0)
    assert not deg[0]
    return f32(np.median(np.abs(sr.residual(P, plane[0]))))


def planted():
    """the scene of the README: a sphere (kind 0) on a table (1) with a clump lying on the table (2), shuffled"""
    if "planted" not in _CACHE:
        rng = np.random.default_rng(1)
        s = rng.normal(size=(2000, 3))
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        tab = np.stack([rng.uniform(-2, 2, 3000), rng.uniform(-2, 2, 3000), -1 + rng.normal(size=3000) * 0.002], 1)
        cl = np.array([1.5, 1.2, -0.9]) + rng.normal(size=(60, 3)) * 0.04
        P = np.concatenate([s, tab, cl]).astype(f32)
        kind = np.repeat([0, 1, 2], [2000, 3000, 60])
        perm = rng.permutation(len(P))
        _CACHE["planted"] = (np.ascontiguousarray(P[perm]), kind[perm])
    return _CACHE["planted"]


def room():
    """a floor (kind 0, 3000 points), a wall (1, 1500) and a sphere (2, 1000), shuffled"""
    if "room" not in _CACHE:
        rng = np.random.default_rng(21)
        floor = np.stack([rng.uniform(-2, 2, 3000), rng.uniform(-2, 2, 3000), 0.003 * rng.normal(size=3000)], 1)
        wall = np.stack([-2 + 0.003 * rng.normal(size=1500), rng.uniform(-2, 2, 1500), rng.uniform(0.05, 2, 1500)], 1)
        s = rng.normal(size=(1000, 3))
        s = 0.6 * s / np.linalg.norm(s, axis=1, keepdims=True) + [0.5, 0.3, 1.0]
        P = np.concatenate([floor, wall, s]).astype(f32)
        kind = np.repeat([0, 1, 2], [3000, 1500, 1000])
        perm = rng.permutation(len(P))
        _CACHE["room"] = (np.ascontiguousarray(P[perm]), kind[perm])
    return _CACHE["room"]


def test_the_module_exports_the_kernel_constants(fg, gpu_required):
    assert (fg.SEGMENT_TILE, fg.SEGMENT_CHUNK) == (TILE, CHUNK)
    src = open(os.path.join(REPO, "fast-go-icp_amd", "csrc", "device", "segment_score.hpp")).read()
    assert re.search(r"kSegBlock = 256, kSegPerThread = 4, kSegTile = kSegBlock \* kSegPerThread, kSegChunk = 256;", src)


def test_smallest_shapes(fg, gpu_required):
    for n in (1, 2):
        P = uniform(n, 30 + n)
        (kept, label, idx, models, info), _ = check(fg, P, 0.5, 64)
        assert not models and info["planes"] == 0 and info["kept"] == n and np.all(label == -1) and kept.tobytes() == P.tobytes()
    P = uniform(3, 33)
    (kept, label, idx, models, info), ref = check(fg, P, 0.01, 64)
    assert len(models) == 1 and models[0]["inliers"] == 3 and models[0]["hypothesis_inliers"] == 3 and np.all(label == 0) and info["kept"] == 0 and kept.shape == (0, 3)
    assert models[0]["hypothesis"] == int(np.flatnonzero(~sr.hypotheses(P, 64, 0, 0)[2])[0])  # the first hypothesis of three distinct indices
    (kept, *_), _ = check(fg, P, 0.01, 64, keep="planes")
    assert kept.tobytes() == P.tobytes()


@pytest.mark.parametrize("n,K", [(63, 64), (64, 64), (65, 64), (129, 64), (TILE, CHUNK), (TILE + 1, CHUNK + 1), (2 * TILE + 1, 1), (2 * TILE + 1, 2 * CHUNK + 1)])
def test_wave_tile_and_chunk_boundaries(fg, gpu_required, n, K):
    """a partial wave, a full one, one lane over, a partial block; one tile of the scoring kernel, one point over, two tiles and one point;
    one hypothesis, one chunk of hypotheses, one over, two chunks and one.  T is the median |r| of hypothesis 0: inliers and outliers both
    occur under the winner"""
    P = uniform(n, 100 + n)
    seed = next(s for s in range(50) if not sr.hypotheses(P, K, s, 0)[2][0])
    T = median_threshold(P, K, seed)
    (_, label, _, models, info), ref = check(fg, P, T, K, seed=seed)
    assert len(models) == 1 and 3 <= models[0]["hypothesis_inliers"] < n and 0 < int((label == 0).sum()) < n
    assert models[0]["hypothesis_inliers"] >= n // 2  # hypothesis 0 alone has the median within T
    check(fg, P, T, K, seed=seed, refit=False)


def lattice():
    g = np.arange(12, dtype=f32)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([np.concatenate([xy, np.full((144, 1), z, f32)], 1) for z in (0, 1, 2)]).astype(f32))


def test_points_exactly_at_the_threshold_are_inliers(fg, gpu_required):
    """three layers z = 0, 1, 2 of a 12 x 12 integer lattice, T = 1: a hypothesis with its three samples in one layer has the normal (0, 0, +-1)
    and an integral d exactly, so |r| is exactly 1 on the neighbouring layers — <= counts them.  Such a hypothesis of the middle layer holds
    all 432 points, one of an outer layer 288; no tilted plane holds all 432, so with a middle-layer hypothesis among the K the winner is the
    first of them"""
    P = lattice()
    K, seed = 256, 0
    idx, plane, deg = sr.hypotheses(P, K, seed, 0)
    z = P[idx, 2]
    layer = (z[:, 0] == z[:, 1]) & (z[:, 0] == z[:, 2]) & ~deg
    assert layer.any() and np.all(np.abs(plane[layer, 2]) == 1.0) and not plane[layer, :2].any() and np.all(plane[layer, 3] == np.round(plane[layer, 3]))
    cnt = sr.counts(P, plane, deg, 1.0, np.ones(len(P), bool))
    assert np.array_equal(cnt[layer], np.where(z[layer, 0] == 1, 432, 288))  # |r| = 1 exactly is within T
    win = int(np.argmax(cnt))
    assert layer[win] and z[win, 0] == 1 and cnt[win] == 432 and int((cnt == 432).sum()) >= 2  # a tie in counts: the lowest h wins
    assert win == int(np.flatnonzero(cnt == 432)[0]) and win > 0
    (_, label, _, models, info), ref = check(fg, P, 1.0, K, seed=seed, refit=False)
    assert models[0]["hypothesis"] == win and models[0]["inliers"] == 432 and np.all(label == 0) and info["kept"] == 0
    check(fg, P, 1.0, K, seed=seed, refit=True)
    # an outer layer alone wins when the middle one is not there to be drawn: the two lower layers, every in-layer hypothesis holds both
    Q = np.ascontiguousarray(P[:288])
    idx, plane, deg = sr.hypotheses(Q, K, seed, 0)
    zq = Q[idx, 2]
    cnt = sr.counts(Q, plane, deg, 1.0, np.ones(len(Q), bool))
    inlayer = (zq[:, 0] == zq[:, 1]) & (zq[:, 0] == zq[:, 2]) & ~deg
    assert inlayer.any() and np.all(cnt[inlayer] == 288)
    (_, label, _, models, _), _ = check(fg, Q, 1.0, K, seed=seed, refit=False)
    assert models[0]["inliers"] == 288 and np.all(label == 0)


def test_degenerate_clouds_have_no_plane(fg, gpu_required):
    equal = np.ascontiguousarray(np.tile(np.array([[0.25, -1.5, 3.0]], f32), (300, 1)))
    t = np.arange(300, dtype=f32)[:, None]
    line = np.ascontiguousarray(t * np.array([[1.0, 2.0, -0.5]], f32) + np.array([[4.0, 0.0, 1.0]], f32))  # exact in fp32
    for P in (equal, line):
        assert sr.hypotheses(P, 128, 2, 0)[2].all()
        (kept, label, idx, models, info), _ = check(fg, P, 0.5, 128, seed=2, max_planes=3)
        assert not models and info["planes"] == 0 and info["on_planes"] == 0 and info["kept"] == len(P) and np.all(label == -1) and kept.tobytes() == P.tobytes()


def test_the_planted_scene_and_why_the_call_exists(fg, gpu_required):
    """the table goes, and with it the connection between the sphere and the clump: keep-the-largest then keeps the sphere alone"""
    P, kind = planted()
    (rest, label, idx, models, info), ref = check(fg, P, 0.02, 256, seed=3)
    r = ref["models"][0]
    on = label == 0
    by_kind = [int((on & (kind == k)).sum()) for k in range(3)]
    print(f"winner h = {r['hypothesis']}, {r['hypothesis_inliers']} hypothesis inliers, {r['inliers']} after the refit: {by_kind} of sphere, table, clump")
    assert len(models) == 1 and by_kind[1] == 3000 and by_kind[0] < 60 and by_kind[2] < 10 and models[0]["inliers"] == sum(by_kind)
    assert abs(abs(models[0]["plane"][2]) - 1.0) < 1e-5 and abs(abs(models[0]["plane"][3]) - 1.0) < 1e-3
    assert fg.cluster_dbscan(P, 0.2).tobytes() == P.tobytes()  # one component as long as the table is there
    assert fg.segment_planes(P, 0.02, 256, seed=3).tobytes() == rest.tobytes()
    kept, _, _, size, cidx, cinfo = fg.cluster_dbscan(rest, 0.2, return_map=True)
    assert cinfo["clusters"] == 2 and np.all(kind[idx[cidx]] == 0) and len(kept) == int((~on & (kind == 0)).sum())  # every sphere point off the table, nothing else
    assert sorted(int(s) for s in size) == sorted([len(kept), int((~on & (kind == 2)).sum())])


def test_two_planes_and_the_prefix_property(fg, gpu_required):
    P, kind = room()
    (rest, label, idx, models, info), ref = check(fg, P, 0.02, 256, seed=5, max_planes=3, min_inliers=500)
    assert len(models) == 2 and len(ref["count_vectors"]) == 3 and ref["count_vectors"][2].max() < 500  # the third peel ran and stopped
    assert int(((label == 0) & (kind == 0)).sum()) == 3000 and int(((label == 1) & (kind == 1)).sum()) == 1500
    assert models[1]["candidates"] == len(P) - models[0]["inliers"]
    (_, label1, _, first, info1), _ = check(fg, P, 0.02, 256, seed=5, max_planes=1, min_inliers=500)
    assert len(first) == 1 and first[0].keys() == models[0].keys()
    for key in first[0]:  # the prefix property: plane 0 does not depend on how many are asked for
        assert np.asarray(first[0][key]).tobytes() == np.asarray(models[0][key]).tobytes(), key
    assert np.array_equal(label1 == 0, label == 0)
    (planes, *_), _ = check(fg, P, 0.02, 256, seed=5, max_planes=3, min_inliers=500, keep="planes")
    assert len(planes) + len(rest) == len(P) and planes.tobytes() == P[label >= 0].tobytes()
    (_, _, _, plain, _), _ = check(fg, P, 0.02, 256, seed=5, max_planes=3, min_inliers=500, refit=False)
    assert len(plain) == 2 and _bytes64(plain[0]["plane"]) == _bytes64(models[0]["hypothesis_plane"])


def test_scale(fg, gpu_required):
    """300 000 points — a floor, a wall and 3000 small blobs — and 512 hypotheses: 293 tiles of the scoring kernel, 1172 rows of the moment
    fold (more than its 1024 threads), about 1.5e8 plane distances restated in numpy"""
    rng = np.random.default_rng(9)
    floor = np.stack([rng.uniform(-4, 4, 120000), rng.uniform(-4, 4, 120000), 0.004 * rng.normal(size=120000)], 1)
    wall = np.stack([rng.uniform(-4, 4, 60000), 4 + 0.004 * rng.normal(size=60000), rng.uniform(0, 3, 60000)], 1)
    centres = rng.uniform([-4, -4, 0.3], [4, 4, 3], (3000, 3))
    blobs = (centres[:, None, :] + 0.03 * rng.normal(size=(3000, 40, 3))).reshape(-1, 3)
    P = np.concatenate([floor, wall, blobs]).astype(f32)
    P = np.ascontiguousarray(P[rng.permutation(len(P))])
    assert len(P) == 300000
    (rest, label, idx, models, info), ref = check(fg, P, 0.02, 512, seed=1, max_planes=2, min_inliers=30000)
    assert len(models) == 2 and models[0]["inliers"] > 115000 and models[1]["inliers"] > 55000


def test_two_calls_return_the_same_bytes(fg, gpu_required):
    P, _ = room()
    a = fg.segment_planes(P, 0.02, 256, seed=5, max_planes=3, min_inliers=500, return_map=True)
    b = fg.segment_planes(P, 0.02, 256, seed=5, max_planes=3, min_inliers=500, return_map=True)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert len(a[3]) == len(b[3]) == 2
    for ma, mb in zip(a[3], b[3]):
        assert ma.keys() == mb.keys() and all(np.asarray(ma[k]).tobytes() == np.asarray(mb[k]).tobytes() for k in ma)
    assert a[4].keys() == b[4].keys() and all(np.float64(a[4][k]).tobytes() == np.float64(b[4][k]).tobytes() for k in a[4])
    c = fg.segment_planes(P, 0.02, 256, seed=6, max_planes=3, min_inliers=500, return_map=True)
    assert not np.array_equal(c[3][0]["sample"], a[3][0]["sample"])  # another seed, other draws


def _raw(fg, P, T, K, seed, max_planes, min_inliers, capacity, capacity_models, arrays=True, fill=0xA5, device=0, model_size=None, keep_planes=0):
    lib = fg._lib.load()
    L = fg._lib
    n = len(P)
    out = np.empty((max(capacity, 1), 3), f32)
    out.view(np.uint8)[...] = fill
    idx = np.full(max(capacity, 1), fill * 0x01010101, np.uint32)
    label = np.full(n, fill * 0x01010101, np.uint32).view(np.int32)
    size = C.sizeof(L.SegmentModel)
    models = np.full(16 * size, fill, np.uint8)
    info = L.SegmentInfo()
    ptr = lambda a, t: a.ctypes.data_as(t) if arrays else None
    rc = lib.fgoicp_segment_planes(P.ctypes.data_as(L.c_float_p), n, C.c_float(T), K, seed, max_planes, min_inliers, 1, keep_planes, device, ptr(out, L.c_float_p), capacity,
                                   ptr(idx, L.c_uint32_p), ptr(label, C.POINTER(C.c_int32)), ptr(models, C.POINTER(L.SegmentModel)), capacity_models,
                                   size if model_size is None else model_size, C.byref(info))
    return rc, info, out, idx, label, models


def test_capacity_count_only_and_model_size(fg, gpu_required):
    P, _ = room()
    ref = fg.segment_planes(P, 0.02, 256, seed=5, max_planes=3, min_inliers=500, return_map=True)
    kept, planes = ref[4]["kept"], ref[4]["planes"]
    assert planes == 2 and 0 < kept < len(P)
    msg = lambda: fg._lib.load().fgoicp_last_error().decode()
    untouched = lambda *arrays: all(np.all(a.view(np.uint8) == 0xA5) for a in arrays)
    rc, info, out, idx, label, models = _raw(fg, P, 0.02, 256, 5, 3, 500, kept - 1, 16)
    assert rc == TOO_LARGE and "capacity_points" in msg()
    assert (info.points, info.planes, info.on_planes, info.kept, info.iterations, info.max_planes, info.refit, info.keep_planes, info.min_inliers, info.seed) == \
        (len(P), 2, len(P) - kept, kept, 256, 3, 1, 0, 500, 5) and info.distance_threshold == float(f32(0.02))
    assert untouched(out, idx, label, models)
    rc, info, out, idx, label, models = _raw(fg, P, 0.02, 256, 5, 3, 500, kept, 2)  # exactly enough of both
    assert rc == OK and out[:kept].tobytes() == ref[0].tobytes() and np.array_equal(idx[:kept], ref[2]) and np.array_equal(label, ref[1])
    size = C.sizeof(fg._lib.SegmentModel)
    got = (fg._lib.SegmentModel * 2).from_buffer_copy(models[:2 * size].tobytes())
    assert [int(m.inliers) for m in got] == [m["inliers"] for m in ref[3]] and _bytes64(np.array(got[1].plane)) == _bytes64(ref[3][1]["plane"])
    assert untouched(models[2 * size:])
    rc, info, out, idx, label, models = _raw(fg, P, 0.02, 256, 5, 3, 500, kept, 1)  # one model short
    assert rc == TOO_LARGE and "capacity_models" in msg() and info.planes == 2 and info.kept == kept
    assert untouched(out, idx, label, models)
    rc, info, *_ = _raw(fg, P, 0.02, 256, 5, 3, 500, 0, 0, arrays=False)  # all arrays NULL: the counts only
    assert rc == OK and (info.kept, info.planes, info.on_planes) == (kept, 2, len(P) - kept)
    rc, info, *_ = _raw(fg, P, 0.02, 256, 5, 3, 500, len(P), 16, device=99)  # an ordinal above the device count
    assert rc == INVALID_ARG and msg().startswith("fgoicp_segment_planes: device ordinal")
    # a caller compiled with a shorter model: entry j starts at j * model_size and no byte beyond it is written
    short = fg._lib.SegmentModel.plane.offset  # ends before `plane`
    rc, info, out, idx, label, models = _raw(fg, P, 0.02, 256, 5, 3, 500, len(P), 16, model_size=short)
    assert rc == OK and info.planes == 2
    full = np.frombuffer(bytes((fg._lib.SegmentModel * 2).from_buffer_copy(_raw(fg, P, 0.02, 256, 5, 3, 500, len(P), 16)[5][:2 * size].tobytes())), np.uint8)
    assert models[:short].tobytes() == full[:short].tobytes() and models[short:2 * short].tobytes() == full[size:size + short].tobytes()
    assert untouched(models[2 * short:])


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def _config(tmp_path, tag, extra, target="tgt.txt"):
    (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/{target}"\nsource = "{tmp_path}/src.txt"\nalignment = "{tmp_path}/{tag}_align.txt"\n'
                                          f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.01\nseed = 3\n{extra}')
    return str(tmp_path / f"{tag}.toml")


def _run(args):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines


def _g(v):
    return format(0.0 if abs(v) < 5e-7 else v, "g")  # six significant digits, as the CLI's stream prints a double


def test_cli_registers_the_filtered_clouds(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    P, kind = planted()
    order = np.argsort(kind != 0, kind="stable")  # the sphere first: a kept row's index tells whether it is a sphere point
    P, kind = np.ascontiguousarray(P[order]), kind[order]
    _write_txt(tmp_path / "tgt.txt", P)
    _write_txt(tmp_path / "src.txt", P[:600])  # sphere points; the loader keeps about half of them
    # what the CLI must find: the call with the CLI's arguments (seed = params.seed, a tenth of the cloud at least)
    rest, label, idx, models, info = fg.segment_planes(P, 0.02, 256, seed=3, min_inliers=506, return_map=True)
    sphere_left = int(((label < 0) & (kind == 0)).sum())
    assert info["planes"] == 1 and sphere_left > 1900
    pl = models[0]["plane"]
    want = (f"{len(P)} -> {len(rest)} points, distance 0.02, 256 hypotheses: 1 plane of {models[0]['inliers']} points, normal ({_g(pl[0])} {_g(pl[1])} {_g(pl[2])}), "
            f"offset {_g(pl[3])}")
    keys = "target_plane_distance = 0.02\ntarget_plane_iterations = 256\n"
    for tag, extra in (("plain", ""), ("with", keys)):
        rc, log = _run([exe, "-c", _config(tmp_path, tag, extra)])
        assert rc == 0, log[-2000:]
        rows = np.loadtxt((tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:], ndmin=2)
        line = [ln for ln in log.splitlines() if "Plane filter" in ln]
        if tag == "plain":
            assert not line and np.all(rows[:, 3] < len(P))
        else:
            assert len(line) == 1 and line[0].endswith("Plane filter (target): " + want), (line, want)
            assert len(rows) and np.all(rows[:, 3] < len(rest)) and np.all(rows[:, 3] >= 0)
    # the order against the other filters: the plane filter before the cluster filter, which starts from its count and now keeps the sphere alone
    rc, log = _run([exe, "-c", _config(tmp_path, "both", keys + "target_cluster_eps = 0.2\n")])
    assert rc == 0, log[-2000:]
    lines = [ln for ln in log.splitlines() if "Plane filter" in ln or "Cluster filter" in ln]
    assert len(lines) == 2 and lines[0].endswith("Plane filter (target): " + want), lines
    assert f"Cluster filter (target): {len(rest)} -> {sphere_left} points" in lines[1], lines
    # no plane of the size asked for: the cloud stays as it is
    rc, log = _run([exe, "-c", _config(tmp_path, "none", keys + "target_plane_min_fraction = 0.9\n")])
    assert rc == 0, log[-2000:]
    line = [ln for ln in log.splitlines() if "Plane filter" in ln]
    assert len(line) == 1 and line[0].endswith(f"Plane filter (target): {len(P)} -> {len(P)} points, distance 0.02, 256 hypotheses: no plane of at least 4554 points: unchanged")
    # --batch: each config is filtered with its own keys; the source's seed is params.seed + 1
    a = _config(tmp_path, "a", keys)
    b = _config(tmp_path, "b", keys + "target_plane_count = 2\ntarget_plane_min_fraction = 0.001\nsource_plane_distance = 0.05\nsource_plane_iterations = 64\n")
    (tmp_path / "list.txt").write_text(f"{os.path.basename(a)}\n{os.path.basename(b)}\n")
    rc, log = _run([exe, "--batch", str(tmp_path / "list.txt")])
    assert rc == 0, log[-2000:]
    lines = [ln.split("Plane filter ")[1] for ln in log.splitlines() if "Plane filter" in ln]
    assert len(lines) == 3, log[-2000:]
    assert lines[0] == "(target): " + want
    two = fg.segment_planes(P, 0.02, 256, seed=3, max_planes=2, min_inliers=6, return_map=True)
    assert two[4]["planes"] == 2
    assert lines[1].startswith(f"(target): {len(P)} -> {two[4]['kept']} points, distance 0.02, 256 hypotheses: 2 planes of {two[3][0]['inliers']} and {two[3][1]['inliers']} points, normal (")
    assert lines[2].startswith("(source): ") and ", distance 0.05, 64 hypotheses: " in lines[2]
    # a filter that keeps no point ends the run
    flat = np.ascontiguousarray(P[kind == 1][:500])
    _write_txt(tmp_path / "flat.txt", flat)
    rc, log = _run([exe, "-c", _config(tmp_path, "flat", "target_plane_distance = 0.05\n", target="flat.txt")])
    assert rc == 1 and "params.target_plane_distance = 0.05: the filter keeps no point" in log
