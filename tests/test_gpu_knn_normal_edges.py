"""GPU: the k-nearest walk (knn_walk of kernels.hip, in target_knn_kernel and outlier_knn_kernel) and the normal epilogue of
target_knn_kernel on the designed clouds of tests/knn_normal_cases.py — lattices whose equal distances are equal bits, at the sizes where
the tree gains a level (2048 | 2049, 4097, 140 608 = two top boxes), a plane (leaf boxes of zero height, thin slabs), a line, the three fill
states of the walk's seed, k = nt, and neighbourhoods that are planar, collinear, isotropic or a single position.

The bounds.  Neighbour sets are exact: indices and distance bits equal the brute force over (bits(d2) << 32) | index.  Normals follow the
rule of tests/knn_normal_cases.py (check_normals) on EVERY row against eigenvectors computed in exact arithmetic (the fixture
tests/golden/knn_normal_cases.npz), and the designed ones are exact bits.  tests/test_knn_normal_cases_host.py shows without a GPU that the
clouds have these properties and that a restatement of the epilogue around the product's svd3_jacobi passes the same rule."""
import numpy as np
import pytest

from tests import knn_normal_cases as kc
from tests.nn_restatement import I3, ZERO3

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def context(fg, pts, source=None, flags=0):
    return fg.Registration(pts, kc.source_of(pts) if source is None else source, kc.BOX, kc.RES, flags=flags)


def check_knn(reg, pts, k, rows, where):
    idx, d2 = reg.target_knn(k)
    want = kc.brute_knn(pts, k, rows)
    sel = slice(None) if rows is None else rows
    wrong = np.flatnonzero((idx[sel] != kc.key_index(want)).any(axis=1))
    assert len(wrong) == 0, (where, k, f"{len(wrong)} rows differ in their indices", wrong[:8], idx[sel][wrong[:2]], kc.key_index(want)[wrong[:2]])
    assert np.array_equal(kc.bits(d2[sel]), kc.key_d2_bits(want)), (where, k)
    return idx, d2


# ---- 1. the neighbour sets ------------------------------------------------------------------------------------------------------------
KNN = [(name, order) for name in kc.KNN_CASES for order in ("shuffled", "reversed")]


@pytest.mark.parametrize("name,order", KNN, ids=[f"{n}-{o}" for n, o in KNN])
def test_neighbour_sets_equal_the_brute_force_in_indices_and_bits(fg, gpu_required, name, order):
    reverse = order == "reversed"
    pts, rows = kc.cloud(name, reverse), kc.sample_rows(name, reverse)
    reg = context(fg, pts)
    try:
        for k in kc.KNN_CASES[name]:
            idx, d2 = check_knn(reg, pts, k, rows, (name, order))
            if name == "duplicates":  # the 40 copies list each other — the 32 lowest caller indices, ascending — at +0.0
                held = np.flatnonzero((pts == kc._points([kc.DUP_A])[0]).all(axis=1))
                assert len(held) == kc.DUP_A_COPIES
                assert np.array_equal(idx[held], np.tile(held[:k].astype(np.uint32), (len(held), 1))) and not kc.bits(d2[held]).any()
    finally:
        reg.close()


# ---- 2. the filter's epilogue on ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("lattice52", 10), ("plane", 6)])
def test_outlier_filter_reads_the_walks_list_on_ties(fg, gpu_required, name, k):
    pts, rows = kc.cloud(name), kc.sample_rows(name)
    rows = np.arange(len(pts)) if rows is None else rows
    keys = kc.brute_knn(pts, k, rows)
    _, _, _, mean_dist, kth, info = fg.remove_statistical_outliers(pts, k=k, std_ratio=1.0, return_map=True)
    assert info["k"] == k and info["points"] == len(pts)
    assert np.array_equal(kc.bits(kth[rows]), kc.key_d2_bits(keys)[:, k - 1]), name
    interior = kc.rows_at(name, [[0, 0, 0]], z_plane=name == "plane")
    assert len(interior) == 1 and kth[interior[0]] == f32(2.0 / 4096.0)  # 1 + 6 (or 4) nearer points, then the tied shell at 2/4096
    root = np.sqrt(kc.key_d2(keys).astype(f64))
    mean_ref = np.zeros(len(rows))
    for j in range(k):  # list order, left to right
        mean_ref = mean_ref + root[:, j]
    mean_ref = mean_ref / f64(k)
    dev = np.abs(mean_dist[rows] - mean_ref)
    print(f"{name} k {k}: largest |mean_dist - restatement| = {dev.max():.3e}")
    assert np.all(dev <= 2 * np.spacing(mean_ref))


# ---- 3. normals, target side --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", kc.NORMAL_CASES, ids=[kc.tag(*t) for t in kc.NORMAL_CASES])
def test_estimated_normals_follow_the_rule_on_every_row(fg, gpu_required, name, k):
    pts = kc.cloud(name)
    reg = context(fg, pts)
    try:
        check_knn(reg, pts, k, None, name)  # the neighbourhoods are those of the fixture: whatever fails below is the epilogue's
        reg.set_target_normals(k=k)
        n = reg.target_normals()
        report = kc.check_normals(n, kc.load_exact(name, k), where=(name, k))
        print(f"{kc.tag(name, k)}: {report}")
        kc.check_designed(name, n, where=(name, k))
        if name == "line":
            assert report["flat"] == len(pts)
            assert (np.abs(n.astype(f64) @ kc.LINE_DIR) <= kc.EPS_STORE + kc.C_ANGLE * 2.0 ** -52).all()
    finally:
        reg.close()


def test_plane_moments_count_the_inliers_whose_correspondent_has_a_normal(fg, gpu_required):
    """the duplicates cloud at k = 32: the 40 copies of one position have no normal, the 31 copies of the other have one.  A source of 8
    points on the first position, 8 on the second and 48 lattice points, at the identity: every point finds a target at distance 0 — the
    lowest caller index of its position — and the 8 whose correspondent has the zero normal are not counted."""
    pts = kc.cloud("duplicates")
    held_a, held_b = kc.rows_at("duplicates", [kc.DUP_A]), kc.rows_at("duplicates", [kc.DUP_B])
    others = np.setdiff1d(np.arange(len(pts)), np.concatenate([held_a, held_b]))
    src = np.ascontiguousarray(pts[np.concatenate([held_a[-8:], held_b[-8:], others[:48]])])
    reg = context(fg, pts, source=src)
    try:
        reg.set_target_normals(k=32)
        n = reg.target_normals()
        kc.check_designed("duplicates", n)
        a = reg.alignment(I3, ZERO3)
        assert not kc.bits(a.dist2).any()
        assert (a.indices[:8] == held_a.min()).all() and (a.indices[8:16] == held_b.min()).all() and np.array_equal(a.indices[16:], others[:48])
        got = reg.plane_moments(I3, ZERO3)
        assert got.points == 64 and got.correspondences == int(n[a.indices].any(axis=1).sum()) == 56
    finally:
        reg.close()


# ---- 4. normals, source side --------------------------------------------------------------------------------------------------------------
def test_source_normals_come_back_at_the_callers_index_under_every_source_order(fg, gpu_required):
    """the plates as the SOURCE: every caller row's normal is its plate's axis, so a wrong permutation between the one-shot tree's order, the
    caller's order and the context's slot order (slot_order_kernel) shows on every point; flags 0, FLAG_NO_MORTON and FLAG_CURVE_ORDER store
    the source in three different orders and return the same bytes"""
    src, ex = kc.cloud("plates"), kc.load_exact("plates", 9)
    got = []
    for flags in (0, fg.FLAG_NO_MORTON, fg.FLAG_CURVE_ORDER):
        reg = context(fg, kc.cloud("cube"), source=src, flags=flags)
        try:
            reg.set_source_normals(k=9)
            n = reg.source_normals()
        finally:
            reg.close()
        kc.check_normals(n, ex, where=("plates as the source", flags))
        kc.check_designed("plates", n, where=("plates as the source", flags))
        got.append(n)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes(fg, gpu_required):
    pts = kc.cloud("lattice4097")
    reg = context(fg, pts)
    try:
        first = reg.target_knn(32)
        second = reg.target_knn(32)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        normals = []
        for _ in range(2):
            reg.set_target_normals(k=10)
            normals.append(reg.target_normals())
        assert normals[0].tobytes() == normals[1].tobytes()
    finally:
        reg.close()
