"""CPU: the designed clouds of tests/knn_normal_cases.py are what tests/test_gpu_knn_normal_edges.py takes them for — exact squared
distances, ties at the cut and across the boxes of the tree, the seed's three fill states — the fixture is what exact_normals computes, C_ANGLE
stands on the recorded numpy measurement, and the epilogue of target_knn_kernel, restated around the product's svd3_jacobi, passes the rule
the device is held to on every checked row."""
import numpy as np
import pytest

from tests import knn_normal_cases as kc

f32, f64 = np.float32, np.float64


def keys_behind_the_cut(name, k):
    """-> rows, keys (len(rows), k + 1): the k nearest and the key behind the cut"""
    pts, rows = kc.cloud(name), kc.sample_rows(name)
    return (np.arange(len(pts)) if rows is None else rows), kc.brute_knn(pts, k + 1, rows)


# ---- 1. exact distances ---------------------------------------------------------------------------------------------------------------
def test_dist_sq_is_exact_for_every_difference_of_multiples_of_one_64th():
    """all 129^3 differences (nx, ny, nz)/64, 0 <= n <= 128 (dist_sq squares them: the signs do not matter): fp32 equals fp64"""
    g = np.arange(129, dtype=f64) / 64.0
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    got = kc.npr.dist_sq(d.astype(f32), np.zeros(3, f32))
    assert got.dtype == f32 and np.array_equal(got.astype(f64), (d * d).sum(axis=1))


@pytest.mark.parametrize("name", sorted(kc.KNN_CASES) + ["plates", "cube", "tilted_lattice"])
def test_every_designed_dist_sq_is_exact(name):
    """A cloud on the 1/64 lattice (or in one plane z = 0.1f of it) has exact differences, which the test above covers pair by pair.  The
    line (far pairs need more than 24 bits) and the plates (0.1f meets multiples of 1/64 between two plates) are exact where the cut
    lies: fp32 dist_sq equals the fp64 one on the 33 nearest of every (sampled) row — asserted for every cloud."""
    pts, rows = kc.cloud(name), kc.sample_rows(name)
    p64 = pts.astype(f64)
    if name in kc.EXACT_EVERYWHERE:
        on_lattice = p64 * 64.0 == np.rint(p64 * 64.0)
        assert on_lattice[:, :2].all() and (on_lattice[:, 2].all() or (pts[:, 2] == kc.Z_PLANE).all()) and np.abs(p64).max() <= 1.0, name
    else:
        assert name in ("line", "plates")
    rows_ = np.arange(len(pts)) if rows is None else rows
    keys = kc.brute_knn(pts, min(kc.KMAX, len(pts)), rows)
    d = p64[rows_][:, None, :] - p64[kc.key_index(keys)]
    assert np.array_equal(kc.key_d2(keys).astype(f64), (d * d).sum(axis=2)), name


@pytest.mark.parametrize("name", ["box2049", "lattice52", "tetra5", "duplicates"])
def test_the_reference_of_a_reversed_cloud_is_the_plain_sort_of_its_own_keys(name):
    """brute_knn takes a reversed cloud's distances from the forward one: the keys are those of a sort over the whole row all the same"""
    for reverse in (False, True):
        pts, rows = kc.cloud(name, reverse), kc.sample_rows(name, reverse)
        kk = min(kc.KMAX, len(pts))
        keys = kc.brute_knn(pts, kk, rows)
        rows_ = np.arange(len(pts)) if rows is None else rows
        for i in (0, 3, len(rows_) // 2, len(rows_) - 1):
            d2 = kc.npr.dist_sq(pts[rows_[i]][None, :], pts).astype(f32)
            want = np.sort((kc.bits(d2).astype(np.uint64) << np.uint64(32)) | np.arange(len(pts), dtype=np.uint64))[:kk]
            assert np.array_equal(keys[i], want), (name, reverse, i)


def test_clouds_have_their_sizes_and_a_shuffled_order():
    sizes = {name: len(kc.cloud(name)) for name in kc.CLOUDS}
    assert sizes["box2048"] == 2048 and sizes["box2049"] == 2049 and sizes["lattice4097"] == 4097 and sizes["lattice52"] == 140608 == 131072 + 4 * 2048 + 1344
    assert sizes["plane"] == 2560 and sizes["line"] == 2731 and sizes["plates"] == 1587 and sizes["plates"] % 64 and sizes["tetra4"] == 4 and sizes["tetra5"] == 5
    assert sizes["duplicates"] == 40 + 31 + 216 and sizes["cube"] == 8 + 125
    assert all(600 <= sizes[name] <= 1500 for name in kc.RANDOM_FAMILIES)
    for name in kc.CLOUDS:
        p = kc.cloud(name)
        assert p.dtype == f32 and np.abs(p).max() <= 1.0, name
        assert np.array_equal(kc.cloud(name, reverse=True), p[::-1]), name
        assert np.array_equal(np.sort(kc._permutation(name)), np.arange(len(p))), name
        if len(p) > 8:
            assert not np.array_equal(p, kc._generated(name)), name
    nxt = np.nextafter(f32(1365 * 3 / 4096), f32(2))
    assert 1366 * 3 / 4096 > 1.0 >= nxt  # the line is the longest run of (1, 2, 3)/4096 steps about the origin inside [-1, 1]
    pts, plate = kc.cloud("plates"), kc.plate_of_row()
    for a, c in enumerate((f32(-0.5), f32(0.25), kc.Z_PLANE)):
        assert (pts[plate == a, a] == c).all() and (plate == a).sum() == 23 * 23
    d = np.sqrt(((pts[:, None, :].astype(f64) - pts[None, :, :]) ** 2).sum(axis=2))
    assert d[plate[:, None] != plate[None, :]].min() >= 0.5  # the plates are at least 0.5 apart


# ---- 2. ties at the cut -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(name, k) for name in sorted(kc.TIE_KS) for k in kc.TIE_KS[name]])
def test_at_least_half_of_a_lattices_rows_have_a_tie_at_the_cut(name, k):
    rows, keys = keys_behind_the_cut(name, k)
    d2 = kc.key_d2_bits(keys)
    tied = d2[:, k - 1] == d2[:, k]
    print(f"{name} k {k}: {int(tied.sum())} of {len(rows)} rows have a tie at the cut")
    assert 2 * int(tied.sum()) >= len(rows)
    assert (kc.key_index(keys)[tied, k - 1] < kc.key_index(keys)[tied, k]).all()  # the reference gives the tie to the lower caller index


MULTI_LEVEL = {"box2049": 1, "lattice4097": 100, "lattice52": 100, "plane": 100, "line": 1, "box2048+31": 1, "box2048+32": 1, "box2048+33": 1}


@pytest.mark.parametrize("name", sorted(MULTI_LEVEL))
def test_tie_partners_at_the_cut_lie_in_other_boxes_of_the_tree(name):
    """Rows whose tie at the cut is decided against a point of ANOTHER super-leaf (and, for 52^3, of the other top box): the partner is
    the last key inside the cut or the first behind it, the two that win and lose the index rule.  At least 100 rows where a boundary
    between two populated super-leaves runs through the lattice (4097, 52^3 on its sampled rows, the plane); the clouds that put 1 to 33
    points, or a line's two ends, behind the boundary have as many such rows as those few points are tied with, at least one.
    Slots: kd_order of csrc/device/morton.hpp through tests/host_harness.point_order, as bvh_build_host calls it (leaf 32, no fine order)."""
    pts = kc.cloud(name)
    slot = kc.slot_of(pts)
    assert np.array_equal(np.sort(slot), np.arange(len(pts)))
    other_super, other_top = set(), set()
    for k in kc.KNN_CASES[name]:
        rows, keys = keys_behind_the_cut(name, k)
        d2, idx = kc.key_d2_bits(keys), kc.key_index(keys).astype(np.int64)
        tied = d2[:, k - 1] == d2[:, k]
        for rank in (k - 1, k):
            other_super |= set(rows[tied & (slot[idx[:, rank]] // kc.SUPER != slot[rows] // kc.SUPER)])
            other_top |= set(rows[tied & (slot[idx[:, rank]] // kc.TOP != slot[rows] // kc.TOP)])
    print(f"{name}: {len(other_super)} rows with a tie partner in another super-leaf, {len(other_top)} in the other top box")
    assert len(other_super) >= MULTI_LEVEL[name]
    if name == "lattice52":
        assert len(other_top) >= 10
        assert (slot >= kc.TOP).sum() == 140608 - 131072 and -(-(140608 - 131072) // kc.SUPER) == 5  # two top boxes, the second with 5 super-leaves


@pytest.mark.parametrize("r", [31, 32, 33])
def test_the_last_waves_own_leaves_hold_r_points(r):
    """2048 + r points: the wave of slots 2048 .. 2111 has r real points, so at k = 32 its seed list stays short of k (the seed is empty),
    is exactly full, or full with one spare"""
    pts = kc.cloud(f"box2048+{r}")
    slot = kc.slot_of(pts)
    assert len(pts) == 2048 + r and int((slot // 64 == 32).sum()) == r and int((slot // 64 == 31).sum()) == 64
    assert (r >= 32) == (int((slot // 64 == 32).sum()) >= 32)


def test_the_duplicates_cloud_has_the_neighbourhoods_it_is_named_for():
    pts = kc.cloud("duplicates")
    keys = kc.brute_knn(pts, 32)
    idx, d2 = kc.key_index(keys), kc.key_d2(keys)
    held_a, held_b = kc.rows_at("duplicates", [kc.DUP_A]), kc.rows_at("duplicates", [kc.DUP_B])
    assert len(held_a) == 40 and len(held_b) == 31
    for r in held_a:  # the 32 lowest caller indices of the 40, ascending, at +0.0 — the row itself among them or not
        assert np.array_equal(idx[r], np.sort(held_a)[:32]) and not kc.bits(d2[r]).any()
    for r in held_b:  # the 31 copies and exactly one foreign point, the lowest caller index of the four nearest lattice points
        assert np.array_equal(idx[r, :31], np.sort(held_b)) and idx[r, 31] not in held_b and d2[r, 30] == 0 and d2[r, 31] > 0
        nearest = np.flatnonzero(kc.npr.dist_sq(pts[r][None, :], pts) == d2[r, 31])
        assert len(nearest) == 4 and idx[r, 31] == nearest.min()
    # k = 4 and 10: the lattice is symmetric about the 40 copies, so every split of the tree divides them — 10 per wave, in 4 waves.  A
    # copy's seed from its wave's own leaves is then full at distance 0, the bound of its walk is 0, and the copies of lower caller index
    # lie in OTHER leaves whose box distance is 0 as well: 0 shrunk is not above 0, so the strict rule visits them; a non-strict one
    # would skip every box.  At k = 32 the seed is not full.
    for reverse in (False, True):
        p = kc.cloud("duplicates", reverse)
        copies = np.flatnonzero((p == kc._points([kc.DUP_A])[0]).all(axis=1))
        per_wave = np.bincount(kc.slot_of(p)[copies] // 64)
        assert per_wave.tolist() == [10, 10, 10, 10] and set(kc.KNN_CASES["duplicates"]) == {4, 10, 32}
        for k in (4, 10):
            lists = kc.key_index(kc.brute_knn(p, k))[copies]
            wave = kc.slot_of(p) // 64
            assert (lists == copies[:k]).all()
            assert int((~np.isin(wave[copies], wave[copies[:k]])).sum()) >= 20  # for most copies the whole answer lies in other waves' leaves


# ---- 3. the fixture and C_ANGLE ---------------------------------------------------------------------------------------------------------
def test_fixture_regenerates_byte_for_byte_and_c_angle_stands_on_its_measurement(tmp_path):
    recorded = kc.recorded_numpy_c()
    worst = max(recorded.values())
    print(f"numpy.linalg.eigh needs c = {worst:.3f} at most ({max(recorded, key=recorded.get)}); C_ANGLE = {kc.C_ANGLE}")
    assert kc.C_ANGLE >= 16 * worst and kc.C_ANGLE == 2.0 ** np.ceil(np.log2(16 * worst))
    pytest.importorskip("mpmath")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_knn_normal_cases", os.path.join(kc.HERE, "golden", "make_knn_normal_cases.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    fresh = make.record()  # exact_normals of every entry, packed as the fixture stores it, and the numpy measurement again
    for name, k in kc.NORMAL_CASES:
        t, got = kc.tag(name, k), kc.load_exact(name, k)
        assert np.array_equal(fresh[t + "_row"], got["row"]) and np.array_equal(fresh[t + "_l"], got["l"]) and np.array_equal(fresh[t + "_v0"], got["v0"]), t
        assert np.array_equal(fresh[t + "_v2"], got["v2"][fresh[t + "_v2_rows"].astype(np.int64)]), t
        assert float(fresh[t + "_numpy_c"]) == recorded[(name, k)], t
        zero, gap, flat, _ = kc.classes(got["l"])
        assert np.allclose(np.linalg.norm(got["v0"][gap], axis=1), 1.0, atol=1e-15) and np.allclose(np.linalg.norm(got["v2"][flat], axis=1), 1.0, atol=1e-15), t
        assert (got["l"][zero] == 0).all() and (np.diff(got["l"], axis=1) >= 0).all(), t
    make.write(str(tmp_path / "again.npz"), fresh)
    assert (tmp_path / "again.npz").read_bytes() == open(kc.FIXTURE, "rb").read()
    assert os.path.getsize(kc.FIXTURE) < 340 * 1024


# ---- 4. the epilogue, restated, against the rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", kc.NORMAL_CASES, ids=[kc.tag(*t) for t in kc.NORMAL_CASES])
def test_restated_epilogue_passes_the_rule_on_every_checked_row(name, k):
    pts, idx = kc.normal_case(name, k)
    n = kc.epilogue_normals(pts, idx)
    report = kc.check_normals(n, kc.load_exact(name, k), where=(name, k))
    kc.check_designed(name, n, where=(name, k))
    print(f"{kc.tag(name, k)}: {report}")
    assert report["rows"] == len(pts) == report["zero"] + report["gap"] + report["flat"] + report["round"]
    if name == "line":  # every row: one direction of variance, the normal perpendicular to it
        assert report["flat"] == len(pts)
        assert (np.abs(n.astype(f64) @ kc.LINE_DIR) <= kc.EPS_STORE + kc.C_ANGLE * 2.0 ** -52).all()
    if name in ("plates", "plane"):
        assert report["gap"] == len(pts)


def test_the_rule_refuses_wrong_normals():
    """check_normals fails on a normal turned by 3e-7 rad, on one off the unit sphere by 5e-7, on -0.0 for a neighbourhood without extent
    and on a unit vector there; a flat row may turn freely about v2 but not towards it"""
    name, k = "noisy_sphere", 8
    pts, idx = kc.normal_case(name, k)
    ex = kc.load_exact(name, k)
    good = kc.epilogue_normals(pts, idx)
    kc.check_normals(good, ex)
    v0 = ex["v0"][ex["row"]]
    side = np.cross(v0, np.roll(v0, 1, axis=1))
    side /= np.linalg.norm(side, axis=1)[:, None]
    turned = good.copy()
    turned[17] = (np.cos(3e-7) * v0[17] + np.sin(3e-7) * side[17]).astype(f32)
    with pytest.raises(AssertionError, match="angle"):
        kc.check_normals(turned, ex)
    long = good.copy()
    long[5] = (good[5].astype(f64) * (1 + 5e-7)).astype(f32)
    with pytest.raises(AssertionError, match="unit"):
        kc.check_normals(long, ex)
    pts, idx = kc.normal_case("duplicates", 32)
    ex = kc.load_exact("duplicates", 32)
    good = kc.epilogue_normals(pts, idx)
    held_a = kc.rows_at("duplicates", [kc.DUP_A])
    for bad in (f32([0, 0, -0.0]), f32([0, 0, 1])):
        wrong = good.copy()
        wrong[held_a[3]] = bad
        with pytest.raises(AssertionError, match="without extent"):
            kc.check_normals(wrong, ex)
        with pytest.raises(AssertionError):
            kc.check_designed("duplicates", wrong)
    pts, idx = kc.normal_case("line", 4)
    ex = kc.load_exact("line", 4)
    e = np.cross(kc.LINE_DIR, [1.0, 0, 0])
    e /= np.linalg.norm(e)
    kc.check_normals(np.tile(e.astype(f32), (len(pts), 1)), ex)
    tilt = np.tile((np.cos(1e-6) * e + np.sin(1e-6) * kc.LINE_DIR).astype(f32), (len(pts), 1))
    with pytest.raises(AssertionError, match="largest variance"):
        kc.check_normals(tilt, ex)


def test_designed_neighbourhoods_give_the_exact_bits_listed():
    """planes x, y, z = const (any fp32 constant, square or rectangular spread) give the axis; lines along x, y, z give e_z, e_z, e_x; a line
    along (1, 2, 3)/64 a unit vector perpendicular to it; k identical points the zero vector"""
    rng = np.random.default_rng(7)
    for axis in range(3):
        for const in (f32(0.1), f32(-0.5), f32(0.7654321), f32(1e-3)):
            for shape in ((3, 3), (2, 5), (4, 8)):
                g = kc._grid(shape[0], shape[1], 1)[:, :2].astype(f64) / 64.0
                p = np.insert(g, axis, const, axis=1).astype(f32)[rng.permutation(len(g))]
                n = kc.epilogue_normals(p, np.arange(len(p))[None, :])[0]
                assert np.array_equal(kc.bits(np.abs(n)), kc.bits(np.eye(3, dtype=f32)[axis])), (axis, const, shape, n)
    for axis, want in ((0, 2), (1, 2), (2, 0)):
        p = np.zeros((7, 3), f32)
        p[:, axis] = np.arange(7) / 64.0
        n = kc.epilogue_normals(p, np.arange(7)[None, :])[0]
        assert np.array_equal(kc.bits(np.abs(n)), kc.bits(np.eye(3, dtype=f32)[want])), (axis, n)
    p = (np.arange(-3, 4)[:, None] * np.array([1.0, 2.0, 3.0]) / 64.0).astype(f32)
    n = kc.epilogue_normals(p, np.arange(7)[None, :])[0].astype(f64)
    assert abs(np.linalg.norm(n) - 1) <= 2e-7 and abs(n @ kc.LINE_DIR) <= kc.EPS_STORE
    p = np.tile(f32([0.3, -0.7, 0.1]), (32, 1))
    assert not kc.bits(kc.epilogue_normals(p, np.arange(32)[None, :])).any()
