"""GPU: the fixed-radius walk (radius_walk of kernels.hip, in cluster_count_kernel, cluster_hook_kernel and cluster_border_kernel) behind
fgoicp_cluster_dbscan on the designed clouds of tests/radius_walk_cases.py — lattices whose equal distances are equal bits, so that
neighbours at exactly d2 == eps2 lie in other leaves, other super-leaves (2 049 ... 4 097 points) and the other top box (140 608), behind a
tilted leaf slab at distance exactly eps (tilted_pair_wide), and are gone at the radius one ulp below; border rows tied between two
clusters (striped), where the label shows which key won; a radius whose square is +0.0, +inf or a subnormal; exact ties on generic
fp32 data.

Every call goes through check() of tests/test_gpu_cluster.py: labels, neighbour counts, sizes and kept indices as integers, the kept
points as bytes, every info count and eps2 in bits — against the integer reference of tests/radius_walk_cases.py, which
tests/test_radius_walk_cases_host.py holds against the n x n restatement without a GPU, and on all 140 608 rows of the largest cloud."""
import numpy as np
import pytest

from tests import radius_walk_cases as rc
from tests.test_gpu_cluster import check, d2_rows, restate, uniform

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
KEEP = (0, 2)  # the largest cluster; every cluster of at least two points


def run(fg, name, radius, reverse=False, keeps=KEEP, min_pts=None):
    pts = rc.cloud(name, reverse)
    m = rc.min_points(name, radius) if min_pts is None else min_pts
    ref = rc.reference(name, radius, m, reverse)
    out = None
    for keep_min_size in keeps:
        out = check(fg, pts, rc.EPS[radius], m, keep_min_size, ref=ref)
    if len(pts) > rc.SUPER:  # a component that spans super-leaves
        print(f"{name} {'reversed' if reverse else 'shuffled'} eps = {radius}, min_points = {m}: {out[5]['clusters']} clusters, {out[5]['rounds']} rounds")
    return out


# ---- 1. the lattices ------------------------------------------------------------------------------------------------------------------
CASES = [(name, reverse) for name in rc.CLOUDS if name != "lattice52" for reverse in ((False, True) if name in rc.REVERSED_TOO else (False,))]


@pytest.mark.parametrize("name,reverse", CASES, ids=[f"{n}-{'reversed' if r else 'shuffled'}" for n, r in CASES])
def test_every_output_equals_the_integer_reference(fg, gpu_required, name, reverse):
    for radius in rc.radii(name):
        info = run(fg, name, radius, reverse)[5]
        if name in rc.PLANE_PAIRS and radius in ("3", "9"):  # the one offset across joins the planes; one ulp below there are two clusters
            assert info["clusters"] == 1
        if name in rc.PLANE_PAIRS and radius in ("3-", "9-"):
            assert info["clusters"] == 2
        if (name, radius) == ("striped", "1"):  # four slabs, and 800 border rows between them that join the one of the lower caller index
            assert info["clusters"] == 4


@pytest.mark.parametrize("radius", ["1", "3"])
def test_two_top_boxes_on_all_140608_rows(fg, gpu_required, radius):
    info = run(fg, "lattice52", radius)[5]
    assert info["points"] == 140608 and info["clusters"] == 1 and info["core_points"] == {"1": 125000, "3": 124392}[radius]


# ---- 2. the control: one ulp below the radius -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reverse", CASES, ids=[f"{n}-{'reversed' if r else 'shuffled'}" for n, r in CASES])
def test_one_ulp_below_the_radius_loses_exactly_the_tied_neighbours(fg, gpu_required, name, reverse):
    """the counts at nextafter(eps, 0) are lower than at eps by the number of offsets at exactly |o|^2 == r2 that exist per row — on the
    device and in the reference, each against its own other result, so a `<` for `<=` cannot hide behind a wrong reference"""
    whole = rc.radii(name)[-2]
    below = rc.BELOW[whole]
    tied = rc.tied_neighbours(name, whole, reverse)
    pts = rc.cloud(name, reverse)
    got = [fg.cluster_dbscan(pts, rc.EPS[r], min_points=rc.min_points(name, r), return_map=True)[2].astype(np.int64) for r in (whole, below)]
    want = [rc.reference(name, r, reverse=reverse)["neighbours"].astype(np.int64) for r in (whole, below)]
    assert np.array_equal(got[0] - got[1], tied) and np.array_equal(want[0] - want[1], tied)
    if name in rc.TIE_LATTICES:
        assert (tied >= 1).all()
    else:  # the plates: as the plane; striped: a lattice with gaps; duplicates (pitch 8) and tilted_lattice (d2 of 2, 6, 8) hold no pair at 9
        assert tied.any() == (name in ("plates", "striped"))


# ---- 3. duplicates: eps2 == +0.0 -----------------------------------------------------------------------------------------------------------
def test_a_radius_whose_square_is_zero_counts_the_holders_of_a_position(fg, gpu_required):
    """eps = 1e-23f is positive and eps * eps is +0.0: d2 <= 0 holds between the copies of one position and nowhere else"""
    pts = rc.cloud("duplicates")
    a = (pts == 0).all(axis=1)
    b = (pts == f32([0.5, 0, 0])).all(axis=1)
    assert a.sum() == 40 and b.sum() == 31
    kept, label, nbr, size, idx, info = run(fg, "duplicates", "0", min_pts=31)
    assert rc.bits(info["eps2"])[0] == 0 and info["eps2"] == 0.0
    assert (nbr[a] == 40).all() and (nbr[b] == 31).all() and (nbr[~a & ~b] == 1).all()
    assert sorted(size.tolist()) == [31, 40] and info["clusters"] == 2 and info["noise_points"] == len(pts) - 71 and (label[~a & ~b] == -1).all()
    kept, label, nbr, size, idx, info = run(fg, "duplicates", "0", min_pts=32)
    assert size.tolist() == [40] and (label[a] == 0).all() and (label[~a] == -1).all() and info["noise_points"] == len(pts) - 40
    kept, label, nbr, size, idx, info = run(fg, "duplicates", "0", min_pts=41)
    assert info["clusters"] == 0 and info["rounds"] == 0 and info["noise_points"] == len(pts) and (label == -1).all() and len(kept) == 0
    # eps = 1/64, min_points = 41: the 40 copies are not core; whatever the reference says of them (noise: no core point anywhere)
    kept, label, nbr, size, idx, info = run(fg, "duplicates", "1", min_pts=41)
    assert (nbr[a] == 40).all() and info["core_points"] == 0


# ---- 4. eps2 == +inf ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["box2049", "uniform129"])
def test_a_finite_radius_whose_square_overflows_reaches_every_point(fg, gpu_required, which):
    pts = rc.cloud("box2049") if which == "box2049" else uniform(129, 50 + 129)
    n = len(pts)
    eps = f32(2e19)
    assert np.isfinite(eps) and np.isposinf(rc.eps2_of(eps))
    for m in (10, n):
        for keep_min_size in (0, n, n + 1):
            kept, label, nbr, size, idx, info = check(fg, pts, eps, m, keep_min_size, ref=rc.everything(n, m, np.inf))
            assert np.isposinf(info["eps2"]) and (nbr == n).all() and info["clusters"] == 1 and size.tolist() == [n] and (label == 0).all()
            assert info["kept"] == (n if keep_min_size <= n else 0)
    kept, label, nbr, size, idx, info = check(fg, pts, eps, n + 1, ref=rc.everything(n, n + 1, np.inf))
    assert (nbr == n).all() and (label == -1).all() and info["clusters"] == 0 and info["noise_points"] == n and info["rounds"] == 0


# ---- 5. d2 == eps2 on generic fp32 data -----------------------------------------------------------------------------------------------------
def test_exact_ties_at_the_radius_on_a_uniform_cloud(fg, gpu_required):
    """three pairs (i, j) of uniform(2049) whose fp32 d2 is the exact square of an fp32 eps, near the median squared distance to the 8th
    neighbour: at eps the pair is counted by both of its ends, at nextafter(eps, 0) it is not — against the n x n restatement"""
    n = 2049
    pts = uniform(n, 50 + n)
    d2 = d2_rows(pts, np.arange(n))
    assert np.array_equal(d2, d2.T)
    target = np.median(np.sort(d2, axis=1)[:, 8])
    i, j = np.triu_indices(n, 1)
    v = d2[i, j]
    near = np.argsort(np.abs(v - target), kind="stable")[:64]
    found = []
    for at in near:
        eps = np.sqrt(v[at])  # fp32, correctly rounded
        if eps.dtype == f32 and rc.bits(rc.eps2_of(eps))[0] == rc.bits(v[at])[0] and all(v[at] != w for _, _, w, _ in found):
            found.append((int(i[at]), int(j[at]), v[at], eps))
        if len(found) == 3:
            break
    assert len(found) == 3, "about half of all pairs qualify"
    for a, b, value, eps in found:
        below = np.nextafter(eps, f32(0))
        assert rc.eps2_of(below) < value == rc.eps2_of(eps)
        ref, ref_below = restate(pts, float(eps), 8), restate(pts, float(below), 8)
        nbr = check(fg, pts, eps, 8)[2].astype(np.int64)
        nbr_below = check(fg, pts, below, 8)[2].astype(np.int64)
        lost = ((d2 <= rc.eps2_of(eps)) & ~(d2 <= rc.eps2_of(below))).sum(axis=1)
        assert lost[a] >= 1 and lost[b] >= 1 and np.array_equal(nbr - nbr_below, lost)
        assert np.array_equal(ref["neighbours"].astype(np.int64) - ref_below["neighbours"], lost)
        kinds = ref["core"].sum(), ((ref["label"] >= 0) & ~ref["core"]).sum(), (ref["label"] < 0).sum()
        print(f"pair ({a}, {b}), d2 = eps2 = {value!r}: core / border / noise {kinds}")
        assert min(kinds) >= 1


# ---- 6. subnormal squared distances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box2049", "duplicates"])
def test_subnormal_squared_distances_give_the_outputs_of_the_unscaled_cloud(fg, gpu_required, name):
    """the cloud times 2^-66 (exact) at eps = 3 * 2^-72: eps2 = 9 * 2^-144 and every d2 up to far beyond it are exact fp32 subnormals, so
    every output but eps2 is that of the unscaled cloud at eps = 3/64"""
    pts = np.ascontiguousarray(rc.cloud(name) * f32(2.0 ** -66))
    assert np.array_equal(pts.astype(f64) * 2.0 ** 66, rc.cloud(name).astype(f64))
    eps = f32(3.0 * 2.0 ** -72)
    eps2 = rc.eps2_of(eps)
    assert 0 < eps2 < np.finfo(f32).tiny and f64(eps2) == 9.0 * 2.0 ** -144
    m = rc.min_points(name, "3")
    ref = dict(rc.reference(name, "3", m), eps2=eps2)
    for keep_min_size in KEEP:
        info = check(fg, pts, eps, m, keep_min_size, ref=ref)[5]
    assert info["core_points"] == int(ref["core"].sum()) > 0


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes(fg, gpu_required):
    """every array and every info field, `rounds` among them, as tests/test_gpu_cluster.py does on its planted cloud"""
    pts = rc.cloud("lattice4097")
    a = fg.cluster_dbscan(pts, rc.EPS["3"], min_points=100, keep_min_size=0, return_map=True)
    b = fg.cluster_dbscan(pts, rc.EPS["3"], min_points=100, keep_min_size=0, return_map=True)
    for x, y in zip(a[:5], b[:5]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert a[5].keys() == b[5].keys() and all(np.float64(a[5][key]).tobytes() == np.float64(b[5][key]).tobytes() for key in a[5]), (a[5], b[5])
