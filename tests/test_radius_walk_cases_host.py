"""CPU: the clouds, radii and integer reference of tests/radius_walk_cases.py are what tests/test_gpu_radius_walk_edges.py takes them for.

1. The radii square as stated (9/4096 exactly, just below it, +0.0, +inf, a subnormal), and the balls hold 7, 123 and 93 offsets.
2. The integer reference equals restate() of tests/test_gpu_cluster.py — the fp32 d2 matrix written from the header — in every array,
   on every cloud of at most 5 600 points, at every radius, in both caller orders where both are run.
3. Ties at d2 == eps2 across the tree.  Rows with a neighbour at exactly the radius that lies in another super-leaf / in another top
   box (slots: the product's kd_order through tests/host_harness), measured here in the shuffled and in the reversed caller order:

       cloud              eps = 1: shuffled      reversed       eps = 3 (9 for the wide pair): shuffled   reversed
       box2048            0 / 0                  0 / 0          0 / 0                                     0 / 0     (one super-leaf: the control)
       box2049            2 / 0                  2 / 0          5 / 0                                     5 / 0     (one point behind the boundary)
       box2048+31         62 / 0                 62 / 0         158 / 0                                   158 / 0
       box2048+32         64 / 0                 64 / 0         160 / 0                                   160 / 0
       box2048+33         66 / 0                 66 / 0         165 / 0                                   165 / 0
       lattice4097        342 / 0                343 / 0        1 004 / 0                                 1 010 / 0
       plane              80 / 0                 80 / 0         240 / 0                                   240 / 0
       lattice52          46 768 / 5 408         46 737 / 5 408 107 883 / 16 224                          107 843 / 16 224
       tilted_pair        (no pair within 1)                    440 / 0                                   442 / 0
       tilted_pair_wide   (not run)                             1 277 / 0                                 1 277 / 0

   Every row of every one of these has at least one neighbour at exactly d2 == eps2.
4. Kinds of point at the min_points the device is given: core and border points occur on every lattice at every radius with a pair inside
   it, noise too on the volumes; the planar lattices at the two larger radii and the plane pairs have no noise point (a corner of a
   planar lattice still sees a core point), which the test states instead of asserting the contrary.
5. Border ties: border rows with two or more core neighbours tied for the smallest d2, so the index decides / those of them whose tied
   partners lie in different super-leaves (shuffled order; the reversed one in the test's output):

       cloud              eps = 1     eps = 3 (9)    just below
       box2048            0 / 0       320 / 0        256 / 0     (a face point of a volume has ONE core neighbour at distance 1)
       box2049            0 / 0       320 / 0        256 / 0
       box2048+31         14 / 0      300 / 0        232 / 0
       box2048+32         14 / 0      300 / 0        224 / 0
       box2048+33         14 / 0      300 / 0        224 / 0
       lattice4097        19 / 2      405 / 2        325 / 8
       lattice52          0 / 0       1 248 / 32     1 184 / 12
       plane              0 / 0       0 / 0          0 / 0       (the nearest core point of a border row is one: straight inwards)
       tilted_pair        -           113 / 0        117 / 0
       tilted_pair_wide   -           210 / 0        170 / 0

   At least 100 tied rows are required at the larger radii of every volume and plane pair; at least 10 split ones only of lattice52,
   the one cloud that reaches it (lattice4097: at least 1, it has 1 to 9; the clouds of 2 048 + r points have their second super-leaf
   on one face, whose border rows find their nearest core points inside the first).  The plane has none at all and is left out.
   On all of these the tied neighbours belong to ONE cluster, so the label does not say which of them won.  The striped cloud is
   there for that: 858 border rows with one core neighbour in each of two clusters, both at d2 == eps2; 412 (reversed: 446) join the
   slab below them, the others the one above; 3 (2) have the two partners in different super-leaves — the k-d cuts run along x.
6. The plane pairs.  tilted_pair: EVERY leaf holds points of both planes, so no partner lies behind a slab at distance eps (asserted as
   found: the cloud stays in the GPU cases for its ties and its two-against-one cluster count).  tilted_pair_wide: two thirds of its
   leaves lie in one plane and about 3 000 rows (at least 1 000 are required) have their +-(6, 6, 3) partner in such a leaf of the other
   plane; no other neighbour in the other plane, so those hits — and the single cluster they make of the two planes — exist only if a
   leaf at slab distance exactly eps is scanned."""
import numpy as np
import pytest

from tests import radius_walk_cases as rc
from tests.test_gpu_cluster import restate

f32, f64 = np.float32, np.float64


# ---- 1. the radii -----------------------------------------------------------------------------------------------------------------------
def test_the_radii_square_as_stated():
    assert rc.bits(rc.eps2_of(rc.EPS["1"]))[0] == rc.bits(f32(2.0 ** -12))[0]
    for whole, below, r2 in (("3", "3-", 9), ("9", "9-", 81), ("1", "1-", 1)):
        assert rc.bits(rc.eps2_of(rc.EPS[whole]))[0] == rc.bits(f32(r2 / 4096.0))[0]
        assert f32((r2 - 1) / 4096.0) < rc.eps2_of(rc.EPS[below]) < f32(r2 / 4096.0) and rc.R2[whole] == r2 and rc.R2[below] == r2 - 1
        assert rc.EPS[below] < rc.EPS[whole] and np.nextafter(rc.EPS[below], f32(1)) == rc.EPS[whole]
    assert rc.EPS["0"] > 0 and rc.bits(rc.eps2_of(rc.EPS["0"]))[0] == 0  # +0.0
    assert np.isfinite(f32(2e19)) and np.isposinf(rc.eps2_of(f32(2e19)))
    tiny = f32(3.0 * 2.0 ** -72)
    assert f64(tiny) == 3.0 * 2.0 ** -72 and f64(rc.eps2_of(tiny)) == 9.0 * 2.0 ** -144 and rc.eps2_of(tiny) < np.finfo(f32).tiny  # an exact subnormal
    for r2, size, at in ((1, 7, 6), (9, 123, 30), (8, 93, 12), (81, 3071, 102), (0, 1, 1)):
        o, d = rc.ball(r2)
        assert len(o) == size and int((d == r2).sum()) == at and (d == (o * o).sum(1)).all() and (np.diff(d) >= 0).all()


def test_clouds_lie_on_the_lattice_in_a_shuffled_order():
    sizes = {name: len(rc.cloud(name)) for name in rc.CLOUDS}
    assert sizes["tilted_pair"] == 5531 and sizes["tilted_pair_wide"] == 5369 and sizes["striped"] == 5472 and sizes["lattice52"] == 140608
    assert all(sizes[name] <= rc.SMALL for name in rc.CLOUDS if name != "lattice52")
    for name in rc.CLOUDS:
        p = rc.cloud(name)
        q, kind = rc.integer_coordinates(p)  # asserts: multiples of 1/64, or 0.1f in z
        assert p.dtype == f32 and np.abs(p).max() <= 1.0 and np.array_equal(rc.cloud(name, reverse=True), p[::-1]), name
        assert (rc.positions(name).size == 1).all() == (name != "duplicates"), name
    for name, s in rc.PLANE_PAIRS.items():
        q, _ = rc.integer_coordinates(rc.cloud(name))
        level = 2 * q[:, 0] + 2 * q[:, 1] + q[:, 2]
        assert set(level) == {0, 9 * s} and np.abs(q[:, :2]).max() == 30 and np.abs(q[:, 2]).max() <= 60
        assert not np.array_equal(q, rc._plane_pair(s)) and np.array_equal(np.unique(q, axis=0), np.unique(rc._plane_pair(s), axis=0))
        assert np.array_equal(rc.plane_of(name), (level != 0).astype(np.int64))


# ---- 2. the reference against the n x n restatement ---------------------------------------------------------------------------------------
def same(a, b, where):
    assert rc.bits(a["eps2"])[0] == rc.bits(b["eps2"])[0], where
    for key in ("neighbours", "core", "label", "sizes"):
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (where, key)


SMALL_CASES = [(name, reverse) for name in rc.CLOUDS if name != "lattice52" for reverse in ((False, True) if name in rc.REVERSED_TOO else (False,))]


@pytest.mark.parametrize("name,reverse", SMALL_CASES, ids=[f"{n}-{'reversed' if r else 'shuffled'}" for n, r in SMALL_CASES])
def test_integer_reference_equals_the_restatement_in_every_array(name, reverse):
    pts = rc.cloud(name, reverse)
    assert len(pts) <= rc.SMALL
    for radius in rc.radii(name):
        same(rc.reference(name, radius, reverse=reverse), restate(pts, float(rc.EPS[radius]), rc.min_points(name, radius)), (name, reverse, radius))


def test_integer_reference_of_the_duplicates_at_eps2_zero_and_of_everything():
    pts = rc.cloud("duplicates")
    for m in (31, 32, 41):
        same(rc.reference("duplicates", "0", m), restate(pts, float(rc.EPS["0"]), m), m)
    assert sorted(set(rc.reference("duplicates", "0", 31)["neighbours"])) == [1, 31, 40]
    same(rc.reference("duplicates", "1", 41), restate(pts, float(rc.EPS["1"]), 41), "the 40 copies are not core")
    for n, m in ((129, 1), (129, 129), (129, 130)):
        p = np.ascontiguousarray(np.random.default_rng(n).uniform(-1.0, 1.0, (n, 3)).astype(f32))
        with np.errstate(over="ignore"):
            same(rc.everything(n, m, np.inf), restate(p, 2e19, m), (n, m))


# ---- 3. ties at the radius across the tree ------------------------------------------------------------------------------------------------
# cloud -> radius -> the least number of rows with a neighbour at exactly d2 == eps2 in another super-leaf, in another top box (both orders)
ACROSS = {
    "box2049": {"1": (1, 0), "3": (1, 0)},
    "box2048+31": {"1": (31, 0), "3": (100, 0)},
    "box2048+32": {"1": (32, 0), "3": (100, 0)},
    "box2048+33": {"1": (33, 0), "3": (100, 0)},
    "lattice4097": {"1": (100, 0), "3": (1000, 0)},
    "plane": {"1": (80, 0), "3": (100, 0)},
    "lattice52": {"1": (40000, 1000), "3": (100000, 1000)},
    "tilted_pair": {"3": (100, 0)},
    "tilted_pair_wide": {"9": (1000, 0)},
}


@pytest.mark.parametrize("name", rc.TIE_LATTICES)
def test_ties_at_the_radius_reach_across_super_leaves_and_top_boxes(name):
    for reverse in (False, True):
        slot = rc.slots(name, reverse)
        assert np.array_equal(np.sort(slot), np.arange(len(slot)))
        for radius in ("1", "3", "9"):
            if radius not in rc.radii(name) or (name in rc.PLANE_PAIRS and radius == "1"):
                continue
            tie = rc.rows_with_a_tie_elsewhere(name, radius, reverse)
            got = int(tie["super"].sum()), int(tie["top"].sum())
            print(f"{name} {'reversed' if reverse else 'shuffled'} eps = {radius}: {got[0]} rows with a neighbour at d2 == eps2 in another super-leaf, {got[1]} in another top box")
            assert tie["any"].all(), (name, radius, "a row without a neighbour at exactly the radius")
            if name == "box2048":
                assert got == (0, 0) and slot.max() < rc.SUPER
            else:
                need = ACROSS[name][radius]
                assert got[0] >= need[0] and got[1] >= need[1], (name, radius, got, need)
            if name != "lattice52":
                assert slot.max() < rc.TOP and got[1] == 0
    if name == "box2049":  # one point behind the boundary
        assert int((rc.slots(name) >= rc.SUPER).sum()) == 1
    if name == "lattice52":
        assert int((rc.slots(name) >= rc.TOP).sum()) == 140608 - 131072


# ---- 4. kinds of point ------------------------------------------------------------------------------------------------------------------
def kinds(ref):
    core, label = ref["core"], ref["label"]
    return int(core.sum()), int(((label >= 0) & ~core).sum()), int((label < 0).sum())


@pytest.mark.parametrize("name", rc.TIE_LATTICES + ("plates", "tilted_lattice"))
def test_core_border_and_noise_points_occur(name):
    for radius in rc.radii(name):
        core, border, noise = kinds(rc.reference(name, radius))
        n = len(rc.cloud(name))
        print(f"{name} eps = {radius}, min_points = {rc.min_points(name, radius)}: {core} core, {border} border, {noise} noise")
        if radius == "1" and (name in rc.PLANE_PAIRS or name == "tilted_lattice"):  # no pair within eps: n clusters of one point
            assert (core, border, noise) == (n, 0, 0) and len(rc.reference(name, radius)["sizes"]) == n
            continue
        assert core >= n // 4 and border >= n // 50 and core + border + noise == n
        if name in rc.VOLUMES or radius == "1" or (name, radius) == ("tilted_pair_wide", "9-"):
            assert noise >= 1
        else:  # as found: a corner of a planar lattice, or an edge of a plane pair, still has a core point within the radius
            assert noise == 0
    if name == "box2048":
        assert kinds(rc.reference(name, "1"))[0] == 1176 and kinds(rc.reference(name, "3"))[0] == 1032
    if name in rc.PLANE_PAIRS:  # the one offset that joins the planes decides between one cluster and two
        whole, below = rc.radii(name)[-2:]
        assert len(rc.reference(name, whole)["sizes"]) == 1 and len(rc.reference(name, below)["sizes"]) == 2


# ---- 5. border ties ---------------------------------------------------------------------------------------------------------------------
# cloud -> the least number of tied border rows at the radii with ties and just below, and of those split over two super-leaves
BORDER_TIES = {"box2048": (100, 0), "box2049": (100, 0), "box2048+31": (100, 0), "box2048+32": (100, 0), "box2048+33": (100, 0), "lattice4097": (100, 1),
               "lattice52": (100, 10), "tilted_pair": (100, 0), "tilted_pair_wide": (100, 0)}


@pytest.mark.parametrize("name", sorted(BORDER_TIES))
def test_border_rows_whose_label_the_index_decides(name):
    for reverse in (False, True) if name in rc.REVERSED_TOO else (False,):
        for radius in rc.radii(name):
            tied, split, _ = rc.border_ties(name, radius, reverse)
            print(f"{name} {'reversed' if reverse else 'shuffled'} eps = {radius}: {len(tied)} border rows with tied nearest core neighbours, {len(split)} with them in different super-leaves")
            if radius != "1":
                assert len(tied) >= BORDER_TIES[name][0] and len(split) >= BORDER_TIES[name][1], (name, reverse, radius, len(tied), len(split))
    tied, split, _ = rc.border_ties("plane", "3")
    assert len(tied) == 0 and len(split) == 0  # as found, see the head of this file


def test_the_striped_cloud_has_border_rows_tied_between_two_clusters():
    """every cloud above is ONE cluster at its larger radii: whichever tied core neighbour wins, the label is the same.  Here the tied
    neighbours of a border row between two slabs belong to different clusters, so the label says which of them won"""
    for reverse in (False, True):
        ref = rc.reference("striped", "1", reverse=reverse)
        core, border, noise = kinds(ref)
        tied, split, contested = rc.border_ties("striped", "1", reverse)
        label, q = ref["label"], rc.integer_coordinates(rc.cloud("striped", reverse))[0]
        between = np.isin(q[:, 0], rc.STRIPED_SPARSE)
        lower = {-3: -4, 0: -1, 3: 2}  # the layer below a sparse one
        took_lower = np.array([label[r] == label[np.flatnonzero((q == [lower[q[r, 0]], q[r, 1], q[r, 2]]).all(axis=1))[0]] for r in contested])
        print(f"striped {'reversed' if reverse else 'shuffled'}: {core} core, {border} border, {noise} noise, {len(ref['sizes'])} clusters; {len(tied)} tied border rows, "
              f"{len(contested)} between two clusters ({int(took_lower.sum())} join the slab below them), {len(np.intersect1d(split, contested))} of those with the partners in different super-leaves")
        assert len(ref["sizes"]) == 4 and not ref["core"][between].any()
        assert len(contested) >= 500 and between[contested].all() and len(np.intersect1d(split, contested)) >= 1  # 3 here: the k-d cuts run along x
        assert 100 <= took_lower.sum() <= len(contested) - 100  # both outcomes occur: the caller order, not the geometry, decides


# ---- 6. the plane pairs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.PLANE_PAIRS))
def test_the_partner_across_is_the_only_neighbour_in_the_other_plane(name):
    s = rc.PLANE_PAIRS[name]
    whole = rc.radii(name)[-2]
    for reverse in (False, True):
        pos, slot, plane = rc.positions(name, reverse), rc.slots(name, reverse), rc.plane_of(name, reverse)
        row = pos.first
        offsets, d = rc.ball(rc.R2[whole])
        for o in offsets:
            u, v = pos.shifted(o)
            across = plane[row[u]] != plane[row[v]]
            assert (across.all() if tuple(int(c) for c in o) in ((2 * s, 2 * s, s), (-2 * s, -2 * s, -s)) else not across.any()), o
        u, v = pos.shifted((2 * s, 2 * s, s))
        i, j = row[u], row[v]
        assert len(i) >= 2000 and (plane[i] == 0).all() and (plane[j] == 1).all()
        leaf = slot // rc.LEAF
        leaves = int(leaf.max()) + 1
        in0, in1 = np.bincount(leaf[plane == 0], minlength=leaves), np.bincount(leaf[plane == 1], minlength=leaves)
        pure = (in0 == 0) | (in1 == 0)
        behind = (leaf[i] != leaf[j]) & pure[leaf[j]]  # the partner's leaf lies in the other plane alone: its slab is at distance exactly eps
        behind_back = (leaf[i] != leaf[j]) & pure[leaf[i]]
        print(f"{name} {'reversed' if reverse else 'shuffled'}: {len(i)} pairs across, {int((leaf[i] != leaf[j]).sum())} in different leaves; {int(pure.sum())} of {leaves} leaves lie "
              f"in one plane; {int(behind.sum()) + int(behind_back.sum())} rows have their partner in such a leaf")
        if name == "tilted_pair":
            assert not pure.any()  # as found: the planes are closer than a leaf is wide
        else:
            assert pure.sum() >= leaves // 2 and int(behind.sum()) + int(behind_back.sum()) >= 1000
