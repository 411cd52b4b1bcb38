"""CPU: the two checkers of tests/test_gpu_lut_geometry.py — the C++ oracle and the numpy restatement — at the grid shapes of
tests/lut_geometry_cases.py, against a hand-derived case, a metamorphic property and each other; and the proof that the clouds of those
cases really reach the boundaries the GPU tests are about (a test on inputs that never touch node d - 1 of the long axis proves nothing)."""
import numpy as np
import pytest

from oracle import np_restatement as npr
from tests import lut_geometry_cases as lg

f32 = np.float32
IDS = [lg.grid_id(g) for g in lg.GRIDS]


@pytest.fixture(scope="module")
def built(oracle):
    """(case, oracle registration, its LUT) per grid, made once"""
    cache = {}

    def get(dims):
        if dims not in cache:
            c = lg.make_case(dims)
            orc = oracle.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
            assert orc.lut_dims() == dims == npr.lut_dims(c["bounds"], c["res"])
            cache[dims] = (c, orc, orc.lut_get())
        return cache[dims]
    return get


def test_single_node_grid_by_hand(oracle, built):
    """1x1x1: the padded LUT holds one value T0 = the smallest squared distance from the node (the lower corner of the bounds) to a target
    point.  All eight texels of every footprint are that value and fma(w, q - p, p) with q == p is p, so every lookup has the bits of T0
    whatever the query; with no rotation slack and a span-zero translation node every per-point value is sqrtf(T0)."""
    c, orc, lut = built((1, 1, 1))
    shifted = (c["tgt"] + (-c["bounds"][:, 0])[None, :]).astype(f32)  # the targets as the LUT sees them: the node is the origin
    T0 = npr.dist_sq(shifted, np.zeros((1, 3), f32)).min()
    assert lut.shape == (1, 1, 1) and lut[0, 0, 0].view(np.uint32) == T0.view(np.uint32)
    rng = np.random.default_rng(1)
    q = np.concatenate([rng.uniform(-3, 3, (500, 3)), lg.lookup_queries(c)[:-4], [[1e6, -1e6, 0.0]]]).astype(f32)
    for got in (orc.lut_search(q), npr.lut_search(lut, c["bounds"], c["res"], q)):
        assert np.all(got.view(np.uint32) == T0.view(np.uint32))
    for R in (np.eye(3, dtype=f32), c["rn"].q.R):
        for t in c["tnodes"]:
            e = npr.point_distances(lut, c["bounds"], c["res"], c["src"], R, 0.0, [t[0], t[1], t[2], 0.0], True)
            assert np.all(e.view(np.uint32) == np.sqrt(T0).view(np.uint32))
            lb, ub = orc.compute_bounds(R, 0.0, np.array([[t[0], t[1], t[2], 0.0]], f32), True)
            want = float((np.sqrt(T0) * np.sqrt(T0)).astype(f32)) * len(c["src"])
            assert lg.close_rel(ub, want) and lg.close_rel(lb, want)


@pytest.mark.parametrize("dims", lg.GRID_CLASSES["one_node_axis"], ids=lg.grid_id)
def test_one_node_axis_ignores_its_coordinate(oracle, built, dims):
    """Both texels of a one-node axis are the same node: moving a query along that axis changes no bit of the lookup."""
    c, orc, lut = built(dims)
    axis = dims.index(1)
    q = lg.lookup_queries(c)[:-4]
    rng = np.random.default_rng(2)
    ref_o = orc.lut_search(q)
    ref_n = npr.lut_search(lut, c["bounds"], c["res"], q)
    assert len(np.unique(ref_o)) > 50  # the other two axes do matter
    for move in (rng.uniform(-2, 2, len(q)), np.full(len(q), 1e4), np.full(len(q), -float(c["res"]) * 0.25)):
        q2 = q.copy()
        q2[:, axis] = (q[:, axis] + move).astype(f32)
        assert np.array_equal(orc.lut_search(q2).view(np.uint32), ref_o.view(np.uint32))
        assert np.array_equal(npr.lut_search(lut, c["bounds"], c["res"], q2).view(np.uint32), ref_n.view(np.uint32))


@pytest.mark.parametrize("dims", lg.GRIDS, ids=IDS)
def test_oracle_lookups_equal_the_restatement(built, dims):
    """lut_search of the oracle and of the restatement on the oracle's LUT: bit for bit, at every kind of query the GPU test uses"""
    c, orc, lut = built(dims)
    q = lg.lookup_queries(c)[:-4]  # (the restatement's fma emulation is not meant for infinities)
    assert np.array_equal(orc.lut_search(q).view(np.uint32), npr.lut_search(lut, c["bounds"], c["res"], q).view(np.uint32))


@pytest.mark.parametrize("fix_rot", [True, False])
@pytest.mark.parametrize("dims", lg.GRIDS, ids=IDS)
def test_oracle_sums_equal_the_restatement(built, dims, fix_rot):
    """fp64 sums of the restatement's per-point terms (e * e for the upper bound, max(e - sqrt3 * span, 0)^2 for the lower) against the
    oracle's bounds, 1e-6 relative: both sides hold the same fp32 terms and add them in fp64."""
    c, orc, lut = built(dims)
    rn = c["rn"]
    lbo, ubo = orc.compute_bounds(rn.q.R, rn.span, c["tnodes"], fix_rot)
    for t, lb1, ub1 in zip(c["tnodes"], lbo, ubo):
        e = npr.point_distances(lut, c["bounds"], c["res"], c["src"], rn.q.R, rn.span, t, fix_rot)
        lb, ub = lg.restated_sums(e, t[3])
        assert lg.close_rel(ub, ub1) and lg.close_rel(lb, lb1), (t, lb, lb1, ub, ub1)
    assert float(ubo.max()) > 0


@pytest.mark.parametrize("dims", lg.GRIDS, ids=IDS)
def test_the_clouds_reach_the_boundaries(dims):
    """Footprints (floor(u - 0.5) per axis, clamped) of the case's cloud under its translation nodes, in the restatement's arithmetic:
    some point has its lower texel at -1 on every axis, some point at d - 1 on every axis, every index in between occurs on a short axis
    and both halves of a long one are populated.  On the two addressing grids the highest row of a footprint — texel (y1, z1) =
    (y0 + 1, z0 + 1), row (z0 + 2) * py + (y0 + 2) of the padded LUT — reaches 2^23 - py, on the wide one 2^23; the lower texel's own row
    (z0 + 1) * py + (y0 + 1) reaches its maximum dz * py + dy, which is 2^23 - py - 2 on the narrow grid and 2^23 - 2 on the wide one."""
    c = lg.make_case(dims)
    d = np.asarray(dims)
    fl = np.concatenate([lg.lower_texels(c, t) for t in c["tnodes"]])
    centre_only = lg.lower_texels(c, c["tnodes"][0])
    assert np.any(np.all(centre_only == -1, axis=1)) and np.any(np.all(centre_only == d - 1, axis=1))
    for a in range(3):
        seen = np.unique(fl[:, a])
        assert seen[0] == -1 and seen[-1] == d[a] - 1
        if d[a] <= 33:
            assert len(seen) == d[a] + 1, (a, seen)
        else:
            assert np.sum(seen < d[a] // 8) >= 3 and np.sum(seen > d[a] - d[a] // 8) >= 3 and len(seen) > 60, (a, len(seen))
    if dims in lg.ADDRESSING_GRIDS:
        py = dims[1] + 2
        low_row = (fl[:, 2] + 1) * py + (fl[:, 1] + 1)
        top_row = (fl[:, 2] + 2) * py + (fl[:, 1] + 2)
        assert low_row.max() == dims[2] * py + dims[1]
        assert top_row.max() >= 2 ** 23 - py
        assert (top_row.max() >= 2 ** 23) == (dims == lg.WIDE_GRID)
        assert (py * (dims[2] + 2) > 2 ** 23) == (dims == lg.WIDE_GRID)
        assert np.sum(top_row >= 2 ** 23 - 4 * py) >= 8  # not the clamped corner point alone


def test_the_table_covers_every_layout_and_item_size():
    """what the shipped build derives for the cases of the GPU test (restated rule): all three layouts and all four item sizes occur"""
    seen = {lg.expected_layout_and_item(g, lg.NS) for g in lg.GRIDS}
    for g in lg.SMALL_GRIDS:
        below, at = lg.threshold_ns(g)
        assert below >= 1 and lg.expected_layout_and_item(g, below)[0] == 4 and lg.expected_layout_and_item(g, at)[0] == 1
        seen |= {lg.expected_layout_and_item(g, below), lg.expected_layout_and_item(g, at)}
    assert {s[0] for s in seen} == {1, 2, 4} and {s[1] for s in seen} == {256, 512, 1024, 2048}
    for g in lg.GRIDS:
        assert (lg.expected_layout_and_item(g, lg.NS)[0] == 2) == (max(g) + 2 >= 1024 and lg.NS / lg.face_voxels(g) < 0.5)
