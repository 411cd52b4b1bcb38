"""No GPU: tests/nn_restatement.py against an fp64 exact nearest neighbour, and every designed input of tests/test_gpu_nn_scan.py against
the property it is designed for."""
import numpy as np
import pytest

from tests import nn_restatement as nr

f32 = np.float32


def _tie_counts(pct, q):
    """per query: how many targets attain the smallest fp32 squared distance"""
    d2 = nr._dist_sq(np.asarray(q, f32), np.asarray(pct, f32))
    return (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1), d2


@pytest.mark.parametrize("nt,ns,seed", [(3000, 500, 0), (33, 64, 1), (1, 5, 2)])
def test_restatement_is_the_exact_nearest_neighbour_to_rounding(nt, ns, seed):
    """the fp32 minimum lies within 4e-7 relative of the fp64 one (the rounding bound csrc/device/bvh.hpp states), the index attains the
    smallest square root and is the first to do so"""
    rng = np.random.default_rng(seed)
    pct = rng.uniform(-0.5, 0.5, (nt, 3)).astype(f32)
    q = nr.query_mix(rng, pct, ns)
    idx, d2 = nr.brute_force(pct, q, nr.I3, nr.ZERO3)
    exact = nr.exact_min_d2(pct, q)
    assert np.all(np.abs(d2.astype(np.float64) - exact) <= 4e-7 * exact)
    all_d2 = nr._dist_sq(q, pct)
    roots = np.sqrt(all_d2)
    assert np.array_equal(np.sqrt(d2), roots.min(axis=1)) and np.array_equal(roots[np.arange(ns), idx], roots.min(axis=1))
    assert np.array_equal(idx, (roots == roots.min(axis=1, keepdims=True)).argmax(axis=1))
    assert np.array_equal(nr.bits(nr._moved(nr.I3, nr.ZERO3, q)), nr.bits(q))  # the identity moves nothing, bit for bit
    # the chunking changes nothing
    idx1, d21 = nr.brute_force(pct, q, nr.I3, nr.ZERO3, chunk=7)
    assert np.array_equal(idx, idx1) and np.array_equal(nr.bits(d2), nr.bits(d21))


def test_node_restatement_is_the_exact_minimum_to_rounding():
    c = nr.tree_edge_case(2049)
    ref = nr.reference(c)
    assert len(ref["xyz"]) == 256 and len(np.unique(ref["xyz"][:8], axis=0)) == 8
    dims = nr.lut_dims(c.bounds, c.res)
    assert dims == (16, 16, 16) and ref["xyz"].min() == 0 and np.array_equal(ref["xyz"].max(axis=0), np.array(dims) - 1)
    # the definition's operands are fp32: the targets shifted by the bounds, the node index times the resolution (registration.cu:265, :289-296)
    shifted = (c.pct + (-c.bounds[:, 0])[None, :]).astype(f32)
    exact = nr.exact_min_d2(shifted, (ref["xyz"].astype(f32) * f32(c.res)).astype(f32))
    assert np.all(np.abs(ref["nodes"].astype(np.float64) - exact) <= 4e-7 * exact)


def test_mixed_set_has_one_far_query_among_near_ones():
    """the far query's nearest distance is at least 100 x the largest near one, in every tree-edge case that holds a whole mixed set"""
    for nt in (1, 31, 32, 33, 2048, 2049, 4097):
        c = nr.tree_edge_case(nt)
        assert len(c.pct) == nt and len(c.q) == 320
        d = np.sqrt(nr.reference(c)["d2"][:64].astype(np.float64))
        near = np.delete(d, nr.FAR_ROW)
        assert d[nr.FAR_ROW] >= 100.0 * near.max() and near.max() > 0.0
    for ns in (1, 63, 64, 65):
        c = nr.tree_edge_case(2049, ns)
        assert len(c.q) == ns
        if ns >= 64:
            d = np.sqrt(nr.reference(c)["d2"][:64].astype(np.float64))
            assert d[nr.FAR_ROW] >= 100.0 * np.delete(d, nr.FAR_ROW).max()


def test_single_point_target_answers_zero():
    c = nr.single_point_case()
    assert len(c.pct) == 2049 and len(np.unique(c.pct, axis=0)) == 1
    assert not nr.reference(c)["idx"].any()


def test_sphere_centre_is_equidistant_to_rounding():
    c = nr.sphere_case()
    assert len(c.pct) == 2049 and len(c.q) == 128 and not c.q[0].any()
    d2 = nr._dist_sq(c.q[:1], c.pct)[0].astype(np.float64)
    assert (d2.max() - d2.min()) / d2.min() < 1e-6
    assert np.all(np.abs(c.q[1:64]).max(axis=1) <= 1e-3)
    assert np.count_nonzero(nr.reference(c)["d2"][64:96] == 0) == 32  # the target points among the queries


def test_lattice_ties():
    cells, faces, rev = nr.lattice_cases()
    assert len(cells.pct) == 4097 and np.array_equal(cells.pct[0], cells.pct[4096]) and max(len(cells.q), len(faces.q), len(rev.q)) <= 320
    n, d2 = _tie_counts(cells.pct, cells.q)
    assert np.all(n == 8) and np.all(d2.min(axis=1) == f32(0.75))  # exactly 8 targets attain the minimal d2
    n, d2 = _tie_counts(faces.pct, faces.q)
    assert n[0] == 9 and n[1] == 2 and set(n[2:]) == {2, 4} and set(d2.min(axis=1)) == {f32(0.0), f32(0.25), f32(0.5), f32(0.75)}
    assert nr.reference(faces)["idx"][0] == 0 and nr.reference(faces)["idx"][1] == 0
    # reversed caller order: the winner is the new lowest index, i.e. the tie set's highest index of the original order
    assert np.array_equal(rev.pct, cells.pct[::-1])
    fwd, _ = nr.brute_force(cells.pct, rev.q, nr.I3, nr.ZERO3)
    d2 = nr._dist_sq(rev.q, cells.pct)
    highest = 4096 - (d2 == d2.min(axis=1, keepdims=True))[:, ::-1].argmax(axis=1)
    back = nr.reference(rev)["idx"]
    assert np.array_equal(4096 - back.astype(np.int64), highest) and np.all(4096 - back.astype(np.int64) != fwd)


def test_sqrt_tie_case_is_decided_by_the_rule_not_the_minimum():
    """for every one of the 16 queries the winner's d2 is not the smallest d2: its partner's is, one ulp below, with the same square root"""
    c = nr.sqrt_tie_case()
    assert len(c.pct) == 2049 and len(c.q) == 64
    ref = nr.reference(c)
    d2 = nr._dist_sq(c.q[:16], c.pct)
    k = np.arange(16)
    assert np.array_equal(ref["idx"][:16], k)  # the partner with the larger square carries the lower caller index, and wins
    assert np.array_equal(d2.argmin(axis=1), 16 + k)
    assert np.array_equal(nr.bits(d2[k, k]), nr.bits(d2[k, 16 + k]) + 1) and np.all(d2[k, k] > ref["d2"][:16])
    assert np.array_equal(np.sqrt(d2[k, k]), np.sqrt(d2[k, 16 + k]))
    assert np.all((np.sqrt(d2) == np.sqrt(d2.min(axis=1, keepdims=True))).sum(axis=1) == 2)  # nobody else is in the tie
    # opposite sides of the query, 41 points behind each partner
    far, near = c.pct[:16] - c.q[:16], c.pct[16:32] - c.q[:16]
    assert np.all((far * near).sum(axis=1) < -0.9 * np.linalg.norm(far, axis=1) * np.linalg.norm(near, axis=1))
    assert np.all(np.linalg.norm((c.pct[:16] - c.pct[16:32]).astype(np.float64), axis=1) > 1.0)
    from tests.test_oracle_kat import sqrt_tie_pair
    a, b = sqrt_tie_pair()
    assert np.array_equal(c.pct[16], a) and np.array_equal(c.pct[0], -b) and not c.q[0].any()
    # the other 48 queries have no tie
    d2o = nr._dist_sq(c.q[16:], c.pct)
    assert np.all((np.sqrt(d2o) == np.sqrt(d2o.min(axis=1, keepdims=True))).sum(axis=1) == 1)


def test_plane_case_is_thin_and_its_queries_are_of_three_kinds():
    c = nr.plane_case()
    assert len(c.pct) == 4097 and len(c.q) == 320 and np.ptp(c.pct[:, 2]) < 1e-3
    d = np.sqrt(nr.reference(c)["d2"].astype(np.float64))
    off = np.abs(c.q[:, 2] - 0.25) >= 1.0
    away = np.abs(c.q[:, 0]) >= 3.0
    assert off.sum() == 80 and away.sum() == 80 and np.all(d[off] >= 1.0) and np.all(d[away] >= 2.5) and np.all(d[~off & ~away] < 1e-3)


def test_every_case_is_small_enough_for_the_numpy_reference():
    cases = [nr.single_point_case(), nr.sphere_case(), nr.sqrt_tie_case(), nr.plane_case(), *nr.lattice_cases()]
    for c in cases:
        assert len(c.pct) <= 4097 and len(c.q) <= 320, c.name
    assert len({c.name for c in cases}) == len(cases)
