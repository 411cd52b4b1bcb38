"""GPU: the box-scan nearest neighbour (csrc/device/kernels.hip: box_walk, box_scan, scan_min_d2; nn_scan_kernel<0>, nn_scan_kernel<1>,
nn_scan_dual_kernel, lut_build_scan_coarse_kernel, lut_build_scan_kernel) at the edges of its tree, of its launch shapes and of its tie
rule, against the numpy brute force of tests/nn_restatement.py, bit for bit.  The queries are passed as the source cloud and the transform
is the identity with a zero translation, so a moved query is the caller's point bit for bit.  Every query of every case is compared.

The inputs and the properties they are designed for: tests/nn_restatement.py, asserted without a GPU by tests/test_nn_restatement_host.py."""
import numpy as np
import pytest

from tests import nn_restatement as nr
from tests.nn_restatement import I3, ZERO3, bits, reference
from tests.test_gpu_ops import REL  # sums over points: identical fp32 terms, fp64 accumulation in another order, rounded once

pytestmark = pytest.mark.gpu
f32 = np.float32


def check_case(fg, case, flags=0):
    """alignment, procrustes, SSE and LUT nodes of one context against the numpy answers of its case"""
    ref = reference(case)
    reg = fg.Registration(case.pct, case.q, case.bounds, case.res, flags=flags)
    try:
        a = reg.alignment(I3, ZERO3)
        wrong = np.flatnonzero((a.indices != ref["idx"]) | (bits(a.dist2) != bits(ref["d2"])))
        assert wrong.size == 0, (case.name, flags, wrong[:8], a.indices[wrong[:8]], ref["idx"][wrong[:8]], a.dist2[wrong[:8]], ref["d2"][wrong[:8]])
        assert np.array_equal(reg.procrustes(case.q)[-1].astype(np.uint32), ref["idx"]), (case.name, flags)
        sse = reg.compute_sse_error(I3, ZERO3)
        assert bits(sse) == bits(a.sse), (case.name, flags)
        assert abs(float(sse) - ref["sse64"]) <= REL * ref["sse64"], (case.name, flags, float(sse), ref["sse64"])
        assert np.array_equal(bits(reg.lut_nodes(ref["xyz"])), bits(ref["nodes"])), (case.name, flags)
    finally:
        reg.close()


# ---- a. tree edges -----------------------------------------------------------------------------------------------------------------
# A leaf holds 32 points, a super-leaf 64 leaves (2048 points), a top box 64 super-leaves (131 072 points): 33, 2049 and 131 073 points
# gain a level, and half of the new level's leaves are empty (inverted boxes, points padded at FLT_MAX).
@pytest.mark.parametrize("nt,ns", [(nt, 320) for nt in (1, 31, 32, 33, 2048, 2049, 4097, 131072, 131073)] + [(2049, ns) for ns in (1, 63, 64, 65)])
def test_tree_edges(fg, gpu_required, nt, ns):
    """FGOICP_FLAG_NO_MORTON keeps the caller's query order on the device (create_source in ctx.hip: the permutation is the identity), so
    the mixed set — 63 near queries and one far one in caller rows 0..63 — is one wave of the scan under that flag; under the default k-d
    order the same queries are dealt to waves of neighbours.  Both orders are checked."""
    case = nr.tree_edge_case(nt, ns)
    for flags in (fg.FLAG_NO_MORTON, 0):
        check_case(fg, case, flags)


@pytest.mark.parametrize("nt", [33, 2049, 131073, 196609])
def test_every_target_point_finds_itself(fg, gpu_required, nt):
    """One point past a full leaf, super-leaf or top box sits ALONE in the new level's second box, and which caller point that is depends on
    the k-d order: with the target as its own query cloud every point of every leaf is somebody's answer — index i at distance 0 (the
    points are distinct), no reference needed.  196 609 points fill half of the second top box."""
    pct = np.random.default_rng(nt).uniform(-0.5, 0.5, (nt, 3)).astype(f32)
    assert len(np.unique(pct, axis=0)) == nt
    for flags in (0, fg.FLAG_NO_MORTON):
        reg = fg.Registration(pct, pct, nr.UNIT_BOX, 1.0 / 16, flags=flags)
        a = reg.alignment(I3, ZERO3)
        wrong = np.flatnonzero((a.indices != np.arange(nt)) | (a.dist2 != 0))
        assert wrong.size == 0, (flags, wrong[:8], a.indices[wrong[:8]], a.dist2[wrong[:8]])
        assert np.array_equal(reg.procrustes(pct)[-1], np.arange(nt)) and reg.compute_sse_error(I3, ZERO3) == 0 == a.sse
        reg.close()


# ---- b. launch shapes --------------------------------------------------------------------------------------------------------------
# launch_nn_scan (kernels.hip), groups = ceil(n / 64) and nparts = 4:
#     while (nparts < 8 && groups * nparts < 4096) nparts <<= 1;    8 waves per group while groups < 1024, i.e. n <= 1023 * 64 = 65 472
#     dyn = groups * nparts <= 8192                                   with 4 waves: dynamic claims while groups <= 2048, i.e. n <= 131 072
# so 65 472 | 65 473 and 131 072 | 131 073 are the two edges between its three shapes (8 waves dynamic, 4 waves dynamic, 4 waves
# round-robin).  Whoever changes either line moves these sizes.
LAUNCH_SIZES = (65472, 65473, 131072, 131073)


@pytest.mark.parametrize("ns", LAUNCH_SIZES)
def test_launch_shapes(fg, gpu_required, ns):
    case = nr.launch_case(ns)
    out = []
    for flags in (0, fg.FLAG_BRUTE_FORCE_NN):
        reg = fg.Registration(case.pct, case.q, case.bounds, case.res, flags=flags)
        a = reg.alignment(I3, ZERO3)
        assert bits(a.sse) == bits(reg.compute_sse_error(I3, ZERO3)), flags
        out.append(a)
        reg.close()
    tree, brute = out
    assert np.array_equal(tree.indices, brute.indices) and np.array_equal(bits(tree.dist2), bits(brute.dist2))
    assert bits(tree.sse) == bits(brute.sse)
    sub = np.arange(4096) * (ns // 4096)  # a fixed-stride subset against numpy
    idx, d2 = nr.brute_force(case.pct, case.q[sub], I3, ZERO3)
    assert np.array_equal(tree.indices[sub], idx) and np.array_equal(bits(tree.dist2[sub]), bits(d2))


# ---- c. the dual walk --------------------------------------------------------------------------------------------------------------
def _rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f32)


def _icp_pair(ns, nt=2049, outliers=0, seed=0):
    """a source that is the target resampled with 1e-2 noise (and `outliers` points of 3 x the box), to be started 10 degrees off"""
    rng = np.random.default_rng(4000 + seed)
    pct = rng.uniform(-0.5, 0.5, (nt, 3)).astype(f32)
    pcs = np.concatenate([nr.near_queries(rng, pct, ns - outliers, noise=1e-2), rng.uniform(-1.5, 1.5, (outliers, 3)).astype(f32)])
    return pct, pcs[rng.permutation(ns)]


def _icp(fg, pct, pcs, flags, k=None, bounds=nr.UNIT_BOX, res=1.0 / 16):
    reg = fg.Registration(pct, pcs, bounds, res, flags=flags)
    if k:
        reg.set_inliers(k)
    icp = fg.IterativeClosestPoint3D(reg, max_iter=3, convergence_threshold=1e-7, R=_rot_z(10.0), t=ZERO3)
    sse, R, t = icp.run()
    reg.close()
    return icp.iterations, sse, R, t


def _same_icp(a, b):
    assert a[0] == b[0] >= 2, (a[0], b[0])  # the same iteration count (an ICP that stops at once compares nothing)
    assert bits(a[1]) == bits(b[1]) and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3])), (a, b)


def test_icp_loops_of_tree_and_brute_force_contexts_agree_at_the_tiny_case(fg, gpu_required, tiny_case):
    """what the comparisons below rest on: the loop over the scans and the loop over the O(ns * nt) kernels return the same bits"""
    c = tiny_case
    _same_icp(_icp(fg, c["pct"], c["pcs"], 0, bounds=c["bounds"], res=c["res"]), _icp(fg, c["pct"], c["pcs"], fg.FLAG_BRUTE_FORCE_NN, bounds=c["bounds"], res=c["res"]))


@pytest.mark.parametrize("ns,k", [(262145, None), (700, 600)], ids=["untrimmed", "trimmed"])
def test_dual_walk_icp_is_the_brute_force_icp(fg, gpu_required, ns, k):
    """nn_scan_dual_kernel serves the ICP of contexts above 262 144 source points (262 145: the first) and of trimmed ones (700 points, 100
    of them outliers: the smallest shape whose walk carries skip lists); three iterations from a 10 degree start against the context of
    the brute-force kernels: the same iteration count and the same bits of sse, R and t"""
    pct, pcs = _icp_pair(ns, outliers=100 if k else 0, seed=ns)
    _same_icp(_icp(fg, pct, pcs, 0, k), _icp(fg, pct, pcs, fg.FLAG_BRUTE_FORCE_NN, k))


# ---- d. geometry -------------------------------------------------------------------------------------------------------------------
def test_target_of_one_repeated_point(fg, gpu_required):
    case = nr.single_point_case()
    assert not reference(case)["idx"].any()  # 2049 copies: every index is 0
    check_case(fg, case)
    check_case(fg, case, fg.FLAG_NO_MORTON)


def test_sphere_seen_from_its_centre(fg, gpu_required):
    """every leaf is a candidate of the centre and of the 63 queries next to it; the caller's order keeps them one wave with nothing else"""
    check_case(fg, nr.sphere_case(), fg.FLAG_NO_MORTON)
    check_case(fg, nr.sphere_case())


@pytest.mark.parametrize("which", [0, 1, 2], ids=["cell_centres", "faces_edges", "reversed"])
def test_lattice_ties_go_to_the_lowest_caller_index(fg, gpu_required, which):
    """8 targets at d2 = 0.75 exactly (cell centres), 4 and 2 (face centres, edge midpoints), 9 with a duplicated point; and the same cloud
    in reversed caller order, where the winner is the new lowest index"""
    check_case(fg, nr.lattice_cases()[which])


def test_sqrt_tie_partners_in_different_leaves(fg, gpu_required):
    """16 queries whose nearest point loses to a partner one ulp farther in d2 with the same fp32 square root and a lower caller index,
    the partners on opposite sides of the query in different leaves: the re-scan's business, in one wave with 48 queries that need none"""
    case = nr.sqrt_tie_case()
    assert np.array_equal(reference(case)["idx"][:16], np.arange(16))
    check_case(fg, case, fg.FLAG_NO_MORTON)
    check_case(fg, case)


def test_planar_target_with_thin_slabs(fg, gpu_required):
    check_case(fg, nr.plane_case())
    check_case(fg, nr.plane_case(), fg.FLAG_NO_MORTON)


# ---- development build: the launch knobs -------------------------------------------------------------------------------------------
def _knob_cases():
    return [nr.tree_edge_case(2049), nr.lattice_cases()[0], nr.sphere_case()]


def _knob_icps(fg):
    pct, pcs = _icp_pair(700, outliers=100, seed=1)
    return _icp(fg, pct, pcs, 0), _icp(fg, pct, pcs, 0, 600)  # the two scans of nn_scan_kernel; the dual walk with skip lists


@pytest.fixture(scope="module")
def default_icps(fg, gpu_required):
    import os
    assert not any(k.startswith("FGOICP_NN_") for k in os.environ)
    return _knob_icps(fg)


@pytest.mark.parametrize("parts,claim,flat", [(p, c, None) for p in (1, 2, 4, 8, 16) for c in (0, 1)] + [(8, None, 1)])
def test_scan_knobs_change_no_bit(fg, gpu_required, monkeypatch, default_icps, parts, claim, flat):
    """FGOICP_NN_PARTS (waves per 64 queries; 1: the wave radius tightens after every leaf), FGOICP_NN_CLAIM (1: candidate leaves claimed
    from an LDS counter, 0: dealt round-robin) and FGOICP_NN_FLAT (the flat form of the walk), read per launch by the development build:
    alignment and LUT nodes against numpy, one untrimmed and one trimmed 3-iteration ICP against the default setting's bits"""
    monkeypatch.setenv("FGOICP_NN_PARTS", str(parts))
    if claim is not None:
        monkeypatch.setenv("FGOICP_NN_CLAIM", str(claim))
    if flat is not None:
        monkeypatch.setenv("FGOICP_NN_FLAT", str(flat))
    for case in _knob_cases():
        check_case(fg, case)
        check_case(fg, case, fg.FLAG_NO_MORTON)
    for got, want in zip(_knob_icps(fg), default_icps):
        _same_icp(got, want)
