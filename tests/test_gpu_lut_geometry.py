"""GPU: the distance LUT, its lookups and the bounds kernel at the grid shapes where the addressing changes (tests/lut_geometry_cases.py:
one-node and two-node axes, every remainder of the apron bricks, the apron copy's 10-bit index limit on each axis, the longest axis, both
sides of the 24-bit row limit of the narrow texel addressing, the cell shift of the tick sort) — every check against the CPU oracle or
the numpy restatement (tests/test_lut_geometry_host.py verifies those two at the same shapes), never against another device path.

A mistake at one of these boundaries would not fault: some points would read a neighbouring texel and the bounds would stay plausible.
Hence the per-point check: on a trimmed context the device hands back the per-point value behind a bound, which must equal the
restatement's bit for bit — a single misread texel cannot pass it."""
import time

import numpy as np
import pytest

from oracle import np_restatement as npr
from tests import lut_geometry_cases as lg

pytestmark = pytest.mark.gpu
f32 = np.float32
REL = lg.REL

# every grid with the default cloud; the small grids also with a cloud on either side of half a point per face voxel
CASES = [(g, lg.NS) for g in lg.GRIDS] + [(g, n) for g in lg.SMALL_GRIDS for n in lg.threshold_ns(g)]
CASE_IDS = [f"{lg.grid_id(g)}-ns{n}" for g, n in CASES]

_refs = {}


def _ref(oracle, dims, ns=lg.NS):
    """the case and everything the oracle says about it, computed once per (grid, cloud) and shared"""
    key = (tuple(dims), ns)
    if key not in _refs:
        t0 = time.perf_counter()
        c = lg.make_case(dims, ns)
        orc = oracle.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
        assert orc.lut_dims() == tuple(dims)
        rn, k = c["rn"], int(0.8 * ns)
        ref = dict(case=c, orc=orc, k=k, queries=lg.lookup_queries(c), full={}, trimmed={}, oracle_seconds=0.0)
        ref["lut"] = orc.lut_get()
        ref["search"] = orc.lut_search(ref["queries"])
        for fix in (True, False):
            ref["full"][fix] = orc.compute_bounds(rn.q.R, rn.span, c["tnodes"], fix)
        if 1 <= k < ns:
            orc.set_inliers(k)
            for fix in (True, False):
                ref["trimmed"][fix] = orc.compute_bounds(rn.q.R, rn.span, c["tnodes"], fix)
            orc.set_inliers(0)
        ref["oracle_seconds"] = time.perf_counter() - t0
        _refs[key] = ref
    return _refs[key]


def _check_sums(got, want, what):
    (lb, ub), (lbo, ubo) = got, want
    assert np.max(np.abs(ub.astype(np.float64) - ubo) / np.maximum(np.abs(ubo.astype(np.float64)), 1e-30)) <= REL, (what, ub, ubo)
    # lower bounds can be exactly 0: compared absolutely against the ub scale, as tests/test_gpu_ops.py::test_bounds_batch_parity does
    assert np.max(np.abs(lb.astype(np.float64) - lbo)) <= REL * float(np.max(ubo)), (what, lb, lbo)


def _check_per_point(hip, ref, lut, quant=True, tnodes=None):
    """fgoicp_bounds_point_distances against the restatement on the device's own LUT, bit for bit (the context must be trimmed)"""
    c = ref["case"]
    rn = c["rn"]
    for fix in (True, False):
        for t in (c["tnodes"] if tnodes is None else tnodes):
            e = hip.point_distances(rn.q.R, rn.span, t, fix)
            want = npr.point_distances(lut, c["bounds"], c["res"], c["src"], rn.q.R, rn.span, t, fix, quant=quant)
            bad = np.flatnonzero(e.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (fix, t, bad[:8], e[bad[:8]], want[bad[:8]], lg.lower_texels(c, t)[bad[:8]])


@pytest.fixture(scope="module", params=CASES, ids=CASE_IDS)
def pair(request, fg, oracle, gpu_required):
    """the context pair of one grid: the device's and the oracle's, with the same node counts"""
    dims, ns = request.param
    ref = _ref(oracle, dims, ns)
    c = ref["case"]
    t0 = time.perf_counter()
    hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
    made = time.perf_counter() - t0
    assert hip.lut_dims() == ref["orc"].lut_dims() == tuple(dims)
    print(f"[lut geometry] {lg.grid_id(dims)} ns={ns}: oracle {ref['oracle_seconds']:.2f} s, device context {made:.2f} s, info {hip.info()}")
    yield hip, ref
    hip.close()


def test_the_shipped_build_picks_the_layout_and_item_size_of_the_grid(pair):
    """4 (apron-bricked quads) on the sparse grids up to a padded 1023, 2 (quad runs) from a padded 1024 on — the shipped build's only way
    into that layout —, 1 (z-pairs) from half a source point per face voxel on; the item size follows the same density."""
    hip, ref = pair
    dims, ns = ref["case"]["dims"], len(ref["case"]["src"])
    info = hip.info()
    layout, item = lg.expected_layout_and_item(dims, ns)
    assert info["lut_dims"] == dims and info["lut_layout"] == layout and info["points_per_item"] == item, info
    if ns / lg.face_voxels(dims) < 0.5:
        assert layout == (2 if max(dims) + 2 >= 1024 else 4)
    cls = lg.class_of(dims)
    if ns == lg.NS and cls in ("apron_10_bit_limit", "largest_axis", "row_limit_24_bit"):
        assert (layout, item) == ((4, 256) if max(dims) == 1021 else (2, 256))
    if ns == lg.NS and cls in ("single_node", "one_node_axis", "two_node_axes", "apron_remainder"):
        assert (layout, item) == (1, 2048)
    if ns != lg.NS:
        below, at = lg.threshold_ns(dims)
        assert layout == (4 if ns == below else 1)


def test_lut_nodes_bit_exact(pair):
    hip, ref = pair
    a = hip.lut_read()
    assert a.shape == ref["lut"].shape and np.array_equal(a.view(np.uint32), ref["lut"].view(np.uint32))


def test_lut_search_bit_exact(pair):
    """inside, on nodes, on texel centres, on the ties of the 1.8 fixed-point weight, half a voxel outside each face, far outside"""
    hip, ref = pair
    got = hip.lut_search(ref["queries"])
    bad = np.flatnonzero(got.view(np.uint32) != ref["search"].view(np.uint32))
    assert bad.size == 0, (bad[:8], ref["queries"][bad[:8]], got[bad[:8]], ref["search"][bad[:8]])


def test_bound_sums_match_the_oracle(pair):
    hip, ref = pair
    c = ref["case"]
    for fix in (True, False):
        _check_sums(hip.compute_sse_error(c["rn"], c["tnodes"], fix), ref["full"][fix], (c["dims"], fix))


def test_per_point_lookups_of_the_bounds_kernel_bit_exact(pair):
    """trimmed context: the per-point values of every translation node, both kinds of rotation node — and the trimmed sums"""
    hip, ref = pair
    if not ref["trimmed"]:
        assert len(ref["case"]["src"]) == 1  # one point cannot be trimmed; its sums are checked above
        return
    lut = hip.lut_read()
    hip.set_inliers(ref["k"])
    try:
        _check_per_point(hip, ref, lut)
        c = ref["case"]
        for fix in (True, False):
            _check_sums(hip.compute_sse_error(c["rn"], c["tnodes"], fix), ref["trimmed"][fix], (c["dims"], fix, "trimmed"))
    finally:
        hip.set_inliers(0)


def test_the_exact_side_matches_the_oracle(pair, fg):
    """exact SSE and the correspondences: the scan seeds its bound with a LUT node clamped into the same grid, so a wrong node there shows
    as a wrong neighbour"""
    hip, ref = pair
    c, orc = ref["case"], ref["orc"]
    rng = np.random.default_rng(3)
    for t in (c["tnodes"][0][:3], c["tnodes"][2][:3], c["tnodes"][-1][:3]):
        R = c["rn"].q.R
        a, b = float(hip.compute_sse_error(R, t)), float(orc.compute_sse_error(R, t))
        assert abs(a - b) <= REL * b
        w = (c["src"] @ R.T + t).astype(f32)
        assert np.array_equal(hip.procrustes(w)[4], orc.procrustes(w)[4])
    R = fg.synth.random_rotation(rng, 50.0).astype(f32)
    a, b = float(hip.compute_sse_error(R, c["centre"])), float(orc.compute_sse_error(R, c["centre"]))
    assert abs(a - b) <= REL * b


@pytest.mark.parametrize("dims", lg.ONE_PER_CLASS, ids=lg.grid_id)
def test_unquantised_weights_at_every_class_of_grid(fg, oracle, gpu_required, dims):
    """FLAG_NO_WEIGHT_QUANT: the lookups against the oracle's, the bounds kernel's per-point values against the restatement's"""
    ref = _ref(oracle, dims)
    c = ref["case"]
    hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]), flags=fg.FLAG_NO_WEIGHT_QUANT)
    orc = oracle.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]), build_lut=False, quantize=False)
    orc.lut_set(ref["lut"])
    assert np.array_equal(hip.lut_search(ref["queries"]).view(np.uint32), orc.lut_search(ref["queries"]).view(np.uint32))
    hip.set_inliers(ref["k"])
    _check_per_point(hip, ref, ref["lut"], quant=False)
    hip.close()


def test_one_node_past_the_largest_axis_is_refused(fg, gpu_required):
    for dims in ((4095, 4, 4), (4, 4095, 4), (4, 4, 4095)):
        bounds, res = lg.geometry(dims)
        pts = np.zeros((4, 3), f32)
        with pytest.raises(fg.FgoicpError, match="out of range"):
            fg.Registration(pts, pts, bounds, float(res))


def _tick(c, rng, rows_per_group):
    """groups of one tick: the case's rotation node with both kinds of bound, and a second rotation; translation nodes all over the box"""
    from fgoicp_amd.nodes import RotNode
    lo, hi = c["bounds"][:, 0], c["bounds"][:, 1]
    nodes = [c["rn"], c["rn"], RotNode(-0.25, 0.125, 0.0625, 0.0625), c["rn"], c["rn"], RotNode(0.0, 0.0, 0.0, 0.015625)]
    fixes = [True, False, False, True, False, True]
    groups = []
    for g in range(len(nodes)):
        t = c["centre"] + rng.uniform(-0.6, 0.6, (rows_per_group, 3)) * (hi - lo)
        groups.append(np.concatenate([t, rng.choice([0.0, 0.005, 0.02, 0.1], (rows_per_group, 1))], 1).astype(f32))
    return nodes, fixes, groups


@pytest.mark.parametrize("dims", lg.GRID_CLASSES["sort_cell_shift"], ids=lg.grid_id)
def test_sorted_tick_at_the_cell_shift_edges(fg, oracle, gpu_required, dims):
    """32 / 33 and 64 / 65 nodes on the long axis: the tick sort shifts node indices by 0 / 1 and 1 / 2 bits into its 5 bits per axis.  A
    tick of more items than the small-tick limit is sorted; its rows are, bit for bit, the rows of the unsorted per-group calls, and those
    match the oracle."""
    ref = _ref(oracle, dims)
    c, orc = ref["case"], ref["orc"]
    hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
    info = hip.info()
    nodes, fixes, groups = _tick(c, np.random.default_rng(11), 700)
    assert info["items_per_evaluation"] * sum(len(g) for g in groups) > 4096 >= info["items_per_evaluation"] * 700
    before = hip.sort_fallbacks()
    tick = hip.compute_bounds_multi([n.q.R for n in nodes], [n.span for n in nodes], fixes, groups)
    after = hip.sort_fallbacks()
    assert after[0] - before[0] > 0 and after[1] == 0
    for n, fix, g, (lb, ub) in zip(nodes, fixes, groups, tick):
        lb1, ub1 = hip.compute_sse_error(n, g, fix)
        assert np.array_equal(lb.view(np.uint32), lb1.view(np.uint32)) and np.array_equal(ub.view(np.uint32), ub1.view(np.uint32))
        _check_sums((lb1, ub1), orc.compute_bounds(n.q.R, n.span, g, fix), (dims, fix))
    assert hip.sort_fallbacks() == after  # the per-group calls were small ticks
    hip.close()


# ---- development build: every layout meets every geometry, through the sort ----
@pytest.mark.parametrize("layout", [1, 2, 4])
@pytest.mark.parametrize("dims", lg.GRIDS, ids=[lg.grid_id(g) for g in lg.GRIDS])
def test_forced_layouts_at_every_grid(fg, oracle, gpu_required, monkeypatch, dims, layout):
    """FGOICP_LUT_ZPAIR = 1 / 2 / 4 on every grid with the 300-point cloud, FGOICP_SMALL_TICK = 0 so that even these ticks are sorted: the
    per-point values against the restatement, the sums (plain and trimmed) against the oracle.  The apron layout on a grid above its 10-bit
    limit must fall back to the quad runs."""
    monkeypatch.setenv("FGOICP_LUT_ZPAIR", str(layout))
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    ref = _ref(oracle, dims)
    c = ref["case"]
    rn = c["rn"]
    hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
    assert hip.info()["lut_layout"] == (2 if layout == 4 and max(dims) + 2 >= 1024 else layout)
    lut = hip.lut_read()
    assert np.array_equal(lut.view(np.uint32), ref["lut"].view(np.uint32))
    fixes = [True, False]
    got = hip.compute_bounds_multi([rn.q.R, rn.q.R], [rn.span, rn.span], fixes, [c["tnodes"], c["tnodes"]])
    for fix, rows in zip(fixes, got):
        _check_sums(rows, ref["full"][fix], (dims, layout, fix))
    sorted_ticks, fallbacks = hip.sort_fallbacks()
    assert sorted_ticks > 0 and fallbacks == 0
    hip.set_inliers(ref["k"])
    _check_per_point(hip, ref, lut)
    got = hip.compute_bounds_multi([rn.q.R, rn.q.R], [rn.span, rn.span], fixes, [c["tnodes"], c["tnodes"]])
    for fix, rows in zip(fixes, got):
        _check_sums(rows, ref["trimmed"][fix], (dims, layout, fix, "trimmed"))
    assert hip.sort_fallbacks()[1] == 0
    hip.close()
