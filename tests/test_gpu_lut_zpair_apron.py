"""GPU: the z-pair apron copy of the LUT (layout 6: 4 x 4 z-pairs per 128-byte line, lines overlapping by one x and one y; kernels.hip
zpair_apron_index) — the same texels in the same blend order as every other layout, so every value it yields is compared bit for bit:
per point against the numpy restatement (oracle/np_restatement.py) on the device's own LUT, row for row against the same submissions
under layouts 1 and 4, against the recorded bits of tests/golden/item_kernel_bits.npz, in a fused tick of fgoicp_batch against each
context's own rows, and over a whole certify run against layout 4.

Shapes (tests/lut_geometry_cases.py builds grid and cloud): every remainder of (d - 1) mod 3 on x and on y (2 ... 6 nodes), one-node
axes, two z-nodes (the padded count is d + 2, so a grid has at least three padded slices: the two-node and the one-node z-axis are the
thinnest there are), a padded 1023 on each axis and 1024 (which must fall back to layout 2), both sides of the 4 GiB byte offset of the
narrow addressing; clouds of 1, 63, 64, 65 and 300 points with FGOICP_SMALL_TICK = 0, so that the sorted path runs with odd and even
lanes, a lone lane and a partial last pass.  The shipped build's selection rule (layout 6 where the apron-bricked quads would exceed
256 MiB) is checked on the shipped build at both sides of the rule."""
import os

import numpy as np
import pytest

from oracle import np_restatement as npr
from tests import lut_geometry_cases as lg

pytestmark = pytest.mark.gpu
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_kernel_bits.npz")

REMAINDER_GRIDS = [(2, 3, 4), (3, 4, 5), (4, 5, 6), (5, 6, 2), (6, 2, 3)]  # 2 ... 6 nodes on x and on y: (d - 1) mod 3 = 1, 2, 0, 1, 2 on both
ONE_NODE_GRIDS = lg.GRID_CLASSES["single_node"] + lg.GRID_CLASSES["one_node_axis"]
LIMIT_GRIDS = lg.GRID_CLASSES["apron_10_bit_limit"]  # 1021 / 1022 nodes = a padded 1023 / 1024 on each axis
EDGE_GRIDS = REMAINDER_GRIDS + ONE_NODE_GRIDS + LIMIT_GRIDS
CLOUDS = (1, 63, 64, 65, 300)
# lines = ceil(px / 3) * ceil(py / 3) * pz of 128 bytes; 2^25 lines are 4 GiB: 256 x 256 bricks and 511 / 512 padded slices
OFFSET_GRIDS = [(764, 764, 509), (764, 764, 510)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _packed_bytes(dims, layout):
    """kernels.hip packed_lut_bytes, restated"""
    px, py, pz = (d + 2 for d in dims)
    if layout == 6:
        return ((px + 2) // 3) * ((py + 2) // 3) * pz * 128
    if layout == 4:
        return ((px + 2) // 3) * ((py + 1) // 2) * pz * 128
    return px * py * pz * (16 if layout == 2 else 8)


def _wide(dims, layout):
    """kernels.hip bounds_lut_wide, restated"""
    return (dims[1] + 2) * (dims[2] + 2) > (1 << 23) or _packed_bytes(dims, layout) + 64 > (1 << 32)


def _expected(dims, forced):
    return 2 if forced in (4, 6) and max(dims) + 2 >= 1024 else forced


def _check_per_point(hip, c, lut, quant):
    rn = c["rn"]
    for fix in (True, False):
        for t in c["tnodes"]:
            e = hip.point_distances(rn.q.R, rn.span, t, fix)
            want = npr.point_distances(lut, c["bounds"], c["res"], c["src"], rn.q.R, rn.span, t, fix, quant=quant)
            bad = np.flatnonzero(e.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (c["dims"], len(c["src"]), fix, t, bad[:8], e[bad[:8]], want[bad[:8]], lg.lower_texels(c, t)[bad[:8]])


def _submissions(hip, c, cut):
    """One context's rows: both kinds of rotation node; the two as twins (dual items) with thresholds and terminal rows; the trimmed
    rows.  `cut`: the thresholds (None: taken from this context's own exact rows) -> (rows, cut)"""
    rn, tn = c["rn"], c["tnodes"]
    n, ns = len(tn), len(c["src"])
    Rs, spans, fixes, groups = [rn.q.R, rn.q.R], [rn.span, rn.span], [True, False], [tn, tn]
    rows = {"exact": hip.compute_bounds_multi(Rs, spans, fixes, groups)}
    if cut is None:
        cut = np.array([np.median(lb) for lb, _ in rows["exact"]], f32)
    twin = np.concatenate([np.arange(n, 2 * n), np.arange(n)]).astype(np.int32)
    rows["cut"] = hip.compute_bounds_cut(Rs, spans, fixes, groups, cut)
    rows["dual, terminal"] = hip.compute_bounds_cut(Rs, spans, fixes, groups, cut, twin=twin, ub_below_span=np.array([0.05, 0.01], f32))
    k = int(0.8 * ns)
    if 1 <= k < ns:
        hip.set_inliers(k)
        rows["trimmed"] = hip.compute_bounds_multi(Rs, spans, fixes, groups)
        hip.set_inliers(0)
    return rows, cut


def _assert_same_rows(got, want, what):
    assert got.keys() == want.keys()
    for key in got:
        for g, ((lb, ub), (lb2, ub2)) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(_bits(lb), _bits(lb2)) and np.array_equal(_bits(ub), _bits(ub2)), (what, key, g, lb, lb2, ub, ub2)


@pytest.mark.parametrize("dims", EDGE_GRIDS, ids=lg.grid_id)
def test_grid_edges_keep_every_bit(fg, gpu_required, monkeypatch, dims):
    """FGOICP_LUT_ZPAIR = 6 at every edge grid and every cloud, through the sort: per point against the restatement; the rows (exact,
    with thresholds, dual and terminal, trimmed) against the same submissions under layouts 1 and 4; the 300-point cloud also without the
    weight quantisation.  A padded 1024 reports layout 2."""
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    for ns in CLOUDS:
        c = lg.make_case(dims, ns)
        for flags, quant in ((0, True), (fg.FLAG_NO_WEIGHT_QUANT, False)):
            if not quant and ns != lg.NS:
                continue
            rows, cut = {}, None
            for layout in (1, 4, 6):
                monkeypatch.setenv("FGOICP_LUT_ZPAIR", str(layout))
                hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]), flags=flags)
                info = hip.info()
                assert info["lut_dims"] == tuple(dims) and info["lut_layout"] == _expected(dims, layout), info
                assert info["lut_bytes"] == int(np.prod(np.asarray(dims) + 2)) * 4 + _packed_bytes(dims, info["lut_layout"]), info
                rows[layout], cut = _submissions(hip, c, cut)
                sorted_ticks, fallbacks = hip.sort_fallbacks()
                assert sorted_ticks > 0 and fallbacks == 0
                if layout == 6 and int(0.8 * ns) >= 1:
                    hip.set_inliers(int(0.8 * ns))
                    _check_per_point(hip, c, hip.lut_read(), quant)
                hip.close()
            assert float(max(ub.max() for _, ub in rows[6]["exact"])) > 0
            _assert_same_rows(rows[6], rows[1], (dims, ns, quant, "layout 6 against 1"))
            _assert_same_rows(rows[6], rows[4], (dims, ns, quant, "layout 6 against 4"))


@pytest.mark.parametrize("dims", OFFSET_GRIDS, ids=lg.grid_id)
def test_both_sides_of_the_narrow_byte_offset(fg, gpu_required, monkeypatch, dims):
    """2^25 - 2^16 and 2^25 lines: the last copy whose byte offsets fit 32 bits and the first that takes the 64-bit addressing; lookups
    at both ends of every axis, per point against the restatement"""
    monkeypatch.setenv("FGOICP_LUT_ZPAIR", "6")
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    assert [_wide(g, 6) for g in OFFSET_GRIDS] == [False, True] and _packed_bytes(OFFSET_GRIDS[1], 6) == 1 << 32
    c = lg.make_case(dims)
    hip = fg.Registration(c["tgt"], c["src"], c["bounds"], float(c["res"]))
    info = hip.info()
    assert info["lut_dims"] == tuple(dims) and info["lut_layout"] == 6, info
    hip.set_inliers(int(0.8 * lg.NS))
    _check_per_point(hip, c, hip.lut_read(), True)
    assert hip.sort_fallbacks()[0] > 0
    hip.close()


@pytest.mark.parametrize("workload,res,chunk", [("tiny", 0.05, "256"), ("small", 0.02, "256"), ("small", 0.013, "1024")])
def test_golden_submission_keeps_every_bit(fg, gpu_required, monkeypatch, workload, res, chunk):
    """the recorded 60-row submission (four groups, twelve twins; a cloud three points short of whole passes) under layout 6 against the
    bits recorded for the sparse layouts (z4; z2 holds the same), trimmed and not, both weight modes"""
    import ctypes as C
    ref = np.load(GOLDEN)
    pct, pcs, bounds = ref[workload + "_pct"], ref[workload + "_pcs"], ref[workload + "_bounds"]
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    monkeypatch.setenv("FGOICP_CHUNK_PTS", chunk)
    monkeypatch.setenv("FGOICP_LUT_ZPAIR", "6")
    lib = fg._lib.load()
    R9, spans, fix, offs, tn4, twin = (np.ascontiguousarray(ref[k]) for k in ("R9", "spans", "fix", "offs", "tn", "twin"))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    for noquant in (False, True):
        for trim in (False, True):
            reg = fg.Registration(pct, pcs, bounds, res, flags=fg.FLAG_NO_WEIGHT_QUANT if noquant else 0)
            info = reg.info()
            assert info["lut_layout"] == 6 and info["points_per_item"] == int(chunk), info
            if trim:
                reg.set_inliers(int(0.8 * len(pcs)))
            lb, ub = np.zeros(60, f32), np.zeros(60, f32)
            assert lib.fgoicp_bounds_submit_twins(reg._h, 0, 4, R9.ctypes.data_as(fp), spans.ctypes.data_as(fp), fix.ctypes.data_as(ip), offs.ctypes.data_as(ip),
                                                  tn4.ctypes.data_as(fp), twin.ctypes.data_as(ip)) == 0
            assert lib.fgoicp_bounds_collect(reg._h, 0, lb.ctypes.data_as(fp), ub.ctypes.data_as(fp)) == 0
            reg.close()
            for z in ("4", "2"):
                key = f"{workload}_{res}_{chunk}_{'noquant' if noquant else 'quant'}_z{z}_{'trim' if trim else 'full'}"
                assert np.array_equal(_bits(lb), _bits(ref[key + "_lb"])) and np.array_equal(_bits(ub), _bits(ref[key + "_ub"])), key
            assert float(ub.max()) > 0


def test_mixed_batch_with_a_layout_6_pair_returns_the_solo_bits(fg, gpu_required, monkeypatch):
    """one fused tick over contexts of layouts 1, 4 and 6 (both weight modes for 6): a launch per class, every row as the context's own;
    the same with all of them trimmed (fused_trim_item_kernel)"""
    from tests.test_gpu_batch_ops import _requests, assert_same_bits, own_rows, tick
    from tests.test_gpu_batch_trim import trim_tick
    tgt, src, _, _ = fg.synth.make_pair(3000, 1500, (1.0, 0.8, 0.6), seed=61, angle_deg=40.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    specs = [("6", 1500, 0), ("1", 1500, 0), ("4", 1500, 0), ("6", 321, fg.FLAG_NO_WEIGHT_QUANT), ("6", 65, 0)]
    regs = []
    for layout, ns, flags in specs:
        monkeypatch.setenv("FGOICP_LUT_ZPAIR", layout)
        regs.append(fg.Registration(pct, pcs[:ns], bounds, 0.03, flags=flags))
        assert regs[-1].info()["lut_layout"] == int(layout)
    rng = np.random.default_rng(62)
    reqs = [q for k in range(len(regs)) for q in _requests(fg, rng, k)]
    got, launches = tick(fg, regs, reqs)
    assert launches == 4  # layouts 1, 4, 6 and layout 6 without the weight quantisation
    assert_same_bits(got, [own_rows(regs[q.k], q) for q in reqs], "fused rows != the context's own rows")
    assert all(float(ub.max()) > 0 for _, ub in got if ub.size)
    for r in regs:
        r.set_inliers(int(0.8 * r.ns))
    reqs = [q for q in reqs if all(len(g) for g in q.groups)]
    got, launches, _ = trim_tick(fg, regs, reqs)
    assert launches == 4
    assert_same_bits(got, [own_rows(regs[q.k], q) for q in reqs], "fused trimmed rows != the context's own rows")
    for r in regs:
        r.close()


@pytest.mark.parametrize("sched_name", ["serial", "round"])
def test_whole_run_under_layouts_4_and_6(fg, gpu_required, monkeypatch, sched_name):
    """the tiny pair's certify run (150 degrees, mse 5e-5): equal counters, R, t and best error under both layouts"""
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=150.0, min_angle_deg=110.0)
    sched, K = (fg.SCHEDULE_SERIAL, 1) if sched_name == "serial" else (fg.SCHEDULE_ROUND, 0)
    out = {}
    for layout in ("4", "6"):
        monkeypatch.setenv("FGOICP_LUT_ZPAIR", layout)
        s = fg.FastGoICP(tgt, src, 0.02, 5e-5, schedule=sched, round_width=K)
        assert s.registration.info()["lut_layout"] == int(layout)
        R, t = s.run()
        out[layout] = (R.copy(), t.copy(), np.float32(s.get_best_error()), s.stats())
        s.close()
    (R0, t0, e0, st0), (R1, t1, e1, st1) = out["4"], out["6"]
    assert np.array_equal(_bits(R0), _bits(R1)) and np.array_equal(_bits(t0), _bits(t1)) and e0.view(np.uint32) == e1.view(np.uint32)
    for k in ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb", "rounds"):
        assert st0[k] == st1[k], k
    assert st1["trans_cubes"] > 0


# ---- the shipped build's rule ----
@pytest.mark.parametrize("d,layout", [(229, 4), (231, 6)])
def test_the_shipped_build_selects_layout_6_above_256_mib(fg, gpu_required, d, layout):
    """a sparse context (300 source points) whose apron-bricked quad copy would take 252 MiB keeps it; at 260 MiB the z-pair apron copy
    is built instead, a third smaller; lut_bytes = the padded fp32 LUT + the packed copy of the reported layout"""
    dims = (d, d, d)
    assert (_packed_bytes(dims, 4) > (256 << 20)) == (layout == 6) and abs(_packed_bytes(dims, 4) / (256 << 20) - 1) < 0.02
    bounds, res = lg.geometry(dims)
    rng = np.random.default_rng(d)
    tgt = rng.uniform(bounds[:, 0], bounds[:, 1], (300, 3)).astype(f32)
    src = rng.uniform(bounds[:, 0] * 0.5, bounds[:, 1] * 0.5, (300, 3)).astype(f32)
    reg = fg.Registration(tgt, src, bounds, float(res))
    info = reg.info()
    assert info["lut_dims"] == dims and info["source_points_per_face_voxel"] < 0.5 and info["lut_layout"] == layout, info
    assert info["lut_bytes"] == (d + 2) ** 3 * 4 + _packed_bytes(dims, layout), info
    if layout == 6:
        assert _packed_bytes(dims, 6) == 78 * 78 * 233 * 128 and _packed_bytes(dims, 6) < 0.68 * _packed_bytes(dims, 4)
    rn = lg.rot_node()
    tn = np.array([[0, 0, 0, 0.02], [0.01, -0.02, 0.015, 0.0]], f32)
    lb, ub = reg.compute_sse_error(rn, tn, True)
    want = npr.bounds(reg.lut_read(), bounds, res, src, rn.q.R, rn.span, tn, True)
    assert lg.close_rel(ub, want[1]) and np.all(np.abs(lb.astype(np.float64) - want[0]) <= lg.REL * float(np.max(want[1])))
    reg.close()
