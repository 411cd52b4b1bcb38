"""GPU: the two device paths of fgoicp_batch that no solo run uses, row by row — the fused bounds tick (HipBatchBackend::bounds,
fused_bounds_item_kernel, fused_bounds_finalize_kernel) and the stepped ICP (ctx_icp_step_begin / ctx_icp_step) — through the test
hooks fgoicp_batch_test_bounds / fgoicp_batch_test_icp, which run the backend's own code over contexts made here.

Bars (as tests/test_gpu_ops.py): every row bit for bit against the pair's own context (fgoicp_bounds_multi, fgoicp_icp), and the
oracle to REL = 1e-6 (lower bounds absolutely against the upper bounds' scale)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-6
ERR_INVALID_ARG = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_kernel_bits.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Req:
    """One bounds request (fgoicp_bounds_multi's arguments) for context `k` of a tick."""

    def __init__(self, k, Rs, spans, fixes, groups):
        self.k, self.Rs, self.spans, self.fixes = k, list(Rs), list(spans), [bool(f) for f in fixes]
        self.groups = [np.ascontiguousarray(g, np.float32).reshape(-1, 4) for g in groups]

    @property
    def rows(self):
        return sum(len(g) for g in self.groups)


def tick(fg, regs, reqs, expect_rc=0):
    """All requests in ONE fused tick: -> (list of (lb, ub) per request, fused launches)"""
    from fgoicp_amd.nodes import to_glm
    lib = fg._lib.load()
    fp, ip = fg._lib.c_float_p, fg._lib.c_int_p
    ctxs = (C.c_void_p * len(regs))(*[r._h.value for r in regs])
    req_ctx = np.array([q.k for q in reqs], np.int32)
    req_G = np.array([len(q.groups) for q in reqs], np.int32)
    R9 = np.concatenate([to_glm(R) for q in reqs for R in q.Rs] + [np.zeros(0, np.float32)]).astype(np.float32)
    spans = np.array([s for q in reqs for s in q.spans], np.float32)
    fix = np.array([int(f) for q in reqs for f in q.fixes], np.int32)
    offs = np.concatenate([np.concatenate([[0], np.cumsum([len(g) for g in q.groups])]) for q in reqs] + [np.zeros(0)]).astype(np.int32)
    tn = np.ascontiguousarray(np.concatenate([g for q in reqs for g in q.groups] + [np.zeros((0, 4), np.float32)]), np.float32)
    n = len(tn)
    lb, ub = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    launches = C.c_uint64(0)
    rc = lib.fgoicp_batch_test_bounds(ctxs, len(regs), len(reqs), req_ctx.ctypes.data_as(ip), req_G.ctypes.data_as(ip), R9.ctypes.data_as(fp),
                                      spans.ctypes.data_as(fp), fix.ctypes.data_as(ip), offs.ctypes.data_as(ip), tn.ctypes.data_as(fp),
                                      lb.ctypes.data_as(fp), ub.ctypes.data_as(fp), C.byref(launches))
    assert rc == expect_rc, (rc, lib.fgoicp_last_error())
    if rc:
        return None, None
    out, e = [], 0
    for q in reqs:
        out.append((lb[e:e + q.rows].copy(), ub[e:e + q.rows].copy()))
        e += q.rows
    return out, launches.value


def own_rows(reg, q):
    """the request through the pair's own context: -> (lb, ub) over all its rows"""
    parts = reg.compute_bounds_multi(q.Rs, q.spans, q.fixes, q.groups)
    lb = np.concatenate([p[0] for p in parts] + [np.zeros(0, np.float32)])
    ub = np.concatenate([p[1] for p in parts] + [np.zeros(0, np.float32)])
    return lb, ub


def assert_same_bits(got, want, what):
    assert len(got) == len(want)
    for i, ((lb, ub), (lb2, ub2)) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(lb), _bits(lb2)) and np.array_equal(_bits(ub), _bits(ub2)), (what, i)


def _tnodes(rng, B, span, reach=0.7):
    t = rng.uniform(-reach, reach, size=(B, 3)).astype(np.float32)
    return np.concatenate([t, np.full((B, 1), span, np.float32)], axis=1)


def _requests(fg, rng, k):
    """two requests of four groups (both fix_rot, rotation spans 1 .. 1/64, translation spans 1/64 .. 1, nodes inside and far outside
    the LUT: clamped lookups) and one whose first group is empty"""
    nodes = [fg.RotNode(0.25, -0.125, 0.375, 1.0), fg.RotNode(-0.5, 0.25, 0.125, 0.25), fg.RotNode(0.125, 0.0625, -0.25, 1 / 16),
             fg.RotNode(0.03125, -0.4375, 0.0, 1 / 64)]
    reqs = []
    for r in range(2):
        groups = [_tnodes(rng, 5 + 3 * r, 1.0), _tnodes(rng, 7, 1 / 64, reach=2.5), _tnodes(rng, 4 + r, 0.25), _tnodes(rng, 6, 1 / 8, reach=1.6)]
        sel = nodes[r:] + nodes[:r]
        reqs.append(Req(k, [n.q.R for n in sel], [n.span for n in sel], [True, False, r == 0, r == 1], groups))
    reqs.append(Req(k, [nodes[1].q.R, nodes[2].q.R], [nodes[1].span, nodes[2].span], [False, True], [np.zeros((0, 4), np.float32), _tnodes(rng, 3, 0.5)]))
    return reqs


# ---- 1. golden bits, every layout (development build: the layout and the chunk size are forced) ----------------------------------
@pytest.mark.dev_knobs
def test_fused_tick_keeps_every_golden_bit(fg, gpu_required, monkeypatch):
    """tests/golden/item_kernel_bits.npz's 60-row submission (4 groups, both fix_rot; its twins as plain rows) on contexts of its tiny
    and small clouds under every recorded (resolution, chunk size, weight mode, layout), all in ONE tick: every untrimmed row bit for bit
    as recorded, and one fused launch per (layout, addressing, weight mode) class."""
    from fgoicp_amd.nodes import from_glm
    ref = np.load(GOLDEN)
    R9, spans, fix, offs, tn4 = (np.ascontiguousarray(ref[k]) for k in ("R9", "spans", "fix", "offs", "tn"))
    Rs = [from_glm(R9[9 * g:9 * g + 9]) for g in range(4)]
    groups = [tn4.reshape(-1, 4)[offs[g]:offs[g + 1]] for g in range(4)]
    regs, reqs, keys = [], [], []
    for workload, res, chunk in (("tiny", 0.05, "256"), ("small", 0.02, "256"), ("small", 0.013, "1024")):
        pct, pcs, bounds = ref[workload + "_pct"], ref[workload + "_pcs"], ref[workload + "_bounds"]
        monkeypatch.setenv("FGOICP_CHUNK_PTS", chunk)
        for quant in ("quant", "noquant"):
            for layout in ("1", "2", "4"):
                monkeypatch.setenv("FGOICP_LUT_ZPAIR", layout)
                reg = fg.Registration(pct, pcs, bounds, res, flags=fg.FLAG_NO_WEIGHT_QUANT if quant == "noquant" else 0)
                info = reg.info()
                assert info["lut_layout"] == int(layout) and info["points_per_item"] == int(chunk), info
                reqs.append(Req(len(regs), Rs, spans, fix, groups))
                regs.append(reg)
                keys.append(f"{workload}_{res}_{chunk}_{quant}_z{layout}_full")
    got, launches = tick(fg, regs, reqs)
    assert launches == 6  # layouts {1, 2, 4} x weights {quant, noquant}, all with 32-bit addressing
    for (lb, ub), key in zip(got, keys):
        assert np.array_equal(_bits(lb), _bits(ref[key + "_lb"])) and np.array_equal(_bits(ub), _bits(ref[key + "_ub"])), key
        assert float(ub.max()) > 0
    for r in regs:
        r.close()


# ---- 2. a mixed tick on the shipped build --------------------------------------------------------------------------------------
def _cloud_pair(fg, ns, seed, nt=6000):
    tgt, src, _, _ = fg.synth.make_pair(nt, ns, (1.0, 0.8, 0.6), seed=seed, angle_deg=40.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    return pct, pcs, bounds


# (ns, LUT resolution, flags): sparse clouds (apron-bricked quads, 256 points per item; 40 000 points at 0.005 = 157 items per row, so
# the finalize kernel's lanes stride three times) and dense ones (z-pairs, 2048 points per item); both weight modes, both source orders
MIXED = [(1, 0.02, ""), (63, 0.02, "noquant"), (64, 0.05, ""), (65, 0.05, "noquant"), (257, 0.02, "nomorton"), (4999, 0.05, ""),
         (4999, 0.05, "noquant curve"), (40000, 0.005, ""), (40000, 0.05, "noquant nomorton")]


def _flags(fg, spec):
    names = {"noquant": fg.FLAG_NO_WEIGHT_QUANT, "nomorton": fg.FLAG_NO_MORTON, "curve": fg.FLAG_CURVE_ORDER}
    return sum(names[t] for t in spec.split())


@pytest.fixture(scope="module")
def mixed(fg, oracle, gpu_required):
    pct, pcs, bounds = _cloud_pair(fg, 40000, seed=71)
    regs, orcs = [], []
    for ns, res, spec in MIXED:
        flags = _flags(fg, spec)
        reg = fg.Registration(pct, pcs[:ns], bounds, res, flags=flags)
        # the oracle's operators on the same LUT (bit-identical: test_gpu_ops.py::test_lut_nodes_bit_exact), without its O(nodes * nt) build
        orc = oracle.Registration(pct, pcs[:ns], bounds, res, build_lut=False, quantize=not flags & fg.FLAG_NO_WEIGHT_QUANT)
        orc.lut_set(reg.lut_read())
        regs.append(reg)
        orcs.append(orc)
    rng = np.random.default_rng(72)
    reqs = [q for k in range(len(MIXED)) for q in _requests(fg, rng, k)]
    yield dict(regs=regs, orcs=orcs, reqs=reqs)
    for r in regs:
        r.close()


def test_mixed_tick_equals_each_context_and_the_oracle(fg, mixed):
    regs, orcs, reqs = mixed["regs"], mixed["orcs"], mixed["reqs"]
    infos = [r.info() for r in regs]
    assert {i["lut_layout"] for i in infos} >= {1, 4}, infos
    assert 256 in {i["points_per_item"] for i in infos} and max(i["points_per_item"] for i in infos) >= 1024, infos
    assert max(i["items_per_evaluation"] for i in infos) > 128, infos  # the finalize kernel's lanes stride three times
    got, launches = tick(fg, regs, reqs)
    classes = {(i["lut_layout"], "noquant" in spec) for i, (_, _, spec) in zip(infos, MIXED)}
    assert launches == len(classes), (launches, classes)
    assert_same_bits(got, [own_rows(regs[q.k], q) for q in reqs], "fused rows != the context's own rows")
    for q, (lb, ub) in zip(reqs, got):
        e = 0
        for R, span, f, g in zip(q.Rs, q.spans, q.fixes, q.groups):
            n = len(g)
            if n:
                lb_o, ub_o = orcs[q.k].compute_bounds(R, span, g, f)
                scale = max(float(np.max(ub_o)), 1e-30)
                assert np.max(np.abs(ub[e:e + n].astype(np.float64) - ub_o) / np.maximum(np.abs(ub_o), 1e-30)) <= REL, (MIXED[q.k], ub[e:e + n], ub_o)
                assert np.max(np.abs(lb[e:e + n].astype(np.float64) - lb_o)) <= REL * scale, (MIXED[q.k], lb[e:e + n], lb_o)
            e += n
    assert all(float(ub.max()) > 0 for _, ub in got if ub.size)


def test_mixed_tick_does_not_depend_on_its_company(fg, mixed):
    """The same requests permuted, and split over one, two and three ticks: the same bits."""
    regs, reqs = mixed["regs"], mixed["reqs"]
    base, _ = tick(fg, regs, reqs)
    rng = np.random.default_rng(73)
    perm = rng.permutation(len(reqs))
    got, _ = tick(fg, regs, [reqs[i] for i in perm])
    inv = np.argsort(perm)
    assert_same_bits([got[int(inv[i])] for i in range(len(reqs))], base, "permuted")
    for parts in (1, 2, 3):
        out = [None] * len(reqs)
        for idx in np.array_split(rng.permutation(len(reqs)), parts):
            rows, _ = tick(fg, regs, [reqs[int(i)] for i in idx])
            for i, r in zip(idx, rows):
                out[int(i)] = r
        assert_same_bits(out, base, f"split over {parts} ticks")


# ---- 3. 64-bit texel addressing ---------------------------------------------------------------------------------------------------
def _lut_wide(dims, layout):
    """kernels.hip bounds_lut_wide, restated"""
    px, py, pz = (d + 2 for d in dims)
    if layout == 4:
        nbytes = ((px + 2) // 3) * ((py + 1) // 2) * pz * 8 * 16
    else:
        nbytes = px * py * pz * (16 if layout == 2 else 8)
    return py * pz > (1 << 23) or nbytes + 64 > (1 << 32)


def test_wide_texel_addressing_in_a_tick(fg, gpu_required):
    """The test/bunny.toml shape at resolution 0.002 (~6e8 LUT nodes, a packed copy above 4 GiB): the fused rows of the 64-bit
    addressing class equal the context's own, with both fix_rot; a small context in the same tick lands in a class of its own."""
    tgt, src, _, _ = fg.synth.workload("bunny_toml", angle_deg=150.0, min_angle_deg=110.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    big = fg.Registration(pct, pcs, bounds, 0.002)
    small = fg.Registration(pct, pcs[:500], bounds, 0.05)
    ib, isml = big.info(), small.info()
    assert _lut_wide(ib["lut_dims"], ib["lut_layout"]) and not _lut_wide(isml["lut_dims"], isml["lut_layout"]), (ib, isml)
    rng = np.random.default_rng(31)
    nodes = [fg.RotNode(0.125, -0.25, 0.375, 0.25), fg.RotNode(-0.375, 0.125, 0.25, 1 / 32)]
    reqs = [Req(0, [n.q.R for n in nodes], [n.span for n in nodes], [True, False], [_tnodes(rng, 40, 0.125), _tnodes(rng, 30, 1 / 64, reach=1.5)]),
            Req(1, [nodes[0].q.R], [nodes[0].span], [False], [_tnodes(rng, 20, 0.25)]),
            Req(0, [nodes[1].q.R], [nodes[1].span], [True], [_tnodes(rng, 25, 0.5)])]
    got, launches = tick(fg, [big, small], reqs)
    assert launches == 2
    assert_same_bits(got, [own_rows([big, small][q.k], q) for q in reqs], "wide class")
    assert float(got[0][1].max()) > 0
    big.close()
    small.close()


# ---- 4. a tick above 2^26 work items ---------------------------------------------------------------------------------------------
def test_tick_above_2_pow_26_items(fg, gpu_required):
    """One sparse context of 262 144 points (256 points per item: 1024 items per row) with 65 600 rows, and a small context, in ONE
    tick: more than 2^26 items, more 64-thread blocks than one launch can address in a 32-bit grid.  Every row equals the context's
    own fgoicp_bounds_multi (which windows the same rows)."""
    pct, pcs, bounds = _cloud_pair(fg, 262144, seed=81, nt=20000)
    big = fg.Registration(pct, pcs, bounds, 0.002)
    small = fg.Registration(pct, pcs[:3000], bounds, 0.05)
    info = big.info()
    assert info["points_per_item"] == 256 and info["items_per_evaluation"] == 1024, info
    rng = np.random.default_rng(82)
    nodes = [fg.RotNode(*(float(v) for v in rng.uniform(-0.5, 0.5, 3)), 1 / 16) for _ in range(41)]
    big_req = Req(0, [n.q.R for n in nodes], [n.span for n in nodes], [g % 2 == 0 for g in range(len(nodes))], [_tnodes(rng, 1600, 1 / 32) for _ in nodes])
    assert big_req.rows * 1024 > (1 << 26)
    reqs = [Req(1, [nodes[0].q.R], [nodes[0].span], [False], [_tnodes(rng, 50, 0.25)]), big_req]
    got, _ = tick(fg, [big, small], reqs)
    own = [own_rows(small, reqs[0]), own_rows(big, reqs[1])]
    for (lb, ub), (lb2, ub2), what in zip(got, own, ("small", "big")):
        bad = np.flatnonzero((_bits(lb) != _bits(lb2)) | (_bits(ub) != _bits(ub2)))
        assert bad.size == 0, (what, bad.size, bad[:8])
    assert float(got[1][1].min()) > 0
    big.close()
    small.close()


# ---- 5. stepped ICP ------------------------------------------------------------------------------------------------------------
def icp_steps(fg, regs, start_pass, R0s, t0s, max_iter, thr):
    from fgoicp_amd.nodes import from_glm, to_glm
    lib = fg._lib.load()
    fp, ip = fg._lib.c_float_p, fg._lib.c_int_p
    n = len(regs)
    ctxs = (C.c_void_p * n)(*[r._h.value for r in regs])
    sp = np.asarray(start_pass, np.int32)
    R0 = np.concatenate([to_glm(R) for R in R0s]).astype(np.float32)
    t0 = np.ascontiguousarray(np.asarray(t0s, np.float32).reshape(-1))
    mi = (C.c_size_t * n)(*[int(m) for m in max_iter])
    th = np.asarray(thr, np.float32)
    sse, Ro, to, it = np.zeros(n, np.float32), np.zeros(9 * n, np.float32), np.zeros(3 * n, np.float32), np.zeros(n, np.int32)
    rc = lib.fgoicp_batch_test_icp(ctxs, n, sp.ctypes.data_as(ip), R0.ctypes.data_as(fp), t0.ctypes.data_as(fp), mi, th.ctypes.data_as(fp),
                                   sse.ctypes.data_as(fp), Ro.ctypes.data_as(fp), to.ctypes.data_as(fp), it.ctypes.data_as(ip))
    assert rc == 0, lib.fgoicp_last_error()
    return [(sse[i], from_glm(Ro[9 * i:9 * i + 9]), to[3 * i:3 * i + 3].copy(), int(it[i])) for i in range(n)]


def icp_solo(fg, reg, R0, t0, max_iter, thr):
    icp = fg.IterativeClosestPoint3D(reg, None, None, max_iter, thr, R0, t0)
    sse, R, t = icp.run()
    return sse, R, t, icp.iterations


def test_stepped_icp_runs_keep_their_solo_bits(fg, oracle, gpu_required):
    """Runs on contexts of 1 .. 40 000 points, one above 262 144 (its whole loop when it starts) and one brute-force context, started
    staggered so that runs at different stages share every step: each run's (sse, R, t, iterations) are fgoicp_icp's on the same
    context, called before and after; one run also agrees with the oracle's ICP (test_gpu_ops.py::test_icp_parity's bar)."""
    pct, pcs, bounds = _cloud_pair(fg, 300000, seed=91)
    # (ns, flags, max_iter, thr)
    specs = [(1, 0, 2, 1e-3), (100, 0, 1, 0.5), (2000, 0, 1000, 1e-3), (40000, fg.FLAG_NO_MORTON, 7, 1e-7), (300000, 0, 1000, 1e-3),
             (3000, fg.FLAG_BRUTE_FORCE_NN, 1000, 0.0), (5000, fg.FLAG_NO_WEIGHT_QUANT, 0, 1.0), (700, fg.FLAG_CURVE_ORDER, 1000, 1.0),
             (20000, 0, 1000, 1e-7)]
    regs = [fg.Registration(pct, pcs[:ns], bounds, 0.05, flags=f) for ns, f, _, _ in specs]
    rng = np.random.default_rng(92)
    angles = [(30.0, 150.0)[i % 2] for i in range(len(specs))]
    R0s = [fg.synth.random_rotation(rng, a, a - 1e-3).astype(np.float32) for a in angles]
    t0s = [rng.uniform(-0.05, 0.05, 3).astype(np.float32) for _ in specs]
    max_iter = [s[2] for s in specs]
    thr = [s[3] for s in specs]
    start = [i % 4 for i in range(len(specs))]
    before = [icp_solo(fg, r, R0, t0, m, th) for r, R0, t0, m, th in zip(regs, R0s, t0s, max_iter, thr)]
    got = icp_steps(fg, regs, start, R0s, t0s, max_iter, thr)
    after = [icp_solo(fg, r, R0, t0, m, th) for r, R0, t0, m, th in zip(regs, R0s, t0s, max_iter, thr)]
    for i, (g, b, a) in enumerate(zip(got, before, after)):
        for ref in (b, a):
            assert g[3] == ref[3], (specs[i], g[3], ref[3])
            assert _bits(g[0]) == _bits(ref[0]) and np.array_equal(_bits(g[1]), _bits(ref[1])) and np.array_equal(_bits(g[2]), _bits(ref[2])), specs[i]
    assert got[6][3] == 0 and float(got[6][0]) == pytest.approx(1e10)  # max_iter 0: the loop body never runs (icp3d.cu:94,106)
    assert got[2][3] > 2 and got[4][3] > 2 and got[8][3] > 2
    # the 2000-point run against the oracle
    orc = oracle.Registration(pct, pcs[:2000], bounds, 0.05, build_lut=False)
    sse_o, R_o, t_o, it_o = orc.icp(R0s[2], t0s[2], 1000, 1e-3)
    sse, R, t, it = got[2]
    assert it == it_o
    assert abs(float(sse) - float(sse_o)) <= 1e-5 * float(sse_o)
    assert np.allclose(R, R_o, atol=1e-5) and np.allclose(t, t_o, atol=1e-5)
    for r in regs:
        r.close()


# ---- 6. refusals on the device -----------------------------------------------------------------------------------------------------
def test_refused_ticks_leave_the_other_contexts_alone(fg, gpu_required):
    """A trimmed context in a tick and a request naming a context out of range are refused before any device work, and the rows of
    the other contexts are the same before and after; so is an ICP list that names a context twice."""
    pct, pcs, bounds = _cloud_pair(fg, 5000, seed=101)
    a = fg.Registration(pct, pcs[:3000], bounds, 0.02)
    b = fg.Registration(pct, pcs, bounds, 0.05)
    trimmed = fg.Registration(pct, pcs[:2000], bounds, 0.05)
    trimmed.set_inliers(1500)
    rng = np.random.default_rng(102)
    reqs = _requests(fg, rng, 0) + _requests(fg, rng, 1)
    first, _ = tick(fg, [a, b, trimmed], reqs)
    extra = [_tnodes(rng, 4, 0.25)]
    tick(fg, [a, b, trimmed], reqs + [Req(2, [np.eye(3, dtype=np.float32)], [0.5], [False], extra)], expect_rc=ERR_INVALID_ARG)
    tick(fg, [a, b, trimmed], reqs + [Req(3, [np.eye(3, dtype=np.float32)], [0.5], [False], extra)], expect_rc=ERR_INVALID_ARG)
    again, _ = tick(fg, [a, b, trimmed], reqs)
    assert_same_bits(again, first, "rows changed after a refused tick")
    assert_same_bits(first, [own_rows([a, b][q.k], q) for q in reqs], "rows != the contexts' own")
    lib = fg._lib.load()
    fp, ip = fg._lib.c_float_p, fg._lib.c_int_p
    ctxs = (C.c_void_p * 2)(a._h.value, a._h.value)
    buf = np.zeros(18, np.float32)
    it = np.zeros(2, np.int32)
    assert lib.fgoicp_batch_test_icp(ctxs, 2, it.ctypes.data_as(ip), buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), (C.c_size_t * 2)(5, 5),
                                     buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), buf.ctypes.data_as(fp),
                                     it.ctypes.data_as(ip)) == ERR_INVALID_ARG
    for r in (a, b, trimmed):
        r.close()
