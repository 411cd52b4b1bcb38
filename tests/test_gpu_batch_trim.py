"""GPU: trimmed pairs in fgoicp_batch.  The fused trimmed bounds (fused_trim_item_kernel into the batch's e-row arena, then
fused_trim_select_kernel) row by row through the test hook fgoicp_batch_test_trim_bounds, against each context's own rows
(fgoicp_bounds_multi, fgoicp_bounds_submit_twins) and the recorded bits of tests/golden/item_kernel_bits.npz; and whole runs of
FastGoICPBatch with trimmed and untrimmed pairs mixed against solo FastGoICP(..., trim_fraction=f) runs, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONTRACT = ("trans_cubes", "rot_cubes", "inner_bnb", "icp_runs", "icp_iters", "rounds", "initial_icp_sse")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_kernel_bits.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Req:
    def __init__(self, k, Rs, spans, fixes, groups):
        self.k, self.Rs, self.spans, self.fixes = k, list(Rs), list(spans), [bool(f) for f in fixes]
        self.groups = [np.ascontiguousarray(g, np.float32).reshape(-1, 4) for g in groups]

    @property
    def rows(self):
        return sum(len(g) for g in self.groups)


def trim_tick(fg, regs, reqs, arena_rows=0):
    """all requests in ONE tick of the batch's bounds path: -> (list of (lb, ub) per request, bounds launches, selection launches)"""
    from fgoicp_amd.nodes import to_glm
    lib = fg._lib.load()
    fp, ip = fg._lib.c_float_p, fg._lib.c_int_p
    ctxs = (C.c_void_p * len(regs))(*[r._h.value for r in regs])
    req_ctx = np.array([q.k for q in reqs], np.int32)
    req_G = np.array([len(q.groups) for q in reqs], np.int32)
    R9 = np.concatenate([to_glm(R) for q in reqs for R in q.Rs]).astype(np.float32)
    spans = np.array([s for q in reqs for s in q.spans], np.float32)
    fix = np.array([int(f) for q in reqs for f in q.fixes], np.int32)
    offs = np.concatenate([np.concatenate([[0], np.cumsum([len(g) for g in q.groups])]) for q in reqs]).astype(np.int32)
    tn = np.ascontiguousarray(np.concatenate([g for q in reqs for g in q.groups]), np.float32)
    n = len(tn)
    lb, ub = np.zeros(n, np.float32), np.zeros(n, np.float32)
    launches, sel = C.c_uint64(0), C.c_uint64(0)
    rc = lib.fgoicp_batch_test_trim_bounds(ctxs, len(regs), len(reqs), req_ctx.ctypes.data_as(ip), req_G.ctypes.data_as(ip), R9.ctypes.data_as(fp),
                                           spans.ctypes.data_as(fp), fix.ctypes.data_as(ip), offs.ctypes.data_as(ip), tn.ctypes.data_as(fp),
                                           lb.ctypes.data_as(fp), ub.ctypes.data_as(fp), C.byref(launches), int(arena_rows), C.byref(sel))
    assert rc == 0, lib.fgoicp_last_error()
    out, e = [], 0
    for q in reqs:
        out.append((lb[e:e + q.rows].copy(), ub[e:e + q.rows].copy()))
        e += q.rows
    return out, launches.value, sel.value


def own_rows(reg, q):
    parts = reg.compute_bounds_multi(q.Rs, q.spans, q.fixes, q.groups)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _tnodes(rng, B, span, reach=0.7):
    t = rng.uniform(-reach, reach, size=(B, 3)).astype(np.float32)
    return np.concatenate([t, np.full((B, 1), span, np.float32)], axis=1)


def _requests(fg, rng, k):
    """two requests of four groups (both fix_rot, rotation spans 1 .. 1/64, translation spans 1/64 .. 1, nodes far outside the LUT too)"""
    nodes = [fg.RotNode(0.25, -0.125, 0.375, 1.0), fg.RotNode(-0.5, 0.25, 0.125, 0.25), fg.RotNode(0.125, 0.0625, -0.25, 1 / 16),
             fg.RotNode(0.03125, -0.4375, 0.0, 1 / 64)]
    reqs = []
    for r in range(2):
        groups = [_tnodes(rng, 5 + 3 * r, 1.0), _tnodes(rng, 7, 1 / 64, reach=2.5), _tnodes(rng, 4 + r, 0.25), _tnodes(rng, 6, 1 / 8, reach=1.6)]
        sel = nodes[r:] + nodes[:r]
        reqs.append(Req(k, [n.q.R for n in sel], [n.span for n in sel], [True, False, r == 0, r == 1], groups))
    return reqs


def _contexts(fg):
    """trimmed contexts (ns not a multiple of 4 or 64; several k; a tie-heavy cloud on a coarse grid with duplicated points) next to two
    untrimmed ones: -> list of (Registration, trimmed)"""
    out = []
    for i, (ns, frac, res, tie) in enumerate([(2001, 0.1, 0.02, False), (4099, 0.25, 0.05, False), (4099, 0.5, 0.02, False), (3001, 0.2, 0.05, True),
                                              (2500, 0.0, 0.05, False), (1999, 0.0, 0.02, False)]):
        tgt, src, _, _ = fg.synth.make_pair(5000, ns, (1.0, 0.8, 0.6), seed=300 + i, angle_deg=35.0)
        if tie:  # many equal distances: the source snapped to a coarse grid, half of it duplicated
            src = np.round(src * 8.0) / 8.0
            src[ns // 2:] = src[:ns - ns // 2]
        pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
        reg = fg.Registration(pct, pcs, bounds, res, flags=fg.FLAG_CURVE_ORDER if frac else 0)
        if frac:
            reg.set_inliers(int(ns * (1.0 - frac)))
        out.append((reg, frac > 0))
    return out


def test_trimmed_rows_match_each_context_bit_for_bit(fg, gpu_required):
    rng = np.random.default_rng(11)
    ctxs = _contexts(fg)
    regs = [r for r, _ in ctxs]
    reqs = [q for k in range(len(regs)) for q in _requests(fg, rng, k)]
    reqs = reqs[1::2] + reqs[0::2]  # the requests of a context apart from each other
    got, launches, sel = trim_tick(fg, regs, reqs)
    ntrim_rows = 0
    for q, (lb, ub) in zip(reqs, got):
        lb2, ub2 = own_rows(regs[q.k], q)
        assert np.array_equal(_bits(lb), _bits(lb2)) and np.array_equal(_bits(ub), _bits(ub2)), (q.k, ctxs[q.k][1])
        assert float(ub.max()) > 0
        ntrim_rows += q.rows if ctxs[q.k][1] else 0
    assert sel == 1  # one fill of the arena holds every trimmed row
    # the arena in fills of 1, 3 and 7 rows: the same bits, one selection launch per fill
    for fill in (1, 3, 7):
        got2, launches2, sel2 = trim_tick(fg, regs, reqs, arena_rows=fill)
        for (lb, ub), (lb2, ub2) in zip(got, got2):
            assert np.array_equal(_bits(lb), _bits(lb2)) and np.array_equal(_bits(ub), _bits(ub2)), fill
        assert sel2 == -(-ntrim_rows // fill), (fill, sel2)
        assert launches2 > launches
    for r in regs:
        r.close()


def test_trimmed_rows_match_the_dual_walk_and_the_golden_bits(fg, gpu_required):
    """item_kernel_bits.npz's 60-row submission with its twelve twin pairs: a trimmed context's own rows come from the dual walk
    (fgoicp_bounds_submit_twins: one lookup for both variants); the batch evaluates every row on its own — same bits, as recorded"""
    from fgoicp_amd.nodes import from_glm
    ref = np.load(GOLDEN)
    lib = fg._lib.load()
    fp, ip = fg._lib.c_float_p, fg._lib.c_int_p
    R9, spans, fix, offs, tn4, twin = (np.ascontiguousarray(ref[k]) for k in ("R9", "spans", "fix", "offs", "tn", "twin"))
    Rs = [from_glm(R9[9 * g:9 * g + 9]) for g in range(4)]
    groups = [tn4.reshape(-1, 4)[offs[g]:offs[g + 1]] for g in range(4)]
    regs, reqs, keys = [], [], []
    for workload, res in (("tiny", 0.05), ("small", 0.02)):
        pct, pcs, bounds = ref[workload + "_pct"], ref[workload + "_pcs"], ref[workload + "_bounds"]
        for quant in (0, fg.FLAG_NO_WEIGHT_QUANT):
            reg = fg.Registration(pct, pcs, bounds, res, flags=quant)
            reg.set_inliers(int(0.8 * len(pcs)))
            lb, ub = np.zeros(60, np.float32), np.zeros(60, np.float32)
            assert lib.fgoicp_bounds_submit_twins(reg._h, 0, 4, R9.ctypes.data_as(fp), spans.ctypes.data_as(fp), fix.ctypes.data_as(ip), offs.ctypes.data_as(ip),
                                                  tn4.ctypes.data_as(fp), twin.ctypes.data_as(ip)) == 0
            assert lib.fgoicp_bounds_collect(reg._h, 0, lb.ctypes.data_as(fp), ub.ctypes.data_as(fp)) == 0
            info = reg.info()
            reqs.append((Req(len(regs), Rs, spans, fix, groups), lb, ub, info["lut_layout"]))
            regs.append(reg)
            keys.append(f"{workload}_{res}_{info['points_per_item']}_{'noquant' if quant else 'quant'}")
    assert regs
    got, _, _ = trim_tick(fg, regs, [q for q, *_ in reqs])
    for (lb, ub), (q, lb_dual, ub_dual, layout), key in zip(got, reqs, keys):
        assert np.array_equal(_bits(lb), _bits(lb_dual)) and np.array_equal(_bits(ub), _bits(ub_dual)), key
        gk = f"{key}_z{layout}_trim"
        if gk + "_lb" in ref.files:  # (recorded at 256 points per item)
            assert np.array_equal(_bits(lb), _bits(ref[gk + "_lb"])) and np.array_equal(_bits(ub), _bits(ref[gk + "_ub"])), gk
    for r in regs:
        r.close()


# ---- whole runs --------------------------------------------------------------------------------------------------------------------
def _pairs(fg, seed=0):
    """(tgt, src, lut, mse, trim): trimmed (0.1, 0.25) and untrimmed pairs mixed; partial overlap for the trimmed ones"""
    rng = np.random.default_rng(seed)
    out = []
    for i, frac in enumerate((0.1, 0.0, 0.25, 0.1, 0.0, 0.25)):
        ns = int(rng.integers(800, 3001))
        # large rotations and a tight threshold: the initial ICP does not end the search, the BnB runs
        tgt, src, _, _ = fg.synth.make_pair(int(rng.integers(3000, 8001)), ns, (1.0, 0.8, 0.6), seed=500 + 7 * seed + i, angle_deg=150.0, min_angle_deg=100.0,
                                            outlier_frac=0.05 if frac else 0.0)
        out.append((tgt, src, (0.02, 0.05)[i % 2], (1e-4, 2e-4)[i % 2], frac))
    return out


def _solo(fg, pairs, schedule, round_width):
    res = []
    for tgt, src, lut, mse, frac in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=schedule, round_width=round_width, trim_fraction=frac)
        R, t = s.run()
        res.append((R, t, s.get_best_error(), s.stats()))
        s.close()
    return res


def _check(batch, out, solo, idx):
    for k, i in enumerate(idx):
        R, t, e, st = solo[i]
        assert out[k] is not None, (k, batch.status(k))
        Rb, tb = out[k]
        assert np.array_equal(Rb.view(np.uint32), R.view(np.uint32)), k
        assert np.array_equal(tb.view(np.uint32), t.view(np.uint32)), k
        assert np.float32(batch.get_best_error(k)).view(np.uint32) == np.float32(e).view(np.uint32), k
        sb = batch.stats(k)
        for key in CONTRACT:
            assert sb[key] == st[key], (k, key, sb[key], st[key])


@pytest.mark.parametrize("schedule,round_width", [(0, 1), (1, 2), (1, 0)], ids=["serial", "round-fixed", "round-adaptive"])
def test_mixed_batch_matches_solo_trimmed_runs(fg, gpu_required, schedule, round_width):
    pairs = _pairs(fg)
    solo = _solo(fg, pairs, schedule, round_width)
    assert all(st["bounds_calls"] > 0 for *_, st in solo)  # every pair searched
    b = fg.FastGoICPBatch(pairs, schedule=schedule, round_width=round_width)
    _check(b, b.run(), solo, range(len(pairs)))
    b.close()


def test_window_and_order_do_not_matter_for_trimmed_pairs(fg, gpu_required):
    pairs = _pairs(fg, seed=1)
    solo = _solo(fg, pairs, 1, 0)
    for max_live in (1, 2, 0):
        b = fg.FastGoICPBatch(pairs, schedule=1, round_width=0, max_live=max_live)
        _check(b, b.run(), solo, range(len(pairs)))
        b.close()
    perm = [4, 2, 0, 5, 3, 1]
    b = fg.FastGoICPBatch([pairs[i] for i in perm], schedule=1, round_width=0, max_live=2)
    _check(b, b.run(), solo, perm)
    b.close()


def test_large_trimmed_pair_runs_its_whole_icp_loop(fg, gpu_required):
    """a trimmed pair above 262144 source points (ctx_icp's whole loop on the launcher thread) next to small pairs"""
    big_t, big_s, _, _ = fg.synth.make_pair(40000, 270000, (1.0, 0.8, 0.6), seed=77, angle_deg=20.0)
    small = _pairs(fg, seed=2)[:3]
    pairs = [small[0], (big_t, big_s, 0.02, 1e-3, 0.1), small[1], small[2]]
    solo = _solo(fg, pairs, 0, 1)
    b = fg.FastGoICPBatch(pairs)
    _check(b, b.run(), solo, range(len(pairs)))
    b.close()


def test_trimmed_pairs_share_bounds_launches(fg, gpu_required):
    pairs = [p for p in _pairs(fg, seed=3) if p[4] > 0]
    assert len(pairs) == 4
    solo_calls = 0
    for tgt, src, lut, mse, frac in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, trim_fraction=frac)
        s.run()
        solo_calls += s.stats()["bounds_calls"]
        s.close()
    b = fg.FastGoICPBatch(pairs)
    assert all(o is not None for o in b.run())
    bl, _ = b.launches()
    assert 0 < bl < solo_calls, (bl, solo_calls)
    b.close()


def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def test_cli_batch_of_trimmed_configs_writes_what_lone_runs_write(fg, gpu_required, tmp_path):
    """--batch with two trimmed configs of different fractions and one untrimmed config: the output TOML (but `seconds`) and the PLY
    of every config as a lone -c run of it writes them"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fast-go-icp_amd", "lib", "fast-go-icp")
    (tmp_path / "cfgs").mkdir()
    names = []
    chosen = [p for p in _pairs(fg, seed=4)][:3]  # trims 0.1, 0.0, 0.25
    for i, (tgt, src, lut, mse, frac) in enumerate(chosen):
        _write_txt(tmp_path / f"tgt{i}.txt", tgt)
        _write_txt(tmp_path / f"src{i}.txt", src)
        for tag in ("lone", "batch"):
            (tmp_path / "cfgs" / f"{tag}{i}.toml").write_text(
                f'[io]\ntarget = "{tmp_path}/tgt{i}.txt"\nsource = "{tmp_path}/src{i}.txt"\noutput = "{tmp_path}/{tag}{i}.toml"\n'
                f'visualization = "{tmp_path}/{tag}{i}.ply"\n[params]\nlut_resolution = {lut}\nmse_threshold = {mse}\nseed = 3\n'
                f'trim = {"true" if frac else "false"}\ntrim_fraction = {frac}\n')
        names.append(f"cfgs/batch{i}.toml")
        p = subprocess.run([exe, "-c", str(tmp_path / "cfgs" / f"lone{i}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for i in range(len(chosen)):
        lone = [ln for ln in (tmp_path / f"lone{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        bat = [ln for ln in (tmp_path / f"batch{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        assert lone == bat, (lone, bat)
        assert (tmp_path / f"lone{i}.ply").read_bytes() == (tmp_path / f"batch{i}.ply").read_bytes()
