"""GPU: terminal rows of the early exit (fgoicp_bounds_submit_leaf; csrc/device/bounds_item.hpp, bounds_finalize_kernel / tick_keys_kernel /
cut_prefill in csrc/device/kernels.hip) at the smallest shapes where they can go wrong, against the exact rows of fgoicp_bounds_submit_twins.

ub_below_span[g] marks the rows of group g with a smaller translation span as TERMINAL (a leaf of the inner BnB, never split): such a row
comes back as {T, T} once its UPPER bound is >= T = cut_above[g]; every other row follows fgoicp_bounds_submit_cut (lower bound >= T); a row
that is not answered {T, T} keeps every bit.  What the kernel got to skip must not show.

Shapes: 1297 source points = 6 chunks of 256, two chunks per item, 17 points in the last pass; 768 points = 3 chunks, the last item of an
evaluation is ONE chunk; a small cloud on a coarse LUT, where an item holds more than 256 points.  Submissions of 4 x 32 rows (the small
path: descriptors read in place, no sort, gates from tick_prefill_kernel), of 24 x 32 rows (with two chunks per item 2304 items at most:
the small path too, window and group bookkeeping of many groups) and of 256 x 64 rows (the sorted two-tier path — tick_keys_kernel writes
the gates and guesses the tiers — and many times the waves the device holds, so that items do start after their evaluation is over: the
counter of not-evaluated items is asserted there only).  Groups come in pairs on one rotation node, fix_rot 1 and 0, sharing eight
translation nodes (dual evaluations); spans 0.0625 (terminal under ub_below_span = 0.1) and 0.125 (not) alternate inside every group;
the last pair carries ub_below_span = 0: no terminal rows there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TINY = np.float32(1e-30)
INF = np.float32(np.inf)
LEAF = np.float32(0.1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _submission(fg, seed, pairs, rows, twins=8):
    rng = np.random.default_rng(seed)
    Rs, spans, fixes, groups, leaf = [], [], [], [], []
    for p in range(pairs):
        rn = fg.RotNode(*rng.uniform(-0.4, 0.4, 3), float(rng.choice([0.0625, 0.03125, 0.125])))
        a, b = [np.concatenate([rng.uniform(-0.6, 0.6, (rows, 3)), np.where(np.arange(rows) % 2 == 0, 0.0625, 0.125)[:, None]], axis=1).astype(np.float32) for _ in range(2)]
        b[2:2 + twins] = a[5:5 + twins]  # (whole nodes: a twin pair has one span; the rows' parities differ, so both spans occur among the twins)
        Rs += [rn.q.R, rn.q.R]; spans += [rn.span, rn.span]; fixes += [True, False]; groups += [a, b]
        leaf += [LEAF if p + 1 < pairs else np.float32(0.0)] * 2
    offs = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    twin = np.full(offs[-1], -1, np.int32)
    for p in range(pairs):
        for k in range(twins):
            i, j = offs[2 * p] + 5 + k, offs[2 * p + 1] + 2 + k
            twin[i], twin[j] = j, i
    return dict(args=(Rs, spans, fixes, groups), twin=twin, leaf=np.asarray(leaf, np.float32))


def _context(fg, ns, res):
    tgt, src, _, _ = fg.synth.make_pair(2000, ns, (0.156, 0.152, 0.118), seed=70 + ns, angle_deg=30.0)
    pct, pcs, _, _, _, bounds = fg.synth.preprocess(tgt, src)
    return pct, pcs, bounds, res


SHAPES = {"1297": (1297, 0.02), "768": (768, 0.02), "coarse": (1500, 0.1)}
SUBS = {"4x32": (2, 32), "24x32": (12, 32)}


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request, fg, gpu_required):
    """The clouds, the submissions and their exact rows (fgoicp_bounds_submit_twins: computed once, never changed)."""
    ns, res = SHAPES[request.param]
    ctx = _context(fg, ns, res)
    reg = fg.Registration(*ctx)
    info = reg.info()
    if request.param == "coarse":
        assert info["points_per_item"] > 256
    else:
        assert info["points_per_item"] == 256 and info["chunks_per_item_with_thresholds"] == 2 and info["items_per_evaluation"] == (ns + 255) // 256
    subs = {}
    for name, (pairs, rows) in SUBS.items():
        if name == "24x32" and request.param != "1297":
            continue
        sub = _submission(fg, 100 * ns + pairs, pairs, rows)
        sub["exact"] = [(lb.copy(), ub.copy()) for lb, ub in reg.compute_bounds_cut(*sub["args"], None, twin=sub["twin"])]
        for a in sub["exact"]:
            for b in a:
                b.setflags(write=False)
        subs[name] = sub
    reg.close()
    return dict(name=request.param, ctx=ctx, subs=subs, items=-(-info["items_per_evaluation"] // info["chunks_per_item_with_thresholds"]))


def _check_rows(got, sub, cut, leaf):
    """Every row by its rule; leaf = None: the lower-bound rule for all (fgoicp_bounds_submit_cut).  Returns (rows answered {T, T}, of them by the upper bound alone)."""
    n_cut = n_leaf = 0
    for g, ((lb, ub), (lbx, ubx)) in enumerate(zip(got, sub["exact"])):
        terminal = np.zeros(len(lbx), bool) if leaf is None else sub["args"][3][g][:, 3] < leaf[g]
        above = np.where(terminal, ubx >= cut[g], lbx >= cut[g])
        assert np.array_equal(_bits(lb[~above]), _bits(lbx[~above])) and np.array_equal(_bits(ub[~above]), _bits(ubx[~above])), g
        assert np.all(lb[above] == cut[g]) and np.all(ub[above] == cut[g]), g
        n_cut += int(above.sum()); n_leaf += int((above & (lbx < cut[g])).sum())
    return n_cut, n_leaf


def _pivot(sub, g):
    """A terminal row of group g with a positive lower bound: the one with the median upper bound among them."""
    lbx, ubx = sub["exact"][g]
    pos = np.flatnonzero((sub["args"][3][g][:, 3] < LEAF) & (lbx > 0))
    assert len(pos) > 0
    return int(pos[np.argsort(ubx[pos])[len(pos) // 2]])


def _threshold(kind, sub, g):
    ubx = sub["exact"][g][1]
    at = np.float32(ubx[_pivot(sub, g)])
    return {"inf": INF, "tiny": TINY, "median": np.float32(np.sort(ubx)[len(ubx) // 2]), "at": at, "above": np.nextafter(at, INF)}[kind]


KINDS = ["inf", "tiny", "median", "at", "above"]


def test_terminal_rows_follow_the_upper_bound_rule(fg, case):
    reg = fg.Registration(*case["ctx"])
    try:
        for sub in case["subs"].values():
            _check_submission(reg, sub)
        assert reg.sort_fallbacks()[0] == 0  # all of this took the small, unsorted path
    finally:
        reg.close()


def _check_submission(reg, sub):
    G = len(sub["exact"])
    by_ub = 0
    for shift in range(len(KINDS)):  # every kind of threshold in every group of a pair; the dual evaluations get pairs of kinds
        cut = np.array([_threshold(KINDS[(g + shift) % len(KINDS)], sub, g) for g in range(G)], np.float32)
        for twin in (sub["twin"], None):
            got = reg.compute_bounds_cut(*sub["args"], cut, twin=twin, slot=shift & 1, ub_below_span=sub["leaf"])
            by_ub += _check_rows(got, sub, cut, sub["leaf"])[1]
            again = reg.compute_bounds_cut(*sub["args"], cut, twin=twin, slot=shift & 1, ub_below_span=sub["leaf"])
            for (lb, ub), (lb2, ub2) in zip(got, again):  # the same submission twice: identical rows, whatever was cut short
                assert np.array_equal(_bits(lb), _bits(lb2)) and np.array_equal(_bits(ub), _bits(ub2))
            for g in range(G):
                if sub["leaf"][g] == 0:
                    continue
                k, kind = _pivot(sub, g), KINDS[(g + shift) % len(KINDS)]
                if kind == "at":  # exactly the row's upper bound: {T, T} — although its lower bound is below T
                    assert sub["exact"][g][0][k] < cut[g] and got[g][0][k] == cut[g] and got[g][1][k] == cut[g]
                if kind == "above":  # the next float above it: the row's exact bits
                    assert _bits(got[g][0])[k] == _bits(sub["exact"][g][0])[k] and _bits(got[g][1])[k] == _bits(sub["exact"][g][1])[k]
            # fgoicp_bounds_submit_cut on the same input: the lower-bound rule only; so does a span of 0 in every group
            _check_rows(reg.compute_bounds_cut(*sub["args"], cut, twin=twin, slot=1 - (shift & 1)), sub, cut, None)
            _check_rows(reg.compute_bounds_cut(*sub["args"], cut, twin=twin, ub_below_span=np.zeros(G, np.float32)), sub, cut, None)
    assert by_ub > 0  # rows that only the new rule decides did occur
    # without thresholds the hint has no effect; markers do not outlive their window
    got = reg.compute_bounds_cut(*sub["args"], None, twin=sub["twin"], ub_below_span=sub["leaf"])
    _check_rows(got, sub, np.full(G, INF), sub["leaf"])


def test_terminal_rows_on_the_sorted_two_tier_path_skip_work(fg, case):
    """256 groups x 64 rows (15360 evaluations, 3 or 2 items each on the sparse shapes: beyond the 4096 items of the small path, and several times the waves the
    device holds).  With every group's threshold at the median of its exact upper bounds the terminal rule leaves items unevaluated, and more
    of them than the lower-bound rule alone on the same input; the rows keep their rules either way."""
    reg = fg.Registration(*case["ctx"])
    try:
        sub = _submission(fg, 7, 128, 64)
        G = 256
        sub["exact"] = reg.compute_bounds_cut(*sub["args"], None, twin=sub["twin"])
        cut = np.array([_threshold("median", sub, g) for g in range(G)], np.float32)
        reg.cut_stats(reset=True)
        n_cut, by_ub = _check_rows(reg.compute_bounds_cut(*sub["args"], cut, twin=sub["twin"], ub_below_span=sub["leaf"]), sub, cut, sub["leaf"])
        offered, skipped = reg.cut_stats(reset=True)
        _check_rows(reg.compute_bounds_cut(*sub["args"], cut, twin=sub["twin"]), sub, cut, None)
        offered_lb, skipped_lb = reg.cut_stats(reset=True)
        print(f"{case['name']}: {n_cut} rows at their threshold, {by_ub} of them by the upper bound alone; chunks not evaluated {skipped} of {offered} (lower-bound rule alone: {skipped_lb})")
        assert offered == offered_lb > 4096 * 2 and by_ub > 0
        if case["items"] >= 2:  # (one item per evaluation: nothing to leave out)
            assert skipped > 0
        else:
            assert skipped == 0
        cut = np.array([_threshold(KINDS[g % len(KINDS)], sub, g) for g in range(G)], np.float32)
        _check_rows(reg.compute_bounds_cut(*sub["args"], cut, twin=sub["twin"], ub_below_span=sub["leaf"]), sub, cut, sub["leaf"])
        _check_rows(reg.compute_bounds_cut(*sub["args"], None, twin=sub["twin"], ub_below_span=sub["leaf"]), sub, np.full(G, INF), sub["leaf"])
        assert reg.sort_fallbacks()[0] >= 4  # windows that went through the sort
    finally:
        reg.close()


@pytest.mark.parametrize("sched_name", ["serial", "round"])
def test_leaf_rule_leaves_the_search_alone(fg, gpu_required, sched_name):
    """A whole certify run (the tiny pair, 150 degrees, mse 5e-5) with the early exit — the driver now marks the leaves of its inner BnBs
    as terminal — and with every subcube evaluated in full: the same counters, the same incumbent bit for bit, and work items left out."""
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=150.0, min_angle_deg=110.0)
    sched, K = (fg.SCHEDULE_SERIAL, 1) if sched_name == "serial" else (fg.SCHEDULE_ROUND, 0)
    out = {}
    for on in (False, True):
        s = fg.FastGoICP(tgt, src, 0.02, 5e-5, schedule=sched, round_width=K)
        s.set_early_exit(on)
        reg = s.registration
        reg.cut_stats(reset=True)
        R, t = s.run()
        out[on] = (R, t, float(s.get_best_error()), s.stats(), reg.cut_stats())
        s.close()
    (R0, t0, e0, st0, c0), (R1, t1, e1, st1, c1) = out[False], out[True]
    assert np.array_equal(R0, R1) and np.array_equal(t0, t1) and e0 == e1
    for k in ("trans_cubes", "bounds_calls", "rot_cubes", "icp_runs", "icp_iters", "inner_bnb", "rounds"):
        assert st0[k] == st1[k], k
    assert c0 == (0, 0)
    offered, skipped = c1
    print(f"{sched_name}: {st1['trans_cubes']} subcubes, {offered} work items, {skipped} not evaluated ({skipped / max(offered, 1):.3f})")
    assert offered > 0 and skipped > 0
