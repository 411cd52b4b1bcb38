"""GPU: the early exit's gate and its pre-filled "not evaluated" partials (fgoicp_bounds_submit_cut; csrc/device/bounds_item.hpp,
tick_keys_kernel / tick_prefill_kernel in csrc/device/kernels.hip) at the smallest shapes where they can go wrong.

A work item of a window with thresholds reads its evaluation's gate and, if the evaluation is over, ends without a store: the partial
that says "not evaluated, at the threshold" was written for every chunk ahead of the bounds kernel, by the key kernel of the sorted path
or by the prefill kernel of the small, unsorted path.  What is reported must not depend on any of that: a row below its threshold T
comes back bit for bit as from a run without thresholds, every other row as {T, T}.

Shapes: 900 source points = 4 chunks of 256 with a ragged last one (132 points), two chunks per item; 700 points = 3 chunks, so the
second item of an evaluation holds ONE chunk; exactly 512 points = one whole item per evaluation.  64 evaluations (72 rows) in four
groups — fix_rot, rotation and 8 dual evaluations (twins of groups 0 and 1) — with every kind of threshold in every group: +inf (the
evaluation is not cutting), tiny (decided by the first finished item), the row's own lower bound (the row is AT its threshold) and the
next float above it (the row is just below).

The counter of not-evaluated items is asserted on a submission of 16384 evaluations: an item is only skipped if it STARTS after another
item of its evaluation has finished, and the 128 one-wave workgroups of 64 evaluations are all resident at once (the device holds
more than 4000 such waves), so there the count depends on nothing the code does — it is printed, not asserted.  32768 items are eight
times what the device holds, and they take the sorted path in the shipped build (more than 4096 items), which the 64 evaluations only
do with the development build's FGOICP_SMALL_TICK."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TINY = np.float32(1e-30)
RES = 0.02  # LUT resolution: coarse enough to build in no time, fine enough that the clouds count as sparse (256 points per chunk, two chunks per item)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _submission(fg, seed, per_group=(16, 16, 20, 20), twins=8):
    """Four groups: 0 fix_rot and 1 not, on the same rotation node and sharing `twins` translation nodes (dual evaluations); 2 not fix_rot; 3 fix_rot."""
    rng = np.random.default_rng(seed)
    rn = [fg.RotNode(0.125, -0.25, 0.375, 0.0625), fg.RotNode(-0.375, 0.125, 0.25, 0.03125), fg.RotNode(0.25, 0.25, -0.125, 0.125)]
    spans = (0.125, 0.125, 0.0625, 0.25)
    groups = [np.concatenate([rng.uniform(-0.6, 0.6, (n, 3)), np.full((n, 1), s)], axis=1).astype(np.float32) for n, s in zip(per_group, spans)]
    groups[1][2:2 + twins] = groups[0][4:4 + twins]
    offs = np.concatenate([[0], np.cumsum(per_group)])
    twin = np.full(offs[-1], -1, np.int32)
    for k in range(twins):
        twin[4 + k] = offs[1] + 2 + k
        twin[offs[1] + 2 + k] = 4 + k
    return dict(Rs=[rn[0].q.R, rn[0].q.R, rn[1].q.R, rn[2].q.R], spans=[rn[0].span, rn[0].span, rn[1].span, rn[2].span], fixes=[True, False, False, True],
                groups=groups, twin=twin)


@pytest.fixture(scope="module", params=[900, 700, 512])
def case(request, fg, gpu_required):
    """The clouds, the submission and its rows WITHOUT thresholds (computed once, never changed)."""
    ns = request.param
    tgt, src, _, _ = fg.synth.make_pair(2000, ns, (0.156, 0.152, 0.118), seed=40 + ns, angle_deg=30.0)
    pct, pcs, _, _, _, bounds = fg.synth.preprocess(tgt, src)
    sub = _submission(fg, ns)
    reg = fg.Registration(pct, pcs, bounds, RES)
    info = reg.info()
    assert info["points_per_item"] == 256 and info["chunks_per_item_with_thresholds"] == 2 and info["items_per_evaluation"] == (ns + 255) // 256
    exact = [(lb.copy(), ub.copy()) for lb, ub in reg.compute_bounds_multi(sub["Rs"], sub["spans"], sub["fixes"], sub["groups"])]
    reg.close()
    assert all(float(lb.max()) > 0 for lb, _ in exact)
    for a in exact:
        for b in a:
            b.setflags(write=False)
    return dict(ns=ns, pct=pct, pcs=pcs, bounds=bounds, sub=sub, exact=exact)


def _check_rows(got, exact, cut):
    for g, ((lb, ub), (lbx, ubx)) in enumerate(zip(got, exact)):
        below = lbx < cut[g]
        assert np.array_equal(_bits(lb[below]), _bits(lbx[below])) and np.array_equal(_bits(ub[below]), _bits(ubx[below])), g
        assert np.all(lb[~below] == cut[g]) and np.all(ub[~below] == cut[g]), g


def _pivot(lbx):
    """Index of the row with the median of the positive lower bounds."""
    pos = np.flatnonzero(lbx > 0)
    assert len(pos) > 0
    return int(pos[np.argsort(lbx[pos])[len(pos) // 2]])


def _threshold(kind, lbx):
    """One group's threshold of the given kind; `at` / `above` sit on the pivot row."""
    pivot = np.float32(lbx[_pivot(lbx)])
    return {"inf": np.float32(np.inf), "tiny": TINY, "at": pivot, "above": np.nextafter(pivot, np.float32(np.inf))}[kind]


def _run_cases(fg, case, expect_sorted):
    sub, exact = case["sub"], case["exact"]
    args = (sub["Rs"], sub["spans"], sub["fixes"], sub["groups"])
    reg = fg.Registration(case["pct"], case["pcs"], case["bounds"], RES)
    try:
        kinds = ["inf", "tiny", "at", "above"]
        for shift in range(4):  # every kind in every group; the dual evaluations get every pair of kinds of groups 0 and 1
            cut = np.array([_threshold(kinds[(g + shift) % 4], exact[g][0]) for g in range(4)], np.float32)
            for twin in (sub["twin"], None):
                got = reg.compute_bounds_cut(*args, cut, twin=twin, slot=shift & 1)
                _check_rows(got, exact, cut)
                for g in range(4):  # the pivot row itself: AT its threshold it reports the threshold, just below it its exact bits
                    k = _pivot(exact[g][0])
                    if kinds[(g + shift) % 4] == "at":
                        assert got[g][0][k] == cut[g] and got[g][1][k] == cut[g]
                    if kinds[(g + shift) % 4] == "above":
                        assert _bits(got[g][0])[k] == _bits(exact[g][0])[k] and _bits(got[g][1])[k] == _bits(exact[g][1])[k]
        # the counter: nothing is skipped without a finite threshold; with tiny ones the count is a matter of timing at this size (module docstring)
        reg.cut_stats(reset=True)
        cut = np.full(4, np.inf, np.float32)
        _check_rows(reg.compute_bounds_cut(*args, cut, twin=sub["twin"]), exact, cut)
        offered, skipped = reg.cut_stats(reset=True)
        assert offered == 64 * ((case["ns"] + 255) // 256) and skipped == 0
        cut = np.full(4, TINY, np.float32)
        _check_rows(reg.compute_bounds_cut(*args, cut, twin=sub["twin"]), exact, cut)
        offered, skipped = reg.cut_stats(reset=True)
        print(f"ns {case['ns']}, 64 evaluations, tiny thresholds: {skipped} of {offered} chunks not evaluated")
        assert offered == 64 * ((case["ns"] + 255) // 256) and 0 <= skipped < offered
        # pre-filled markers do not outlive their window: thresholds, then none, then thresholds again, on the same slot
        for cut in (np.full(4, TINY, np.float32), None, np.array([_threshold("at", exact[g][0]) for g in range(4)], np.float32), None):
            got = reg.compute_bounds_cut(*args, cut, twin=sub["twin"], slot=1)
            _check_rows(got, exact, np.full(4, np.inf, np.float32) if cut is None else cut)
        assert (reg.sort_fallbacks()[0] > 0) == expect_sorted
    finally:
        reg.close()


def test_gate_and_prefilled_partials_on_the_small_unsorted_path(fg, case):
    """64 evaluations are at most 128 work items: the shipped build reads their descriptors in place and skips the sort, so the gates and
    the "not evaluated" partials come from tick_prefill_kernel."""
    _run_cases(fg, case, expect_sorted=False)


@pytest.mark.dev_knobs
def test_gate_and_prefilled_partials_on_the_sorted_path(fg, case, monkeypatch):
    """The same through the sort (development build: FGOICP_SMALL_TICK=0), where tick_keys_kernel writes them on its way, one thread per
    item of two chunks (of one: the last item of 700 points)."""
    monkeypatch.setenv("FGOICP_SMALL_TICK", "0")
    _run_cases(fg, case, expect_sorted=True)


def test_tiny_thresholds_skip_items_once_the_device_is_full(fg, case):
    """16384 evaluations (18432 rows, 32768 work items at 900 points: eight times the waves the device holds, and the sorted path in the
    shipped build): with a tiny threshold in every group most items start after their evaluation is over and are not evaluated; with
    +inf none is; the rows keep the contract either way, and a window without thresholds on the same slot afterwards is exact."""
    sub = _submission(fg, 1000 + case["ns"], per_group=(4096, 4096, 5120, 5120), twins=2048)
    args = (sub["Rs"], sub["spans"], sub["fixes"], sub["groups"])
    reg = fg.Registration(case["pct"], case["pcs"], case["bounds"], RES)
    try:
        exact = reg.compute_bounds_multi(*args)
        nchunk = (case["ns"] + 255) // 256
        reg.cut_stats(reset=True)
        cut = np.full(4, np.inf, np.float32)
        _check_rows(reg.compute_bounds_cut(*args, cut, twin=sub["twin"]), exact, cut)
        assert reg.cut_stats(reset=True) == (16384 * nchunk, 0)
        cut = np.full(4, TINY, np.float32)
        _check_rows(reg.compute_bounds_cut(*args, cut, twin=sub["twin"]), exact, cut)
        offered, skipped = reg.cut_stats(reset=True)
        print(f"ns {case['ns']}, 16384 evaluations, tiny thresholds: {skipped} of {offered} chunks not evaluated")
        assert offered == 16384 * nchunk
        if nchunk > 2:  # (512 points: one item per evaluation, nothing to skip)
            assert 0 < skipped < offered
        else:
            assert skipped == 0
        cut = np.array([_threshold(k, exact[g][0]) for g, k in enumerate(["above", "at", "tiny", "inf"])], np.float32)
        _check_rows(reg.compute_bounds_cut(*args, cut, twin=sub["twin"]), exact, cut)
        _check_rows(reg.compute_bounds_cut(*args, None, twin=sub["twin"]), exact, np.full(4, np.inf, np.float32))
        assert reg.sort_fallbacks()[0] >= 4
    finally:
        reg.close()
