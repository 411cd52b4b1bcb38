"""GPU: the k-smallest selection and the inlier mask (trim_select_kernel, select_wide_*_kernel, icp_inlier_mask_kernel,
icp_inlier_ties_kernel; launch_inlier_mask and launch_icp_inliers) on rows of squared distances designed bit by bit
(tests/selection_rows.py), against a sort: radix digits at their edges, rows that are mostly one value, k = 1 and k = n, rows of zeros,
the switch between the one-block and the device-wide selection, ragged slices of the wide sum, and the index select of the ties.

The bounds.  The mask, v_k and the count are exact.  The kernels add at most 2^22 fp32 values in fp64 and round once, so their sum is
within one fp32 ulp of float32(fsum(inliers)) — and differs at all only when the exact sum lies within about n 2^-53 relative of a
rounding midpoint."""
import numpy as np
import pytest

from tests import selection_rows as sr
from tests.selection_rows import I3, ZERO3, bits, pattern_of

pytestmark = pytest.mark.gpu


def all_flags(fg):
    return [("default", 0), ("no_morton", fg.FLAG_NO_MORTON), ("curve_order", fg.FLAG_CURVE_ORDER), ("brute_force_nn", fg.FLAG_BRUTE_FORCE_NN)]


def check_report(row, k, a, skip_sse):
    """one report and one fgoicp_sse of a context trimmed to k, against the sort"""
    mask, vk, need, sse_ref = row.ref.at(k)
    where = (row.name, k, need)
    assert np.array_equal(bits(a.dist2), row.pattern), where  # the designed bits again: whatever fails below is the selection's
    assert not a.indices.any(), where
    assert a.inliers == k == int(a.inlier.sum()), where
    assert pattern_of(a.max_inlier_dist2) == vk, (where, hex(pattern_of(a.max_inlier_dist2)), hex(vk))
    wrong = np.flatnonzero(a.inlier != mask)
    assert len(wrong) == 0, (where, wrong[:8], row.pattern[wrong[:8]])
    assert sr.ulp_apart(a.sse, sse_ref) <= 1, (where, float(a.sse), float(sse_ref))
    # the report searches every query; fgoicp_sse leaves out those whose LUT lower bound lies above the cut
    assert pattern_of(skip_sse) == pattern_of(a.sse), (where, float(skip_sse), float(a.sse))
    if vk == 0:
        assert pattern_of(a.sse) == 0 and pattern_of(a.max_inlier_dist2) == 0, where  # +0.0


def same_report(a, b, where):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(bits(a.dist2), bits(b.dist2)), where
    assert np.array_equal(a.inlier, b.inlier) and np.array_equal(a.target_hit, b.target_hit), where
    assert (a.inliers, a.targets_hit, pattern_of(a.max_inlier_dist2), pattern_of(a.sse)) == (b.inliers, b.targets_hit, pattern_of(b.max_inlier_dist2), pattern_of(b.sse)), where


def run_row(fg, row, flags, passes=2):
    """One context for the row, k looped inside it: every k against the sort; then trimming off — the plain sum; then every k again — the
    same bytes, so nothing stays behind in the selection scratch or the tie count.  Returns the reports of the first pass."""
    reg = fg.Registration(row.target, row.points, sr.BOX, sr.RES, flags=flags)
    try:
        first = []
        for k in row.ks:
            reg.set_inliers(k)
            a = reg.alignment(I3, ZERO3)
            s = reg.compute_sse_error(I3, ZERO3)
            check_report(row, k, a, s)
            first.append((a, s))
        if passes > 1:
            reg.set_inliers(0)
            total = reg.compute_sse_error(I3, ZERO3)
            assert sr.ulp_apart(total, row.ref.total()) <= 1, (row.name, float(total), float(row.ref.total()))
            for k, (a, s) in zip(row.ks, first):
                reg.set_inliers(k)
                same_report(reg.alignment(I3, ZERO3), a, (row.name, k, "second pass"))
                assert pattern_of(reg.compute_sse_error(I3, ZERO3)) == pattern_of(s), (row.name, k, "second pass")
    finally:
        reg.close()
    return [a for a, _ in first]


def run_row_under_all_flags(fg, row):
    row.check_design()
    base = None
    for name, flags in all_flags(fg):
        reports = run_row(fg, row, flags)
        if base is None:
            base = reports
        else:
            for k, a, b in zip(row.ks, base, reports):
                same_report(a, b, (row.name, k, name))
    return base


REPORT_FAMILIES = ("digit_edges", "dense_run", "all_equal", "two_values", "zeros")
SIZES = sr.ONE_BLOCK_SIZES + sr.WIDE_SIZES
REPORT_CASES = [(fam, n, order) for fam in REPORT_FAMILIES for n in SIZES if sr.applies(fam, n) for order in sr.ORDERS]
DECOY_CASES = [(fam, n) for fam in REPORT_FAMILIES for n in (257, 131073)]


# ---- 1. the report and the skip path: every family at every size in three caller orders, four kinds of context each --------------------------
# (one case per row: a trimmed context of 32767 points or more takes most of a second to set up, whatever is asked of it afterwards)
@pytest.mark.parametrize("family,n,order", REPORT_CASES, ids=[f"{f}-{n}-{o}" for f, n, o in REPORT_CASES])
def test_report_and_sse_select_what_the_sort_selects(fg, gpu_required, family, n, order):
    run_row_under_all_flags(fg, sr.Row(family, n, order, "origin"))


@pytest.mark.parametrize("family,n", DECOY_CASES, ids=[f"{f}-{n}" for f, n in DECOY_CASES])
def test_report_and_sse_against_a_target_of_two_leaves(fg, gpu_required, family, n):
    """the origin and 32 decoys near the corners of the box: the origin is still every point's neighbour, the tree has two leaves"""
    run_row_under_all_flags(fg, sr.Row(family, n, "shuffled", "decoys"))


# ---- 2. the ICP path: launch_icp_inliers ----------------------------------------------------------------------------------------------
def check_procrustes(reg, row, k):
    mask = row.ref.at(k)[0]
    reg.set_inliers(k)
    R, t, cen, ABt, idx = reg.procrustes(row.points)
    idx = idx.view(np.uint32)
    found = idx != sr.NO_CORRESPONDENCE
    assert not idx[found].any(), (row.name, k)  # the origin, target point 0
    assert found[mask].all(), (row.name, k, np.flatnonzero(mask & ~found)[:8])  # every inlier of the sort has its correspondence
    want = row.points[mask].astype(np.float64).mean(axis=0)
    assert np.allclose(cen[:3], want, rtol=1e-6, atol=1e-7), (row.name, k, cen[:3], want)
    assert np.allclose(cen[3:], 0.0, atol=1e-7), (row.name, k)


ICP_CASES = [("directional_ties", n) for n in (16,) + SIZES if sr.applies("directional_ties", n)] + [("all_equal", 40000)]


@pytest.mark.parametrize("family,n", ICP_CASES, ids=[f"{f}-{n}" for f, n in ICP_CASES])
def test_icp_inlier_cut_takes_the_lowest_caller_indices_of_the_tied(fg, gpu_required, family, n):
    made = sr.FAMILIES[family](n)
    rows = [(sr.Row(family, n, order, "origin", made), 0) for order in sr.ORDERS]
    rows += [(rows[2][0], fg.FLAG_CURVE_ORDER), (sr.Row(family, n, "shuffled", "decoys"), 0)]
    for row, flags in rows:
        row.check_design()
        if family == "directional_ties":
            assert max(row.ks) <= sr.TIES_MAX_K and sr.ties_separation(row.pattern, row.signs, max(row.ks)) > 1e-3
        reg = fg.Registration(row.target, row.points, sr.BOX, sr.RES, flags=flags)
        try:
            a = reg.alignment(I3, ZERO3)
            assert np.array_equal(bits(a.dist2), row.pattern), (row.name, flags)
            for rep in range(2):  # the second round finds the tie count and the scratch as the first left them
                for k in row.ks:
                    check_procrustes(reg, row, k)
        finally:
            reg.close()


# ---- 3. the switch between the one-block and the device-wide selection ----------------------------------------------------------------------
@pytest.mark.parametrize("flags_name", ["default", "no_morton", "curve_order", "brute_force_nn"])
def test_one_row_cut_to_either_side_of_the_path_switch(fg, gpu_required, flags_name):
    flags = dict(all_flags(fg))[flags_name]
    sizes = (32767, 32768, 32769)
    made = {n: sr.digit_edges(n) for n in sizes}
    ks = sorted({k for n in sizes for k in made[n][2] if k <= sizes[0]} | {1, sizes[0] - 1})
    rows, reports = {}, {}
    for n in sizes:
        rows[n] = sr.Row("digit_edges", n, "generated", "origin", made[n])
        rows[n].ks = ks + [k for k in (n - 1, n) if k not in ks]
        assert np.array_equal(rows[n].pattern[:sizes[0]], rows[sizes[0]].pattern)  # one row, cut and extended
        rows[n].check_design()
        reports[n] = run_row(fg, rows[n], flags)
    for lo, hi in zip(sizes, sizes[1:]):
        for i, k in enumerate(ks):  # the shared prefix: a point added behind it takes an inlier's place only if it lies below the cut
            changed = np.flatnonzero(reports[hi][i].inlier[:lo] != reports[lo][i].inlier)
            want = np.flatnonzero(rows[hi].ref.at(k)[0][:lo] != rows[lo].ref.at(k)[0])
            assert np.array_equal(changed, want) and len(changed) <= 1, (lo, hi, k)
            assert len(changed) == int(reports[hi][i].inlier[lo:].sum()), (lo, hi, k)


# ---- 4. either selection above 32768 points, on the development build --------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["digit_edges", "two_values"])
def test_both_selections_agree_with_the_sort_at_40000_points(fg, gpu_required, monkeypatch, family):
    """FGOICP_SELECT_WIDE=0 keeps trim_select_kernel for every row (the context allocates no wide scratch), 1 is the default"""
    row = sr.Row(family, 40000, "shuffled")
    row.check_design()
    reports = []
    for wide in ("0", "1"):
        monkeypatch.setenv("FGOICP_SELECT_WIDE", wide)
        reports.append(run_row(fg, row, 0))
    for k, a, b in zip(row.ks, *reports):
        same_report(a, b, (row.name, k, "FGOICP_SELECT_WIDE 0 and 1"))


# ---- 5. tied caller indices with a non-zero first radix digit ---------------------------------------------------------------------------------
def test_ties_beyond_two_million_caller_indices(fg, gpu_required):
    """all equal at n = 2^21 + 1000, k = 2^21 - 1, 2^21, 2^21 + 1: the index select of icp_inlier_ties_kernel picks a first digit of 0, 0
    and 1.  The one large case of this file."""
    row = sr.Row("all_equal", sr.TIES_FIRST_DIGIT_N)
    assert row.ks == [2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1]
    row.check_design()
    run_row(fg, row, 0, passes=1)
    reg = fg.Registration(row.target, row.points, sr.BOX, sr.RES, flags=fg.FLAG_CURVE_ORDER)
    try:
        for k in row.ks:
            check_procrustes(reg, row, k)
    finally:
        reg.close()
