"""CPU: the designed rows of tests/selection_rows.py are what tests/test_gpu_selection_rows.py takes them for — the restated scan returns
the designed bits, the reference is the plain sort, the edge patterns have the radix digits they are named for, and every k of a
family cuts where the family says."""
import numpy as np
import pytest

from tests import selection_rows as sr

SIZES = sr.ONE_BLOCK_SIZES + sr.WIDE_SIZES
CASES = [(fam, n) for fam in sr.FAMILIES for n in SIZES + (16, 40000) if sr.applies(fam, n)]


def naive(pattern, k):
    """the reference again, with sorted() on (bits, caller index) pairs"""
    pairs = sorted((int(u), i) for i, u in enumerate(pattern))[:k]
    mask = np.zeros(len(pattern), bool)
    mask[[i for _, i in pairs]] = True
    vk = pairs[-1][0]
    total = 0.0
    for u, _ in pairs:  # few and small enough here for the plain fp64 sum to be exact: at most 257 values of 24 bits within 2^20 of each other
        total += float(np.uint32(u).view(np.float32))
    return mask, vk, sum(1 for u, _ in pairs if u == vk), np.float32(total)


def check_ks(row):
    """every k of the family lands where the family says"""
    ref, n, ks = row.ref, row.n, row.ks
    assert ks == sorted(set(ks)) and 1 <= ks[0] and ks[-1] <= n
    at = {k: ref.at(k) for k in ks}
    for k, (mask, vk, need, sse) in at.items():
        below, count = ref.rank_range(vk)
        assert int(mask.sum()) == k and below + need == k and 1 <= need <= count
        assert np.array_equal(np.sort(row.pattern[mask]), ref.sorted[:k])
        tied = np.flatnonzero(row.pattern == vk)
        assert mask[tied[:need]].all() and not mask[tied[need:]].any()  # ties to the lowest caller index
    fam = row.family
    if fam == "digit_edges":
        hi = sr.TARGETS[row.name.rsplit("-", 1)[1]][1]
        for j, (name, u) in enumerate(sr.edge_patterns(hi)):
            below, count = ref.rank_range(u)
            assert count >= 1 + j % 3, name
            for c in range(1, count + 1):  # the cut on the pattern, inside its copies (need < count) and on the last of them
                assert at[below + c][1:3] == (u, c), (name, c)
        assert any(need < ref.rank_range(vk)[1] for _, vk, need, _ in at.values())
    elif fam == "dense_run":
        assert len(np.unique(row.pattern)) == n and int(ref.sorted[-1]) - int(ref.sorted[0]) == n - 1
        B = (int(ref.sorted[-1]) >> 21) << 21
        assert int(ref.sorted[0]) < B and sum(1 for u in (int(ref.sorted[0]), int(ref.sorted[-1])) if u >> 21 == B >> 21) == 1  # one multiple of 2^21 crossed
        crossing = ref.rank_range(B)[0]
        assert {1, n, crossing, crossing + 1} <= set(ks) and at[crossing][1] == B - 1 and at[crossing + 1][1] == B
        assert sr.digits(B - 1)[1:] == (0x7FF, 0x3FF) and sr.digits(B)[1:] == (0, 0)
        if n >= 4096:
            assert len(np.unique(ref.sorted >> 10)) >= n // 1024
    elif fam == "all_equal":
        assert len(np.unique(row.pattern)) == 1 and {1, n} <= set(ks)
        if n >= 4:
            assert len(np.unique(row.points, axis=0)) == 4  # the four directions
        for k, (mask, vk, need, _) in at.items():
            assert need == k and np.array_equal(np.flatnonzero(mask), np.arange(k))
        if 2049 < n < 2 ** 21:
            assert {1023, 1024, 1025, 2047, 2048, 2049, n - 1} <= set(ks)
    elif fam == "two_values":
        P, Q = (int(u) for u in np.unique(row.pattern))
        assert Q == P + 1 and sr.digits(Q)[1:] == (0, 0) and sr.digits(P)[0] == sr.digits(Q)[0] - 1
        nP = ref.rank_range(P)[1]
        assert nP == n // 2 and {nP, nP + 1} <= set(ks) and at[nP][1:3] == (P, nP) and at[nP + 1][1:3] == (Q, 1)
        if n >= 16:
            assert any(vk == P and need < nP for _, vk, need, _ in at.values()) and any(vk == Q and 1 < need < n - nP for _, vk, need, _ in at.values())
    elif fam == "zeros":
        z = sr.zeros_count(n)
        assert ref.rank_range(0) == (0, z) and {1, z, n} <= set(ks)
        for k, (mask, vk, need, sse) in at.items():
            assert (vk == 0 and sr.pattern_of(sse) == 0) if k <= z else (vk >= sr.LO and sse > 0)
        if n > z:
            assert z + 1 in ks
    elif fam == "directional_ties":
        below, count = ref.rank_range(sr.TIED_PATTERN)
        assert count == sr.TIE_COPIES and ks == [below + c for c in range(1, 9)] and ks[-1] <= sr.TIES_MAX_K
        assert all(at[below + c][1:3] == (sr.TIED_PATTERN, c) for c in range(1, 9))
        assert sr.ties_separation(row.pattern, row.signs, ks[-1]) > 1e-3


@pytest.mark.parametrize("family,n", CASES, ids=[f"{f}-{n}" for f, n in CASES])
def test_rows_are_what_they_are_designed_to_be(family, n):
    made = sr.FAMILIES[family](n)
    generated = None
    for order, target in [(o, "origin") for o in sr.ORDERS] + [("shuffled", "decoys")]:
        row = sr.Row(family, n, order, target, made if target == "origin" else None)
        row.check_design()
        if target == "origin":
            assert (np.abs(row.points) <= 1).all()
        else:
            assert (row.pattern < sr.HI_DECOYS).all() and len(row.target) == 33 and not row.target[0].any()
        check_ks(row)
        if n <= 257:
            for k in row.ks:
                got, want = row.ref.at(k), naive(row.pattern, k)
                assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3] and sr.pattern_of(got[3]) == sr.pattern_of(want[3]), (row.name, k)
                one_off = sr.reference(row.pattern, k)
                assert np.array_equal(one_off[0], got[0]) and one_off[1:] == got[1:]
        if order == "generated":
            generated = row
        elif target == "origin":  # the same multiset of (pattern, direction) in another order
            assert np.array_equal(row.ref.sorted, generated.ref.sorted) and row.ks == generated.ks


def test_edge_patterns_have_the_digits_they_are_named_for():
    for hi in (sr.HI, sr.HI_DECOYS):
        edges = dict(sr.edge_patterns(hi))
        assert len(edges) == 21 and len(set(edges.values())) == 21 and all(sr.LO <= u < hi for u in edges.values())
        for j in range(3):
            B, M = edges[f"B{j}"], edges[f"M{j}"]
            assert B % (1 << 21) == 0 and M % (1 << 10) == 0 and M % (1 << 21) != 0
            assert [edges[f"B{j}{s}"] - B for s in ("-2", "-1", "+1")] == [-2, -1, 1] and [edges[f"M{j}{s}"] - M for s in ("-1", "+1")] == [-1, 1]
            d0 = B >> 21
            assert [sr.digits(edges[f"B{j}{s}"]) for s in ("-2", "-1", "", "+1")] == [(d0 - 1, 0x7FF, 0x3FE), (d0 - 1, 0x7FF, 0x3FF), (d0, 0, 0), (d0, 0, 1)]
            m0, m1, _ = sr.digits(M)
            assert [sr.digits(edges[f"M{j}{s}"]) for s in ("-1", "", "+1")] == [(m0, m1 - 1, 0x3FF), (m0, m1, 0), (m0, m1, 1)]
        assert [sr.digits(edges[f"M{j}"])[1] for j in range(3)] == [0x7FF, 0x001, 0x400]
    assert any(B % (1 << 23) == 0 for n, B in sr.edge_patterns() if n in ("B0", "B1", "B2"))  # one B is a power of two: B-1 -> B steps the exponent
    # digits() is the split the kernels use: 11 + 11 + 10 bits
    u = 0xDEADBEEF
    assert (sr.digits(u)[0] << 21) | (sr.digits(u)[1] << 10) | sr.digits(u)[2] == u


def test_digit_edges_rows_are_prefixes_of_each_other():
    """the path-switch test cuts one row to 32767, 32768 and 32769 points"""
    rows = [sr.digit_edges(n) for n in (32767, 32768, 32769)]
    for (p, s, _), (q, t, _) in zip(rows, rows[1:]):
        assert np.array_equal(q[:len(p)], p) and np.array_equal(t[:len(s)], s)


def test_targets():
    t = sr.target_decoys()
    assert t.shape == (33, 3) and t.dtype == np.float32 and not t[0].any() and (np.abs(t) <= 1).all()
    assert (np.abs(t[1:]) >= 0.9).all() and len({tuple(np.sign(p)) for p in t[1:]}) == 8
    assert sr.target_origin().shape == (1, 3) and not sr.target_origin().any()
    # the farthest designed point of a row against the decoys is nearer to the origin than to any decoy, with room to spare
    far = sr.design(np.array([sr.HI_DECOYS - 1] * 8, np.uint32), np.arange(8))
    d = np.linalg.norm(far[:, None, :].astype(np.float64) - t[None, 1:, :], axis=2)
    assert d.min() > 1.2 and np.linalg.norm(far, axis=1).max() < 0.32


def test_design_hits_random_patterns_in_all_eight_directions():
    rng = np.random.default_rng(11)
    u = rng.integers(sr.LO, sr.HI, 20000, dtype=np.uint32)
    u[:3] = (0, sr.LO, sr.HI - 1)
    for target in (sr.target_origin(), sr.target_decoys()):
        uu = u if len(target) == 1 else np.minimum(u, sr.HI_DECOYS - 1).astype(np.uint32)
        pts = sr.design(uu, rng.integers(0, 8, len(uu)))
        idx, d2 = sr.brute_force(target, pts, sr.I3, sr.ZERO3)
        assert np.array_equal(sr.bits(d2), uu) and not idx.any()
    assert not sr.design(np.zeros(4, np.uint32), np.arange(4)).any()


def test_the_two_million_point_row():
    """all equal at n = 2^21 + 1000, built and checked once: the k = 2^21 - 1, 2^21, 2^21 + 1 lowest caller indices are the inliers, so
    the highest inlier's index has first digit 0, 0 and 1 in the index select of icp_inlier_ties_kernel"""
    n = sr.TIES_FIRST_DIGIT_N
    row = sr.Row("all_equal", n)
    assert row.ks == [2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1] and n < 2 ** 22  # (the one-ulp bound of the sums is derived for at most 2^22 terms)
    row.check_design()
    for k in row.ks:
        mask, vk, need, sse = row.ref.at(k)
        assert vk == sr.ALL_EQUAL_PATTERN and need == k and mask[:k].all() and not mask[k:].any()
        assert sr.digits(k - 1)[0] == (0 if k <= 2 ** 21 else 1)
        exact = k * float(np.uint32(vk).view(np.float32))  # k < 2^22 times a 24-bit value: exact in fp64
        assert sse == np.float32(exact)
