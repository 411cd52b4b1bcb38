"""Designed rows of squared distances for the k-smallest selection and the inlier mask (trim_select_kernel, the select_wide_* kernels,
icp_inlier_mask_kernel, icp_inlier_ties_kernel), and their plain reference: a sort.  Test infrastructure, in the style of
tests/nn_restatement.py: the properties the rows are designed for are asserted without a GPU by tests/test_selection_rows_host.py.

The construction.  The scans compute d2 = fma(dz, dz, fma(dy, dy, dx * dx)) (csrc/device/dist_sq.hpp).  Against a target point at the
origin, under R = I and t = 0, a source point (x, 0, z) gives d2 = fl(z^2 + fl(x^2)).  For a wanted fp32 value v take x = fl32(sqrt(0.875 v)),
A = fl32(x * x), z = fl32(sqrt(v - A)), the roots in fp64 and rounded to fp32: the last fma rounds to v, bit for bit (every test asserts it
through tests/nn_restatement.brute_force before it believes a row).  Negating x and / or z gives the same bits in another direction, and so
does (0, x, z): fma(dy, dy, 0 * 0) = fl(x^2) again.  Pattern 0 is a point on the target."""
import math

import numpy as np

from tests.nn_restatement import I3, ZERO3, bits, brute_force  # noqa: F401  (re-exported for the tests)

f32 = np.float32


def pattern_of(v):
    """the bit pattern of one fp32 value, as an int"""
    return int(np.array([v], f32).view(np.uint32)[0])


BOX = np.array([[-1.0, 1.0]] * 3, f32)  # the LUT bounds of every context here
RES = 0.25                              # and its resolution
LO = pattern_of(2.0 ** -20)     # the patterns of a row: {0} and [LO, hi)
HI = pattern_of(1.0)
HI_DECOYS = pattern_of(0.1)     # against the 33-point target: d2 < 0.1, so that the origin stays the nearest target point

ONE_BLOCK_SIZES = (1, 2, 255, 256, 257, 32767)       # trim_select_kernel
WIDE_SIZES = (32768, 32769, 131072, 131073)          # select_wide_*: 131072 = 512 x 256 is the last size whose sum slices are whole blocks
TIES_FIRST_DIGIT_N = (1 << 21) + 1000                # the smallest cloud whose tied caller indices have a non-zero first radix digit
NO_CORRESPONDENCE = 0x7fffffff


def digits(u):
    """the three radix digits of a pattern as the selections take them: (bits >> 21, (bits >> 10) & 0x7FF, bits & 0x3FF)"""
    u = int(u)
    return u >> 21, (u >> 10) & 0x7FF, u & 0x3FF


def design(pattern, signs=None):
    """(n,) uint32 patterns -> (n, 3) float32 points whose squared distance to the origin, as the device computes it, has those bits.
    signs (n,) in 0..7: bit 0 negates x, bit 1 negates z (the four directions in the y = 0 plane), bit 2 puts x on the y axis instead
    (four more, in the x = 0 plane)."""
    u = np.ascontiguousarray(pattern, np.uint32)
    v = u.view(f32).astype(np.float64)
    x = np.sqrt(0.875 * v).astype(f32)
    A = (x * x).astype(f32)
    z = np.sqrt(v - A.astype(np.float64)).astype(f32)
    s = np.zeros(len(u), np.int64) if signs is None else np.asarray(signs, np.int64)
    assert s.shape == u.shape and s.min(initial=0) >= 0 and s.max(initial=0) <= 7
    x = np.where(s & 1, -x, x).astype(f32)
    z = np.where(s & 2, -z, z).astype(f32)
    zero = np.zeros(len(u), f32)
    on_y = (s & 4) != 0
    return np.ascontiguousarray(np.stack([np.where(on_y, zero, x), np.where(on_y, x, zero), z], 1), f32)


class Reference:
    """The sort of one row, taken once: order = lexsort((caller index, bits)); at(k) answers for every k."""

    def __init__(self, pattern):
        self.pattern = np.ascontiguousarray(pattern, np.uint32)
        self.order = np.lexsort((np.arange(len(self.pattern)), self.pattern))
        self.sorted = self.pattern[self.order]
        self._values = self.sorted.view(f32).astype(np.float64).tolist()
        self._at = {}

    def at(self, k):
        """-> (mask (n,) bool, bits of v_k, need = copies of v_k among the k smallest, sse_ref = float32(fsum of the inliers in fp64))"""
        assert 1 <= k <= len(self.pattern)
        if k not in self._at:
            self._at[k] = self._answer(k)
        return self._at[k]

    def _answer(self, k):
        mask = np.zeros(len(self.pattern), bool)
        mask[self.order[:k]] = True
        vk = int(self.sorted[k - 1])
        need = k - int(np.searchsorted(self.sorted, vk, side="left"))
        return mask, vk, need, f32(math.fsum(self._values[:k]))

    def total(self):
        return f32(math.fsum(self._values))

    def rank_range(self, u):
        """(number of elements below u, number of copies of u)"""
        a, b = np.searchsorted(self.sorted, [u, u + 1], side="left")
        return int(a), int(b - a)


def reference(pattern, k):
    return Reference(pattern).at(k)


def ulp_apart(a, b):
    return abs(pattern_of(a) - pattern_of(b))


# ---- caller orders and targets ------------------------------------------------------------------------------------------------------
ORDERS = ("generated", "reversed", "shuffled")


def caller_order(name, n):
    """the permutation p of a caller order: the row handed over is (pattern[p], signs[p])"""
    if name == "generated":
        return np.arange(n)
    if name == "reversed":
        return np.arange(n)[::-1].copy()
    assert name == "shuffled"
    return np.random.default_rng(4242).permutation(n)


def target_origin():
    return np.zeros((1, 3), f32)


def target_decoys():
    """the origin (caller index 0) and 32 decoys within 0.1 of the box corners: 33 points are two leaves of the tree.  A decoy is at least
    0.9 sqrt(3) - sqrt(0.1) > 1.2 from any designed point of a row below HI_DECOYS, the origin at most sqrt(0.1) < 0.32."""
    rng = np.random.default_rng(33)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    decoys = np.repeat(corners, 4, axis=0) * rng.uniform(0.9, 1.0, (32, 3))
    return np.concatenate([np.zeros((1, 3)), decoys]).astype(f32)


TARGETS = {"origin": (target_origin, HI), "decoys": (target_decoys, HI_DECOYS)}


# ---- the row families: each returns (pattern (n,) uint32, signs (n,) in 0..7, ks) or None where the size does not fit -------------------------
def _ks(n, ks):
    return sorted({int(k) for k in ks if 1 <= k <= n})


def _multiples_of_2_21(hi, count=3):
    """`count` multiples of 2^21 spread over (LO, hi), each with room for a dense run of 131 073 patterns about it"""
    a, b = (LO >> 21) + 2, ((hi - 1) >> 21) - 1
    return [int(a + (b - a) * (2 * i + 1) // (2 * count)) << 21 for i in range(count)]


def edge_patterns(hi=HI):
    """-> list of (name, pattern): around three multiples B of 2^21 the patterns B-2, B-1, B, B+1 (the second and third digits wrap from
    0x7FF / 0x3FF to 0x000, the first digit steps), and around three multiples M of 2^10 that are no multiples of 2^21 — second digit
    0x7FF, 0x001 and 0x400 — the patterns M-1, M, M+1 (the third digit wraps)"""
    out = []
    Bs = _multiples_of_2_21(hi)
    for j, B in enumerate(Bs):
        out += [(f"B{j}-2", B - 2), (f"B{j}-1", B - 1), (f"B{j}", B), (f"B{j}+1", B + 1)]
    for j, M in enumerate((Bs[0] - (1 << 10), Bs[1] + (1 << 10), Bs[2] + (0x400 << 10))):
        out += [(f"M{j}-1", M - 1), (f"M{j}", M), (f"M{j}+1", M + 1)]
    return out


def digit_edges(n, hi=HI, seed=7):
    """The edge patterns 1 to 3 times each (1, 2, 3, 1, ... in the order of edge_patterns) at the head of the row, a seeded random
    background behind them (so that a shorter row is a prefix of a longer one).  ks: the cut on every edge pattern — all its copies — and
    inside the copies of a repeated one (need = 1 .. count - 1)."""
    if n < 255:
        return None
    edges = edge_patterns(hi)
    head = np.concatenate([np.full(1 + j % 3, u, np.uint32) for j, (_, u) in enumerate(edges)])
    rng = np.random.default_rng(seed)
    back = rng.integers(LO, hi, 200000, dtype=np.uint32)[:n - len(head)]  # drawn whole, cut to size: prefixes agree
    assert len(back) == n - len(head)
    pattern = np.concatenate([head, back])
    signs = rng.integers(0, 4, 200000 + len(head))[:n]
    ref = Reference(pattern)
    ks = []
    for _, u in edges:
        below, count = ref.rank_range(u)
        ks += [below + c for c in range(1, count + 1)]
    return pattern, signs, _ks(n, ks)


def dense_run(n, hi=HI):
    """The consecutive patterns P .. P+n-1 across one multiple B of 2^21 (and about n / 1024 multiples of 2^10), shuffled.  ks: 1, 2,
    n / 2, the ranks of B-1 and B, n-1, n."""
    if n < 2:
        return None
    B = _multiples_of_2_21(hi)[1]
    P = B - n // 2
    assert P >= LO and P + n <= hi and P < B < P + n and (P + n - 1) >> 21 == B >> 21 and P >> 21 == (B >> 21) - 1
    rng = np.random.default_rng(8)
    pattern = (P + rng.permutation(n)).astype(np.uint32)
    return pattern, rng.integers(0, 4, n), _ks(n, [1, 2, n // 2, B - P, B - P + 1, n - 1, n])


ALL_EQUAL_PATTERN = 0x3D2B851F  # 0.0419..., below 0.1; its digits are (0x1E9, 0x2E1, 0x11F)


def all_equal(n, hi=HI):
    """n copies of one pattern in the four directions.  The mask must be the k lowest caller indices."""
    pattern = np.full(n, ALL_EQUAL_PATTERN, np.uint32)
    ks = [2 ** 21 - 1, 2 ** 21, 2 ** 21 + 1] if n > 2 ** 21 else [1, 1023, 1024, 1025, 2047, 2048, 2049, n - 1, n]
    return pattern, np.arange(n) % 4, _ks(n, ks)


def two_values(n, hi=HI):
    """P = B-1 and Q = B for a multiple B of 2^21, alternating by caller index (even: Q, odd: P, so that the copies of the smaller value
    do not start the row).  ks: inside the Ps, #P, #P + 1, inside the Qs."""
    if n < 2:
        return None
    B = _multiples_of_2_21(hi)[0]
    pattern = np.where(np.arange(n) % 2 == 0, B, B - 1).astype(np.uint32)
    nP = n // 2
    return pattern, (np.arange(n) // 2) % 4, _ks(n, [1, nP // 2, nP - 1, nP, nP + 1, nP + 2, nP + (n - nP + 1) // 2, n - 1, n])


def zeros(n, hi=HI):
    """z = ceil(n / 3) points on the target, the rest positive.  ks: 1, z-1, z, z+1, n."""
    z = (n + 2) // 3
    rng = np.random.default_rng(9)
    pattern = np.concatenate([np.zeros(z, np.uint32), rng.integers(LO, hi, n - z, dtype=np.uint32)])
    p = rng.permutation(n)
    return pattern[p], rng.integers(0, 4, n), _ks(n, [1, z - 1, z, z + 1, n])


def zeros_count(n):
    return (n + 2) // 3


TIED_PATTERN = 0x3D4CCCCD  # 0.05
TIE_COPIES, TIES_MAX_K = 8, 64


def directional_ties(n, hi=HI):
    """For the ICP path: min(20, n - 8) values below the cut, 8 points tied at the cut in eight different directions, the rest above it.
    ks: need = 1 .. 8 of the tied points.  A wrong pick among the tied points swaps two points that differ by at least 2 min|coordinate|
    in some coordinate, so the centroid of the k inliers moves by 2 min|coordinate| / k — asserted here to be more than 1e-3."""
    if n < 16:
        return None
    below = min(20, n - TIE_COPIES)
    rng = np.random.default_rng(10)
    lo_v, hi_v = pattern_of(0.01), pattern_of(0.04)
    ab_lo, ab_hi = pattern_of(0.06), min(hi, pattern_of(0.5))
    pattern = np.concatenate([rng.integers(lo_v, hi_v, below, dtype=np.uint32), np.full(TIE_COPIES, TIED_PATTERN, np.uint32),
                              rng.integers(ab_lo, ab_hi, n - below - TIE_COPIES, dtype=np.uint32)])
    signs = np.concatenate([rng.integers(0, 8, below), np.arange(TIE_COPIES), rng.integers(0, 8, n - below - TIE_COPIES)])
    p = rng.permutation(n)
    pattern, signs = pattern[p], signs[p]
    ks = _ks(n, [below + c for c in range(1, TIE_COPIES + 1)])
    assert ks and max(ks) <= TIES_MAX_K
    assert ties_separation(pattern, signs, max(ks)) > 1e-3
    return pattern, signs, ks


def ties_separation(pattern, signs, k):
    """2 min|non-zero coordinate of a tied point| / k, and that the tied points lie in pairwise different directions"""
    tied = design(pattern, signs)[pattern == TIED_PATTERN]
    assert len(tied) == TIE_COPIES and len({tuple(np.sign(p)) for p in tied}) == TIE_COPIES
    return 2.0 * float(np.abs(tied)[tied != 0].min()) / k


FAMILIES = {"digit_edges": digit_edges, "dense_run": dense_run, "all_equal": all_equal, "two_values": two_values, "zeros": zeros,
            "directional_ties": directional_ties}


MIN_N = {"digit_edges": 255, "dense_run": 2, "all_equal": 1, "two_values": 2, "zeros": 1, "directional_ties": 16}  # below: the family returns None


class Row:
    """One row in one caller order against one target: pattern and signs as handed over, points = design(...), ks, ref (Reference)."""

    def __init__(self, family, n, order="generated", target="origin", made=None):
        make_target, hi = TARGETS[target]
        made = FAMILIES[family](n, hi) if made is None else made
        assert made is not None, (family, n)
        pattern, signs, self.ks = made
        p = caller_order(order, n)
        self.name = f"{family}-{n}-{order}-{target}"
        self.family, self.n = family, n
        self.pattern, self.signs = np.ascontiguousarray(pattern[p], np.uint32), np.asarray(signs)[p]
        assert ((self.pattern == 0) | ((self.pattern >= LO) & (self.pattern < hi))).all()
        self.points = design(self.pattern, self.signs)
        self.target = make_target()
        self.ref = Reference(self.pattern)

    def check_design(self):
        """the restated scan returns the designed bits, and the origin as every point's neighbour"""
        idx, d2 = brute_force(self.target, self.points, I3, ZERO3)
        assert np.array_equal(bits(d2), self.pattern), self.name
        assert not idx.any(), self.name


def applies(family, n):
    return n >= MIN_N[family]
