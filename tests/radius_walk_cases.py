"""Designed clouds and radii for the fixed-radius walk (radius_walk of kernels.hip, in cluster_count_kernel, cluster_hook_kernel and
cluster_border_kernel behind fgoicp_cluster_dbscan), with a reference of the whole call in exact integers.  Test infrastructure, in the
style of tests/knn_normal_cases.py, whose clouds these are: the properties they are used for are asserted without a GPU by
tests/test_radius_walk_cases_host.py; tests/test_gpu_radius_walk_edges.py runs them.

The clouds.  Every coordinate is a multiple of 1/64 (a planar cloud's z is the constant 0.1f, absent from every difference), so with q the
coordinates in units of 1/64 the fp32 dist_sq of two points is |q_i - q_j|^2 / 4096 exactly, and "d2 <= eps2" is a comparison of
integers.  Two clouds are new here, both the lattice points of two planes with |x|, |y| <= 30, |z| <= 60, 3 s units apart along
(2, 2, 1)/3 — a normal without an fp32 representation:
  tilted_pair       2x + 2y + z = 0 and = 9   (s = 1, 5 531 points): the offset +-(2, 2, 1) joins the planes at d2 = 9/4096 exactly
  tilted_pair_wide  2x + 2y + z = 0 and = 27  (s = 3, 5 369 points): +-(6, 6, 3) at d2 = 81/4096 exactly
and no other offset of squared length <= 9 s^2 does (Cauchy-Schwarz: 2a + 2b + c = 9 s and a^2 + b^2 + c^2 <= 9 s^2 leave nothing else).
The first was meant to put each partner behind a leaf slab at distance exactly eps.  It does not: its planes are closer together than a
leaf of 32 points is wide, the k-d splits never part them, and EVERY leaf holds points of both planes — a partner's leaf has the query
inside its slab (tests/test_radius_walk_cases_host.py asserts this state of affairs).  The second is there for that purpose: two thirds
of its leaves lie in one plane, and over 1 000 of its rows have their partner in such a leaf, whose slab is at distance exactly
eps = 9/64 from them in exact arithmetic.

A third new cloud, striped (5 472 points), is there for the border key: four dense slabs two lattice layers thick (x = -5, -4 | -2, -1
| 1, 2 | 4, 5; y, z = -12 ... 11), and between two slabs one layer holding every other point (y + z even).  At eps = 1, min_points = 6 the
slabs are four clusters, and a point between two of them is a border point with ONE core neighbour in each, both at d2 == eps2: the lower
caller index decides which cluster it joins.  On every other lattice here the tied core neighbours belong to one cluster, and any rule
gives the same label.

The radii, in units of 1/64, as the integer r2 with  d2 <= eps2  <=>  |q_i - q_j|^2 <= r2:
  "1"   eps = 1/64           eps2 = 2^-12 exactly        r2 = 1: the 6 lattice edges tie with eps2
  "3"   eps = 3/64           eps2 = 9/4096 exactly       r2 = 9: 123 offsets, 30 of them — (+-3, 0, 0) and (+-2, +-2, +-1), permuted — at d2 == eps2
  "3-"  eps = nextafter(3/64, 0): eps2 < 9/4096          r2 = 8: the 30 drop out, 93 remain
  "9", "9-"  the same pair at 9/64 (r2 = 81 and 80; 3 071 offsets, 102 of them at 81), for tilted_pair_wide alone
  "1-"  eps = nextafter(1/64, 0): eps2 < 2^-12            r2 = 0, for the striped cloud alone
  "0"   eps = 1e-23f: eps2 = +0.0                        r2 = 0: a point's neighbours are the holders of its own position
(tests/test_radius_walk_cases_host.py asserts the squares.)

The reference (reference(), exact()).  The integer coordinates are encoded, sorted and grouped (the duplicates cloud holds one position
many times: a group is a position, its points share every distance); for each offset of the ball the shifted code is looked up with
searchsorted.  That gives neighbours and core; the core adjacency as a sparse matrix over the groups, its components from
scipy.sparse.csgraph.connected_components, numbered by the lowest caller index among their core members; a border point's label from
the smallest (bits(f32(r2 / 4096)) << 32) | index over its core neighbours — per neighbouring position the lowest caller index, which
is the smallest key there.  No n x n matrix: 140 608 points at r2 = 9 take a few seconds."""
import zlib

import numpy as np

from tests import knn_normal_cases as kc

f32, f64 = np.float32, np.float64
bits = kc.bits
LEAF, SUPER, TOP = kc.LEAF, kc.SUPER, kc.TOP

# ---- the clouds -------------------------------------------------------------------------------------------------------------------------
VOLUMES = ("box2048", "box2049", "box2048+31", "box2048+32", "box2048+33", "lattice4097", "lattice52")
TIE_LATTICES = VOLUMES + ("plane", "tilted_pair", "tilted_pair_wide")  # every row has a neighbour at exactly d2 == eps2 (the pairs: at 3 and 9 only)
OTHERS = ("duplicates", "plates", "tilted_lattice", "striped")  # plates: as the plane, per plate; tilted_lattice: in-plane d2 of 2, 6, 8 / 4096, no tie
CLOUDS = TIE_LATTICES + OTHERS
REVERSED_TOO = ("lattice4097", "box2048+33", "tilted_pair", "tilted_pair_wide", "striped")
SMALL = 5600  # clouds of at most this many points are also held against the n x n restatement of tests/test_gpu_cluster.py

_CACHE = {}


def _plane_pair(s):
    """the lattice points of the planes 2x + 2y + z = 0 and 2x + 2y + z = 9 s with |x|, |y| <= 30 and |z| <= 60: 3 s units apart"""
    x, y = np.meshgrid(np.arange(-30, 31), np.arange(-30, 31), indexing="ij")
    planes = []
    for c in (0, 9 * s):
        z = c - 2 * x - 2 * y
        keep = np.abs(z) <= 60
        planes.append(np.stack([x[keep], y[keep], z[keep]], 1))
    return np.concatenate(planes).astype(np.int64)


PLANE_PAIRS = {"tilted_pair": 1, "tilted_pair_wide": 3}
STRIPED_DENSE, STRIPED_SPARSE = (-5, -4, -2, -1, 1, 2, 4, 5), (-3, 0, 3)


def _striped():
    layer = kc._grid(1, 24, 24, (0, -12, -12))
    sparse = layer[(layer[:, 1] + layer[:, 2]) % 2 == 0]
    return np.concatenate([layer + [x, 0, 0] for x in STRIPED_DENSE] + [sparse + [x, 0, 0] for x in STRIPED_SPARSE]).astype(np.int64)


OWN = {"tilted_pair": lambda: _plane_pair(1), "tilted_pair_wide": lambda: _plane_pair(3), "striped": _striped}


def cloud(name, reverse=False):
    """knn_normal_cases.cloud, and the two plane pairs in the same way: a shuffled caller order seeded by the name; not to be written to"""
    if name not in OWN:
        return kc.cloud(name, reverse)
    key = ("cloud", name, bool(reverse))
    if key not in _CACHE:
        q = OWN[name]()
        p = kc._points(q)[np.random.default_rng(zlib.crc32(name.encode())).permutation(len(q))]
        p = np.ascontiguousarray(p[::-1] if reverse else p)
        p.setflags(write=False)
        _CACHE[key] = p
    return _CACHE[key]


def plane_of(name, reverse=False):
    """a plane pair's rows: 0 or 1, the plane"""
    q = integer_coordinates(cloud(name, reverse))[0]
    return (2 * q[:, 0] + 2 * q[:, 1] + q[:, 2] != 0).astype(np.int64)


def integer_coordinates(pts):
    """-> q (n, 3) int64 in units of 1/64 and kind (n,): 0 for a point on the 1/64 lattice, 1 for one at z = 0.1f (q_z = 0 there).  Two
    points of different kinds are never looked up against each other; reference() asserts that they lie farther apart than the radius."""
    p = np.asarray(pts, f64) * 64.0
    q = np.rint(p).astype(np.int64)
    on = q == p
    kind = (~on[:, 2]).astype(np.int64)
    assert on[:, :2].all() and (on[:, 2] | (np.asarray(pts)[:, 2] == kc.Z_PLANE)).all(), "a coordinate that is neither a multiple of 1/64 nor 0.1f"
    q[kind == 1, 2] = 0
    return q, kind


# ---- the radii ------------------------------------------------------------------------------------------------------------------------
EPS = {"1": f32(1.0 / 64.0), "3": f32(3.0 / 64.0), "3-": np.nextafter(f32(3.0 / 64.0), f32(0)), "9": f32(9.0 / 64.0), "9-": np.nextafter(f32(9.0 / 64.0), f32(0)),
       "1-": np.nextafter(f32(1.0 / 64.0), f32(0)), "0": f32(1e-23)}
R2 = {"1": 1, "3": 9, "3-": 8, "9": 81, "9-": 80, "1-": 0, "0": 0}
BELOW = {"3": "3-", "9": "9-", "1": "1-"}  # a radius with ties -> the one just below it


def radii(name):
    """the radii a cloud is run at"""
    return {"tilted_pair_wide": ("9", "9-"), "striped": ("1", "1-")}.get(name, ("1", "3", "3-"))


def min_points(name, radius):
    """the density asked of the device per cloud and radius: about half of a lattice's points are core, the rest border and noise.
    Volumes: 7 of the 7 in the ball, 100 of 123, 76 of 93.  Planar square lattices: 5 of 5, 25 of 29, 21 of 25.  tilted_pair: 12 of the
    13 in its plane and the one across (3-: 8 of 9); tilted_pair_wide: 80 of the 89 / 84 in its plane and the one across; tilted_lattice: 16 of
    19 at both larger radii.  The tilted clouds hold no pair within eps = 1: min_points = 1 there makes every point a cluster of its own.
    duplicates: 31, the smaller of its two stacks, at eps = 1 and below; 32 above."""
    if name in VOLUMES:
        return {"1": 7, "3": 100, "3-": 76}[radius]
    if name in ("plane", "plates"):
        return {"1": 5, "3": 25, "3-": 21}[radius]
    if name == "tilted_pair":
        return {"1": 1, "3": 12, "3-": 8}[radius]
    if name == "tilted_lattice":
        return {"1": 1, "3": 16, "3-": 16}[radius]
    if name == "tilted_pair_wide":
        return {"9": 80, "9-": 80}[radius]
    if name == "striped":  # 6: a slab's point, its 4 neighbours in the layer and the one in the slab's other layer
        return {"1": 6, "1-": 1}[radius]
    if name == "duplicates":
        return {"0": 31, "1": 31, "3": 32, "3-": 32}[radius]
    raise KeyError(name)


def eps2_of(eps):
    with np.errstate(over="ignore", under="ignore"):
        return f32(eps) * f32(eps)


def ball(r2):
    """the integer offsets o with |o|^2 <= r2 and their squared lengths, ascending in (|o|^2, o)"""
    r = int(np.floor(np.sqrt(r2)))
    g = np.arange(-r, r + 1)
    o = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    d = (o * o).sum(1)
    o, d = o[d <= r2], d[d <= r2]
    order = np.lexsort((o[:, 2], o[:, 1], o[:, 0], d))
    return o[order], d[order]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
PAD = 4  # the largest offset component, and one


class Positions:
    """the distinct positions of a cloud, sorted by their code: per group its size and its lowest caller index; per point its group"""

    def __init__(self, q, kind):
        q = np.asarray(q, np.int64)
        c = q - q.min(axis=0) + PAD
        self.side = int(c.max()) + PAD + 1
        assert (int(kind.max()) + 1) * self.side ** 3 < 2 ** 62
        code = ((kind * self.side + c[:, 0]) * self.side + c[:, 1]) * self.side + c[:, 2]
        self.code, self.group, self.size = np.unique(code, return_inverse=True, return_counts=True)
        self.group = self.group.reshape(-1)
        self.first = np.full(len(self.code), len(q), np.int64)
        np.minimum.at(self.first, self.group, np.arange(len(q)))
        self.n = len(q)

    def shifted(self, o):
        """-> (u, v): the groups u whose position + o is held, and the group v that holds it"""
        want = self.code + (int(o[0]) * self.side + int(o[1])) * self.side + int(o[2])
        at = np.minimum(np.searchsorted(self.code, want), len(self.code) - 1)
        u = np.flatnonzero(self.code[at] == want)
        return u, at[u]


def positions(name, reverse=False):
    key = ("positions", name, bool(reverse))
    if key not in _CACHE:
        _CACHE[key] = Positions(*integer_coordinates(cloud(name, reverse)))
    return _CACHE[key]


def exact(pos, r2, min_points, eps2):
    """the call's outputs from the positions, as restate() of tests/test_gpu_cluster.py returns them: dict(eps2, neighbours, core, label,
    sizes)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    offsets, d = ball(r2)
    g = len(pos.code)
    hits = [pos.shifted(o) for o in offsets]
    count = np.zeros(g, np.int64)
    for u, v in hits:
        count[u] += pos.size[v]
    core_g = count >= min_points
    # components of the core positions
    rows = np.concatenate([u[core_g[u] & core_g[v]] for u, v in hits]) if g else np.zeros(0, np.int64)
    cols = np.concatenate([v[core_g[u] & core_g[v]] for u, v in hits]) if g else np.zeros(0, np.int64)
    _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(g, g)).tocsr(), directed=False)
    comp = np.where(core_g, comp, -1)
    lowest = np.full(comp.max() + 2, pos.n, np.int64)  # per component the lowest caller index of a core member (the last entry: the non-core positions')
    np.minimum.at(lowest, comp, pos.first)
    number = np.full(len(lowest), -1, np.int64)
    live = np.flatnonzero(lowest[:-1] < pos.n)
    number[live[np.argsort(lowest[live])]] = np.arange(len(live))
    label_g = number[comp]  # comp == -1 reads the last entry: -1
    # border positions: the smallest key over the core neighbours
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(g, none, np.uint64)
    for (u, v), dd in zip(hits, d):
        take = ~core_g[u] & core_g[v]
        key = (np.uint64(int(bits(f32(f64(dd) / 4096.0))[0])) << np.uint64(32)) | pos.first[v[take]].astype(np.uint64)
        best[u[take]] = np.minimum(best[u[take]], key)
    border = ~core_g & (best != none)
    group_of_point = pos.group
    label_g[border] = label_g[group_of_point[(best[border] & np.uint64(0xFFFFFFFF)).astype(np.int64)]]
    label = label_g[group_of_point].astype(np.int32)
    return dict(eps2=f32(eps2), neighbours=count[group_of_point].astype(np.uint32), core=core_g[group_of_point], label=label,
                sizes=np.bincount(label[label >= 0], minlength=len(live)).astype(np.uint64))


def reference(name, radius, min_pts=None, reverse=False):
    """exact() of a cloud at one of the three radii (min_pts: min_points(name, radius) unless given); cached per process"""
    m = min_points(name, radius) if min_pts is None else int(min_pts)
    key = ("reference", name, radius, m, bool(reverse))
    if key not in _CACHE:
        pos = positions(name, reverse)
        kind = integer_coordinates(cloud(name, reverse))[1]
        if kind.min() != kind.max():  # the plates: those on the lattice and those at 0.1f are never compared — they must be out of reach
            p = cloud(name, reverse).astype(f64)
            a, b = p[kind == 0], p[kind == 1]
            assert ((a[:, None, :] - b[None, :, :]) ** 2).sum(2).min() > 4.0 * R2[radius] / 4096.0
        _CACHE[key] = exact(pos, R2[radius], m, eps2_of(EPS[radius]))
    return _CACHE[key]


def everything(n, min_pts, eps2):
    """the outputs when every point is every point's neighbour (eps2 = +inf)"""
    core = np.full(n, n >= min_pts)
    label = np.where(core, 0, -1).astype(np.int32)
    return dict(eps2=f32(eps2), neighbours=np.full(n, n, np.uint32), core=core, label=label, sizes=np.array([n] if core.any() else [], np.uint64))


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------
def slots(name, reverse=False):
    key = ("slots", name, bool(reverse))
    if key not in _CACHE:
        _CACHE[key] = kc.slot_of(cloud(name, reverse))
    return _CACHE[key]


def tied_neighbours(name, radius, reverse=False):
    """per point the number of its neighbours at exactly |o|^2 == r2: what the radius just below must lose, and nothing else"""
    pos = positions(name, reverse)
    offsets, d = ball(R2[radius])
    count = np.zeros(len(pos.code), np.int64)
    for o in offsets[d == R2[radius]]:
        u, v = pos.shifted(o)
        count[u] += pos.size[v]
    return count[pos.group]


def rows_with_a_tie_elsewhere(name, radius, reverse=False):
    """rows (positions are single points on these clouds) with a neighbour at exactly |o|^2 == r2 -> dict(any=, super=, top=, leaf=):
    boolean per row — one exists at all, one lies in another super-leaf, in another top box, in another leaf"""
    pos, slot = positions(name, reverse), slots(name, reverse)
    assert (pos.size == 1).all()
    row = pos.first
    offsets, d = ball(R2[radius])
    out = {k: np.zeros(pos.n, bool) for k in ("any", "leaf", "super", "top")}
    for o in offsets[d == R2[radius]]:
        u, v = pos.shifted(o)
        i, j = row[u], row[v]
        out["any"][i] = True
        for k, width in (("leaf", LEAF), ("super", SUPER), ("top", TOP)):
            out[k][i[slot[i] // width != slot[j] // width]] = True
    return out


def border_ties(name, radius, reverse=False):
    """-> (tied, split, contested): the border rows with two or more core neighbours at the smallest d2 (the index decides), those of
    them whose tied core neighbours lie in different super-leaves, and those whose tied core neighbours belong to different clusters"""
    pos, slot, ref = positions(name, reverse), slots(name, reverse), reference(name, radius, reverse=reverse)
    assert (pos.size == 1).all()
    row, core = pos.first, ref["core"]
    offsets, d = ball(R2[radius])
    big = np.iinfo(np.int64).max
    nearest = np.full(pos.n, big, np.int64)   # the smallest |o|^2 of a core neighbour
    hits = []
    for o, dd in zip(offsets, d):
        u, v = pos.shifted(o)
        i, j = row[u], row[v]
        keep = ~core[i] & core[j]
        hits.append((i[keep], j[keep], dd))
        np.minimum.at(nearest, i[keep], dd)
    many = np.zeros(pos.n, np.int64)
    lo, hi = np.full(pos.n, big, np.int64), np.full(pos.n, -1, np.int64)  # super-leaves of the tied partners
    first, last = np.full(pos.n, big, np.int64), np.full(pos.n, -1, np.int64)  # and their labels
    for i, j, dd in hits:
        at = nearest[i] == dd
        np.add.at(many, i[at], 1)
        np.minimum.at(lo, i[at], slot[j[at]] // SUPER)
        np.maximum.at(hi, i[at], slot[j[at]] // SUPER)
        np.minimum.at(first, i[at], ref["label"][j[at]])
        np.maximum.at(last, i[at], ref["label"][j[at]])
    tied = many >= 2
    return np.flatnonzero(tied), np.flatnonzero(tied & (lo != hi)), np.flatnonzero(tied & (first != last))
