"""Designed clouds for the k-nearest walk (knn_walk, shared by target_knn_kernel and outlier_knn_kernel) and for the normal epilogue of
target_knn_kernel, with their plain references: a brute force over the keys (bits(fp32 dist_sq) << 32) | index, and the eigenvectors of the
covariance of the k fp32 points in exact arithmetic.  Test infrastructure, in the style of tests/selection_rows.py: the properties the
clouds are designed for are asserted without a GPU by tests/test_knn_normal_cases_host.py; tests/test_gpu_knn_normal_edges.py runs them.

The clouds.  Designed coordinates are multiples of 1/64 inside [-1, 1] (the planar ones sit at z = 0.1f, a constant that drops out of every
difference; the line steps by (1, 2, 3)/4096): a difference of two coordinates is n/64 with |n| <= 128, its square n^2/4096 and the sum of
three at most 49152/4096 — every dist_sq is exact in fp32, and equal distances are equal bits.  Every cloud is handed over in a shuffled
caller order (seeded by its name), so that "a tie at the cut goes to the lowest caller index" cuts across the spatial order of the tree.

The rule for a normal n against the exact eigenpairs l0 <= l1 <= l2, v0, v2 of its neighbourhood's scatter matrix (check_normals, applied
to every row):
  l2 == 0                      the zero vector, every float +0.0
  l1 - l0 > 2^-40 l2           | |n| - 1 | <= 2e-7 and the angle to +-v0 <= 2^-23 + C_ANGLE 2^-52 l2 / (l1 - l0)
  else, l2 - l1 > 2^-40 l2     unit length as above and |n . v2| <= 2^-23 + C_ANGLE 2^-52 l2 / (l2 - l1): n lies in the plane of least variance
  else (the cube)              unit length and finite
2^-23 is the fp32 store (three components, each rounded at 2^-24 relative).  C_ANGLE is 16 x what numpy.linalg.eigh in fp64 needs on these
very rows against the exact eigenvectors (measured by tests/golden/make_knn_normal_cases.py, recorded in the fixture, 1.91 at most),
rounded up to a power of two: the factor 16 is for the difference between two backward-stable solvers — the cyclic two-sided Jacobi of
math3.hpp and LAPACK's — plus the k <= 32 fp64 additions of the covariance.  It is never measured on the kernel's output."""
import os
import zlib

import numpy as np

from oracle import np_restatement as npr

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "knn_normal_cases.npz")

BOX = np.array([[-1.0, 1.0]] * 3, f32)  # the LUT bounds of every context here
RES = 0.05                              # and its resolution
Z_PLANE = f32(0.1)                      # the planar clouds' height: no multiple of 1/64, and absent from every difference
C_ANGLE = 32.0                          # see above; tests/test_knn_normal_cases_host.py holds it against the recorded measurement
EPS_STORE = 2.0 ** -23
GAP = 2.0 ** -40
LEAF, SUPER, TOP = 32, 2048, 131072     # points per leaf, per super-leaf (64 leaves), per top box (64 super-leaves): csrc/device/bvh.hpp


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the clouds -----------------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, nz, origin=(0, 0, 0)):
    """the integer lattice [0, nx) x [0, ny) x [0, nz) + origin, x fastest"""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int64) + np.asarray(origin, np.int64)


def _points(ints, z_plane=False):
    """integer coordinates in units of 1/64 -> float32 points"""
    ints = np.asarray(ints, np.int64)
    assert np.abs(ints).max() <= 64
    p = (ints.astype(f64) / 64.0).astype(f32)
    if z_plane:
        p[:, 2] = Z_PLANE
    return p


def _box_2048():
    return _grid(16, 16, 8, (-8, -8, -4))


def _box_2048_plus(r):
    """lattice(16, 16, 8) and the first r points of the next x layer"""
    return np.concatenate([_box_2048(), _grid(1, 16, 8, (8, -8, -4))[:r]])


def _lattice_4097():
    """lattice(13, 13, 13) and the first 1900 points of a 12-layer block behind it in x"""
    return np.concatenate([_grid(13, 13, 13, (-13, -6, -6)), _grid(12, 13, 13, (0, -6, -6))[:4097 - 2197]])


LINE_HALF = 1365  # m = -1365 .. 1365: 3 m / 4096 stays inside [-1, 1]; 2731 points (3000 would leave the box)


def _line():
    m = np.arange(-LINE_HALF, LINE_HALF + 1, dtype=np.int64)
    p = (np.stack([m, 2 * m, 3 * m], 1).astype(f64) / 4096.0).astype(f32)
    assert np.abs(p).max() <= 1.0
    return p


LINE_DIR = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
TETRA = np.array([[32, 32, 32], [32, -32, -32], [-32, 32, -32], [-32, -32, 32]], np.int64)
DUP_A, DUP_B, DUP_A_COPIES, DUP_B_COPIES = (0, 0, 0), (32, 0, 0), 40, 31


def _duplicates():
    """(0, 0, 0) held by 40 points, (0.5, 0, 0) by 31, and a 6 x 6 x 6 lattice of pitch 1/8 about them (which holds neither position)"""
    around = _grid(6, 6, 6) * 8 + np.array([-20, -20, -20])
    return _points(np.concatenate([np.tile([DUP_A], (DUP_A_COPIES, 1)), np.tile([DUP_B], (DUP_B_COPIES, 1)), around]))


PLATE = 23
PLATE_AXES = np.eye(3, dtype=f32)


def _plates_generated():
    """three exact 23 x 23 lattice patches in the planes x = -0.5, y = 0.25, z = 0.1f, 42/64 apart or more; -> points, plate of each point"""
    g = _grid(PLATE, PLATE, 1)
    a, b = g[:, 0], g[:, 1]
    px = _points(np.stack([np.full_like(a, -32), a - 11, b - 11], 1))
    py = _points(np.stack([a + 10, np.full_like(a, 16), b - 11], 1))
    pz = _points(np.stack([a + 10, b - 50, np.zeros_like(a)], 1), z_plane=True)
    return np.concatenate([px, py, pz]), np.repeat(np.arange(3), PLATE * PLATE)


CUBE_CENTRE, CUBE_HALF = (-40, -40, -40), 4


def _cube():
    """the 8 corners of a cube of side 1/8 and, 56/64 away or more, a 5 x 5 x 5 lattice of pitch 1/16 as filler"""
    corners = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.int64) * CUBE_HALF + np.array(CUBE_CENTRE)
    return _points(np.concatenate([corners, _grid(5, 5, 5) * 4 + 20]))


def _noisy_sphere():
    rng = np.random.default_rng(101)
    v = rng.normal(size=(600, 3))
    return (0.7 * v / np.linalg.norm(v, axis=1)[:, None] + 0.01 * rng.normal(size=(600, 3))).astype(f32)


def _uniform_volume():
    return np.random.default_rng(102).uniform(-1.0, 1.0, (600, 3)).astype(f32)


def _tilted_lattice():
    """the lattice points of the plane x + y + z = 0 with |x|, |y|, |z| <= 20: 1261 points"""
    i, j = np.meshgrid(np.arange(-20, 21), np.arange(-20, 21), indexing="ij")
    keep = np.abs(i + j) <= 20
    return _points(np.stack([i[keep], j[keep], -(i + j)[keep]], 1))


def _jittered_plane():
    rng = np.random.default_rng(103)
    return np.concatenate([rng.uniform(-0.9, 0.9, (600, 2)), 0.3 + 2.0 ** -20 * rng.uniform(-1.0, 1.0, (600, 1))], axis=1).astype(f32)


def _small_patch():
    return (0.9 + 2.0 ** -12 * np.random.default_rng(104).uniform(-1.0, 1.0, (600, 3))).astype(f32)


CLOUDS = {
    "box2048": lambda: _points(_box_2048()),             # exactly one super-leaf
    "box2049": lambda: _points(_box_2048_plus(1)),       # one point in a second super-leaf
    "lattice4097": lambda: _points(_lattice_4097()),     # one point in a third super-leaf
    "lattice52": lambda: _points(_grid(52, 52, 52, (-26, -26, -26))),  # 140 608: two top boxes, the second with 5 super-leaves
    "plane": lambda: _points(_grid(64, 40, 1, (-32, -20, 0)), z_plane=True),  # thin slabs, boxes of zero height
    "line": _line,
    "box2048+31": lambda: _points(_box_2048_plus(31)),   # the last wave's own leaves hold k - 1, k, k + 1 points at k = 32
    "box2048+32": lambda: _points(_box_2048_plus(32)),
    "box2048+33": lambda: _points(_box_2048_plus(33)),
    "tetra4": lambda: _points(TETRA),
    "tetra5": lambda: _points(np.concatenate([TETRA, [[0, 0, 0]]])),
    "duplicates": _duplicates,
    "plates": lambda: _plates_generated()[0],
    "cube": _cube,
    "noisy_sphere": _noisy_sphere,
    "uniform_volume": _uniform_volume,
    "tilted_lattice": _tilted_lattice,
    "jittered_plane": _jittered_plane,
    "small_patch": _small_patch,
}
EXACT_EVERYWHERE = ("box2048", "box2049", "lattice4097", "lattice52", "plane", "box2048+31", "box2048+32", "box2048+33", "tetra4", "tetra5",
                    "duplicates", "cube", "tilted_lattice")  # every pair's dist_sq is exact; "line" and "plates": the pairs at and below the cut
RANDOM_FAMILIES = ("noisy_sphere", "uniform_volume", "tilted_lattice", "jittered_plane", "small_patch")

# the neighbour sets asked of the device: cloud -> the ks.  The duplicates cloud also at 4 and 10: the tree deals its 40 copies 10 to a
# wave, so there a copy's seed is full at distance 0 and its walk's bound is 0 while copies of lower index lie in other leaves at box
# distance 0 — a shrunk POSITIVE box distance never equals a key's distance, so this is where strict and non-strict pruning part
KNN_CASES = {"box2048": (4, 10, 32), "box2049": (4, 10, 32), "lattice4097": (4, 10, 32), "lattice52": (10, 20), "plane": (6, 32), "line": (4, 32),
             "box2048+31": (32,), "box2048+32": (32,), "box2048+33": (32,), "tetra4": (4,), "tetra5": (4, 5), "duplicates": (4, 10, 32)}
# the ks at which at least half of a lattice's rows have a tie at the cut
TIE_KS = {"box2048": (10, 20), "box2049": (10, 20), "lattice4097": (10, 20), "lattice52": (10, 20), "plane": (6,), "line": (4,)}
# the normals asked of the device: (cloud, k)
NORMAL_CASES = [(name, k) for name in RANDOM_FAMILIES for k in (8, 16)] + [("plates", 9), ("plane", 6), ("line", 4), ("cube", 8), ("duplicates", 32)]

_CACHE = {}


def _permutation(name):
    return np.random.default_rng(zlib.crc32(name.encode())).permutation(len(_generated(name)))


def _generated(name):
    if ("generated", name) not in _CACHE:
        _CACHE[("generated", name)] = np.ascontiguousarray(CLOUDS[name](), f32)
    return _CACHE[("generated", name)]


def cloud(name, reverse=False):
    """the cloud in its shuffled caller order (reverse: that order backwards); one array per process, not to be written to"""
    key = ("cloud", name, bool(reverse))
    if key not in _CACHE:
        p = _generated(name)[_permutation(name)]
        p = np.ascontiguousarray(p[::-1] if reverse else p)
        p.setflags(write=False)
        _CACHE[key] = p
    return _CACHE[key]


def plate_of_row():
    """the plate (0, 1, 2: its axis) of every caller row of cloud("plates")"""
    return _plates_generated()[1][_permutation("plates")]


def rows_at(name, ints, z_plane=False):
    """caller rows of the points of a cloud at the given integer coordinates (units of 1/64), in the order met; every holder of a position"""
    p = cloud(name)
    want = _points(np.atleast_2d(ints), z_plane)
    return np.concatenate([np.flatnonzero((p == w).all(axis=1)) for w in want])


def source_of(pts):
    """the small source of a context: the first 64 points of the same cloud (a cloud of fewer, repeated)"""
    return np.ascontiguousarray(np.resize(pts, (64, 3)))


SAMPLE = 1024


def sample_rows(name, reverse=False):
    """the rows a cloud is checked on: all of them (None), but 1024 of lattice52 — the 8 corners, a row in the middle of each of the 6
    faces and 12 edges, 256 random rows of the second top box (the 9536 points behind slot 131 072 of the tree), random rows for the rest"""
    if name != "lattice52":
        return None
    key = ("sample", name)
    if key not in _CACHE:
        lo, mid, hi = -26, 0, 25
        special = [(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)]
        for a in range(3):
            for s in (lo, hi):
                face = [mid] * 3
                face[a] = s
                special.append(tuple(face))
            for s in (lo, hi):
                for u in (lo, hi):
                    edge = [s, s, s]
                    edge[a] = mid
                    edge[(a + 1) % 3], edge[(a + 2) % 3] = s, u
                    special.append(tuple(edge))
        rows = list(rows_at(name, np.array(special)))
        assert len(rows) == 26 and len(set(rows)) == 26
        rng = np.random.default_rng(52)
        second = np.flatnonzero(slot_of(cloud(name)) >= TOP)
        rows += list(rng.choice(second, 256, replace=False))
        rest = np.setdiff1d(np.arange(len(cloud(name))), rows)
        rows += list(rng.choice(rest, SAMPLE - len(rows), replace=False))
        _CACHE[key] = np.array(rows, np.int64)
    r = _CACHE[key]
    return len(cloud(name)) - 1 - r if reverse else r


def slot_of(pts):
    """the slot of every caller row in the tree that bvh_build_host builds over pts: the inverse of kd_order(pts, leaf = 32) of
    csrc/device/morton.hpp, through tests/host_harness (the product's own text).  Leaf = slot // 32, super-leaf = slot // 2048, top box =
    slot // 131072; a wave of the walk is 64 consecutive slots."""
    from tests import host_harness as hh
    order = hh.point_order(pts, leaf=LEAF, mode=2, fine=False)
    slot = np.empty(len(pts), np.int64)
    slot[order] = np.arange(len(pts))
    return slot


# ---- the neighbour sets -----------------------------------------------------------------------------------------------------------------
KMAX = 33  # one more than the largest k: the key behind the cut


def _candidates(pts, rows):
    """per row the candidate columns and their fp32 dist_sq: every column whose distance is at most the row's 33rd smallest (all of a tie
    at that distance included), so the 33 smallest keys under ANY order of the indices are among them"""
    n, kk = len(pts), min(KMAX, len(pts))
    out = []
    # oracle.np_restatement.dist_sq on (c, 1, 3) against (1, n, 3), both laid out component by component and c n kept near 2^18 elements:
    # the same values as from the plain arrays, several times sooner on 140 608 points
    cols_of = np.moveaxis(np.ascontiguousarray(pts.T)[:, None, :], 0, -1)
    chunk = max(1, (1 << 18) // n)
    for a in range(0, len(rows), chunk):
        mine = np.moveaxis(np.ascontiguousarray(pts[rows[a:a + chunk]].T)[:, :, None], 0, -1)
        d2 = npr.dist_sq(mine, cols_of).astype(f32)
        cut = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        for i in range(len(d2)):
            cols = np.flatnonzero(d2[i] <= cut[i])
            out.append((cols, d2[i, cols]))
    return out


def brute_knn(pts, k, rows=None):
    """the k smallest keys (bits(fp32 dist_sq) << 32) | index of every row (of `rows`), ascending: (len(rows), k) uint64.  Squared distances
    are >= +0.0, so their bits order as they do.  The 33 smallest are computed once per (cloud, rows) and cut to k; a cloud in the reversed
    caller order takes the distances of the forward one where this process has them (row i, column j there are n-1-i, n-1-j here) and
    sorts its own keys."""
    assert 1 <= k <= min(KMAX, len(pts))
    n = len(pts)
    rows_ = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    ident = lambda p, r: (zlib.crc32(p.tobytes()), p.shape, zlib.crc32(np.ascontiguousarray(r).tobytes()))
    key = ("knn",) + ident(pts, rows_)
    if key not in _CACHE:
        # the forward cloud's candidates, if this is its reversal: asked for the same rows there (all rows: in the opposite sequence)
        there = np.arange(n) if rows is None else n - 1 - rows_
        mirror = ("candidates",) + ident(np.ascontiguousarray(pts[::-1]), there)
        if mirror in _CACHE:
            cand = [(n - 1 - cols, d2) for cols, d2 in (_CACHE[mirror][::-1] if rows is None else _CACHE[mirror])]
        else:
            cand = _CACHE[("candidates",) + ident(pts, rows_)] = _candidates(pts, rows_)
        kk = min(KMAX, n)
        out = np.empty((len(rows_), kk), np.uint64)
        for i, (cols, d2) in enumerate(cand):
            out[i] = np.sort((bits(d2).astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64))[:kk]
        _CACHE[key] = out
    return _CACHE[key][:, :k]


def key_index(keys):
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def key_d2_bits(keys):
    return (keys >> np.uint64(32)).astype(np.uint32)


def key_d2(keys):
    return key_d2_bits(keys).view(f32)


# ---- the exact eigenpairs -----------------------------------------------------------------------------------------------------------------
_SCALE_BITS = 72


def _integer_scatter(pts, idx):
    """per row the six entries (xx, xy, xz, yy, yz, zz) of k 2^144 x the scatter matrix sum (p - mean)(p - mean)^T of its k points, as
    Python integers: k sum(p p^T) - sum(p) sum(p)^T over the coordinates scaled to integers — exact arithmetic"""
    scaled = np.ldexp(pts.astype(f64), _SCALE_BITS)
    assert (scaled == np.rint(scaled)).all(), "a coordinate with bits below 2^-72"
    ints = [[int(v) for v in row] for row in scaled]
    out = []
    for row in np.asarray(idx):
        p = [ints[j] for j in row]
        k = len(p)
        s = [sum(q[a] for q in p) for a in range(3)]
        out.append(tuple(k * sum(q[a] * q[b] for q in p) - s[a] * s[b] for a in range(3) for b in range(a, 3)))
    return out


def exact_normals(pts, idx, numpy_c=False):
    """idx (m, k): per row the eigenvalues l0 <= l1 <= l2 of the scatter matrix of pts[idx[row]] and the unit eigenvectors v0, v2, from the
    exact integer scatter matrix through mpmath's symmetric eigensolver at 60 digits, rounded to fp64 at the end.  Rows with the same
    scatter matrix (a lattice has a handful) are solved once: -> dict(row (m,) index into the unique ones, l (u, 3), v0 (u, 3), v2 (u, 3)).
    l2 == 0 exactly where the k points are one position.  numpy_c: also "numpy_c", the largest c that numpy.linalg.eigh in fp64 (formed as
    eigh_normals of tests/test_gpu_plane.py) needs on these rows in the rule of check_normals without its 2^-23 — measured at 60 digits."""
    import mpmath as mp
    idx = np.asarray(idx)
    k = idx.shape[1]
    scatter = _integer_scatter(pts, idx)
    unique, row = {}, np.empty(len(idx), np.int64)
    for i, s in enumerate(scatter):
        row[i] = unique.setdefault(s, len(unique))
    l, v0, v2, solved = np.zeros((len(unique), 3)), np.zeros((len(unique), 3)), np.zeros((len(unique), 3)), []
    with mp.workdps(60):
        unit = mp.mpf(k * k) * mp.mpf(2) ** (2 * _SCALE_BITS)
        for s, u in unique.items():
            if not any(s):
                solved.append(None)
                continue
            xx, xy, xz, yy, yz, zz = (mp.mpf(v) / unit * k for v in s)  # the scatter matrix itself (k x the covariance)
            E, Q = mp.eigsy(mp.matrix([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
            order = sorted(range(3), key=lambda a: E[a])
            l[u] = [float(E[a]) for a in order]
            v0[u] = [float(Q[r, order[0]]) for r in range(3)]
            v2[u] = [float(Q[r, order[2]]) for r in range(3)]
            solved.append(([E[a] for a in order], [Q[r, order[0]] for r in range(3)], [Q[r, order[2]] for r in range(3)]))
        out = dict(row=row, l=l, v0=v0, v2=v2)
        if numpy_c:
            out["numpy_c"] = _numpy_c(pts, idx, row, solved, mp)
    return out


def eigh_normals(pts, idx):
    """tests/test_gpu_plane.py eigh_normals: fp64 numpy, the eigenvector of the smallest eigenvalue"""
    p = pts[idx].astype(f64)
    d = p - p.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    return v[:, :, 0], w


def _numpy_c(pts, idx, row, solved, mp):
    got, _ = eigh_normals(pts, idx)
    worst = 0.0
    for i, u in enumerate(row):
        if solved[u] is None:
            continue
        (e0, e1, e2), w0, w2 = solved[u]
        n = [mp.mpf(float(v)) for v in got[i]]
        if e1 - e0 > mp.mpf(GAP) * e2:
            cr = [n[1] * w0[2] - n[2] * w0[1], n[2] * w0[0] - n[0] * w0[2], n[0] * w0[1] - n[1] * w0[0]]
            angle = mp.atan2(mp.sqrt(sum(c * c for c in cr)), abs(sum(a * b for a, b in zip(n, w0))))
            worst = max(worst, float(angle * (e1 - e0) / e2 * mp.mpf(2) ** 52))
        elif e2 - e1 > mp.mpf(GAP) * e2:
            worst = max(worst, float(abs(sum(a * b for a, b in zip(n, w2))) * (e2 - e1) / e2 * mp.mpf(2) ** 52))
    return worst


def classes(l):
    """the rule's four classes of rows from their eigenvalues (n, 3): zero, gap (v0 is determined), flat (only v2 is), round (nothing is)"""
    l0, l1, l2 = l[:, 0], l[:, 1], l[:, 2]
    zero = l2 == 0
    gap = ~zero & (l1 - l0 > GAP * l2)
    flat = ~zero & ~gap & (l2 - l1 > GAP * l2)
    return zero, gap, flat, ~zero & ~gap & ~flat


def check_normals(n, exact, c=C_ANGLE, where=""):
    """the rule at the head of this file on every row of n (m, 3) float32 against exact = dict(row, l, v0, v2) of exact_normals or the
    fixture; -> dict of the largest angle (gap rows), the largest |n . v2| (flat rows), each also as a fraction of its bound, and the
    number of rows per class"""
    n32 = np.ascontiguousarray(n, f32)
    assert n32.shape == (len(exact["row"]), 3), (where, n32.shape)
    l, v0, v2 = exact["l"][exact["row"]], exact["v0"][exact["row"]], exact["v2"][exact["row"]]
    zero, gap, flat, round_ = classes(l)
    assert np.isfinite(n32).all(), where
    assert not bits(n32[zero]).any(), (where, "a neighbourhood without extent must get +0.0 three times", np.flatnonzero(zero & bits(n32).any(axis=1))[:8])
    n64 = n32.astype(f64)
    length = np.sqrt((n64 * n64).sum(axis=1))
    off = np.abs(length - 1.0)
    assert (off[~zero] <= 2e-7).all(), (where, "not a unit vector", np.flatnonzero(~zero & (off > 2e-7))[:8], n32[~zero & (off > 2e-7)][:4])
    report = dict(rows=len(n32), zero=int(zero.sum()), gap=int(gap.sum()), flat=int(flat.sum()), round=int(round_.sum()), angle=0.0, angle_of_bound=0.0,
                  out_of_plane=0.0, out_of_plane_of_bound=0.0)
    if gap.any():
        a, w = n64[gap], v0[gap]
        angle = np.arctan2(np.linalg.norm(np.cross(a, w), axis=1), np.abs((a * w).sum(axis=1)))
        bound = EPS_STORE + c * 2.0 ** -52 * l[gap, 2] / (l[gap, 1] - l[gap, 0])
        report["angle"], report["angle_of_bound"] = float(angle.max()), float((angle / bound).max())
        bad = np.flatnonzero(gap)[angle > bound]
        assert len(bad) == 0, (where, "angle to the exact eigenvector", bad[:8], angle[angle > bound][:8], bound[angle > bound][:8])
    if flat.any():
        dot = np.abs((n64[flat] * v2[flat]).sum(axis=1))
        bound = EPS_STORE + c * 2.0 ** -52 * l[flat, 2] / (l[flat, 2] - l[flat, 1])
        report["out_of_plane"], report["out_of_plane_of_bound"] = float(dot.max()), float((dot / bound).max())
        bad = np.flatnonzero(flat)[dot > bound]
        assert len(bad) == 0, (where, "component along the direction of largest variance", bad[:8], dot[dot > bound][:8])
    return report


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def tag(name, k):
    return f"{name}_k{k}"


def normal_case(name, k):
    """-> (points, neighbour indices (nt, k) of the brute force) of one entry of NORMAL_CASES"""
    pts = cloud(name)
    return pts, key_index(brute_knn(pts, k))


def pack(ex):
    """exact_normals' dict as the fixture stores it: v2 only for the unique rows outside the gap class, where the rule reads it"""
    need = np.flatnonzero(~classes(ex["l"])[1])
    return dict(row=ex["row"].astype(np.uint16), l=ex["l"], v0=ex["v0"], v2_rows=need.astype(np.uint16), v2=ex["v2"][need])


def load_exact(name, k, fixture=None):
    """the fixture's entry of (cloud, k) as exact_normals returns it (v2 = NaN where it is not stored)"""
    if fixture is None:
        if "fixture" not in _CACHE:
            with np.load(FIXTURE) as z:
                _CACHE["fixture"] = {key: z[key] for key in z.files}
        fixture = _CACHE["fixture"]
    t = tag(name, k)
    l = fixture[t + "_l"]
    v2 = np.full(l.shape, np.nan)
    v2[fixture[t + "_v2_rows"].astype(np.int64)] = fixture[t + "_v2"]
    return dict(row=fixture[t + "_row"].astype(np.int64), l=l, v0=fixture[t + "_v0"], v2=v2)


def recorded_numpy_c():
    load_exact(*NORMAL_CASES[0])
    return {t: float(_CACHE["fixture"][tag(*t) + "_numpy_c"]) for t in NORMAL_CASES}


# ---- the epilogue of target_knn_kernel, restated --------------------------------------------------------------------------------------------
def epilogue_normals(pts, idx):
    """kernels.hip target_knn_kernel after the walk: centroid, then the scatter matrix about it, of the k points in list order in fp64;
    svd3_jacobi of math3.hpp (tests/host_harness: the text the device compiles); the guards S[0] > 0, S[0] finite and 0.5 < len < 2; the
    last column of V over its length, stored as fp32.  -> (m, 3) float32"""
    from tests import host_harness as hh
    p = pts[np.asarray(idx)].astype(f64)  # (m, k, 3)
    m, k = p.shape[:2]
    cen = np.zeros((m, 3))
    for j in range(k):
        cen = cen + p[:, j]
    cen = cen / f64(k)
    C = np.zeros((m, 3, 3))
    for j in range(k):
        d = p[:, j] - cen
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = C[:, a, b] + d[:, a] * d[:, b]
    C[:, 1, 0], C[:, 2, 0], C[:, 2, 1] = C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    out = np.zeros((m, 3), f32)
    done = {}
    for i in range(m):
        key = C[i].tobytes()
        if key not in done:
            _, S, V = hh.svd3(C[i])
            length = np.sqrt(V[0, 2] * V[0, 2] + V[1, 2] * V[1, 2] + V[2, 2] * V[2, 2])
            n = np.zeros(3, f32)
            if S[0] > 0.0 and S[0] <= 1.7976931348623157e308 and 0.5 < length < 2.0:
                n = (V[:, 2] / length).astype(f32)
            done[key] = n
        out[i] = done[key]
    return out


def check_designed(name, n, where=""):
    """the exact bits of the designed clouds' normals, on top of check_normals; abs(): the sign of a normal is left as it falls"""
    n32 = np.ascontiguousarray(n, f32)
    a = np.abs(n32)
    if name == "plates":
        want = PLATE_AXES[plate_of_row()]
        assert np.array_equal(bits(a), bits(want)), (where, "a plate's normal is its axis, bit for bit", np.flatnonzero((bits(a) != bits(want)).any(axis=1))[:8])
    elif name == "plane":
        want = np.tile(f32([0, 0, 1]), (len(a), 1))
        assert np.array_equal(bits(a), bits(want)), (where, "(0, 0, +-1) on every row", np.flatnonzero((bits(a) != bits(want)).any(axis=1))[:8])
    elif name == "cube":
        corners = np.flatnonzero(_permutation("cube") < 8)  # caller row r holds generated point _permutation[r]
        assert np.array_equal(bits(a[corners]), bits(np.tile(f32([0, 0, 1]), (8, 1)))), (where, "the cube's corners: C = s I gives e_z", n32[corners])
    elif name == "duplicates":
        p = _permutation("duplicates")
        held_a, held_b = np.flatnonzero(p < DUP_A_COPIES), np.flatnonzero((p >= DUP_A_COPIES) & (p < DUP_A_COPIES + DUP_B_COPIES))
        assert len(held_a) == DUP_A_COPIES and not bits(n32[held_a]).any(), (where, "40 copies of one position: no extent, the zero vector")
        assert len(held_b) == DUP_B_COPIES and n32[held_b].any(axis=1).all(), (where, "31 copies and one foreign point: a unit vector")
        assert int((~n32.any(axis=1)).sum()) == DUP_A_COPIES, (where, "no other row is without a normal")
