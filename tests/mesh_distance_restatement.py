"""numpy restatement of fgoicp_mesh_distance and fgoicp_point_triangle (include/fgoicp_amd.h): IEEE fp64 on the fp32 values, one rounding per
operation in the order the header writes them, EVERY participating face for every query — no tree, no pruning.
tests/test_mesh_distance_host.py checks the restatement itself and the host function against it, tests/test_gpu_mesh_distance.py the
device.  FALLBACKS counts the (query, face) pairs that took the fall-back of the interior branch."""
import numpy as np

from tests.mesh_restatement import faces

f64 = np.float64
LEAF = 8  # faces per leaf of the device's tree (info.leaf_faces)
FALLBACKS = {"pairs": 0}


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


# Inside, a vector is a tuple of its three component arrays: numpy runs an operation over a contiguous array several times faster than over
# the columns of an (..., 3) array, and the all-faces pass of mesh_distance is 2e7 pairs.
def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _sub(x, y):
    return (x[0] - y[0], x[1] - y[1], x[2] - y[2])


def _along(x, t, e):
    return (x[0] + t * e[0], x[1] + t * e[1], x[2] + t * e[2])


def _where(m, x, y):
    return tuple(np.where(m, x[k], y[k]) for k in range(3))


def _at(p, c):
    d = _sub(p, c)
    return _dot(d, d)


def _seg(p, x, y, edge, vx, vy):
    e = _sub(y, x)
    num, den = _dot(e, _sub(p, x)), _dot(e, e)
    first, last = ~(num > 0.0), ~(num < den)
    c = _where(first, x, _where(last, y, _along(x, num / den, e)))
    return c, _at(p, c), np.where(first, vx, np.where(last, vy, edge))


def _segment(p, x, y, edge, vx, vy):
    """(closest, dist2, region) of the segment x -> y, the fall-back's step: not (num > 0): x; not (num < den): y; else x + (num / den) e"""
    p, x, y = np.broadcast_arrays(*(np.asarray(v, f64) for v in (p, x, y)))
    with np.errstate(all="ignore"):
        c, d2, region = _seg(*(tuple(v[..., k] for k in range(3)) for v in (p, x, y)), edge, vx, vy)
    return np.stack(c, -1), d2, region


def _point_triangle(p, a, b, c, want_closest=True):
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    m1 = (d1 <= 0.0) & (d2 <= 0.0)
    bp = _sub(p, b)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    m2 = (d3 >= 0.0) & (d4 <= d3)
    vc = d1 * d4 - d3 * d2
    m3 = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0)
    den = d1 - d3
    c3 = _along(a, np.where(den == 0.0, 0.0, d1 / den), ab)
    cp = _sub(p, c)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    m4 = (d6 >= 0.0) & (d5 <= d6)
    vb = d5 * d2 - d1 * d6
    m5 = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0)
    den = d2 - d6
    c5 = _along(a, np.where(den == 0.0, 0.0, d2 / den), ac)
    va = d3 * d6 - d5 * d4
    m6 = (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0)
    den = (d4 - d3) + (d5 - d6)
    c6 = _along(b, np.where(den == 0.0, 0.0, (d4 - d3) / den), _sub(c, b))
    s = (va + vb) + vc
    v, w = vb / s, vc / s
    m7 = (s > 0.0) & (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
    c7 = tuple((a[k] + v * ab[k]) + w * ac[k] for k in range(3))
    fell_back = ~(m1 | m2 | m3 | m4 | m5 | m6 | m7)
    # the first condition that holds, in the definition's order
    closest = _where(m1, a, _where(m2, b, _where(m3, c3, _where(m4, c, _where(m5, c5, _where(m6, c6, c7))))))
    region = np.where(m1, 4, np.where(m2, 5, np.where(m3, 1, np.where(m4, 6, np.where(m5, 3, np.where(m6, 2, 0))))))
    if fell_back.any():
        FALLBACKS["pairs"] += int(fell_back.sum())
        best_c, best_d, best_r = _seg(p, a, b, 1, 4, 5)
        for seg in (_seg(p, b, c, 2, 5, 6), _seg(p, c, a, 3, 6, 4)):
            take = (seg[1] < best_d) | ((seg[1] == best_d) & (seg[2] < best_r))
            best_c, best_d, best_r = _where(take, seg[0], best_c), np.where(take, seg[1], best_d), np.where(take, seg[2], best_r)
        closest, region = _where(fell_back, best_c, closest), np.where(fell_back, best_r, region)
    return closest, _at(p, closest), region, fell_back


def point_triangle(p, a, b, c):
    """p, a, b, c: (..., 3) float64 arrays that broadcast.  Returns (closest (..., 3) float64, dist2, region, fell_back)."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, f64) for x in (p, a, b, c)))
    with np.errstate(all="ignore"):
        closest, d2, region, fell_back = _point_triangle(*(tuple(x[..., k] for k in range(3)) for x in (p, a, b, c)))
    return np.stack(closest, -1), d2, region.astype(np.int64), fell_back


def side_of(p, a, b, c, closest):
    e1, e2 = b - a, c - a
    n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2], e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
    return np.sign(dot(n, p - closest)).astype(np.int64)


def one(p, a, b, c):
    """fgoicp_point_triangle: (closest (3,) float32, dist2 float64, region int, side int) of fp32 inputs"""
    x = [np.asarray(v, np.float32).astype(f64) for v in (p, a, b, c)]
    closest, d2, region, _ = point_triangle(*x)
    return closest.astype(np.float32), f64(d2), int(region), int(side_of(*x, closest))


def mesh_distance(V, T, Q, flags=0, chunk=1 << 17):
    """(dist2 (nq,) float64, face uint32, closest (nq, 3) float32, region uint8, side int8, info) — every participating face for every query"""
    a, e1, e2, n, n2 = faces(V, T)
    X = np.asarray(V, np.float32).astype(f64)
    Tn = np.asarray(T, np.int64)
    part = np.flatnonzero(n2 != 0.0)
    A, B, C = X[Tn[part, 0]], X[Tn[part, 1]], X[Tn[part, 2]]
    P = np.asarray(Q, np.float32).astype(f64)
    nq = len(P)
    best_d = np.full(nq, np.inf)
    best_f = np.zeros(nq, np.int64)
    step = max(1, chunk // max(nq, 1))
    Pc = tuple(np.ascontiguousarray(P[:, k])[:, None] for k in range(3))
    Ac, Bc, Cc = (tuple(np.ascontiguousarray(X[:, k]) for k in range(3)) for X in (A, B, C))
    for lo in range(0, len(part), step):  # blocks of (nq, step) pairs that stay in cache
        with np.errstate(all="ignore"):
            d2 = _point_triangle(Pc, *(tuple(x[None, lo:lo + step] for x in X) for X in (Ac, Bc, Cc)))[1]
        k = np.argmin(d2, axis=1)  # the first minimum: the lowest face index among equal dist2
        d = d2[np.arange(nq), k]
        take = d < best_d  # strict: an earlier chunk holds the lower indices
        best_d, best_f = np.where(take, d, best_d), np.where(take, lo + k, best_f)
    wa, wb, wc = A[best_f], B[best_f], C[best_f]
    closest, d2, region, _ = point_triangle(P, wa, wb, wc)
    assert np.array_equal(d2, best_d)
    side = side_of(P, wa, wb, wc, closest)
    nleaves = -(-len(part) // LEAF)
    info = dict(flags=flags, vertices=len(X), triangles=len(Tn), queries=nq, faces=len(part), zero_area=len(Tn) - len(part), tree_depth=(nleaves - 1).bit_length(),
                leaf_faces=LEAF, max_dist2=float(d2.max()), max_dist2_index=int(np.argmax(d2)))
    return d2, part[best_f].astype(np.uint32), closest.astype(np.float32), region.astype(np.uint8), side.astype(np.int8), info
