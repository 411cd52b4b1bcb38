"""The exact nearest-neighbour rule of the scans, restated in numpy with the device's fp32 arithmetic and the reference's tie rule
(icp3d.cu:20-25: square roots compared, lowest index), and the designed inputs of tests/test_gpu_nn_scan.py.  Test infrastructure: the
properties the inputs are designed for are asserted without a GPU by tests/test_nn_restatement_host.py."""
import numpy as np

f32 = np.float32
UNIT_BOX = np.array([[-0.5, 0.5]] * 3, f32)
I3, ZERO3 = np.eye(3, dtype=f32), np.zeros(3, f32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the fp32 arithmetic of oracle/np_restatement.py, restated here: fma(a, b, c) = float32(float64(a) * float64(b) + float64(c))
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _moved(R, t, p):
    """R*p + t as the scans move their queries: fma(R[r,2], z, fma(R[r,1], y, R[r,0]*x)) + t[r]"""
    R = np.asarray(R, f32); t = np.asarray(t, f32); p = np.asarray(p, f32)
    q = np.empty_like(p)
    for r in range(3):
        q[:, r] = (_fma(R[r, 2], p[:, 2], _fma(R[r, 1], p[:, 1], (R[r, 0] * p[:, 0]).astype(f32))) + t[r]).astype(f32)
    return q


def _dist_sq(q, p):
    """(nq, 3), (np, 3) -> (nq, np): the device's fma(dz, dz, fma(dy, dy, dx * dx)) of d = q - p"""
    d = (q[:, None, :] - p[None, :, :]).astype(f32)
    return _fma(d[..., 2], d[..., 2], _fma(d[..., 1], d[..., 1], (d[..., 0] * d[..., 0]).astype(f32)))


def brute_force(pct, pcs, R, t, chunk=512):
    """-> (indices, dist2): per source point the FIRST target index attaining the smallest sqrt(d2) in fp32 (kernFindNearestNeighbor's
    loop, icp3d.cu:20-25) and the smallest squared distance (registration.cu:162-174)"""
    q = _moved(R, t, pcs)
    pct = np.asarray(pct, f32)
    chunk = max(1, min(chunk, (1 << 22) // len(pct)))  # a few tens of MB per temporary whatever the target's size
    idx = np.empty(len(q), np.uint32)
    d2min = np.empty(len(q), np.float32)
    for a in range(0, len(q), chunk):
        d2 = _dist_sq(q[a:a + chunk], pct)
        d2min[a:a + chunk] = d2.min(axis=1)
        idx[a:a + chunk] = np.argmin(np.sqrt(d2), axis=1)  # fp32 sqrt is correctly rounded; argmin returns the first minimum
    return idx, d2min


def brute_nodes(tgt, bounds, res, xyz):
    """buildLUTKernel for single nodes (registration.cu:258-278): min_j |node * res - (tgt_j - min_bound)|^2 in fp32."""
    pts = (np.asarray(tgt, f32) + (-np.asarray(bounds, f32)[:, 0])[None, :]).astype(f32)
    out = np.empty(len(xyz), f32)
    step = max(1, (1 << 22) // len(pts))
    for a in range(0, len(xyz), step):
        nodes = (np.asarray(xyz[a:a + step]).astype(f32) * f32(res)).astype(f32)
        out[a:a + step] = _dist_sq(nodes, pts).min(axis=1)
    return out


def exact_min_d2(pct, q):
    """fp64: the smallest squared distance of every query, every operation in double"""
    pct = np.asarray(pct, np.float64); q = np.asarray(q, np.float64)
    out = np.empty(len(q))
    step = max(1, (1 << 22) // len(pct))
    for a in range(0, len(q), step):
        d = q[a:a + step, None, :] - pct[None, :, :]
        out[a:a + step] = (d * d).sum(axis=2).min(axis=1)
    return out


def lut_dims(bounds, res):
    b = np.asarray(bounds, f32).reshape(3, 2)
    return tuple(int(np.ceil(f32(f32(b[a, 1] - b[a, 0]) / f32(res)))) for a in range(3))


def sample_nodes(dims, seed, n=256):
    """(n, 3) int32 LUT node indices: the 8 corners, then random ones"""
    rng = np.random.default_rng(seed)
    corners = np.array([[i * (dims[0] - 1), j * (dims[1] - 1), k * (dims[2] - 1)] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.int32)
    rest = np.stack([rng.integers(0, dims[a], n - 8) for a in range(3)], 1).astype(np.int32)
    return np.concatenate([corners, rest])


# ---- the designed inputs -----------------------------------------------------------------------------------------------------------
class Case:
    """One context's worth of input: target, queries (passed as the source cloud), LUT bounds and resolution (at most ~17 nodes per axis)."""

    def __init__(self, name, pct, q, bounds=UNIT_BOX, res=1.0 / 16):
        self.name, self.pct, self.q = name, np.ascontiguousarray(pct, f32), np.ascontiguousarray(q, f32)
        self.bounds, self.res = np.asarray(bounds, f32), float(res)
        assert max(lut_dims(self.bounds, self.res)) <= 17 and min(lut_dims(self.bounds, self.res)) >= 1


_REF = {}


def reference(case):
    """The numpy answers of a case, computed once per process: idx, d2 (brute_force at the identity), sse64 (fp64 sum of d2), xyz (256
    sampled LUT nodes) and nodes (their brute-force values)."""
    if case.name not in _REF:
        idx, d2 = brute_force(case.pct, case.q, I3, ZERO3)
        xyz = sample_nodes(lut_dims(case.bounds, case.res), 1234)
        _REF[case.name] = dict(idx=idx, d2=d2, sse64=float(d2.astype(np.float64).sum()), xyz=xyz, nodes=brute_nodes(case.pct, case.bounds, case.res, xyz))
    return _REF[case.name]


FAR_ROW = 31  # the far query's row among the 64 of the mixed set


def near_queries(rng, pct, n, noise=1e-3):
    return (pct[rng.integers(0, len(pct), n)] + rng.uniform(-noise, noise, (n, 3))).astype(f32)


def query_mix(rng, pct, ns):
    """ns queries about a target in the unit box: the first min(64, ns) caller rows are the MIXED set (near queries and, at FAR_ROW, one
    far one: a large wave radius next to small own bounds when the rows stay one wave); the rest a third each of target points plus 1e-3
    noise, uniform in 1.5 x the box, and the box shifted three box sizes away."""
    m = min(64, ns)
    mixed = near_queries(rng, pct, m)
    if m > FAR_ROW:
        mixed[FAR_ROW] = (2.0, -1.5, 1.0)
    rest = ns - m
    a, b = rest // 3, rest // 3
    parts = [mixed, near_queries(rng, pct, a), rng.uniform(-0.75, 0.75, (b, 3)).astype(f32),
             (rng.uniform(-0.5, 0.5, (rest - a - b, 3)) + np.array([3.0, -3.0, 3.0])).astype(f32)]
    return np.concatenate(parts).astype(f32)


def tree_edge_case(nt, ns=320):
    """Uniform targets in the unit box; nt at the edges of the tree (a leaf = 32 points, a super-leaf = 64 leaves = 2048 points, a top box =
    64 super-leaves = 131 072 points: one point more and the tree gains a level, half of whose leaves are empty)."""
    rng = np.random.default_rng(1000 + nt + 7 * ns)
    pct = rng.uniform(-0.5, 0.5, (nt, 3)).astype(f32)
    return Case(f"tree_{nt}_{ns}", pct, query_mix(rng, pct, ns))


def launch_case(ns, nt=2049):
    """Many queries against a small target: half near the target, two fifths uniform in 1.5 x the box, a tenth three box sizes away"""
    rng = np.random.default_rng(2000 + ns % 1000)
    pct = rng.uniform(-0.5, 0.5, (nt, 3)).astype(f32)
    a, b = ns // 2, (2 * ns) // 5
    q = np.concatenate([near_queries(rng, pct, a), rng.uniform(-0.75, 0.75, (b, 3)).astype(f32),
                        (rng.uniform(-0.5, 0.5, (ns - a - b, 3)) + np.array([3.0, -3.0, 3.0])).astype(f32)])
    return Case(f"launch_{ns}_{nt}", pct, q[rng.permutation(ns)])


def single_point_case(nt=2049, ns=320):
    rng = np.random.default_rng(3001)
    pct = np.tile(np.array([[0.1, 0.2, 0.3]], f32), (nt, 1))
    return Case("single_point", pct, query_mix(rng, pct, ns))


def sphere_case(nt=2049):
    """nt points on the fp32-normalised unit sphere; queries: the centre (every leaf is a candidate: the distances differ in their last
    bits only), 63 points within 1e-3 of it, 32 target points and 32 other points of the sphere"""
    rng = np.random.default_rng(3002)

    def on_sphere(n):
        v = rng.normal(size=(n, 3)).astype(f32)
        return (v / np.sqrt((v * v).sum(axis=1, dtype=f32), dtype=f32)[:, None]).astype(f32)

    pct = on_sphere(nt)
    q = np.concatenate([np.zeros((1, 3), f32), rng.uniform(-1e-3, 1e-3, (63, 3)).astype(f32), pct[rng.integers(0, nt, 32)], on_sphere(32)])
    return Case("sphere", pct, q, bounds=np.array([[-1, 1]] * 3, f32), res=0.125)


def lattice_target():
    """the 16 x 16 x 16 integer lattice, caller index x + 16 y + 256 z, and a duplicate of caller point 0 appended: 4097 points"""
    g = np.arange(16, dtype=f32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(f32)
    return np.concatenate([pts, pts[:1]])


def lattice_cell_centres(n=320):
    """centres of n cells (not the cell at the origin, whose corner has a duplicate): 8 targets at d2 = 0.75 exactly"""
    rng = np.random.default_rng(3003)
    cells = np.array([(i, j, k) for k in range(15) for j in range(15) for i in range(15)][1:], f32)
    return (cells[rng.choice(len(cells), n, replace=False)] + f32(0.5)).astype(f32)


def lattice_faces_edges(n=320):
    """face centres (4 targets at 0.5), edge midpoints (2 at 0.25), the centre of the cell at the origin (9 at 0.75, the duplicate among
    them) and the origin itself (caller points 0 and 4096 at 0)"""
    rng = np.random.default_rng(3004)
    base = rng.integers(0, 15, (n, 3)).astype(f32)
    kind = rng.integers(0, 6, n)  # 0-2: the face normal to that axis; 3-5: the edge along axis kind - 3
    off = np.where(kind[:, None] < 3, f32(0.5), f32(0.0)) * np.ones((n, 3), f32)
    for ax in range(3):
        off[kind == ax, ax] = 0.0
        off[kind == 3 + ax, ax] = 0.5
    q = (base + off).astype(f32)
    q[0] = (0.5, 0.5, 0.5)
    q[1] = (0.0, 0.0, 0.0)
    return q


LATTICE_BOUNDS = np.array([[-0.5, 15.5]] * 3, f32)  # resolution 1: the LUT's nodes are cell centres and their continuation outside


def lattice_cases():
    pct = lattice_target()
    both = np.concatenate([lattice_cell_centres(160), lattice_faces_edges(160)])
    return [Case("lattice_cells", pct, lattice_cell_centres(), LATTICE_BOUNDS, 1.0), Case("lattice_faces_edges", pct, lattice_faces_edges(), LATTICE_BOUNDS, 1.0),
            Case("lattice_reversed", pct[::-1], both, LATTICE_BOUNDS, 1.0)]


def sqrt_tie_partners(q, rng):
    """-> (near, far): two points on opposite sides of q whose fp32 squared distances to q differ by one ulp (far's is the larger) while
    their fp32 square roots are equal — tests/test_oracle_kat.py sqrt_tie_pair() about an arbitrary query.  (That pair itself cannot be
    translated to another query: its coordinates use all 24 bits.)"""
    q = np.asarray(q, f32)
    d2 = lambda p: _dist_sq(q[None, :], p[None, :])[0, 0]
    while True:
        r = rng.uniform(0.3, 0.6, 3).astype(f32)
        near = (q + r).astype(f32)
        far = (q - r).astype(f32)
        dn = d2(near)
        for _ in range(64):  # walk far's z away from q, one ulp at a time, until its square passes near's (q's z is small: fine steps)
            if d2(far) > dn:
                break
            far[2] = np.nextafter(far[2], f32(-np.inf))
        df = d2(far)
        if df > dn and np.sqrt(dn, dtype=f32) == np.sqrt(df, dtype=f32):
            return near, far


def sqrt_tie_case(nt=2049):
    """16 queries on a 4 x 4 grid of pitch 4, each with a sqrt-tie pair about it — the one at the origin is sqrt_tie_pair() itself, its
    second point mirrored — and 48 queries without one.  Caller order: the 16 partners with the LARGER square (0..15), the 16 with the
    smaller (16..31), then 41 filler points behind every partner as seen from its query (so that the two partners of a query, 1.5 apart,
    lie in different 32-point leaves), then background points farther than 1.5 from every query."""
    from tests.test_oracle_kat import sqrt_tie_pair
    rng = np.random.default_rng(3005)
    Q = np.array([(4.0 * i, 4.0 * j, 0.0) for j in range(4) for i in range(4)], f32)
    near, far = np.empty((16, 3), f32), np.empty((16, 3), f32)
    a, b = sqrt_tie_pair()  # |a|^2 < |b|^2 by one ulp, equal roots, about the origin = Q[0]
    near[0], far[0] = a, -b
    for k in range(1, 16):
        near[k], far[k] = sqrt_tie_partners(Q[k], rng)
    filler = []
    for k in range(16):
        for p in (far[k], near[k]):
            r = (p - Q[k]).astype(np.float64)
            u = rng.uniform(0.05, 0.4, (41, 1))
            filler.append((Q[k] + r[None, :] * (1.0 + u) + rng.uniform(-0.01, 0.01, (41, 3))).astype(f32))  # at least 5 % = 0.026 farther, less the jitter's 0.018
    filler = np.concatenate(filler)
    back = np.empty((0, 3), f32)
    while len(back) < nt - 32 - len(filler):
        c = rng.uniform((-1.5, -1.5, -1.5), (13.5, 13.5, 1.5), (4096, 3)).astype(f32)
        keep = np.sqrt(((c[:, None, :] - Q[None, :, :]).astype(np.float64) ** 2).sum(axis=2)).min(axis=1) > 1.5
        back = np.concatenate([back, c[keep]])
    pct = np.concatenate([far, near, filler, back])[:nt]
    others = back[rng.integers(0, len(back), 48)] + rng.uniform(-0.2, 0.2, (48, 3))
    q = np.concatenate([Q, others.astype(f32)])
    bounds = np.array([[-2.0, 14.0], [-2.0, 14.0], [-2.0, 2.0]], f32)
    return Case("sqrt_tie", pct, q, bounds, 1.0)


def plane_case(nt=4097, ns=320):
    """a planar target, z = 0.25 with 1e-4 noise (thin leaf slabs); queries far off the plane, far away within it, and on it"""
    rng = np.random.default_rng(3006)
    pct = np.concatenate([rng.uniform(-0.5, 0.5, (nt, 2)), 0.25 + 1e-4 * rng.normal(size=(nt, 1))], axis=1).astype(f32)
    n1, n2 = ns // 4, ns // 4
    off = np.concatenate([rng.uniform(-0.5, 0.5, (n1, 2)), 0.25 + rng.choice([-1.0, 1.0], (n1, 1)) * rng.uniform(1.0, 3.0, (n1, 1))], axis=1)
    away = np.concatenate([rng.uniform(3.0, 5.0, (n2, 1)) * rng.choice([-1.0, 1.0], (n2, 1)), rng.uniform(-0.5, 0.5, (n2, 1)), 0.25 + 1e-4 * rng.normal(size=(n2, 1))], axis=1)
    on = near_queries(rng, pct, ns - n1 - n2, noise=1e-4)
    q = np.concatenate([off, away, on]).astype(f32)
    return Case("plane", pct, q[rng.permutation(ns)], np.array([[-0.5, 0.5], [-0.5, 0.5], [0.22, 0.28]], f32), 1.0 / 16)
