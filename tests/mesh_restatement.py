"""numpy restatement of fgoicp_mesh_sample (include/fgoicp_amd.h): IEEE fp64 on the fp32 coordinates, one rounding per operation in the
order the header writes them, integer weights, counter-based draws.  tests/test_mesh_host.py checks the restatement itself,
tests/test_gpu_mesh.py the device against it.  Also the meshes both use."""
import numpy as np

from tests.segment_restatement import GOLDEN, mix64

f64, u64 = np.float64, np.uint64
TWO32 = 4294967296.0


def faces(V, T):
    """(a, e1, e2, n, n2) of every face, float64"""
    X = np.asarray(V, np.float32).astype(f64)
    T = np.asarray(T, np.int64)
    a, b, c = X[T[:, 0]], X[T[:, 1]], X[T[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    return a, e1, e2, n, n2


def face_area(V, T):
    return f64(0.5) * np.sqrt(faces(V, T)[4])


def weights(area):
    """(q (nf,) uint64, Q (nf,) uint64: the inclusive scan, A_max)"""
    area = np.asarray(area, f64)
    amax = area.max()
    q = np.floor(area / amax * f64(TWO32)).astype(u64)
    return q, np.cumsum(q, dtype=u64), amax


def hashes(seed, m):
    """(m, 3) uint64: h(k, s)"""
    with np.errstate(over="ignore"):
        k = np.arange(m, dtype=u64)
        return np.stack([mix64(u64(seed) + u64(GOLDEN) * (u64(3) * k + u64(s + 1))) for s in range(3)], 1)


def mulhi64(a, b):
    """the high 64 bits of a[i] * b, exact"""
    b = int(b)
    return np.array([(int(x) * b) >> 64 for x in a], dtype=u64)


def info(V, T, m, area):
    q, Q, amax = weights(area)
    total = int(Q[-1])
    return dict(vertices=len(V), triangles=len(T), samples=m, zero_area=int((np.asarray(area) == 0.0).sum()), unweighted=int((q == 0).sum()), weight_total=total,
                max_area=float(amax), area=float(amax * f64(total) / f64(TWO32)))


def sample(V, T, m, seed=0, area=None):
    """(points (m, 3) float32, normals (m, 3) float32, face (m,) uint32, uv (m, 2) float64, face_area (nf,) float64, info); area: the face
    areas to weigh by (the device's own bits), None = face_area(V, T)"""
    a, e1, e2, n, n2 = faces(V, T)
    area = f64(0.5) * np.sqrt(n2) if area is None else np.asarray(area, f64)
    q, Q, _ = weights(area)
    h = hashes(seed, m)
    r = mulhi64(h[:, 0], Q[-1])
    face = np.searchsorted(Q, r, side="right")  # the first f with Q[f] > r
    u = (h[:, 1] >> u64(11)).astype(f64) * f64(2.0 ** -53)
    v = (h[:, 2] >> u64(11)).astype(f64) * f64(2.0 ** -53)
    flip = u + v > 1.0
    u = np.where(flip, 1.0 - u, u)
    v = np.where(flip, 1.0 - v, v)
    pts = ((a[face] + u[:, None] * e1[face]) + v[:, None] * e2[face]).astype(np.float32)
    nrm = (n[face] / np.sqrt(n2[face])[:, None]).astype(np.float32)
    return pts, nrm, face.astype(np.uint32), np.stack([u, v], 1), area, info(V, T, m, area)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def planted_mesh():
    """A 1 x 2 x 3 box (12 triangles, outward winding), a sliver, a zero-area face that repeats a vertex and a tiny face with 1e-6 edges:
    15 faces, zero_area = 1, unweighted = 2 (the tiny face is more than 2^32 times smaller than the largest)."""
    box = [(x, y, z) for z in (0.0, 3.0) for y in (0.0, 2.0) for x in (0.0, 1.0)]  # vertex = x + 2 y + 4 z in units of the edges
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    T = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    V = box + [(5.0, 0.0, 0.0), (5.0, 1e-3, 0.0), (5.0, 0.0, 4.0)]
    T.append((8, 9, 10))  # the sliver
    T.append((8, 8, 10))  # zero area
    V += [(7.0, 7.0, 7.0), (7.0 + 1e-6, 7.0, 7.0), (7.0, 7.0 + 1e-6, 7.0)]
    T.append((11, 12, 13))  # tiny
    return np.array(V, np.float32), np.array(T, np.uint32)


def random_mesh(nf, seed):
    """nf triangles over 3 nf / 2 + 3 generic fp32 vertices"""
    rng = np.random.default_rng(seed)
    nv = 3 * nf // 2 + 3
    V = rng.normal(size=(nv, 3)).astype(np.float32)
    T = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.uint32)
    return V, T


def bumpy_icosphere(subdivisions=3):
    """A closed mesh without symmetry: an icosphere (20 x 4^subdivisions faces, outward winding) whose radius is modulated by a few
    incommensurate waves."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    V = [tuple(np.array(v, f64) / np.linalg.norm(v)) for v in V]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                w = np.array(V[i], f64) + np.array(V[j], f64)
                V.append(tuple(w / np.linalg.norm(w)))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in T:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = out
    X = np.array(V, f64)
    x, y, z = X.T
    radius = 1.0 + 0.18 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y - 0.9) + 0.12 * np.sin(3.1 * z + 1.3 * x) + 0.15 * x * y + 0.1 * z ** 3 + 0.08 * y
    return (X * radius[:, None]).astype(np.float32), np.array(T, np.uint32)


def write_ply(path, V, polygons, fmt="ascii", list_name="vertex_indices", count_type="uchar", index_type="int", extra_list=None):
    """A PLY of vertices and polygons (lists of vertex indices of any length).  fmt: ascii, binary_little_endian, binary_big_endian.
    extra_list = (element name, list property name, rows): one more element with one list property, written before the faces."""
    np_type = {"uchar": "u1", "char": "i1", "ushort": "u2", "short": "i2", "uint": "u4", "int": "i4"}
    order = ">" if fmt == "binary_big_endian" else "<"
    head = ["ply", f"format {fmt} 1.0", "comment written by tests/mesh_restatement.py", f"element vertex {len(V)}", "property float x", "property float y", "property float z"]
    if extra_list is not None:
        head += [f"element {extra_list[0]} {len(extra_list[2])}", f"property list uchar int {extra_list[1]}"]
    if polygons is not None:
        head += [f"element face {len(polygons)}", f"property list {count_type} {index_type} {list_name}"]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        rows = lambda ct, it, data: b"".join(np.array([len(r)], order + np_type[ct]).tobytes() + np.array(r, order + np_type[it]).tobytes() for r in data)
        if fmt == "ascii":
            f.write("".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in np.asarray(V, np.float32)).encode())
            for data in ([] if extra_list is None else [extra_list[2]]) + ([] if polygons is None else [polygons]):
                f.write("".join(" ".join(str(int(v)) for v in [len(r), *r]) + "\n" for r in data).encode())
        else:
            f.write(np.asarray(V, np.float32).astype(order + "f4").tobytes())
            if extra_list is not None:
                f.write(rows("uchar", "int", extra_list[2]))
            if polygons is not None:
                f.write(rows(count_type, index_type, polygons))
