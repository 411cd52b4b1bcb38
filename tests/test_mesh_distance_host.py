"""Point-to-mesh distance (fgoicp_mesh_distance, fgoicp_point_triangle, io.deviation) as far as it goes without a GPU: the host function
against the numpy restatement of the definition (tests/mesh_distance_restatement.py) in bits on a designed table, the restatement against
a search that knows nothing of its formula, slivers, the struct layout against the header, every refusal that needs no device and the
command-line key.  The device's results are checked in tests/test_gpu_mesh_distance.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_distance_restatement as md
from tests import mesh_restatement as mr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
PREFIX = "fgoicp_mesh_distance: "
f32, f64 = np.float32, np.float64


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the designed table ------------------------------------------------------------------------------------------------------------------
GENERIC = np.array([(0.25, -1.5, 0.75), (2.0, 0.5, -0.5), (-0.75, 1.75, 1.25)], f32)  # few mantissa bits: the edge midpoints are fp32 numbers
ALIGNED = np.array([(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)], f32)
# (u, v) of a + u ab + v ac: one per region, in the order of the region codes 0 .. 6
BY_REGION = [(0.3, 0.3), (0.5, -0.4), (0.8, 0.8), (-0.4, 0.5), (-0.5, -0.5), (1.6, -0.3), (-0.3, 1.6)]
# on the boundaries between regions of ALIGNED, exact in fp32 and in every product: (query, the quantity that is 0, region)
BOUNDARIES = [((0.0, -1.0, 2.0), "d1", 4), ((4.0, -1.0, 1.0), "d3", 5), ((2.0, 0.0, 3.0), "vc", 1), ((-1.0, 4.0, 1.0), "d6", 6), ((0.0, 2.0, -3.0), "vb", 3),
              ((2.0, 2.0, 5.0), "va", 2), ((0.0, 0.0, 2.0), "d1 and d2", 4), ((4.0, 0.0, -2.0), "d3 and d4", 5), ((0.0, 4.0, 2.0), "d5 and d6", 6)]


def designed(tri):
    """the queries of one triangle: (label, query fp32, expected region or None)"""
    a, b, c = tri.astype(f64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    rows = []
    for region, (u, v) in enumerate(BY_REGION):
        for h in (0.0, 0.75, -0.75):  # in the plane, off it on either side
            rows.append((f"region {region}, height {h}", (a + u * (b - a) + v * (c - a) + h * n).astype(f32), region))
    for k, vertex in enumerate(tri):
        rows.append((f"on vertex {k}", vertex, 4 + k))
    for k, (x, y) in enumerate(((0, 1), (1, 2), (2, 0))):
        mid = ((tri[x].astype(f64) + tri[y].astype(f64)) / 2.0).astype(f32)
        assert np.array_equal(mid.astype(f64) * 2.0, tri[x].astype(f64) + tri[y].astype(f64))
        rows.append((f"on edge {k + 1}", mid, 1 + k))
    rows.append(("1e6 away", np.array([1e6, -2e6, 3e6], f32), None))
    return rows


@pytest.mark.parametrize("name", ["generic", "aligned"])
def test_the_host_function_equals_the_restatement_in_bits(fg, name):
    tri = {"generic": GENERIC, "aligned": ALIGNED}[name]
    rows = designed(tri)
    if name == "aligned":
        rows += [(f"boundary {what} == 0", np.array(q, f32), region) for q, what, region in BOUNDARIES]
    regions, sides = set(), set()
    for label, q, region in rows:
        got = fg.point_triangle(q, *tri)
        want = md.one(q, *tri)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and _bits(got[1]) == _bits(want[1]) and got[2:] == want[2:], (label, got, want)
        assert got[0].dtype == f32 and isinstance(got[1], f64)
        if region is not None:
            assert got[2] == region, (label, got)
        if label.startswith("on "):
            assert got[1] == 0.0 and got[3] == 0 and np.array_equal(got[0], q), (label, got)
        if name == "aligned" and "height 0.0" in label:
            assert got[3] == 0, (label, got)  # z == 0 exactly: in the plane
        regions.add(got[2])
        sides.add(got[3])
    assert regions == set(range(7)) and sides == {-1, 0, 1}
    far = fg.point_triangle(np.array([1e6, -2e6, 3e6], f32), *tri)
    assert np.isfinite(far[1]) and far[1] == pytest.approx(1.4e13, rel=1e-3)


def test_the_boundaries_of_the_aligned_triangle_are_exact():
    """every quantity named in BOUNDARIES is exactly 0 for its query — small integers: no operation rounds — and `<=` / `>=` send the query
    to the region the definition's order gives"""
    a, b, c = ALIGNED.astype(f64)
    for q, what, region in BOUNDARIES:
        p = np.array(q, f64)
        ab, ac = b - a, c - a
        d1, d2, d3, d4, d5, d6 = md.dot(ab, p - a), md.dot(ac, p - a), md.dot(ab, p - b), md.dot(ac, p - b), md.dot(ab, p - c), md.dot(ac, p - c)
        val = dict(d1=d1, d2=d2, d3=d3, d4=d4, d5=d5, d6=d6, vc=d1 * d4 - d3 * d2, vb=d5 * d2 - d1 * d6, va=d3 * d6 - d5 * d4)
        for key in what.split(" and "):
            assert val[key] == 0.0, (q, key, val[key])
    got = [md.one(np.array(q, f32), *ALIGNED)[2] for q, _, _ in BOUNDARIES]
    assert got == [4, 5, 1, 6, 3, 2, 4, 5, 6]  # (0, 4, 2) lies over vertex c: d5 = d6 = 0, and step 4 (d6 >= 0 && d5 <= d6) takes it


# ---- the restatement against a search that does not know its formula -------------------------------------------------------------------------
def _grid_min(p, a, b, c, n=400):
    """the minimum of |p - (a + u ab + v ac)|^2 over an n x n barycentric grid, refined once around its best cell at n times the resolution
    (the window reaches two cells to either side: in a skewed triangle the best grid point need not be the one next to the minimum); the v
    range of the refinement is clipped per u, so that the edge u + v = 1 is sampled exactly where the window reaches it.  Every grid point
    lies in the triangle: the value can only be above the true minimum"""
    ab, ac, ap = b - a, c - a, p - a
    k0, k1, k2, k11, k12, k22 = ap @ ap, ab @ ap, ac @ ap, ab @ ab, ab @ ac, ac @ ac

    def scan(u, v):  # |ap - u ab - v ac|^2 expanded: one array operation per term (its cancellation costs 1e-15 of |ap|^2, far inside 1e-9)
        d2 = k0 - 2.0 * (u * k1 + v * k2) + (u * u * k11 + 2.0 * (u * v) * k12 + v * v * k22)
        d2 = np.where(u + v <= 1.0, d2, np.inf)
        k = np.unravel_index(np.argmin(d2), d2.shape)
        return d2[k], u[k], v[k]
    t = np.linspace(0.0, 1.0, n + 1)
    u, v = np.meshgrid(t, t, indexing="ij")
    _, u0, v0 = scan(u, v)
    h = 2.0 / n
    uu = np.linspace(max(0.0, u0 - h), min(1.0, u0 + h), 2 * n + 1)
    vlo, vhi = np.maximum(0.0, v0 - h), np.minimum(1.0 - uu, v0 + h)
    vv = vlo + (np.maximum(vhi, vlo) - vlo)[:, None] * np.linspace(0.0, 1.0, 2 * n + 1)[None, :]
    return scan(np.broadcast_to(uu[:, None], vv.shape), vv)[0]


def test_the_restatement_finds_the_minimum_over_the_triangle():
    """200 random triangles and queries.  The grid's spacing after the refinement is 2 / 400^2 in u and v, so its minimum exceeds the true
    one by at most (|ab| + |ac|)^2 (1 / 400^2)^2 = 3.9e-11 (|ab| + |ac|)^2 (the distance is quadratic about its constrained minimum along
    the sampled directions); the queries are drawn at least 0.3 (|ab| + |ac|) off the plane, dist2 >= 0.09 (|ab| + |ac|)^2, which puts that
    at 4.4e-10 relative — inside the 1e-9 asked for.  Solved back, the closest point has u, v >= 0 and u + v <= 1 to 1e-12."""
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(200):
        a, b, c = rng.uniform(-1.0, 1.0, (3, 3)).astype(f32).astype(f64)
        size = np.linalg.norm(b - a) + np.linalg.norm(c - a)
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        u, v = rng.uniform(-0.5, 1.5, 2)
        p = (a + u * (b - a) + v * (c - a) + rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0) * size * n).astype(f32).astype(f64)
        closest, d2, region, _ = md.point_triangle(p, a, b, c)
        grid = _grid_min(p, a, b, c)
        assert d2 <= grid * (1.0 + 1e-12) and grid <= d2 * (1.0 + 1e-9), (d2, grid, int(region))
        uv = np.linalg.lstsq(np.stack([b - a, c - a], 1), closest - a, rcond=None)[0]
        assert uv[0] >= -1e-12 and uv[1] >= -1e-12 and uv.sum() <= 1.0 + 1e-12, uv
        seen.add(int(region))
    assert seen == set(range(7))


# ---- slivers ---------------------------------------------------------------------------------------------------------------------------------
def _slivers(rng, n, aspect):
    a = rng.normal(size=(n, 3)).astype(f32)
    b = (a + rng.normal(size=(n, 3))).astype(f32)
    t = rng.uniform(0.1, 0.9, (n, 1))
    c = (a.astype(f64) + t * (b.astype(f64) - a) + rng.normal(size=(n, 3)) * aspect).astype(f32)
    return a, b, c


def _near_collinear(rng, n):
    """b and c a few fp32 steps from a along one integer direction, c one step off the line"""
    a = rng.normal(size=(n, 3)).astype(f32)
    ulp = np.spacing(np.abs(a)).astype(f64)
    d = rng.integers(-8, 9, (n, 3))
    b = (a + d * rng.integers(1, 50, (n, 1)) * ulp).astype(f32)
    c = (a + d * rng.integers(1, 50, (n, 1)) * ulp + rng.integers(-1, 2, (n, 3)) * ulp).astype(f32)
    return a, b, c


def test_slivers_have_finite_consistent_answers(fg):
    """Triangles of aspect 1e-3, 1e-5 and 1e-7 and near-collinear fp32 triples, queries in the plane and 1e-6 .. 100 off it.  Every answer is
    finite, its region agrees with its closest point (a vertex region returns the vertex itself; an edge region a point of that edge's
    segment and the interior a point of the triangle, to rounding), it is no farther than the nearest vertex, and the host function
    returns the restatement's bits.

    The fall-back of step 7.  The definition names what happens when the interior test fails; md.FALLBACKS counts how often it does, and
    here and in every family searched while this was written (these; edges of 1e-10 with queries 2^44 .. 2^56 edge lengths up the normal;
    triangles 1e10 .. 1e30 long with queries one fp32 step inside the short edge; queries exactly on an edge's line, at dyadic and
    non-dyadic positions, under a vertex 1e3 .. 1e12 away; 4e6 unconstrained draws of d1 .. d6) the count is 0.  The argument why: step
    7 is reached with one of va, vb, vc <= 0 only through a sign pattern of d1 .. d6 that one of steps 1 - 6 has already taken — the draws of
    d1 .. d6 as free numbers, continuous and on a grid with ties, find no exception —, so s > 0 and v, w >= 0 there; and v + w > 1 needs
    va / s below 2^-54 while v and w round up, but a computed va that is not 0 is at least one unit in the last place of d3 d6 or d5 d4,
    which are of the order of s / 4 on the side of the triangle where va is small: v + w then exceeds 1 by less than half a unit and
    rounds to 1.  This is an argument, not a proof; the branch stays in the definition, the header and the restatement as the net under
    it, and the counter is asserted to be what was observed, 0, so that an input that does reach it shows up here."""
    rng = np.random.default_rng(21)
    md.FALLBACKS["pairs"] = 0
    families = [(f"aspect {x}", _slivers(rng, 4000, x)) for x in (1e-3, 1e-5, 1e-7)] + [("near-collinear", _near_collinear(rng, 4000))]
    for label, (a, b, c) in families:
        n2 = mr.faces(np.concatenate([a, b, c]), np.arange(3 * len(a)).reshape(3, -1).T)[4]
        keep = n2 != 0.0  # the faces that take part
        a, b, c = a[keep], b[keep], c[keep]
        A, B, Cc = a.astype(f64), b.astype(f64), c.astype(f64)
        n = len(a)
        u = rng.uniform(-0.2, 1.2, (n, 1))
        v = rng.uniform(-0.2, 1.2, (n, 1))
        p = (A + u * (B - A) + v * (Cc - A) + rng.normal(size=(n, 3)) * rng.choice([0.0, 1e-6, 1e-3, 1.0, 100.0], (n, 1))).astype(f32)
        P = p.astype(f64)
        closest, d2, region, _ = md.point_triangle(P, A, B, Cc)
        assert np.isfinite(d2).all() and np.isfinite(closest).all() and (region >= 0).all() and (region <= 6).all(), label
        nearest_vertex = np.minimum(np.minimum(((P - A) ** 2).sum(1), ((P - B) ** 2).sum(1)), ((P - Cc) ** 2).sum(1))
        assert (d2 <= nearest_vertex * (1.0 + 1e-12)).all(), label
        for code, vertex in ((4, A), (5, B), (6, Cc)):
            assert np.array_equal(closest[region == code], vertex[region == code]), label
        scale = np.abs(np.stack([A, B, Cc])).max()
        for code, (x, y) in ((1, (A, B)), (2, (B, Cc)), (3, (Cc, A))):  # on the segment: |c - x| + |c - y| = |y - x|
            m = region == code
            gap = np.linalg.norm(closest[m] - x[m], axis=1) + np.linalg.norm(closest[m] - y[m], axis=1) - np.linalg.norm(y[m] - x[m], axis=1)
            assert (np.abs(gap) <= 1e-12 * scale).all(), (label, code)
        m = region == 0  # in the triangle: the three sub-areas add up to the area
        full = np.linalg.norm(np.cross(B[m] - A[m], Cc[m] - A[m]), axis=1)
        parts = sum(np.linalg.norm(np.cross(x[m] - closest[m], y[m] - closest[m]), axis=1) for x, y in ((A, B), (B, Cc), (Cc, A)))
        assert (np.abs(parts - full) <= 1e-12 * scale * scale).all(), label
        for i in range(0, n, 97):  # the host function on a sample of them
            got, want = fg.point_triangle(p[i], a[i], b[i], c[i]), md.one(p[i], a[i], b[i], c[i])
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and _bits(got[1]) == _bits(want[1]) and got[2:] == want[2:], (label, i)
        print(f"{label}: {n} faces, regions {np.bincount(region, minlength=7).tolist()}")
    print(f"fall-backs of the interior branch: {md.FALLBACKS['pairs']}")
    assert md.FALLBACKS["pairs"] == 0


def test_the_fall_back_is_the_nearest_edge():
    """the branch itself, entered by hand: the three segments, the smallest dist2, a tie to the lowest region code — against 2001 samples
    of every edge (spacing 5e-4 of an edge: a quadratic miss of 2.5e-7 |edge|^2 at most)"""
    a, b, c = GENERIC.astype(f64)
    edges = ((a, b, 1, 4, 5), (b, c, 2, 5, 6), (c, a, 3, 6, 4))
    seen = set()
    for p in ((0.25, -1.5, 3.0), (1.125, -0.5, 4.0), (0.625, 1.125, 9.0), (-0.25, 0.125, -2.0), (3.0, 1.0, -1.0), (-2.0, 3.0, 2.0), (-0.75, 1.75, 1.5)):
        p = np.array(p, f64)
        best = min((md._segment(p, x, y, e, vx, vy) for x, y, e, vx, vy in edges), key=lambda s: (float(s[1]), int(s[2])))
        ts = np.linspace(0.0, 1.0, 2001)
        sampled = [(float(((p - (x + t * (y - x))) ** 2).sum()), e if 0.0 < t < 1.0 else (vx if t == 0.0 else vy)) for x, y, e, vx, vy in edges for t in ts]
        d2, region = min(sampled)
        assert float(best[1]) <= d2 and d2 - float(best[1]) <= 2.5e-7 * 12.0, (p, best, d2)  # |edge|^2 <= 12 here
        assert int(best[2]) == region, (p, best, region)
        seen.add(region)
    assert seen == {1, 3, 5, 6}  # edges and vertices both


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
FIELDS = ["struct_size", "flags", "vertices", "triangles", "queries", "faces", "zero_area", "tree_depth", "leaf_faces", "max_dist2_index", "max_dist2"]


def test_the_library_exports_the_calls_and_the_struct_is_the_headers(fg, tmp_path):
    lib = fg._lib.load()
    new = ("fgoicp_mesh_distance", "fgoicp_point_triangle")
    header = open(os.path.join(REPO, "include", "fgoicp_amd.h")).read()
    for name in new:
        assert hasattr(lib, name) and name in fg._lib.exported_symbols() and name + "(" in header
    for path in (fg.build.DEFAULT_LIB, fg.build.DEV_LIB):  # built into both libraries
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        for name in new:
            assert f" T {name}\n" in syms, (path, name)
    assert callable(fg.mesh_distance) and callable(fg.mesh_deviation) and callable(fg.point_triangle)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fgoicp_amd.h"\nint main(void) { printf("%zu %d'
                   + " %zu" * len(FIELDS) + '\\n", sizeof(fgoicp_mesh_distance_info_t), (int)FGOICP_MESH_DISTANCE_BRUTE, '
                   + ", ".join(f"offsetof(fgoicp_mesh_distance_info_t, {f})" for f in FIELDS) + "); return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(REPO, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    M = fg._lib.MeshDistanceInfo
    assert got == [C.sizeof(M), fg._lib.MESH_DISTANCE_BRUTE] + [getattr(M, f).offset for f in FIELDS]
    assert got == [72, 1, 0, 4, 8, 16, 24, 32, 40, 48, 52, 56, 64]
    assert lib.fgoicp_abi_version() == 2  # additions only


def _call(fg, V, T, Q, nv=None, nf=None, nq=None, flags=0, info="full", device=0):
    """the raw call: returns (status, message)"""
    L = fg._lib
    lib = L.load()
    mi = L.MeshDistanceInfo()
    if isinstance(info, int):
        mi.struct_size = info
    rc = lib.fgoicp_mesh_distance(None if V is None else V.ctypes.data_as(L.c_float_p), len(V) if nv is None else nv, None if T is None else T.ctypes.data_as(L.c_uint32_p),
                                  len(T) if nf is None else nf, None if Q is None else Q.ctypes.data_as(L.c_float_p), len(Q) if nq is None else nq, flags, device,
                                  None, None, None, None, None, None if info is None else C.byref(mi))
    return rc, lib.fgoicp_last_error().decode()


def _with(a, i, j, value):
    b = a.copy()
    b[i, j] = value
    return b


INFO_MESSAGE = "out must not be null and out->struct_size = sizeof(fgoicp_mesh_distance_info_t)"
REFUSALS = {
    "null vertices": (lambda V, T, Q: dict(V=None, T=T, Q=Q, nv=5), "the vertices must not be null or empty"),
    "no vertices": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nv=0), "the vertices must not be null or empty"),
    "null triangles": (lambda V, T, Q: dict(V=V, T=None, Q=Q, nf=5), "the triangles must not be null or empty"),
    "no triangles": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nf=0), "the triangles must not be null or empty"),
    "null queries": (lambda V, T, Q: dict(V=V, T=T, Q=None, nq=5), "the queries must not be null or empty"),
    "no queries": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nq=0), "the queries must not be null or empty"),
    "2^31 vertices": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nv=2 ** 31), "more than 2^31 - 1 vertices"),  # refused on the count alone: the array is not read
    "2^31 triangles": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nf=2 ** 31), "more than 2^31 - 1 triangles"),
    "2^31 queries": (lambda V, T, Q: dict(V=V, T=T, Q=Q, nq=2 ** 31), "more than 2^31 - 1 points"),
    "nan vertex": (lambda V, T, Q: dict(V=_with(V, 9, 1, np.nan), T=T, Q=Q), "vertex 9 has a non-finite coordinate"),
    "infinite vertex": (lambda V, T, Q: dict(V=_with(V, 13, 2, -np.inf), T=T, Q=Q), "vertex 13 has a non-finite coordinate"),
    "nan query": (lambda V, T, Q: dict(V=V, T=T, Q=_with(Q, 3, 0, np.nan)), "point 3 has a non-finite coordinate"),
    "infinite query": (lambda V, T, Q: dict(V=V, T=T, Q=_with(Q, 6, 2, np.inf)), "point 6 has a non-finite coordinate"),
    "index = nv": (lambda V, T, Q: dict(V=V, T=_with(T, 6, 2, len(V)), Q=Q), "face 6 has vertex index 14: the mesh has 14 vertices"),
    "index far above nv": (lambda V, T, Q: dict(V=V, T=_with(T, 14, 0, 2 ** 32 - 1), Q=Q), "face 14 has vertex index 4294967295: the mesh has 14 vertices"),
    "null info": (lambda V, T, Q: dict(V=V, T=T, Q=Q, info=None), INFO_MESSAGE),
    "struct_size 0": (lambda V, T, Q: dict(V=V, T=T, Q=Q, info=0), INFO_MESSAGE),
    "struct_size short": (lambda V, T, Q: dict(V=V, T=T, Q=Q, info=64), INFO_MESSAGE),  # ends before `max_dist2` ends
    "struct_size above 4096": (lambda V, T, Q: dict(V=V, T=T, Q=Q, info=4097), INFO_MESSAGE),
    "flag bit 1": (lambda V, T, Q: dict(V=V, T=T, Q=Q, flags=2), "unknown flag bits 2"),
    "flag bits 1 and 31": (lambda V, T, Q: dict(V=V, T=T, Q=Q, flags=2 ** 31 + 3), "unknown flag bits 2147483650"),
}


@pytest.fixture(scope="module")
def planted():
    V, T = mr.planted_mesh()
    return V, T, np.random.default_rng(2).uniform(-1.0, 4.0, (8, 3)).astype(f32)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_need_no_device(fg, planted, case):
    fg._lib.load().fgoicp_voxel_downsample(None, 0, C.c_float(1.0), None, 0, None, 0, None, None, None)  # leaves another call's message behind
    make, message = REFUSALS[case]
    rc, msg = _call(fg, **make(*planted))
    assert rc == INVALID_ARG and msg == PREFIX + message, (case, rc, msg)


def test_a_valid_call_without_a_device_reports_no_device(fg, planted):
    """(with a device the same calls succeed: their results are checked in tests/test_gpu_mesh_distance.py)"""
    V, T, Q = planted
    want = OK if _has_gpu() else NO_DEVICE
    for kw in (dict(), dict(flags=1), dict(info=72), dict(info=4096), dict(nq=1)):
        rc, msg = _call(fg, V, T, Q, **kw)
        assert rc == want and (msg.startswith(PREFIX) or want == OK), (kw, rc, msg)
    if want == NO_DEVICE:
        for call in (lambda: fg.mesh_distance(V, T, Q), lambda: fg.mesh_deviation(V, T, Q, np.eye(3), np.zeros(3), return_map=True)):
            with pytest.raises(fg.FgoicpError) as e:
                call()
            assert e.value.status == NO_DEVICE


def test_the_python_wrappers_check_shapes_first_and_the_host_function_refuses_bad_input(fg, planted):
    V, T, Q = planted
    for bad in (dict(vertices=V[:, :2]), dict(triangles=T[:, :2]), dict(triangles=T.astype(f32)), dict(triangles=T.astype(np.int64) - 1), dict(points=Q.reshape(-1))):
        kw = dict(vertices=V, triangles=T, points=Q)
        kw.update(bad)
        with pytest.raises(ValueError):
            fg.mesh_distance(**kw)
    with pytest.raises(fg.FgoicpError) as e:  # what the wrapper does not check itself, the call refuses
        fg.mesh_distance(V, _with(T, 3, 1, 99), Q)
    assert e.value.status == INVALID_ARG and "face 3 has vertex index 99" in str(e.value)
    lib = fg._lib.load()
    x = np.zeros(3, f32).ctypes.data_as(fg._lib.c_float_p)
    assert lib.fgoicp_point_triangle(None, x, x, x, None, None, None, None) == INVALID_ARG
    assert lib.fgoicp_last_error().decode() == "fgoicp_point_triangle: p3, a3, b3 and c3 must not be null"
    assert lib.fgoicp_point_triangle(x, x, x, x, None, None, None, None) == OK  # every output may be NULL
    with pytest.raises(fg.FgoicpError) as e:
        fg.point_triangle([0, np.inf, 0], *GENERIC)
    assert e.value.status == INVALID_ARG and "fgoicp_point_triangle: a coordinate is not finite" in str(e.value)


# ---- io.deviation: the configuration key, the writer, the refusals that need no device ---------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("deviation_config") / "deviation_config_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(REPO, "include"), "-o", str(exe),
                    os.path.join(REPO, "tests", "host_harness", "deviation_config_check.cpp")], check=True)

    def run(mode, path):
        p = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True, timeout=60)
        return p.returncode, [ln for ln in p.stdout.splitlines() if ln.startswith(("DEVIATION", "SUMMARY", "REFUSED"))]
    return run


def test_the_config_parser_reads_io_deviation(harness, tmp_path):
    def config(io):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "t.ply"\nsource = "s.ply"\n{io}[params]\nseed = 1\n')
        rc, lines = harness("config", tmp_path / "c.toml")
        return rc, lines[-1]
    assert config("") == (0, "DEVIATION [] ALIGNMENT []")  # absent: off
    assert config('deviation = "out/dev.txt"\n') == (0, "DEVIATION [out/dev.txt] ALIGNMENT []")
    assert config('alignment = "a.txt"\ndeviation = "d.txt"\n') == (0, "DEVIATION [d.txt] ALIGNMENT [a.txt]")
    assert config("deviation = 3\n") == (0, "DEVIATION [] ALIGNMENT []")  # not a string: as the other io keys, taken as absent


def test_the_deviation_writer_sums_in_row_order(harness, tmp_path):
    rc, lines = harness("write", tmp_path / "dev.txt")
    assert rc == 0
    got = lines[-1].split()[1:]
    assert [int(x) for x in got[:3] + got[6:]] == [3, 12, 1, 1, 1, 1]
    assert [float(x) for x in got[3:6]] == [(0.5 + 0.0 + 2.0) / 3.0, np.sqrt((0.25 + 0.0 + 4.0) / 3.0), 2.0]
    text = (tmp_path / "dev.txt").read_text().splitlines()
    assert text[0] == "# deviation: points = 3, triangles = 12, zero_area = 1, mean = 0.833333333, rms = 1.19023807, max = 2, negative = 1, on_plane = 1, positive = 1"
    assert text[1:] == ["# x y z face distance side region", "1 2 3 7 0.5 -1 0", "-0.5 0.25 0.00100000005 0 0 0 5", "4 5 6 4000000000 2 1 2"]


def test_cli_refuses_io_deviation_on_a_target_that_holds_no_mesh(fg, tmp_path):
    """a TXT target and a PLY without faces end the run with exit code 1 and the key's name, before any device is asked for; a mesh without
    area is refused by the call itself once a device is there (tests/test_gpu_mesh_distance.py)"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    pts = np.random.default_rng(6).uniform(-1.0, 1.0, (50, 3)).astype(f32)
    (tmp_path / "c.txt").write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))
    mr.write_ply(tmp_path / "cloud.ply", pts, None)

    def run(target, extra_io="", batch=False):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/{target}"\nsource = "{tmp_path}/c.txt"\ndeviation = "{tmp_path}/dev.txt"\n{extra_io}[params]\nseed = 1\n')
        (tmp_path / "list.txt").write_text("c.toml\n")
        args = ["--batch", str(tmp_path / "list.txt")] if batch else ["-c", str(tmp_path / "c.toml")]
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
    for batch in (False, True):
        rc, log = run("c.txt", batch=batch)
        assert rc == 1 and f'io.deviation = "{tmp_path}/dev.txt"' in log and "is not a PLY file" in log, log[-1000:]
        rc, log = run("cloud.ply", batch=batch)
        assert rc == 1 and f'io.deviation = "{tmp_path}/dev.txt"' in log and "has no faces" in log, log[-1000:]
    assert not (tmp_path / "dev.txt").exists()
