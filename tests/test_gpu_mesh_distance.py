"""Point-to-mesh distance on the device (fgoicp_mesh_distance, fg.mesh_distance, fg.mesh_deviation, io.deviation) against the numpy
restatement of its definition (tests/mesh_distance_restatement.py; include/fgoicp_amd.h), which tests every face for every query and prunes
nothing.  The definition contains no square root and no freedom of order — the winner is the smallest (dist2, face index) — so EVERYTHING is
compared in bits: face, region, side, dist2, closest and every info field; and the tree walk against the flag that walks no tree.

The kernel (csrc/device/mesh_distance.hip) gives a wave 64 queries that are neighbours in space and leaves of 8 faces: the sizes below sit
around both."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_distance_restatement as md
from tests import mesh_restatement as mr
from tests.test_gpu_mesh import R_GT, T_GT, _errors

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
LEAF = md.LEAF
f32, f64 = np.float32, np.float64
INFO_KEYS = ("flags", "vertices", "triangles", "queries", "faces", "zero_area", "tree_depth", "leaf_faces", "max_dist2", "max_dist2_index")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bytes(x, y):
    for a, b in zip(x[:5], y[:5]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for key in INFO_KEYS[1:]:
        assert x[5][key] == y[5][key], key
    assert x[5]["dist2"].tobytes() == y[5]["dist2"].tobytes()


def check(fg, V, T, Q, label, brute_too=True):
    got = fg.mesh_distance(V, T, Q, return_map=True)
    dist, face, closest, region, side, info = got
    wd2, wface, wclosest, wregion, wside, winfo = md.mesh_distance(V, T, Q)
    assert face.dtype == np.uint32 and closest.dtype == f32 and region.dtype == np.uint8 and side.dtype == np.int8 and dist.dtype == f64
    assert np.array_equal(face, wface), label
    assert np.array_equal(region, wregion) and np.array_equal(side, wside), label
    assert np.array_equal(_bits(info["dist2"]), _bits(wd2)), label
    assert np.array_equal(_bits(closest), _bits(wclosest)), label
    assert np.array_equal(_bits(dist), _bits(np.sqrt(wd2))), label
    for key in INFO_KEYS:
        assert info[key] == winfo[key] and type(info[key]) is type(winfo[key]), (label, key, info[key], winfo[key])
    if brute_too:
        brute = fg.mesh_distance(V, T, Q, return_map=True, brute=True)
        assert brute[5]["flags"] == 1
        same_bytes(got, brute)
    return got


# ---- the planted mesh ------------------------------------------------------------------------------------------------------------------------
def planted_queries():
    """the box centre (the faces x = 0 and x = 1 are equally near: four triangles tie), points on the box's corners and edges, points just
    inside and outside every face, the sliver's and the tiny face's neighbourhood, a point 1e3 away"""
    q = [(0.5, 1.0, 1.5)]
    q += [(x, y, z) for z in (0.0, 3.0) for y in (0.0, 2.0) for x in (0.0, 1.0)]  # the corners
    q += [(0.5, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 2.0, 1.5), (1.0, 0.0, 2.25), (0.25, 2.0, 3.0), (0.0, 0.5, 3.0)]  # on edges
    for axis, size in enumerate((1.0, 2.0, 3.0)):
        for at in (0.0, size):
            for eps in (-1e-3, 1e-3):
                p = [0.4, 0.7, 1.1]
                p[axis] = at + eps
                q.append(tuple(p))
    q += [(5.0, 5e-4, 2.0), (5.01, 0.0, 1.0), (4.99, 1e-3, 0.5), (5.0, 0.0, 0.0), (5.0, 5e-4, 4.5), (5.0, 2e-3, 3.9), (5.0, -1e-4, 1.0)]  # the sliver
    q += [(7.0, 7.0, 7.0), (7.0 + 5e-7, 7.0 + 2e-7, 7.0001), (6.9, 7.1, 7.0)]  # the tiny face
    q += [(1e3, -1e3, 1e3), (3.0, 1.0, 1.5), (-2.0, -2.0, -2.0)]
    return np.array(q, f32)


@pytest.fixture(scope="module")
def planted():
    V, T = mr.planted_mesh()
    return V, T, planted_queries()


def test_the_planted_mesh_ties_and_edges(fg, gpu_required, planted):
    V, T, Q = planted
    dist, face, closest, region, side, info = check(fg, V, T, Q, "planted")
    assert info["zero_area"] == 1 and info["faces"] == 14 and info["triangles"] == 15 and info["leaf_faces"] == LEAF and info["tree_depth"] == 1
    # the centre: x = 0 is quad 4 (faces 8, 9), x = 1 quad 5 (faces 10, 11); the centre projects onto the diagonal both triangles of a quad share
    assert dist[0] == 0.5 and face[0] == 8
    d2_all = md.point_triangle(Q[0].astype(f64)[None, :], *(V.astype(f64)[T[[8, 9, 10, 11]][:, k]] for k in range(3)))[1]
    assert (d2_all == 0.25).all()  # four triangles at the same distance: the lowest index won
    assert (dist[1:15] == 0.0).all() and (region[1:9] >= 4).all() and (side[1:15] == 0).all()  # corners and edges lie on the surface
    assert np.allclose(dist[15:27], 1e-3, rtol=1e-3) and (region[15:27] == 0).all()
    assert (side[15:27] == np.tile([1, -1, -1, 1], 3)).all()  # outward winding: inside is the negative side
    assert face[30] in (12,) and dist[30] == 0.0  # (5, 0, 0) is the sliver's vertex; face 13 (zero area, the same vertex) takes no part
    assert (face != 13).all()
    assert info["max_dist2_index"] == int(np.flatnonzero(Q[:, 0] == 1e3)[0])


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])  # a partial wave, a full wave and one more; more than one block
def test_the_planted_mesh_at_wave_and_block_edges(fg, gpu_required, planted, nq):
    """the list repeated and permuted to nq queries: wave tails, and duplicates of a query inside one wave"""
    V, T, Q = planted
    rng = np.random.default_rng(nq)
    rows = np.resize(rng.permutation(len(Q)), nq) if nq > 1 else np.array([0])
    got = check(fg, V, T, Q[rows], f"planted, nq = {nq}")
    ref = fg.mesh_distance(V, T, Q, return_map=True)
    for a, b in zip(got[:5], ref[:5]):
        assert a.tobytes() == b[rows].tobytes()  # a query's answer does not depend on its neighbours in the call


# ---- random soups ------------------------------------------------------------------------------------------------------------------------------
def soup_queries(V, n, seed):
    """half in the mesh's box, half in a box three times as wide about the same centre"""
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0).astype(f64), V.max(0).astype(f64)
    mid, half = (lo + hi) / 2.0, (hi - lo) / 2.0
    inner = mid + rng.uniform(-1.0, 1.0, (n // 2, 3)) * half
    outer = mid + rng.uniform(-3.0, 3.0, (n - n // 2, 3)) * half
    return np.concatenate([inner, outer]).astype(f32)


# one leaf, two faces, a leaf less one, a full leaf, the first split, three leaves with a partly empty last one, 65 leaves (seven levels, most of
# the last level's slots empty), 625 leaves
@pytest.mark.parametrize("nf", [1, 2, LEAF - 1, LEAF, LEAF + 1, 2 * LEAF + 1, 64 * LEAF + 1, 5000])
def test_random_soups_match_the_restatement(fg, gpu_required, nf):
    V, T = mr.random_mesh(nf, seed=300 + nf)
    Q = soup_queries(V, 4097, nf)
    info = check(fg, V, T, Q, f"soup, nf = {nf}")[5]
    assert info["faces"] == nf and info["tree_depth"] == {1: 0, 2: 0, LEAF - 1: 0, LEAF: 0, LEAF + 1: 1, 2 * LEAF + 1: 2, 64 * LEAF + 1: 7, 5000: 10}[nf]


# ---- where the bound falls late ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    return mr.bumpy_icosphere(3)


def test_identical_queries_vertex_queries_and_a_far_corner(fg, gpu_required, sphere):
    V, T = sphere
    same = np.tile(np.array([[0.3, -0.2, 0.1]], f32), (200, 1))
    got = check(fg, V, T, same, "identical queries")
    assert len(set(got[1].tolist())) == 1 and len(set(_bits(got[0]).tolist())) == 1
    on_vertices = V[T.reshape(-1)[:1000]]
    got = check(fg, V, T, on_vertices, "queries on vertices")
    assert (got[0] == 0.0).all() and (got[3] >= 4).all() and (got[4] == 0).all()  # dist2 == 0 everywhere, on a vertex, on the plane
    lowest = np.array([np.flatnonzero((T == v).any(1))[0] for v in T.reshape(-1)[:1000]])
    assert np.array_equal(got[1], lowest)  # of the faces that share the vertex, the lowest index
    rng = np.random.default_rng(8)
    cornered = (V.astype(f64) * 0.01 + [10.0, 10.0, 10.0]).astype(f32)  # the mesh in one corner
    far = rng.uniform(-10.0, -9.0, (500, 3)).astype(f32)  # the queries in the opposite one: every box is about as far as every other
    check(fg, cornered, T, far, "a far corner")


# ---- the walk against no walk, at a size numpy does not reach -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sphere", "soup"])
def test_the_tree_returns_the_bytes_of_brute_force(fg, gpu_required, kind):
    """20 000 faces x 20 000 queries on the device, with and without the tree: a margin too small for the rounding of the seven-region
    arithmetic would skip a face that wins or ties somewhere among 4e8 pairs"""
    if kind == "sphere":
        V, T = mr.bumpy_icosphere(5)  # 20 480 faces
        rng = np.random.default_rng(5)
        near = V[rng.integers(0, len(V), 14000)].astype(f64) * rng.uniform(0.97, 1.03, (14000, 1))  # about the surface
        Q = np.concatenate([near, rng.uniform(-2.0, 2.0, (6000, 3))]).astype(f32)
    else:
        rng = np.random.default_rng(77)
        V = rng.normal(size=(30000, 3)).astype(f32)
        T = rng.integers(0, len(V), (20000, 3)).astype(np.uint32)  # (a face that repeats a vertex has no area and takes no part)
        Q = soup_queries(V, 20000, 78)
    tree = fg.mesh_distance(V, T, Q, return_map=True)
    brute = fg.mesh_distance(V, T, Q, return_map=True, brute=True)
    same_bytes(tree, brute)
    assert tree[5]["tree_depth"] == 12 and tree[5]["faces"] + tree[5]["zero_area"] == len(T) and tree[5]["zero_area"] <= 5
    rows = np.random.default_rng(1).permutation(len(Q))[:64]  # and a sample of it against numpy
    want = md.mesh_distance(V, T, Q[rows])
    assert np.array_equal(tree[1][rows], want[1]) and np.array_equal(_bits(tree[5]["dist2"][rows]), _bits(want[0]))


# ---- determinism, resources, the refusal on the device ---------------------------------------------------------------------------------------
def test_calls_are_functions_of_their_inputs_and_leave_nothing_behind(fg, gpu_required, planted, sphere):
    V, T = sphere
    Q = soup_queries(V, 1000, 4)
    before = fg.live_resources()
    a = fg.mesh_distance(V, T, Q, return_map=True)
    b = fg.mesh_distance(V, T, Q, return_map=True)
    same_bytes(a, b)
    assert fg.mesh_distance(V, T, Q).tobytes() == a[0].tobytes()  # the optional outputs change nothing
    assert fg.live_resources() == before
    flat = np.zeros((6, 3), f32)
    flat[:, 0] = np.arange(6)  # six points on a line: every face has area 0
    with pytest.raises(fg.FgoicpError) as e:
        fg.mesh_distance(flat, np.array([[0, 1, 2], [3, 4, 5], [1, 1, 1]], np.uint32), Q)
    assert e.value.status == INVALID_ARG and "fgoicp_mesh_distance: the mesh has no area" in str(e.value)
    with pytest.raises(fg.FgoicpError) as e:
        fg.mesh_distance(V, T, Q, device=99)
    assert e.value.status == INVALID_ARG and "device ordinal out of range" in str(e.value)
    assert fg.live_resources() == before


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(fg, sphere):
    """as tests/test_gpu_mesh.py: 3000 target samples of the bumpy sphere (1280 faces) with their face normals; 400 source samples of another
    seed, moved so that R_GT src + T_GT lies on the mesh"""
    V, T = sphere
    assert len(T) == 1280
    tgt, normals = fg.sample_mesh(V, T, 3000, seed=1, return_map=True)[:2]
    on_mesh = fg.sample_mesh(V, T, 400, seed=2)
    src = ((on_mesh.astype(f64) - T_GT) @ R_GT).astype(f32)  # R_GT^T (q - T_GT)
    return dict(V=V, T=T, tgt=tgt, normals=normals, src=src, on_mesh=on_mesh)


def _true_pose_bound(pair):
    """Three fp32 roundings lie between a point of a face and the query the device sees: the sample itself (fgoicp_mesh_sample rounds the
    fp64 point once), the source point (R_GT^T (q - T_GT), rounded once), and the moved point (R p + t in fp64, rounded once by
    fg.mesh_deviation).  Each moves a point by at most half a unit in the last place per axis, 2^-24 of its coordinate, sqrt(3) 2^-24 of
    the largest |coordinate| in Euclidean length; a rotation does not lengthen an error.  k = 3.  The fp64 operations in between (a
    3 x 3 product, R_GT orthogonal to 1e-16) add 2^-45 of the same measure at most, written next to the 3."""
    big = max(float(np.abs(pair[k]).max()) for k in ("on_mesh", "src"))
    return (3.0 * 2.0 ** -24 + 2.0 ** -45) * np.sqrt(3.0) * big


def test_deviation_at_the_true_pose_is_rounding(fg, gpu_required, pair):
    dist = fg.mesh_deviation(pair["V"], pair["T"], pair["src"], R_GT, T_GT)
    bound = _true_pose_bound(pair)
    print(f"true pose: largest deviation {dist.max():.3e}, bound {bound:.3e}")
    assert dist.shape == (400,) and dist.max() <= bound


def test_deviation_after_a_registration_is_bounded_by_the_pose_error(fg, gpu_required, pair):
    """|R p + t - (R_GT p + T_GT)| <= |R - R_GT| |p| + |t - T_GT| <= e_rot |p| + e_t (a chord is shorter than its arc), and R_GT p + T_GT
    lies on the mesh to the rounding of the test above: every deviation is at most e_rot max|p| + e_t + that rounding."""
    s = fg.FastGoICP(pair["tgt"], pair["src"], 0.05, 1e-3)
    try:
        R, t = s.run()
        s.set_target_normals(pair["normals"])
        fine = s.refine_plane(k=4)
    finally:
        s.close()
    reach = float(np.linalg.norm(pair["src"].astype(f64), axis=1).max())
    rms = []
    for label, (Rx, tx) in (("search", (R, t)), ("refined", (fine.R, fine.t))):
        e_rot, e_t = _errors(Rx, tx)
        dist, face, closest, region, side, info = fg.mesh_deviation(pair["V"], pair["T"], pair["src"], Rx, tx, return_map=True)
        bound = e_rot * reach + e_t + _true_pose_bound(pair)
        rms.append(float(np.sqrt((dist ** 2).mean())))
        print(f"{label}: e_rot {e_rot:.3e} rad, e_t {e_t:.3e}; largest deviation {dist.max():.3e} <= {bound:.3e}; rms {rms[-1]:.3e}; sides {np.bincount(side + 1, minlength=3).tolist()}")
        assert dist.max() <= bound
        assert dist.max() == np.sqrt(info["max_dist2"]) and dist[info["max_dist2_index"]] == dist.max()
    assert rms[1] <= rms[0]


def test_cli_writes_the_deviation_map(fg, gpu_required, pair, tmp_path):
    """io.deviation with an ascii PLY target and params.refine = "plane": the log line, one row per source point, and the distance column
    against fg.mesh_deviation at the pose read back from out.toml's [refined] table.

    The tolerance.  out.toml prints the pose with 9 significant digits, and 9 significant digits name an fp32 number uniquely: read back
    into fp32 the pose is the CLI's own, bit for bit; so are the source points (written and read with 9 digits).  The CLI and
    fg.mesh_deviation then form the same moved points in the same arithmetic and ask the same call: face, side and region must be EQUAL,
    and the distance column differs from fg.mesh_deviation's only by its own printing, 9 significant digits: at most 5e-9 of the value
    (half a unit of the ninth digit of a number that may start with 1)."""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    V, T, src = pair["V"], pair["T"], pair["src"]
    mr.write_ply(tmp_path / "mesh.ply", V, T.tolist())
    with open(tmp_path / "src.txt", "w") as f:
        f.write(f"{len(src)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in src))
    (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/mesh.ply"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/out.toml"\ndeviation = "{tmp_path}/dev.txt"\n'
                                     '[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\ntarget_mesh_points = 2000\nrefine = "plane"\n')
    p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=300)
    log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)
    assert p.returncode == 0, log[-2000:]
    line = [ln.strip() for ln in log.splitlines() if "Deviation (source -> target mesh):" in ln]
    assert len(line) == 1, log[-2000:]
    seen = int(re.search(r"Source point cloud \((\d+)\) loaded", log).group(1))  # the CLI keeps at most half of a source file (params.source_subsample, the reference's clamp)
    assert 0 < seen <= len(src)
    assert f"Deviation (source -> target mesh): {seen} points, {len(T)} triangles (0 zero-area), rms " in line[0] and ", max " in line[0]
    out = (tmp_path / "out.toml").read_text()
    num = r"[-+0-9.eE]+"
    refined = out[out.index("[refined]"):]
    R = np.array([[float(x) for x in row] for row in re.findall(rf"\[({num}), ({num}), ({num})\],", refined)][:3]).astype(f32)
    t = np.array([float(x) for x in re.search(rf"translation = \[({num}), ({num}), ({num})\]", refined).groups()]).astype(f32)
    text = (tmp_path / "dev.txt").read_text().splitlines()
    assert text[0].startswith(f"# deviation: points = {seen}, triangles = {len(T)}, zero_area = 0, mean = ") and text[1] == "# x y z face distance side region"
    rows = np.array([[float(x) for x in ln.split()] for ln in text[2:]])
    assert rows.shape == (seen, 7)  # one row per registered source point
    index = {p.tobytes(): i for i, p in enumerate(src)}
    kept = np.array([index[p.tobytes()] for p in rows[:, :3].astype(f32)])  # the points the registration saw, in the file's units: rows of the file
    assert (np.diff(kept) > 0).all()  # ... in the file's order
    dist, face, closest, region, side, info = fg.mesh_deviation(V, T, src[kept], R, t, return_map=True)
    rel = np.abs(rows[:, 4] - dist) / np.maximum(dist, np.finfo(f64).tiny)
    print(f"CLI: distance column within {rel.max():.3e} (relative) of fg.mesh_deviation at the printed pose; {line[0]}")
    assert (rel <= 5e-9).all()
    assert np.array_equal(rows[:, 3], face) and np.array_equal(rows[:, 5], side) and np.array_equal(rows[:, 6], region)
    head = dict(kv.split(" = ") for kv in text[0][len("# deviation: "):].split(", "))
    assert float(head["max"]) == pytest.approx(dist.max(), rel=5e-9) and float(head["rms"]) == pytest.approx(np.sqrt((dist ** 2).mean()), rel=1e-8)
    assert float(head["mean"]) == pytest.approx(dist.mean(), rel=1e-8)
    assert [int(head[k]) for k in ("negative", "on_plane", "positive")] == [int((side == v).sum()) for v in (-1, 0, 1)]
    rms, mx = float(re.search(rf"rms ({num}),", line[0]).group(1)), float(re.search(rf"max ({num})$", line[0]).group(1))
    assert rms == pytest.approx(float(head["rms"]), rel=1e-5) and mx == pytest.approx(float(head["max"]), rel=1e-5)  # the log prints 6 digits
