"""Point-to-mesh refinement on the device (fgoicp_mesh_moments, fgoicp_mesh_refine; fg.mesh_moments, fg.refine_to_mesh; params.refine = "mesh")
against the numpy restatement of its definition (tests/mesh_refine_restatement.py; include/fgoicp_amd.h), which tests every face for every
point.  Per point everything is compared in bits; the sums against math.fsum within the bound of n fp64 additions and, in the order the
call returns, against the restatement of the device's reduction in bits; the loop against its own definition, one step at a time."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.np_restatement import fixed_order_sum
from tests import mesh_distance_restatement as md
from tests import mesh_refine_restatement as rr
from tests import mesh_restatement as mr
from tests.test_gpu_mesh_distance import planted_queries, soup_queries

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
f32, f64 = np.float32, np.float64
PER_POINT = ("face", "closest", "dist2", "region", "direction", "residual", "weight", "counted", "order")


def rotation(axis, angle):
    k = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


R_POSE = rotation((1.0, 2.0, 2.0), math.radians(3.0)).astype(f32)  # 3 degrees about (1, 2, 2) / 3
T_POSE = np.array([0.02, -0.01, 0.015], f32)
CONFIGS = [dict(), dict(loss="tukey", loss_scale=0.05), dict(loss="huber", loss_scale=0.01, max_distance=0.5), dict(loss="cauchy", loss_scale=2.0, max_distance=1e-3)]


def pulled_back(Q):
    """p with R_POSE p + T_POSE close to q: the moved points are generic fp32 numbers"""
    return ((np.asarray(Q, f64) - T_POSE.astype(f64)) @ R_POSE.astype(f64)).astype(f32)


def angle_between(Ra, Rb):
    return 2.0 * math.asin(min(1.0, float(np.linalg.norm(np.asarray(Ra, f64) - np.asarray(Rb, f64))) / (2.0 * math.sqrt(2.0))))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_result(a, b, per_point=True):
    """two results of the same evaluation: the sums and, per point, every array"""
    for key in ("correspondences", "points", "weight_sum", "sum_dist2", "max_dist2", "faces", "zero_area", "tree_depth"):
        assert getattr(a, key) == getattr(b, key), key
    assert a.m.tobytes() == b.m.tobytes()
    for key in PER_POINT if per_point else ():
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key


def device_rows(got, P, R, t):
    """the 30 summands of every point, restated from the DEVICE's per-point outputs: the search is not repeated"""
    x = rr.moved(P, R, t).astype(f64)
    weighted = got.loss != "none"
    return rr.rows30(rr.terms28(x, got.direction, got.residual, got.weight if weighted else None), got.weight, got.dist2, got.counted)


def sums_of(got):
    return np.concatenate([got.m, [got.weight_sum, got.sum_dist2]])


def check_sums(got, P, R, t, label):
    rows = device_rows(got, P, R, t)
    n = len(rows)
    have = sums_of(got)
    assert got.correspondences == int(got.counted.sum()), label
    worst = 0.0
    for k in range(30):
        exact, total = math.fsum(rows[:, k]), math.fsum(np.abs(rows[:, k]))
        bound = (n - 1) * 2.0 ** -53 * total * (1.0 + 2.0 ** -40)
        worst = max(worst, abs(have[k] - exact) / bound if bound > 0.0 else 0.0)
        assert abs(have[k] - exact) <= bound, (label, k, have[k], exact, bound)
    in_order = fixed_order_sum(rows[got.order.astype(np.int64)])  # block rows of 256 threads, the fold of 1024: the device's shape
    assert np.array_equal(_bits(have), _bits(in_order)), label
    print(f"{label}: {n} points, {got.correspondences} counted; the worst sum uses {worst:.3f} of its bound; the 30 sums are the fixed-order restatement's bits")


def check_points(fg, V, T, P, label, configs=CONFIGS, R=R_POSE, t=T_POSE):
    dist, face, closest, region, side, info = fg.mesh_deviation(V, T, P, R, t, return_map=True)
    for cfg in configs:
        got = fg.mesh_moments(V, T, P, R, t, return_map=True, **cfg)
        want = rr.per_point(V, T, P, R, t, cfg.get("max_distance"), cfg.get("loss"), cfg.get("loss_scale"))
        # ... what fgoicp_mesh_distance returns for the moved point, byte for byte
        assert got.face.tobytes() == face.tobytes() and got.closest.tobytes() == closest.tobytes() and got.region.tobytes() == region.tobytes(), (label, cfg)
        assert got.dist2.tobytes() == info["dist2"].tobytes(), (label, cfg)
        assert np.array_equal(got.face, want["face"]) and np.array_equal(_bits(got.dist2), _bits(want["dist2"])), (label, cfg)
        assert np.array_equal(got.counted, want["counted"]) and got.max_dist2 == want["max_dist2"], (label, cfg)
        for key, ref in (("direction", "g"), ("residual", "residual"), ("weight", "weight")):
            assert np.array_equal(_bits(getattr(got, key)), _bits(want[ref])), (label, cfg, key)
        assert sorted(got.order.tolist()) == list(range(len(P)))
        assert (got.faces, got.zero_area, got.tree_depth, got.leaf_faces, got.triangles, got.vertices) == (info["faces"], info["zero_area"], info["tree_depth"], info["leaf_faces"],
                                                                                                            len(T), len(V))
        check_sums(got, P, R, t, f"{label} {cfg}")
        brute = fg.mesh_moments(V, T, P, R, t, return_map=True, brute=True, **cfg)
        assert brute.flags == 1 and got.flags == 0
        same_result(got, brute)
        again = fg.mesh_moments(V, T, P, R, t, return_map=True, **cfg)
        same_result(got, again)
        assert again.raw == got.raw
        plain = fg.mesh_moments(V, T, P, R, t, **cfg)  # the per-point outputs change nothing
        same_result(got, plain, per_point=False)
    return got


# ---- 1. per point, in bits -------------------------------------------------------------------------------------------------------------------
def test_the_planted_mesh_per_point_and_in_sum(fg, gpu_required):
    V, T = mr.planted_mesh()
    P = pulled_back(planted_queries())
    got = check_points(fg, V, T, P, "planted")
    assert got.faces == 14 and got.zero_area == 1 and got.tree_depth == 1


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 257])  # a lane, a partial wave, a full wave and one more; more than one block
def test_the_planted_mesh_at_lane_wave_and_block_edges(fg, gpu_required, ns):
    V, T = mr.planted_mesh()
    Q = planted_queries()
    rng = np.random.default_rng(ns)
    rows = np.resize(rng.permutation(len(Q)), ns) if ns > 1 else np.array([0])
    check_points(fg, V, T, pulled_back(Q[rows]), f"planted, ns = {ns}", configs=CONFIGS[:2])


@pytest.mark.parametrize("nf", [md.LEAF, md.LEAF + 1])  # one full leaf; the first split
def test_a_leaf_and_the_first_split(fg, gpu_required, nf):
    V, T = mr.random_mesh(nf, seed=300 + nf)
    got = check_points(fg, V, T, pulled_back(soup_queries(V, 130, nf)), f"soup, nf = {nf}", configs=CONFIGS[:2])
    assert got.tree_depth == nf - md.LEAF


# ---- 2. the sums ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    return mr.bumpy_icosphere(2)


@pytest.fixture(scope="module")
def scan(sphere):
    """600 points of the surface, pulled back by the pose: (R_POSE, T_POSE) is the truth"""
    V, T = sphere
    assert len(T) == 320
    return pulled_back(mr.sample(V, T, 600, seed=3)[0])


def test_the_sums_on_the_sphere(fg, gpu_required, sphere, scan):
    V, T = sphere
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    check_points(fg, V, T, scan, "sphere at the start", configs=CONFIGS[:3], R=eye, t=zero)


def test_the_sums_past_the_folds_first_lap(fg, gpu_required, sphere):
    """262 401 points: 1026 block rows, so two threads of the fold add two rows each"""
    V, T = sphere
    rng = np.random.default_rng(11)
    ns = 262401
    P = pulled_back(V[rng.integers(0, len(V), ns)].astype(f64) * rng.uniform(0.9, 1.1, (ns, 1)))
    for cfg in (dict(), dict(loss="tukey", loss_scale=0.05, max_distance=0.08)):
        got = fg.mesh_moments(V, T, P, R_POSE, T_POSE, return_map=True, **cfg)
        assert 0 < got.correspondences <= ns and (got.correspondences == ns) == (not cfg)
        check_sums(got, P, R_POSE, T_POSE, f"ns = {ns} {cfg}")
        same_result(got, fg.mesh_moments(V, T, P, R_POSE, T_POSE, return_map=True, brute=True, **cfg))


# ---- 3. the loop is its definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [dict(), dict(loss="tukey", loss_scale=0.03)])
def test_every_step_of_the_loop_is_a_step_from_the_moments(fg, gpu_required, sphere, scan, cfg):
    V, T = sphere
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    runs = [fg.refine_to_mesh(V, T, scan, eye, zero, max_iter=k, conv_thr=0.0, **cfg) for k in range(6)]
    assert runs[0].iterations == 0 and runs[0].rank == 0 and np.array_equal(runs[0].R, eye) and np.array_equal(runs[0].t, zero)
    for k in range(5):
        at = fg.mesh_moments(V, T, scan, runs[k].R, runs[k].t, **cfg)
        for key in ("correspondences", "weight_sum", "rms_distance"):
            assert getattr(runs[k], key) == getattr(at, key), (k, key)
        assert runs[k].mesh_rmse == float(np.sqrt(f64(at.m[27]) / f64(at.weight_sum)))
        xi, rank = fg.plane_step_from_moments(at.correspondences, at.m)
        R, t = fg.plane_apply_step(runs[k].R, runs[k].t, xi)
        assert runs[k + 1].iterations == k + 1 and runs[k + 1].rank == rank == 6
        assert runs[k + 1].R.tobytes() == R.tobytes() and runs[k + 1].t.tobytes() == t.tobytes(), k
    assert runs[5].loss == cfg.get("loss", "none") and runs[5].loss_scale == cfg.get("loss_scale", 0.0) and not runs[5].scale_estimated
    print(f"{cfg}: rms_distance " + " ".join(f"{r.rms_distance:.3e}" for r in runs))


# ---- 4. it converges ---------------------------------------------------------------------------------------------------------------------------
def test_the_loop_converges_to_the_true_pose(fg, gpu_required, sphere, scan):
    V, T = sphere
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    start = fg.mesh_moments(V, T, scan, eye, zero)
    fine = fg.refine_to_mesh(V, T, scan, eye, zero)
    want = rr.refine(fg, V, T, scan, eye, zero)
    e_rot, e_t = angle_between(fine.R, R_POSE), float(np.linalg.norm(fine.t.astype(f64) - T_POSE))
    print(f"rms_distance {start.rms_distance:.3e} -> {fine.rms_distance:.3e} in {fine.iterations} iterations; {e_rot:.3e} rad and {e_t:.3e} from the truth; "
          f"the restatement's loop: {want['iterations']} iterations, rms {want['rms_distance']:.3e}, {angle_between(fine.R, want['R']):.3e} rad and "
          f"{float(np.linalg.norm(fine.t.astype(f64) - want['t'])):.3e} from the device's")
    assert fine.iterations <= 6 and fine.rank == 6 and fine.correspondences == len(scan) and fine.weight_sum == len(scan)
    assert fine.rms_distance <= 1e-5 and e_rot <= 1e-5 and e_t <= 1e-5
    assert angle_between(fine.R, want["R"]) <= 1e-5 and float(np.linalg.norm(fine.t.astype(f64) - want["t"])) <= 1e-5
    dist = fg.mesh_deviation(V, T, scan, fine.R, fine.t)  # the number minimised is the number the deviation map reports
    assert fine.rms_distance == pytest.approx(float(np.sqrt((dist ** 2).mean())), rel=1e-12)


def test_a_tukey_loss_ignores_displaced_points(fg, gpu_required, sphere, scan):
    V, T = sphere
    rng = np.random.default_rng(5)
    noisy = scan.astype(f64) + rng.normal(size=scan.shape) * 0.002
    out = rng.permutation(len(scan))[:len(scan) // 5]
    noisy[out] += rng.normal(size=(len(out), 3)) * 0.3
    noisy = noisy.astype(f32)
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    plain = fg.refine_to_mesh(V, T, noisy, eye, zero)
    tukey = fg.refine_to_mesh(V, T, noisy, eye, zero, loss="tukey")
    e_plain, e_tukey = angle_between(plain.R, R_POSE), angle_between(tukey.R, R_POSE)
    print(f"20 % displaced: plain {e_plain:.3e} rad off in {plain.iterations} iterations, tukey {e_tukey:.3e} rad off in {tukey.iterations} (scale {tukey.loss_scale:.3e}, "
          f"estimated {tukey.scale_estimated}; weight sum {tukey.weight_sum:.1f} of {tukey.correspondences})")
    assert tukey.scale_estimated and tukey.loss == "tukey" and tukey.loss_scale > 0.0
    assert e_tukey <= 0.02 and 3.0 * e_tukey <= e_plain and tukey.weight_sum < tukey.correspondences


# ---- 5. rank -----------------------------------------------------------------------------------------------------------------------------------
def test_a_plane_constrains_three_motions_and_takes_one_step(fg, gpu_required):
    V = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [10.0, 10.0, 0.0], [-10.0, 10.0, 0.0]], f32)
    T = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    rng = np.random.default_rng(2)
    P = np.concatenate([rng.uniform(-1.0, 1.0, (300, 2)), rng.uniform(0.2, 0.4, (300, 1))], 1).astype(f32)
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    at = fg.mesh_moments(V, T, P, eye, zero, return_map=True)
    assert (at.region == 0).all() and np.array_equal(at.direction, np.tile([0.0, 0.0, 1.0], (300, 1)))
    xi, rank = fg.plane_step_from_moments(at.correspondences, at.m)
    assert rank == 3 and max(abs(xi[2]), abs(xi[3]), abs(xi[4])) < 1e-10  # w_z, v_x, v_y: the motions inside the plane
    fine = fg.refine_to_mesh(V, T, P, eye, zero)
    R, t = fg.plane_apply_step(eye, zero, xi)
    assert fine.iterations == 1 and fine.rank == 3 and fine.R.tobytes() == R.tobytes() and fine.t.tobytes() == t.tobytes()
    assert fine.rms_distance < at.rms_distance


# ---- the refusals on the device, resources --------------------------------------------------------------------------------------------------------
def test_refusals_behind_the_device_and_nothing_left_behind(fg, gpu_required, sphere, scan):
    V, T = sphere
    eye, zero = np.eye(3, dtype=f32), np.zeros(3, f32)
    before = fg.live_resources()
    fg.refine_to_mesh(V, T, scan, eye, zero, max_iter=2, loss="huber")
    fg.mesh_moments(V, T, scan, eye, zero, return_map=True)
    assert fg.live_resources() == before
    flat = np.zeros((6, 3), f32)
    flat[:, 0] = np.arange(6)  # six points on a line: every face has area 0
    for call, name in ((fg.mesh_moments, "fgoicp_mesh_moments"), (fg.refine_to_mesh, "fgoicp_mesh_refine")):
        with pytest.raises(fg.FgoicpError) as e:
            call(flat, np.array([[0, 1, 2], [3, 4, 5], [1, 1, 1]], np.uint32), scan, eye, zero)
        assert e.value.status == INVALID_ARG and f"{name}: the mesh has no area" in str(e.value)
        with pytest.raises(fg.FgoicpError) as e:
            call(V, T, scan, eye, zero, device=99)
        assert e.value.status == INVALID_ARG and f"{name}: device ordinal out of range" in str(e.value)
    on_surface = mr.sample(V, T, 64, seed=9)[0]
    exact = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [10.0, 10.0, 0.0], [-10.0, 10.0, 0.0]], f32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    flat_points = np.concatenate([on_surface[:, :2], np.zeros((64, 1), f32)], 1)  # on the quad: every residual is 0
    with pytest.raises(fg.FgoicpError) as e:
        fg.refine_to_mesh(*exact, flat_points, eye, zero, loss="tukey")
    assert e.value.status == INVALID_ARG and "fgoicp_mesh_refine: the median residual is 0, there is no scale to estimate: pass a scale" in str(e.value)
    assert fg.live_resources() == before


# ---- 6. the command-line tool --------------------------------------------------------------------------------------------------------------------
NUM = r"[-+0-9.eE]+"


def _table(text, name):
    """(R (3, 3) float32, t (3,) float32, the rest of the table as a dict of strings) of out.toml's [name]"""
    body = text[text.index(f"[{name}]"):]
    body = body[:body.index("\n[", 1)] if "\n[" in body[1:] else body
    R = np.array([[float(x) for x in row] for row in re.findall(rf"\[({NUM}), ({NUM}), ({NUM})\],", body)][:3]).astype(f32)
    t = np.array([float(x) for x in re.search(rf"translation = \[({NUM}), ({NUM}), ({NUM})\]", body).groups()]).astype(f32)
    keys = dict(ln.split(" = ") for ln in body.splitlines() if " = " in ln and not ln.startswith(("rotation", "translation")))
    return R, t, keys


def test_cli_refines_against_the_target_files_mesh(fg, gpu_required, tmp_path):
    """params.refine = "mesh" with io.deviation: the log line, the [refined] table, the deviation map taken at the refined pose — its rms
    is the table's rms_distance — and the refined pose against fg.refine_to_mesh from the printed best transform over the printed points
    (9 significant digits name an fp32 number uniquely, so both are the CLI's own bits and the pose must be EQUAL).  The same config
    under --batch writes the same table."""
    from tests.test_gpu_mesh import R_GT, T_GT
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    V, T = mr.bumpy_icosphere(3)
    on_mesh = fg.sample_mesh(V, T, 400, seed=2)
    src = ((on_mesh.astype(f64) - T_GT) @ R_GT).astype(f32)
    mr.write_ply(tmp_path / "mesh.ply", V, T.tolist())
    with open(tmp_path / "src.txt", "w") as f:
        f.write(f"{len(src)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in src))
    (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/mesh.ply"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/out.toml"\ndeviation = "{tmp_path}/dev.txt"\n'
                                     '[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\ntarget_mesh_points = 2000\nrefine = "mesh"\nrefine_knn = 1\n')
    (tmp_path / "list.txt").write_text("c.toml\n")
    tables = []
    for args, prefix in ((["-c", str(tmp_path / "c.toml")], ""), (["--batch", str(tmp_path / "list.txt")], "Pair 0: ")):
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
        log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)
        assert p.returncode == 0, log[-2000:]
        line = [ln for ln in log.splitlines() if "Point-to-mesh refinement:" in ln]
        assert len(line) == 1 and f"{prefix}Point-to-mesh refinement: " in line[0] and " iterations, rank 6, " in line[0] and "rms distance " in line[0] and "mesh RMSE " in line[0], log[-2000:]
        assert " loss" not in line[0]  # the robust suffix only with a loss
        out = (tmp_path / "out.toml").read_text()
        R0, t0, _ = _table(out, "result")
        R1, t1, keys = _table(out, "refined")
        assert list(keys) == ["mesh_rmse", "rms_distance", "iterations", "rank", "correspondences"]
        text = (tmp_path / "dev.txt").read_text().splitlines()
        head = dict(kv.split(" = ") for kv in text[0][len("# deviation: "):].split(", "))
        assert float(head["rms"]) == pytest.approx(float(keys["rms_distance"]), rel=1e-8)  # refine_distance is off: every point is counted
        pts = np.array([[float(x) for x in ln.split()[:3]] for ln in text[2:]]).astype(f32)  # the points the registration saw
        assert int(keys["correspondences"]) == len(pts) == int(head["points"])
        fine = fg.refine_to_mesh(V, T, pts, R0, t0)
        assert fine.R.tobytes() == R1.tobytes() and fine.t.tobytes() == t1.tobytes()
        assert int(keys["iterations"]) == fine.iterations and float(keys["rms_distance"]) == pytest.approx(fine.rms_distance, rel=1e-8)
        before = fg.mesh_moments(V, T, pts, R0, t0).rms_distance
        print(f"{prefix}CLI: {line[0].strip()}; rms distance {before:.3e} at the best transform -> {fine.rms_distance:.3e}")
        assert fine.rms_distance <= before
        tables.append(out[out.index("[refined]"):])
    assert tables[0] == tables[1]


def test_cli_names_the_key_when_the_mesh_has_no_area(fg, gpu_required, tmp_path):
    """the third fatal error: faces that all repeat a vertex.  The search runs on the file's vertices; the refinement's call refuses the mesh"""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    V, T = mr.bumpy_icosphere(1)
    mr.write_ply(tmp_path / "flat.ply", V, [(a, a, b) for a, b, _ in T.tolist()])
    mr.write_ply(tmp_path / "src.ply", V, None)
    (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/flat.ply"\nsource = "{tmp_path}/src.ply"\n[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n'
                                     'refine = "mesh"\n')
    p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=300)
    log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)
    assert p.returncode == 1 and 'params.refine = "mesh": status 1: fgoicp_mesh_refine: the mesh has no area' in log, log[-2000:]
