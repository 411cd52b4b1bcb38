"""The command-line tool's two runners over one configuration: a lone run (-c) and a batch of one (--batch) go through the same preparation
path (csrc/cli/prepare.hpp) and the same refinement outcome and writers (csrc/cli/main.cpp).  One config with every preparation stage on
for both clouds, params.refine = "plane" and three output files; pinned: the stage log lines come in the same order — stage by stage, the
target before the source — the prepared clouds are the same points, and the result files have the same tables and keys.  The poses of the
two runs are compared elsewhere (tests/test_gpu_batch_refine.py, tests/test_gpu_batch*.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ["Mesh sampling", "Voxel grid", "Outlier filter", "Plane filter", "Cluster filter", "Farthest-point sampling"]


def _ellipsoid(centre, radii, rings=8, segments=16):
    """a closed UV ellipsoid: vertices and triangles"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, rings):
        th = np.pi * i / rings
        v += [(np.sin(th) * np.cos(2 * np.pi * j / segments), np.sin(th) * np.sin(2 * np.pi * j / segments), np.cos(th)) for j in range(segments)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * segments + j % segments  # noqa: E731
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(segments)]
    for i in range(1, rings - 1):
        for j in range(segments):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    f += [(len(v) - 1, ring(rings - 1, j + 1), ring(rings - 1, j)) for j in range(segments)]
    return np.asarray(v) * np.asarray(radii) + np.asarray(centre), np.asarray(f)


def _scene():
    """a blob (an ellipsoid with a bump) standing on a plane patch: about 600 surface samples put two thirds on the blob"""
    parts = [(np.array([(-0.6, -0.6, 0.0), (0.6, -0.6, 0.0), (0.6, 0.6, 0.0), (-0.6, 0.6, 0.0)]), np.array([(0, 1, 2), (0, 2, 3)])),
             _ellipsoid((0.05, -0.1, 0.5), (0.45, 0.35, 0.5)), _ellipsoid((0.4, 0.1, 0.8), (0.2, 0.2, 0.2), rings=4, segments=8)]
    vertices, faces, base = [], [], 0
    for v, f in parts:
        vertices.append(v)
        faces.append(f + base)
        base += len(v)
    return np.concatenate(vertices), np.concatenate(faces)


def _write_ply(path, v, f):
    path.write_text(f"ply\nformat ascii 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nelement face {len(f)}\n"
                    "property list uchar int vertex_indices\nend_header\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v) + "".join(f"3 {a} {b} {c}\n" for a, b, c in f))


def _config(tmp_path, tag):
    side = "{0}_mesh_points = 600\n{0}_voxel = 0.03\n{0}_outlier_knn = 8\n{0}_outlier_std = 2.0\n{0}_plane_distance = 0.02\n{0}_cluster_eps = {1}\n{0}_cluster_min_points = 4\n{0}_points = {2}\n"
    (tmp_path / f"{tag}.toml").write_text(
        f'[io]\ntarget = "{tmp_path}/tgt.ply"\nsource = "{tmp_path}/src.ply"\noutput = "{tmp_path}/{tag}_out.toml"\nalignment = "{tmp_path}/{tag}_align.txt"\n'
        f'visualization = "{tmp_path}/{tag}_vis.ply"\n[params]\nlut_resolution = 0.05\nmse_threshold = 0.01\nseed = 5\nrefine = "plane"\n'
        + side.format("target", 0.25, 350) + side.format("source", 0.35, 150))
    return str(tmp_path / f"{tag}.toml")


def _tables(path):
    """the tables of a result file and the keys of each, in file order"""
    tables = []
    for line in path.read_text().splitlines():
        if line.startswith("["):
            tables.append((line.strip("[]"), []))
        elif re.match(r"[a-z_]+ = ", line):
            tables[-1][1].append(line.split(" = ")[0])
    return tables


@pytest.mark.gpu
def test_a_lone_run_and_a_batch_of_one_prepare_refine_and_write_alike(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    v, f = _scene()
    a = np.deg2rad(8.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    _write_ply(tmp_path / "tgt.ply", v, f)
    _write_ply(tmp_path / "src.ply", v @ R.T + np.array([0.05, -0.03, 0.04]), f)
    lone, batch = _config(tmp_path, "lone"), _config(tmp_path, "batch")
    (tmp_path / "list.txt").write_text(os.path.basename(batch) + "\n")
    for tag, args in (("lone", ["-c", lone]), ("batch", ["--batch", str(tmp_path / "list.txt")])):
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        log = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
        assert p.returncode == 0, log[-3000:]
        stages = [m.groups() for m in (re.search(r"\] (" + "|".join(STAGES) + r") \((target|source)\): ", ln) for ln in log.splitlines()) if m]
        print(tag, *[ln for ln in log.splitlines() if any(s in ln for s in STAGES) or "refinement:" in ln], sep="\n")
        assert stages == [(s, side) for s in STAGES for side in ("target", "source")], log[-3000:]
        assert len([ln for ln in log.splitlines() if "Point-to-plane refinement: " in ln]) == 1
    # the prepared clouds are the same: the source rows of io.alignment, the target rows of io.visualization
    xyz = {tag: [ln.split()[:3] for ln in (tmp_path / f"{tag}_align.txt").read_text().splitlines()[2:]] for tag in ("lone", "batch")}
    assert 0 < len(xyz["lone"]) <= 150 and xyz["lone"] == xyz["batch"]
    blue = {tag: [ln for ln in (tmp_path / f"{tag}_vis.ply").read_text().splitlines() if ln.endswith(" 40 90 220")] for tag in ("lone", "batch")}
    assert 0 < len(blue["lone"]) <= 350 and blue["lone"] == blue["batch"]
    # ... and the result files hold the same tables with the same keys in the same order
    tables = _tables(tmp_path / "lone_out.toml")
    assert [t[0] for t in tables] == ["result", "stats", "refined"] and all(t[1] for t in tables)
    assert tables == _tables(tmp_path / "batch_out.toml")
