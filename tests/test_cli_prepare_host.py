"""The CLI's preparation path (fast-go-icp_amd/csrc/cli/prepare.hpp: cli::prepare_pair, the one text a lone run and every pair of a batch go
through) without a GPU: tests/host_harness/prepare_check.cpp runs it over stand-ins for the six device calls, which print their name, the
points they were given and their seed, and pass the cloud through.  Pinned here: the order of the stages (stage-major: target, then source,
stage by stage), the seeds each call takes with and without params.seed, that a stage which is off makes no call, and how a refused call
ends the process.  What the real calls compute is checked in the tests of each filter."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.5, 0.25, 0.125)]
SOURCE = [(x + 0.5, y - 0.25, z + 2.0) for x, y, z in TARGET]
MESH = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n" \
       "0.5 0.25 0.125\n1 0 0\n1 1 0\n0 1 0\n3 0 1 2\n3 0 2 3\n"
STAGES = ["mesh", "voxel", "outlier", "plane", "cluster", "farthest"]
LOG_NAMES = {"Mesh sampling": "mesh", "Voxel grid": "voxel", "Outlier filter": "outlier", "Plane filter": "plane", "Cluster filter": "cluster", "Farthest-point sampling": "farthest"}
ALL_ON = "".join(f"{side}_mesh_points = 40\n{side}_voxel = 0.25\n{side}_outlier_knn = 2\n{side}_plane_distance = 0.01\n{side}_cluster_eps = 0.5\n" for side in ("target", "source")) \
         + "target_points = 5\nsource_points = 2\n"


@pytest.fixture(scope="module")
def prepare(tmp_path_factory):
    """run(params, mesh=False, refuse=False, table=True) -> (exit code, calls [(name, points, seed or None)], the sides the stage log lines
    name [(stage, side)], {"TARGET": points, "SOURCE": points}, the whole output without colours)"""
    d = tmp_path_factory.mktemp("prepare")
    exe = d / "prepare_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(REPO, "tests", "host_harness", "prepare_check.cpp")], check=True)
    for name, pts in (("t.txt", TARGET), ("s.txt", SOURCE)):
        (d / name).write_text(f"{len(pts)}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pts))
    (d / "m.ply").write_text(MESH)

    def run(params, mesh=False, refuse=False, table=True):
        files = ("m.ply", "m.ply") if mesh else ("t.txt", "s.txt")
        (d / "c.toml").write_text(f'[io]\ntarget = "{d}/{files[0]}"\nsource = "{d}/{files[1]}"\n' + (f"[params]\n{params}" if table else ""))
        p = subprocess.run([str(exe), str(d / "c.toml")] + (["refuse"] if refuse else []), capture_output=True, text=True, timeout=60)
        out = re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)  # the logger colours its lines
        calls, logged, clouds, cloud = [], [], {}, None
        for line in out.splitlines():
            w = line.split()
            if line.startswith("CALL "):
                calls.append((w[1], int(w[2]), int(w[3]) if len(w) > 3 else None))
            elif line.startswith(("TARGET ", "SOURCE ")):
                cloud = clouds.setdefault(w[0], [])
            elif line.startswith("P "):
                cloud.append(tuple(float(v) for v in w[1:]))
            else:
                m = re.search(r"\] (" + "|".join(LOG_NAMES) + r") \((target|source)\): ", line)
                if m:
                    logged.append((LOG_NAMES[m.group(1)], m.group(2)))
        return p.returncode, calls, logged, clouds, out
    return run


def test_every_stage_runs_on_the_target_then_on_the_source_with_the_seeds_of_params_seed(prepare):
    rc, calls, logged, clouds, out = prepare("seed = 5\n" + ALL_ON, mesh=True)
    assert rc == 0, out
    assert [c[0] for c in calls] == [s for s in STAGES for _ in range(2)]
    assert logged == [(s, side) for s in STAGES for side in ("target", "source")]  # a call's log line follows it: the sides alternate, stage by stage
    seeds = {s: [c[2] for c in calls if c[0] == s] for s in STAGES}
    assert seeds["mesh"] == [5, 5] and seeds["plane"] == [5, 6]
    assert all(seeds[s] == [None, None] for s in ("voxel", "outlier", "cluster", "farthest"))
    # the samples are thinned by *_subsample as a loaded cloud is (the source's is clamped to 0.5) and every later stage sees what the one
    # before left; the farthest-point sampling, last, leaves the points asked for — the stand-in's mesh has vertex 0 only
    given = {s: [c[1] for c in calls if c[0] == s] for s in STAGES}
    assert given["mesh"] == [40, 40] and given["voxel"][0] == 40 and 2 < given["voxel"][1] <= 20
    assert all(given[s] == given["voxel"] for s in ("outlier", "plane", "cluster", "farthest"))
    assert clouds == {"TARGET": [(0.5, 0.25, 0.125)] * 5, "SOURCE": [(0.5, 0.25, 0.125)] * 2}
    assert "Target point cloud (40) loaded from" in out and f"Source point cloud ({given['voxel'][1]}) loaded from" in out


def test_without_params_seed_the_device_calls_take_seed_zero_and_the_source_plane_search_one(prepare):
    rc, calls, logged, _, out = prepare(ALL_ON, mesh=True)
    assert rc == 0, out
    assert [c[2] for c in calls if c[0] == "mesh"] == [0, 0] and [c[2] for c in calls if c[0] == "plane"] == [0, 1]
    assert logged == [(s, side) for s in STAGES for side in ("target", "source")]


def test_with_every_stage_off_no_call_is_made_and_the_clouds_are_the_files(prepare):
    rc, calls, logged, clouds, out = prepare("", table=False)  # no [params]: no clamp of the source's subsample either
    assert rc == 0 and calls == [] and logged == [], out
    assert clouds == {"TARGET": TARGET, "SOURCE": SOURCE}
    assert "Target point cloud (8) loaded from" in out and "Source point cloud (8) loaded from" in out
    rc, calls, logged, clouds, out = prepare("seed = 5\n")  # [params]: the source is thinned to at most half (utilities.hpp:101-104), in file order
    assert rc == 0 and calls == [] and logged == [], out
    assert clouds["TARGET"] == TARGET and 0 < len(clouds["SOURCE"]) <= 4
    rest = iter(SOURCE)
    assert all(p in rest for p in clouds["SOURCE"])


def test_a_cloud_with_no_more_points_than_asked_is_not_sampled(prepare):
    rc, calls, logged, clouds, out = prepare("seed = 5\ntarget_points = 8\nsource_points = 100\n")
    assert rc == 0 and calls == [], out
    assert logged == [("farthest", "target"), ("farthest", "source")]
    assert "Farthest-point sampling (target): 8 points, at most 8 asked: unchanged" in out
    assert f"Farthest-point sampling (source): {len(clouds['SOURCE'])} points, at most 100 asked: unchanged" in out
    assert clouds["TARGET"] == TARGET
    rc, calls, _, clouds, out = prepare("seed = 5\ntarget_points = 7\n")  # one below: the call is made
    assert rc == 0 and calls == [("farthest", 8, None)] and clouds["TARGET"] == TARGET[:7], out


def test_a_refused_call_ends_the_process_with_exit_code_1_and_names_the_key(prepare):
    """the path calls exit: the harness is the child process"""
    rc, calls, _, clouds, out = prepare("seed = 5\ntarget_voxel = 0.25\nsource_voxel = 0.25\n", refuse=True)
    assert rc == 1 and calls == [("voxel", 8, None)] and clouds == {}, out  # nothing runs after the refusal
    errors = [ln for ln in out.splitlines() if ln.startswith("[Error ")]
    assert len(errors) == 1 and errors[0].endswith("] params.target_voxel = 0.25: status 1: the stand-in refuses"), out
