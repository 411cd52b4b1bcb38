"""Mesh sampling on the device (fgoicp_mesh_sample, fg.sample_mesh, fg.sample_mesh_even, FastGoICP.set_target_normals, params.target_mesh_points)
against the numpy restatement of its definition (tests/mesh_restatement.py; include/fgoicp_amd.h).

The restatement is fed the device's own face areas, so that the one operation whose last bit a device may round differently — the square
root — is judged on its own (within 1 fp64 ulp of numpy's, and the test prints whether it was bit-equal) and everything behind it is compared
EXACTLY: the weights, their scan, the hashes, the multiply-high, the search, u, v and the points contain no further freedom.  The normals
divide by another square root: within 1.2e-7 absolute, two fp32 ulps of a component of a unit vector.

The kernels (csrc/device/mesh.hip) run blocks of 256 threads, four waves of 64, one thread per face or per sample."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_restatement as mr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
INFO_KEYS = ("vertices", "triangles", "samples", "zero_area", "unweighted", "weight_total", "max_area", "area")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check(fg, V, T, m, seed, label):
    pts, nrm, face, uv, area, info = fg.sample_mesh(V, T, m, seed=seed, return_map=True)
    ref_area = mr.face_area(V, T)
    ulps = np.abs(area - ref_area) / np.spacing(np.maximum(ref_area, np.finfo(np.float64).tiny))
    print(f"{label}: face_area bit-equal to numpy's: {bool(np.array_equal(_bits(area), _bits(ref_area)))} (largest difference {ulps.max():.3g} ulp)")
    assert (ulps <= 1.0).all()
    wpts, wnrm, wface, wuv, _, winfo = mr.sample(V, T, m, seed=seed, area=area)
    assert np.array_equal(face, wface)
    assert np.array_equal(_bits(uv), _bits(wuv))
    assert np.array_equal(_bits(pts), _bits(wpts))
    for key in INFO_KEYS:
        assert info[key] == winfo[key] and type(info[key]) is type(winfo[key]), (key, info[key], winfo[key])
    err = np.abs(nrm.astype(np.float64) - wnrm.astype(np.float64)).max()
    print(f"{label}: normals within {err:.3g} of numpy's")
    assert err <= 1.2e-7
    return info


# ---- bits against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 20000])  # a partial wave, a full wave and one more; more than one block
def test_the_planted_mesh_matches_the_restatement(fg, gpu_required, m):
    V, T = mr.planted_mesh()
    info = check(fg, V, T, m, 12345, f"planted, m = {m}")
    assert info["zero_area"] == 1 and info["unweighted"] == 2 and info["triangles"] == 15 and info["max_area"] == 3.0


@pytest.mark.parametrize("nf", [1, 2, 255, 256, 257, 5000])  # around the block of 256 faces; 5000: the scan crosses blocks
def test_random_meshes_match_the_restatement(fg, gpu_required, nf):
    V, T = mr.random_mesh(nf, seed=100 + nf)
    info = check(fg, V, T, 4097, 7, f"random, nf = {nf}")
    if nf == 5000:
        assert info["weight_total"] > 2 ** 32 * 64  # far above 2^32: the multiply-high works on all 64 bits of the hash


# ---- determinism, prefixes, resources, the refusal on the device ---------------------------------------------------------------------------
def test_calls_are_functions_of_mesh_seed_and_k(fg, gpu_required):
    V, T = mr.planted_mesh()
    before = fg.live_resources()
    a = fg.sample_mesh(V, T, 257, seed=9, return_map=True)
    b = fg.sample_mesh(V, T, 257, seed=9, return_map=True)
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()
    assert a[5] == b[5]
    assert fg.sample_mesh(V, T, 257, seed=9).tobytes() == a[0].tobytes()  # the optional outputs change nothing
    other = fg.sample_mesh(V, T, 257, seed=10, return_map=True)
    assert other[0].tobytes() != a[0].tobytes() and other[2].tobytes() != a[2].tobytes()
    short = fg.sample_mesh(V, T, 64, seed=9, return_map=True)
    for x, y in zip(short[:4], a[:4]):
        assert x.tobytes() == y[:64].tobytes()  # every prefix is the sampling of that size
    assert short[4].tobytes() == a[4].tobytes()
    flat = np.zeros((6, 3), np.float32)
    flat[:, 0] = np.arange(6)  # six points on a line: every face has area 0
    with pytest.raises(fg.FgoicpError) as e:
        fg.sample_mesh(flat, np.array([[0, 1, 2], [3, 4, 5], [1, 1, 1]], np.uint32), 10)
    assert e.value.status == INVALID_ARG and "fgoicp_mesh_sample: the mesh has no area" in str(e.value)
    assert fg.live_resources() == before


def test_sample_mesh_even_thins_the_samples_and_carries_normals_and_faces(fg, gpu_required):
    V, T = mr.bumpy_icosphere(2)
    m, factor = 150, 5
    pts, nrm, face, idx, info = fg.sample_mesh_even(V, T, m, init_factor=factor, seed=4, return_map=True)
    assert pts.shape == (m, 3) and nrm.shape == (m, 3) and face.shape == (m,) and idx.shape == (m,) and info["samples"] == m * factor
    base = fg.sample_mesh(V, T, m * factor, seed=4, return_map=True)
    assert len(set(idx.tolist())) == m and idx.max() < m * factor and idx[0] == 0
    assert np.array_equal(_bits(pts), _bits(base[0][idx])) and np.array_equal(_bits(nrm), _bits(base[1][idx])) and np.array_equal(face, base[2][idx])
    plain = fg.sample_mesh_even(V, T, m, init_factor=factor, seed=4)
    assert plain.shape == (m, 3) and plain.tobytes() == pts.tobytes()
    # thinned: the closest pair is farther apart than the closest pair of the first m plain samples
    gap = lambda p: np.sort(((p[:, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(2) + np.eye(len(p)) * 1e9, axis=1)[:, 0].min()
    assert gap(pts) > gap(base[0][:m])


# ---- a registration against a mesh -------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def rot_angle(A, B):
    return float(np.arccos(np.clip((np.trace(np.asarray(A, np.float64) @ np.asarray(B, np.float64).T) - 1) / 2, -1, 1)))


R_GT = rodrigues(np.deg2rad(28.0) * np.array([0.36, -0.48, 0.8]))
T_GT = np.array([0.11, -0.07, 0.05])


@pytest.fixture(scope="module")
def pair(fg):
    """the bumpy sphere (1280 faces): 3000 target samples with their face normals; 400 source samples of another seed, moved so that
    R_GT src + T_GT lies on the mesh"""
    V, T = mr.bumpy_icosphere(3)
    assert len(T) == 1280
    tgt, normals = fg.sample_mesh(V, T, 3000, seed=1, return_map=True)[:2]
    on_mesh, on_mesh_normals = fg.sample_mesh(V, T, 400, seed=2, return_map=True)[:2]
    src = ((on_mesh.astype(np.float64) - T_GT) @ R_GT).astype(np.float32)  # R_GT^T (q - T_GT)
    return dict(V=V, T=T, tgt=tgt, normals=normals, src=src, src_normals=(on_mesh_normals.astype(np.float64) @ R_GT).astype(np.float32))


def _errors(R, t):
    return rot_angle(R, R_GT), float(np.linalg.norm(np.asarray(t, np.float64) - T_GT))


def test_given_normals_make_the_refinement_independent_of_k(fg, gpu_required, pair):
    """and the registration against the mesh's samples ends at the known pose: refined with the faces' normals, the rotation and translation
    errors are at most max(2 x e_est, 1e-4), e_est the error of the same solver refined with estimated normals — the two normal sets differ
    by the estimation noise and the loop stops inside a band, not at a point"""
    a = fg.FastGoICP(pair["tgt"], pair["src"], 0.05, 1e-3)
    b = fg.FastGoICP(pair["tgt"], pair["src"], 0.05, 1e-3)
    try:
        R, t = a.run()
        Rb, tb = b.run()
        assert R.tobytes() == Rb.tobytes() and t.tobytes() == tb.tobytes()
        est32, est4 = a.refine_plane(k=32), b.refine_plane(k=4)
        assert est32.raw != est4.raw  # estimated normals depend on k
        with pytest.raises(fg.FgoicpError) as e:  # bad normals: the context call's refusal, message included
            a.set_target_normals(np.zeros_like(pair["normals"]))
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals: normal 0 is zero or not finite" in str(e.value)
        nan = pair["normals"].copy()
        nan[17, 1] = np.nan
        with pytest.raises(fg.FgoicpError) as e:
            a.set_target_normals(nan)
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals: normal 17 is zero or not finite" in str(e.value)
        with pytest.raises(fg.FgoicpError) as e:
            a.set_source_normals(np.zeros_like(pair["src"]))
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_source_normals: normal 0 is zero or not finite" in str(e.value)
        with pytest.raises(ValueError):
            a.set_target_normals(pair["normals"][:-1])
        a.set_target_normals(pair["normals"])
        assert np.abs(a.registration.target_normals() - pair["normals"]).max() <= 1.2e-7  # in the callers' order, normalised again
        given4, given32 = a.refine_plane(k=4), a.refine_plane(k=32)
        assert given4.raw == given32.raw and given4.raw != est32.raw
        a.set_source_normals(pair["src_normals"])
        assert a.refine_gicp(k=4).raw == a.refine_gicp(k=32).raw
        e_search, e_est, e_given = _errors(R, t), _errors(est32.R, est32.t), _errors(given4.R, given4.t)
        print(f"search: {e_search[0]:.3e} rad, {e_search[1]:.3e}; refined, estimated normals (k = 32): {e_est[0]:.3e} rad, {e_est[1]:.3e}; "
              f"refined, face normals: {e_given[0]:.3e} rad, {e_given[1]:.3e} ({given4.iterations} iterations, rank {given4.rank})")
        assert given4.rank == 6
        assert e_given[0] <= max(2.0 * e_est[0], 1e-4) and e_given[1] <= max(2.0 * e_est[1], 1e-4)
    finally:
        a.close()
        b.close()


def test_cli_samples_a_mesh_target_and_registers_against_it(fg, gpu_required, pair, tmp_path):
    """The run ends at the known pose.  The bound: the target is 2000 samples of a surface of area A, one per A / 2000 — a mean spacing
    s = sqrt(A / 2000) — and the registration matches POINTS: it cannot tell poses apart that move the source by less than half that
    spacing, so the translation error must be <= s / 2 and the rotation error <= (s / 2) / r rad with r = 1, the mean radius of the mesh.
    The pose judged is the one the run ends with, the [refined] table of params.refine = "plane" (normals estimated: the CLI carries no
    face normals).  The search on its own stops as soon as its error is within mse_threshold x points of the optimum, a slack of
    sqrt(0.001) / scale = 0.045 per point in the file's units — above s / 2 = 0.042 — and so promises no such pose: it is printed, not
    asserted (measured: search 0.105 rad, 0.012; refined 1.9e-3 rad, 5.5e-4)."""
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    V, T = pair["V"], pair["T"]
    mr.write_ply(tmp_path / "mesh.ply", V, T.tolist())
    with open(tmp_path / "src.txt", "w") as f:
        f.write(f"{len(pair['src'])}\n" + "".join(f"{x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in pair["src"]))
    info = fg.sample_mesh(V, T, 2000, seed=3, return_map=True)[5]

    def run(target, extra):
        (tmp_path / "c.toml").write_text(f'[io]\ntarget = "{tmp_path}/{target}"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/out.toml"\n'
                                         f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / "c.toml")], capture_output=True, text=True, timeout=300)
        return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)
    rc, log = run("mesh.ply", 'target_mesh_points = 2000\nrefine = "plane"\n')
    assert rc == 0, log[-2000:]
    line = [ln for ln in log.splitlines() if "Mesh sampling (target):" in ln]
    assert len(line) == 1 and "Mesh sampling (source)" not in log, log[-2000:]
    assert f"Mesh sampling (target): {len(V)} vertices, {len(T)} triangles (0 zero-area, 0 unweighted), area " in line[0] and line[0].endswith("-> 2000 points")
    assert float(re.search(r"\), area ([-+0-9.eE]+) ->", line[0]).group(1)) == pytest.approx(info["area"], rel=1e-4)  # printed at the stream's 6 digits
    assert "Target point cloud (2000) loaded" in log
    out = (tmp_path / "out.toml").read_text()
    num = r"[-+0-9.eE]+"
    rows = np.array([[float(x) for x in row] for row in re.findall(rf"\[({num}), ({num}), ({num})\],", out)])  # [result], then [refined]
    ts = np.array([[float(x) for x in row] for row in re.findall(rf"translation = \[({num}), ({num}), ({num})\]", out)])
    assert rows.shape == (6, 3) and ts.shape == (2, 3) and out.index("[refined]") > out.index("[result]")
    half = 0.5 * np.sqrt(info["area"] / 2000.0)
    e_search, (e_rot, e_t) = _errors(rows[:3], ts[0]), _errors(rows[3:], ts[1])
    print(f"CLI: search {e_search[0]:.3e} rad, {e_search[1]:.3e}; refined: rotation error {e_rot:.3e} rad, translation error {e_t:.3e}; bound {half:.3e} for both")
    assert e_rot <= half and e_t <= half
    rc, log = run("src.txt", "target_mesh_points = 2000\n")  # a TXT file holds no mesh
    assert rc != 0 and "params.target_mesh_points" in log
