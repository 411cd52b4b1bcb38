"""GPU: the alignment report — exact correspondences, squared distances, the inlier set and the targets hit — of a context
(fgoicp_alignment), a solver (fgoicp_solver_alignment), a batch (fgoicp_batch_alignment) and the CLI (io.alignment), against a numpy
brute force with the device's fp32 arithmetic and the reference's tie rule (icp3d.cu:20-25: square roots compared, lowest index)."""
import os
import subprocess

import numpy as np
import pytest

from tests.nn_restatement import brute_force

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "goicp_golden.npz"))
CONTRACT = ("trans_cubes", "rot_cubes", "inner_bnb", "icp_runs", "icp_iters", "rounds", "initial_icp_sse")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected_inliers(dist2, k):
    """the k smallest squared distances, ties at the cut to the lowest caller index"""
    order = np.lexsort((np.arange(len(dist2)), _bits(dist2)))
    m = np.zeros(len(dist2), bool)
    m[order[:k]] = True
    return m


def check_consistency(a, nt, k=None):
    ns = len(a.indices)
    assert a.points == ns and a.indices.dtype == np.uint32 and a.indices.max() < nt
    if k is None:
        assert a.inlier.all() and a.inliers == ns
    else:
        assert a.inliers == k == int(a.inlier.sum())
        assert np.array_equal(a.inlier, expected_inliers(a.dist2, k))
    hit = np.zeros(nt, bool)
    hit[a.indices[a.inlier]] = True
    assert np.array_equal(a.target_hit, hit)
    assert a.targets_hit == len(np.unique(a.indices[a.inlier])) == int(hit.sum())
    assert _bits(a.max_inlier_dist2) == _bits(a.dist2[a.inlier].max())


def same_alignment(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(_bits(a.dist2), _bits(b.dist2))
    assert np.array_equal(a.inlier, b.inlier) and np.array_equal(a.target_hit, b.target_hit)
    assert (a.points, a.inliers, a.targets_hit) == (b.points, b.inliers, b.targets_hit)
    assert _bits(a.sse) == _bits(b.sse) and _bits(a.max_inlier_dist2) == _bits(b.max_inlier_dist2) and _bits(a.scaling_factor) == _bits(b.scaling_factor)


def _transforms(fg, rng, n):
    from fgoicp_amd.synth import random_rotation
    out = [(np.eye(3, dtype=f32), np.zeros(3, f32)), (G["syn_sse_R"].astype(f32), G["syn_sse_t"].astype(f32))]
    while len(out) < n:
        out.append((random_rotation(rng, 180.0).astype(f32), rng.uniform(-0.3, 0.3, 3).astype(f32)))
    return out


def _bounds(pct):
    return np.array([[pct[:, k].min(), pct[:, k].max()] for k in range(3)], f32)


# ---- 1. against the brute force ----------------------------------------------------------------------------------------------------
def test_indices_and_distances_are_the_brute_force_bits(fg, gpu_required):
    rng = np.random.default_rng(21)
    pct, pcs = G["syn_pct"].copy(), G["syn_pcs"]
    pct[700:900] = pct[100:300]  # duplicated target points: the lowest index must win
    pct[1400:] = pct[100:200]
    reg = fg.Registration(pct, pcs, G["syn_bounds"], float(G["syn_res"]))
    dup_won = 0
    for R, t in _transforms(fg, rng, 5):
        a = reg.alignment(R, t)
        idx, d2 = brute_force(pct, pcs, R, t)
        assert np.array_equal(_bits(a.dist2), _bits(d2))
        assert np.array_equal(a.indices, idx)
        check_consistency(a, len(pct))
        assert _bits(a.sse) == _bits(reg.compute_sse_error(R, t)) and a.scaling_factor == 1.0
        assert not np.isin(a.indices, np.arange(700, 900)).any() and not (a.indices >= 1400).any()
        dup_won += int(np.isin(a.indices, np.arange(100, 300)).sum())
        assert a.fitness == 1.0 and a.inlier_rmse == pytest.approx(np.sqrt(float(a.sse) / len(pcs)), rel=1e-6)
        assert np.allclose(a.distances, np.sqrt(a.dist2.astype(np.float64)))
    assert dup_won > 0  # the duplicated points are neighbours of some query, so the rule decided
    reg.close()
    # the bunny clouds, pre-processed as the solver does
    pct, pcs, *_, bounds = fg.synth.preprocess(G["bun_pct"], G["bun_pcs"])
    reg = fg.Registration(pct, pcs, bounds, 0.02)
    for R, t in _transforms(fg, rng, 3):
        a = reg.alignment(R, t)
        idx, d2 = brute_force(pct, pcs, R, t)
        assert np.array_equal(_bits(a.dist2), _bits(d2)) and np.array_equal(a.indices, idx)
    reg.close()


# ---- 2. caller order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
def test_permuting_a_cloud_permutes_the_report_and_nothing_else(fg, gpu_required, trimmed):
    rng = np.random.default_rng(22)
    pct, pcs = G["syn_pct"], G["syn_pcs"]
    R, t = G["syn_sse_R"].astype(f32), G["syn_sse_t"].astype(f32)
    k = 1000 if trimmed else None
    flags = fg.FLAG_CURVE_ORDER if trimmed else 0

    def run(tgt, src):
        reg = fg.Registration(tgt, src, G["syn_bounds"], float(G["syn_res"]), flags=flags)
        if trimmed:
            reg.set_inliers(k)
        a = reg.alignment(R, t)
        assert _bits(a.sse) == _bits(reg.compute_sse_error(R, t))
        reg.close()
        return a

    a = run(pct, pcs)
    check_consistency(a, len(pct), k)
    assert len(np.unique(_bits(a.dist2))) == len(pcs)  # no tied distances in this cloud: the inlier set does not depend on the order
    p = rng.permutation(len(pcs))
    b = run(pct, pcs[p])
    assert np.array_equal(b.indices, a.indices[p]) and np.array_equal(_bits(b.dist2), _bits(a.dist2[p])) and np.array_equal(b.inlier, a.inlier[p])
    assert np.array_equal(b.target_hit, a.target_hit)
    assert (b.inliers, b.targets_hit, _bits(b.max_inlier_dist2)) == (a.inliers, a.targets_hit, _bits(a.max_inlier_dist2))
    q = rng.permutation(len(pct))  # target point q[j] gets the label j
    qinv = np.empty(len(pct), np.uint32)
    qinv[q] = np.arange(len(pct), dtype=np.uint32)
    c = run(pct[q], pcs)
    assert np.array_equal(c.indices, qinv[a.indices]) and np.array_equal(_bits(c.dist2), _bits(a.dist2)) and np.array_equal(c.inlier, a.inlier)
    assert np.array_equal(c.target_hit, a.target_hit[q])
    assert (c.inliers, c.targets_hit, _bits(c.max_inlier_dist2)) == (a.inliers, a.targets_hit, _bits(a.max_inlier_dist2))


# ---- 3. sse bits, the inlier set, ties at the cut ----------------------------------------------------------------------------------
def test_trimmed_report_selects_the_k_smallest_with_ties_to_the_lowest_index(fg, gpu_required):
    rng = np.random.default_rng(23)
    tgt, src, _, _ = fg.synth.make_pair(5000, 3001, (1.0, 0.8, 0.6), seed=301, angle_deg=35.0, outlier_frac=0.1)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    R, t = _transforms(fg, rng, 3)[2]
    ns = len(pcs)
    reg = fg.Registration(pct, pcs, bounds, 0.02)
    a0 = reg.alignment(R, t)
    assert _bits(a0.sse) == _bits(reg.compute_sse_error(R, t))
    check_consistency(a0, len(pct))
    reg.close()
    # seven copies of one source point straddle the cut: the point of rank k0 and six copies of it in place of the six farthest points
    k0 = int(ns * 0.8)
    order = np.lexsort((np.arange(ns), _bits(a0.dist2)))
    star = order[k0]
    far = order[-6:]
    assert a0.dist2[order[k0 - 1]] < a0.dist2[star] < a0.dist2[order[k0 + 1]]
    pcs2 = pcs.copy()
    pcs2[far] = pcs[star]
    tied = np.sort(np.concatenate([[star], far]))
    assert len(set(tied)) == 7
    for k in (k0 + 1, k0 + 3, k0 + 7, k0 - 5, k0 + 40):  # 1, 3, all 7, none, all 7 and more of the tied points are inliers
        reg = fg.Registration(pct, pcs2, bounds, 0.02, flags=fg.FLAG_CURVE_ORDER)
        reg.set_inliers(k)
        a = reg.alignment(R, t)
        assert _bits(a.sse) == _bits(reg.compute_sse_error(R, t)), k  # fgoicp_sse skips the provably far queries, the report searches them all
        idx, d2 = brute_force(pct, pcs2, R, t)
        assert np.array_equal(_bits(a.dist2), _bits(d2)) and np.array_equal(a.indices, idx)  # the outliers' true neighbours too
        assert len(np.unique(_bits(a.dist2[tied]))) == 1
        check_consistency(a, len(pct), k)
        want = {k0 + 1: 1, k0 + 3: 3, k0 + 7: 7, k0 - 5: 0, k0 + 40: 7}[k]
        assert int(a.inlier[tied].sum()) == want and a.inlier[tied[:want]].all(), (k, a.inlier[tied])
        assert a.fitness == k / ns
        # the context is left as it was found: an ICP after the report returns what it returned before it
        icp = fg.IterativeClosestPoint3D(reg, max_iter=20, convergence_threshold=0.005, R=R, t=t)
        e2, R2, t2 = icp.run()
        reg.close()
        reg = fg.Registration(pct, pcs2, bounds, 0.02, flags=fg.FLAG_CURVE_ORDER)
        reg.set_inliers(k)
        e1, R1, t1 = fg.IterativeClosestPoint3D(reg, max_iter=20, convergence_threshold=0.005, R=R, t=t).run()
        assert _bits(e1) == _bits(e2) and np.array_equal(_bits(R1), _bits(R2)) and np.array_equal(_bits(t1), _bits(t2))
        reg.close()


# ---- 4. tree, brute force, the large-cloud path ------------------------------------------------------------------------------------
def _same_arrays(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(_bits(a.dist2), _bits(b.dist2))
    assert np.array_equal(a.inlier, b.inlier) and np.array_equal(a.target_hit, b.target_hit)
    assert (a.inliers, a.targets_hit, _bits(a.max_inlier_dist2)) == (b.inliers, b.targets_hit, _bits(b.max_inlier_dist2))


@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
def test_tree_and_brute_force_contexts_give_the_same_report(fg, gpu_required, trimmed):
    rng = np.random.default_rng(24)
    pct, pcs = G["syn_pct"].copy(), G["syn_pcs"]
    pct[900:1000] = pct[:100]
    outs = []
    for flags in (0, fg.FLAG_BRUTE_FORCE_NN, fg.FLAG_NO_MORTON, fg.FLAG_CURVE_ORDER):
        reg = fg.Registration(pct, pcs, G["syn_bounds"], float(G["syn_res"]), flags=flags)
        if trimmed:
            reg.set_inliers(900)
        outs.append([reg.alignment(R, t) for R, t in _transforms(fg, np.random.default_rng(24), 4)])
        for a, (R, t) in zip(outs[-1], _transforms(fg, np.random.default_rng(24), 4)):
            assert _bits(a.sse) == _bits(reg.compute_sse_error(R, t)), flags
        reg.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            _same_arrays(a, b)
            check_consistency(b, len(pct), 900 if trimmed else None)


@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
def test_large_cloud_context_agrees_with_brute_force_kernels(fg, gpu_required, trimmed):
    """above 262 144 source points (the contexts whose ICP takes the dual walk, whose SSE is not fused): 270 000 x 40 000, the tree scan
    against the O(ns * nt) kernels"""
    tgt, src, R_gt, t_gt = fg.synth.make_pair(40000, 270000, (1.0, 0.8, 0.6), seed=77, angle_deg=20.0, outlier_frac=0.1 if trimmed else 0.0)
    pct, pcs, *_, bounds = fg.synth.preprocess(tgt, src)
    k = int(len(pcs) * 0.85) if trimmed else None
    R, t = R_gt.astype(f32), np.zeros(3, f32)
    outs = []
    for flags in (fg.FLAG_CURVE_ORDER if trimmed else 0, fg.FLAG_BRUTE_FORCE_NN):
        reg = fg.Registration(pct, pcs, bounds, 0.02, flags=flags)
        if trimmed:
            reg.set_inliers(k)
        a = reg.alignment(R, t)
        assert _bits(a.sse) == _bits(reg.compute_sse_error(R, t)), flags
        outs.append(a)
        reg.close()
    _same_arrays(outs[0], outs[1])
    check_consistency(outs[0], len(pct), k)


# ---- 5. the solver -----------------------------------------------------------------------------------------------------------------
def _pairs(fg, seed=0, n=4):
    """(tgt, src, lut, mse, trim): trimmed and untrimmed pairs mixed, large rotations and tight thresholds so that the search runs"""
    rng = np.random.default_rng(seed)
    out = []
    for i, frac in enumerate((0.1, 0.0, 0.25, 0.0)[:n]):
        ns = int(rng.integers(800, 2501))
        tgt, src, _, _ = fg.synth.make_pair(int(rng.integers(3000, 6001)), ns, (1.0, 0.8, 0.6), seed=900 + 7 * seed + i, angle_deg=150.0, min_angle_deg=100.0,
                                            outlier_frac=0.05 if frac else 0.0)
        out.append((tgt, src, (0.02, 0.05)[i % 2], (1e-4, 2e-4)[i % 2], frac))
    return out


@pytest.mark.parametrize("schedule,round_width", [(0, 1), (1, 0)], ids=["serial", "round"])
def test_solver_report_at_the_best_transform(fg, gpu_required, schedule, round_width):
    lib = fg._lib.load()
    for tgt, src, lut, mse, frac in _pairs(fg, seed=5)[:2]:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=schedule, round_width=round_width, trim_fraction=frac)
        with pytest.raises(fg.FgoicpError) as e:  # before run(): refused
            s.alignment()
        assert e.value.status == 1 and "has not succeeded" in str(e.value)
        R1, t1 = s.run()
        e1, st1 = s.get_best_error(), s.stats()
        a = s.alignment()
        k = int(len(src) * (1.0 - frac)) if frac else None
        check_consistency(a, len(tgt), k)
        scale = s.preproc()["scale"]
        assert _bits(a.scaling_factor) == _bits(scale)
        rel = abs(float(a.sse) - float(e1)) / float(e1)
        print(f"schedule {schedule} trim {frac}: alignment sse {float(a.sse):.9g}, best error {float(e1):.9g}, relative difference {rel:.3g}")
        assert rel <= 1e-5  # the full-run bar (the ICP's last SSE is taken on an incrementally moved cloud)
        # the same report from the solver's context at the best transform (normalised frame)
        Rb, tb = s.get_best_transform()
        b = s.registration.alignment(Rb, tb)
        assert np.array_equal(a.indices, b.indices) and np.array_equal(_bits(a.dist2), _bits(b.dist2)) and np.array_equal(a.inlier, b.inlier)
        assert _bits(a.sse) == _bits(b.sse) == _bits(s.registration.compute_sse_error(Rb, tb))
        # in the callers' units: the distances between the moved raw source and the raw target points the report names
        moved = src.astype(np.float64) @ np.asarray(R1, np.float64).T + np.asarray(t1, np.float64)
        d = np.linalg.norm(moved - tgt[a.indices].astype(np.float64), axis=1)
        assert np.allclose(a.distances, d, rtol=1e-3, atol=1e-5 * float(np.abs(tgt).max()))
        assert a.inlier_rmse == pytest.approx(float(np.sqrt((d[a.inlier] ** 2).mean())), rel=1e-3)
        # a second run after the call: the first run's bits and counters
        R2, t2 = s.run()
        assert np.array_equal(_bits(R1), _bits(R2)) and np.array_equal(_bits(t1), _bits(t2)) and _bits(e1) == _bits(s.get_best_error())
        st2 = s.stats()
        for key in CONTRACT:
            assert st1[key] == st2[key], key
        same_alignment(a, s.alignment())
        s.close()
    assert lib.fgoicp_solver_alignment(None, None, None, None, None, None) == 1


# ---- 6. the batch ------------------------------------------------------------------------------------------------------------------
def test_batch_reports_are_the_solo_solvers_reports(fg, gpu_required):
    pairs = _pairs(fg, seed=6)
    solo = []
    for tgt, src, lut, mse, frac in pairs:
        s = fg.FastGoICP(tgt, src, lut, mse, schedule=1, round_width=0, trim_fraction=frac)
        R, t = s.run()
        solo.append((R, t, s.get_best_error(), s.stats(), s.alignment()))
        s.close()
    assert any(st["bounds_calls"] > 0 for *_, st, _a in solo)

    def check(b, out, idx):
        for j, i in enumerate(idx):
            R, t, e, st, a = solo[i]
            assert out[j] is not None
            assert np.array_equal(_bits(out[j][0]), _bits(R)) and np.array_equal(_bits(out[j][1]), _bits(t)) and _bits(b.get_best_error(j)) == _bits(e)
            sb = b.stats(j)
            for key in CONTRACT:
                assert sb[key] == st[key], (j, key)
        return [(out[j], b.get_best_error(j), {k: b.stats(j)[k] for k in CONTRACT}) for j in range(len(idx))]

    for max_live, idx in ((1, [0, 1, 2, 3]), (0, [0, 1, 2, 3]), (2, [3, 2, 1, 0])):
        b = fg.FastGoICPBatch([pairs[i] for i in idx], schedule=1, round_width=0, max_live=max_live, alignment=True)
        with pytest.raises(fg.FgoicpError):
            b.alignment(0)  # before run()
        res_on = check(b, b.run(), idx)
        for j, i in enumerate(idx):
            same_alignment(b.alignment(j), solo[i][4])
        b.close()
        b = fg.FastGoICPBatch([pairs[i] for i in idx], schedule=1, round_width=0, max_live=max_live)  # the same batch without the reports
        res_off = check(b, b.run(), idx)
        with pytest.raises(fg.FgoicpError) as e:
            b.alignment(0)
        assert e.value.status == 1
        b.close()
        for (o1, e1, s1), (o0, e0, s0) in zip(res_on, res_off):
            assert np.array_equal(_bits(o1[0]), _bits(o0[0])) and np.array_equal(_bits(o1[1]), _bits(o0[1])) and _bits(e1) == _bits(e0) and s1 == s0


# ---- 7. the CLI and the C++ facade -------------------------------------------------------------------------------------------------
def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def _read_alignment(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# alignment: ") and lines[1] == "# x y z target_index distance inlier"
    summary = {kv.split(" = ")[0]: float(kv.split(" = ")[1]) for kv in lines[0][len("# alignment: "):].split(", ")}
    rows = [ln.split() for ln in lines[2:]]
    xyz = np.array([[np.float32(v) for v in r[:3]] for r in rows], np.float32)
    return summary, xyz, np.array([int(r[3]) for r in rows]), np.array([float(r[4]) for r in rows]), np.array([int(r[5]) for r in rows], bool)


def test_cli_writes_the_report_and_the_same_result_file(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    (tmp_path / "cfgs").mkdir()
    chosen = _pairs(fg, seed=7)[:2]  # trims 0.1, 0.0
    names = []
    for i, (tgt, src, lut, mse, frac) in enumerate(chosen):
        _write_txt(tmp_path / f"tgt{i}.txt", tgt)
        _write_txt(tmp_path / f"src{i}.txt", src)
        for tag in ("plain", "with", "batch"):
            key = "" if tag == "plain" else f'alignment = "{tmp_path}/{tag}{i}_align.txt"\n'
            (tmp_path / "cfgs" / f"{tag}{i}.toml").write_text(
                f'[io]\ntarget = "{tmp_path}/tgt{i}.txt"\nsource = "{tmp_path}/src{i}.txt"\noutput = "{tmp_path}/{tag}{i}.toml"\n{key}'
                f'[params]\nlut_resolution = {lut}\nmse_threshold = {mse}\nseed = 3\ntrim_fraction = {frac}\n')
        names.append(f"cfgs/batch{i}.toml")
        logs = {}
        for tag in ("plain", "with"):
            p = subprocess.run([exe, "-c", str(tmp_path / "cfgs" / f"{tag}{i}.toml")], capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
            logs[tag] = p.stdout
        # the result file of the run without the key, byte for byte but for the wall-clock line
        plain = [ln for ln in (tmp_path / f"plain{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        with_ = [ln for ln in (tmp_path / f"with{i}.toml").read_text().splitlines() if not ln.startswith("seconds")]
        assert plain == with_ and not (tmp_path / f"plain{i}_align.txt").exists()
        summary, xyz, idx, dist, inl = _read_alignment(tmp_path / f"with{i}_align.txt")
        # the same clouds through Python: the source as the CLI registered it (after source_subsample) is in the file
        assert 0 < len(xyz) <= len(src) and summary["points"] == len(xyz)
        s = fg.FastGoICP(tgt, xyz, lut, mse, trim_fraction=frac)
        s.run()
        a = s.alignment()
        assert np.array_equal(idx, a.indices) and np.array_equal(inl, a.inlier)
        assert np.allclose(dist, a.distances, rtol=1e-6, atol=0)
        assert (summary["inliers"], summary["targets_hit"]) == (a.inliers, a.targets_hit)
        assert summary["sse"] == pytest.approx(float(a.sse), rel=1e-7) and summary["inlier_rmse"] == pytest.approx(a.inlier_rmse, rel=1e-6)
        s.close()
    # --batch writes one file per config that names one, with the lone run's lines
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    p = subprocess.run([exe, "--batch", str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for i in range(len(chosen)):
        assert (tmp_path / f"batch{i}_align.txt").read_text() == (tmp_path / f"with{i}_align.txt").read_text()


def test_cpp_facade_reports_what_python_reports(fg, gpu_required, tmp_path):
    import json
    exe = str(tmp_path / "facade_alignment_check")
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "host_harness", "facade_alignment_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    tgt, src, lut, mse, frac = _pairs(fg, seed=8)[0]
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    p = subprocess.run([exe, str(tmp_path / "tgt.txt"), str(tmp_path / "src.txt"), str(lut), str(frac)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    s = fg.FastGoICP(tgt, src, lut, 1e-3, trim_fraction=frac)
    s.run()
    a = s.alignment()
    assert (got["points"], got["inliers"], got["targets_hit"]) == (a.points, a.inliers, a.targets_hit)
    assert np.array_equal(np.array(got["indices"], np.uint32), a.indices) and np.array_equal(np.array(got["inlier"], bool), a.inlier)
    assert np.float32(got["sse"]) == a.sse and got["fitness"] == pytest.approx(a.fitness) and got["inlier_rmse"] == pytest.approx(a.inlier_rmse, rel=1e-6)
    assert got["distance0"] == pytest.approx(a.distances[0], rel=1e-6)
    s.close()
