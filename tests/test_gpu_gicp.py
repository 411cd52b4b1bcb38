"""GPU: Generalized-ICP refinement with device-estimated source normals — the source normals (target_knn_kernel over a throw-away tree of
the source) against numpy.linalg.eigh of brute-force neighbourhoods, the normal equations (refine_moments_kernel, moment_fold_kernel)
against an fp64 numpy sum over the alignment report, the loop against a numpy restatement of it, the solver entry point and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr
from tests.test_gpu_plane import SIZES, _bits, _case, _write_txt, mean_plane_distance, off_pose, rodrigues, rot_angle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
INVALID_ARG = 1
TRIU6 = np.triu_indices(6)
_CACHE = {}


def brute_knn(pts, k):
    """the k smallest of (bits(fp32 dist_sq), index) per point of the cloud, by brute force"""
    key = (pts.tobytes(), k)
    if key not in _CACHE:
        d2 = npr.dist_sq(pts[:, None, :], pts[None, :, :]).astype(f32)
        keys = np.sort((_bits(d2).astype(np.uint64) << np.uint64(32)) | np.arange(len(pts), dtype=np.uint64)[None, :], axis=1)[:, :k]
        _CACHE[key] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return _CACHE[key]


def eigh_normals(pts, idx):
    p = pts[idx].astype(f64)
    d = p - p.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    return v[:, :, 0], w


# ---- 1. the source normals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,ns,k", [(1100, 700, 10), (1100, 300, 16), (1100, 33, 32), (1100, 64, 8), (1100, 65, 8)])
def test_estimated_source_normals_match_eigh_and_do_not_depend_on_the_device_order(fg, gpu_required, nt, ns, k):
    """DESIGN.md section 12's bounds: angle <= 1e-5 rad wherever the two smallest eigenvalues are separated by 5 % of the largest, at most
    2 % of the 700- and 300-point clouds left out by that condition, the norm within 2e-7 of 1.  ns = 33: one partial wave over a tree of
    two leaves; 64 and 65: a full wave, and one point more."""
    c = _case(fg, nt, ns)
    src = c["pcs"]
    got = {}
    for flags in (0, fg.FLAG_CURVE_ORDER, fg.FLAG_NO_MORTON):
        reg = fg.Registration(c["pct"], src, c["bounds"], 0.05, flags=flags)
        with pytest.raises(fg.FgoicpError) as e:
            reg.source_normals()
        assert e.value.status == INVALID_ARG and "not set" in str(e.value)
        for bad in (3, 33, 0, -1, ns + 1):
            assert reg._lib.fgoicp_ctx_set_source_normals(reg._h, None, bad) == INVALID_ARG and "fgoicp_ctx_set_source_normals" in reg._lib.fgoicp_last_error().decode()
        reg.set_source_normals(k=k)
        got[flags] = reg.source_normals()
        reg.close()
    assert got[0].tobytes() == got[fg.FLAG_CURVE_ORDER].tobytes() == got[fg.FLAG_NO_MORTON].tobytes()  # caller order, whatever the device's
    n = got[0].astype(f64)
    want, w = eigh_normals(src, brute_knn(src, k))
    good = (w[:, 1] - w[:, 0]) / w[:, 2] >= 0.05
    ang = np.arctan2(np.linalg.norm(np.cross(n, want), axis=1), np.abs((n * want).sum(axis=1)))
    print(f"ns {ns} k {k}: largest angle {ang[good].max():.3g} rad over {int(good.sum())} points, left out {100 * (1 - good.mean()):.2f} %, "
          f"largest | |n| - 1 | {np.abs(np.linalg.norm(n, axis=1) - 1).max():.3g}")
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 2e-7
    if ns in (700, 300):
        assert (1 - good.mean()) <= 0.02
    assert good.any() and ang[good].max() <= 1e-5


def test_given_source_normals_come_back_normalised_and_bad_ones_are_refused(fg, gpu_required):
    c = _case(fg, 1100, 300)
    for flags in (fg.FLAG_BRUTE_FORCE_NN, fg.FLAG_CURVE_ORDER):  # given normals need no tree; and a permuted device order
        reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=flags)
        rng = np.random.default_rng(1)
        raw = (rng.normal(size=(300, 3)) * rng.uniform(0.1, 50, (300, 1))).astype(f32)
        reg.set_source_normals(raw, k=0)  # k is ignored
        got = reg.source_normals()
        r64 = raw.astype(f64)
        want = r64 / np.sqrt(r64[:, 0] * r64[:, 0] + r64[:, 1] * r64[:, 1] + r64[:, 2] * r64[:, 2])[:, None]
        assert np.array_equal(got, want.astype(f32))
        for bad in (0.0, np.nan, np.inf):
            spoiled = raw.copy()
            spoiled[77] = bad
            with pytest.raises(fg.FgoicpError) as e:
                reg.set_source_normals(spoiled)
            assert e.value.status == INVALID_ARG and "normal 77" in str(e.value)
        assert np.array_equal(reg.source_normals(), got)  # a refused call leaves the normals alone
        if flags == fg.FLAG_BRUTE_FORCE_NN:
            with pytest.raises(fg.FgoicpError) as e:  # estimating needs the tree, as for the target
                reg.set_source_normals(k=8)
            assert e.value.status == INVALID_ARG and "brute-force" in str(e.value)
            assert np.array_equal(reg.source_normals(), got)
        reg.close()


# ---- 2. the normal equations ---------------------------------------------------------------------------------------------------------
def gicp_summands(x, q, nq, np_, R, eps):
    """per pair, in fp64: the 28 terms of J^T M J (upper triangle row by row), J^T M d, d^T M d — (N, 28)"""
    m = np_ @ np.asarray(R, f64).T
    S = 2 * np.eye(3)[None] - (1 - eps) * (nq[:, :, None] * nq[:, None, :] + m[:, :, None] * m[:, None, :])
    M = np.linalg.inv(S)
    J = np.zeros((len(x), 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = x[:, 2], -x[:, 1], -x[:, 2], x[:, 0], x[:, 1], -x[:, 0]  # -[x]x
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    d = x - q
    H = np.einsum("nai,nab,nbk->nik", J, M, J)
    g = np.einsum("nai,nab,nb->ni", J, M, d)
    e = np.einsum("na,nab,nb->n", d, M, d)
    return np.hstack([H[:, TRIU6[0], TRIU6[1]], g, e[:, None]])


def numpy_moments(c, a, tn, sn, R, t, max_dist2, eps):
    """the counted set from the report's arrays and the 28 sums in fp64 over it, with the per-term sum of |summand|; x is the scan's fp32 value"""
    nt = len(c["pct"])
    m = a.inlier & (a.dist2 <= f32(max_dist2)) & (a.indices < nt)
    j = np.where(m, a.indices, 0)
    m &= tn[j].any(axis=1) & sn.any(axis=1)
    x = (npr.rot_apply(np.asarray(R, f32), c["pcs"]) + np.asarray(t, f32)[None, :]).astype(f32)[m].astype(f64)
    s = gicp_summands(x, c["pct"][a.indices[m]].astype(f64), tn[a.indices[m]].astype(f64), sn[m].astype(f64), np.asarray(R, f32), eps)
    return int(m.sum()), s.sum(axis=0), np.abs(s).sum(axis=0)


@pytest.mark.parametrize("nt,ns", SIZES)
def test_moments_match_numpy_on_the_report_and_leave_the_context_alone(fg, gpu_required, nt, ns):
    """every term within 16 x 2^-24 x sum |summand| (the point-to-plane test's bound; x is bit-exact, so what remains is the order of the
    fp64 additions and the inverse), the count exact, two calls the same bytes, the context untouched"""
    c = _case(fg, nt, ns)
    worst = 0.0
    for trimmed in (False, True):
        reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
        if trimmed:
            reg.set_inliers(int(0.8 * ns))
        R, t = c["R"].astype(f32), c["t"].astype(f32)
        for call in (reg.gicp_moments, reg.icp_gicp):  # neither set, then the target's only, then the source's only
            with pytest.raises(fg.FgoicpError) as e:
                call(R, t)
            assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals" in str(e.value)
        reg.set_target_normals(k=10)
        for call in (reg.gicp_moments, reg.icp_gicp):
            with pytest.raises(fg.FgoicpError) as e:
                call(R, t)
            assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_source_normals" in str(e.value)
        reg.set_source_normals(k=10)
        tn, sn = reg.target_normals(), reg.source_normals()
        for R, t in ((R, t), off_pose(c, 5.0, 0.0)):
            before = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t), reg.plane_moments(R, t))
            a = before[2]
            for max_d2 in (np.inf, float(np.sort(a.dist2)[ns // 2])):
                for eps in (1e-3, 0.1):
                    got = reg.gicp_moments(R, t, max_d2, eps)
                    n, want, mag = numpy_moments(c, a, tn, sn, R, t, max_d2, eps)
                    assert got.correspondences == n and got.points == ns and n > 0
                    ratio = float((np.abs(got.m - want) / (16 * 2.0 ** -24 * mag + 1e-300)).max())
                    worst = max(worst, ratio)
                    print(f"nt {nt} trimmed {trimmed} max_d2 {max_d2:.3g} epsilon {eps}: N {n}, largest error / bound {ratio:.3g}")
                    assert (np.abs(got.m - want) <= 16 * 2.0 ** -24 * mag).all()
                    assert reg.gicp_moments(R, t, max_d2, eps).raw == got.raw  # two calls: the same bytes
                    assert np.array_equal(got.JtJ, got.JtJ.T) and got.sum_r2 == got.m[27]
            after = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t), reg.plane_moments(R, t))
            assert _bits(before[0]) == _bits(after[0])
            assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1])) and np.array_equal(_bits(before[1][2]), _bits(after[1][2]))
            for name in ("indices", "inlier", "target_hit"):
                assert np.array_equal(getattr(before[2], name), getattr(after[2], name)), name
            assert np.array_equal(_bits(before[2].dist2), _bits(after[2].dist2)) and _bits(before[2].sse) == _bits(after[2].sse)
            assert before[3].raw == after[3].raw
        reg.close()
    print(f"nt {nt}: largest error / bound over all evaluations {worst:.3g}")


def test_points_without_a_normal_in_either_cloud_are_not_counted_and_a_shorter_struct_is_not_overrun(fg, gpu_required):
    c = _case(fg, 1100, 300)
    tgt, src = c["pct"].copy(), c["pcs"].copy()
    R, t = c["R"].astype(f32), c["t"].astype(f32)
    tgt[[3, 400, 401, 777, 1099]] = tgt[3]  # five equal target points: with k = 4 their neighbourhoods have no extent, hence no normal
    src[:4] = ((tgt[3].astype(f64) - t) @ R.astype(f64)).astype(f32)  # four source points that land on them (equal too: no source normal either)
    src[[100, 150, 200, 250, 299]] = src[100]  # five equal source points elsewhere
    reg = fg.Registration(tgt, src, c["bounds"], 0.05)
    reg.set_target_normals(k=4)
    reg.set_source_normals(k=4)
    tn, sn = reg.target_normals(), reg.source_normals()
    assert not tn[[3, 400, 401, 777, 1099]].any() and int((~tn.any(axis=1)).sum()) == 5
    assert not sn[[100, 150, 200, 250, 299]].any() and not sn[:4].any() and int((~sn.any(axis=1)).sum()) == 9
    a = reg.alignment(R, t)
    cc = dict(c, pct=tgt, pcs=src)
    full = reg.gicp_moments(R, t)
    n, want, mag = numpy_moments(cc, a, tn, sn, R, t, np.inf, 1e-3)
    dropped = np.isin(a.indices, [3, 400, 401, 777, 1099]) | ~sn.any(axis=1)
    assert full.correspondences == n == 300 - int(dropped.sum()) <= 291
    assert (np.abs(full.m - want) <= 16 * 2.0 ** -24 * mag).all()
    # given source normals everywhere: only the target's gaps remain
    reg.set_source_normals(np.tile(f32([0, 0, 1]), (300, 1)))
    assert reg.gicp_moments(R, t).correspondences == 300 - int(np.isin(a.indices, [3, 400, 401, 777, 1099]).sum())
    Rg = fg.to_glm(R)
    fp = fg._lib.c_float_p
    for cls, call in ((fg._lib.PlaneMoments, lambda o: reg._lib.fgoicp_gicp_moments(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), 1e-3, o)),
                      (fg._lib.PlaneResult, lambda o: reg._lib.fgoicp_icp_gicp(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), 0, 1e-6, float("inf"), 1e-3, o))):
        buf = (C.c_ubyte * 512)(*([0xA5] * 512))
        out = C.cast(buf, C.POINTER(cls))
        out.contents.struct_size = 40
        assert call(out) == 0
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 40
        out.contents.struct_size = 0
        assert call(out) == INVALID_ARG and "struct_size" in reg._lib.fgoicp_last_error().decode()
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 0
    for eps in (0.0, -1.0, 2.0, np.nan):
        with pytest.raises(fg.FgoicpError) as e:
            reg.gicp_moments(R, t, np.inf, eps)
        assert e.value.status == INVALID_ARG and "epsilon" in str(e.value)
    reg.close()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------
def numpy_icp_gicp(tgt, src, tn, sn, R, t, max_iter, thr, eps):
    """the same loop in float64 with a brute-force search: evaluate, solve in the span of the eigenvalues above 1e-9 of the largest,
    update by Rodrigues; stop after a step shorter than thr, after a rank-deficient first step, or after max_iter steps"""
    tgt, src, tn, sn, R, t = (np.asarray(v, f64) for v in (tgt, src, tn, sn, R, t))
    it = 0
    while True:
        x = src @ R.T + t
        j = ((x[:, None, :] - tgt[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
        keep = tn[j].any(axis=1) & sn.any(axis=1)
        s = gicp_summands(x[keep], tgt[j[keep]], tn[j[keep]], sn[keep], R, eps).sum(axis=0)
        mse = float(s[27] / keep.sum())
        if it >= max_iter:
            return R, t, it, mse
        A = np.zeros((6, 6))
        A[TRIU6] = s[:21]
        A = np.triu(A) + np.triu(A, 1).T
        w, V = np.linalg.eigh(A)
        ok = w > 1e-9 * w.max()
        xi = -(V[:, ok] / w[ok]) @ (V[:, ok].T @ s[21:27])
        Q = rodrigues(xi[:3])
        R, t = Q @ R, Q @ t + xi[3:]
        it += 1
        if np.linalg.norm(xi[:3]) + np.linalg.norm(xi[3:]) < thr or (it == 1 and ok.sum() < 6):
            max_iter = it  # one more evaluation at the pose returned


def test_loop_converges_like_its_numpy_restatement(fg, gpu_required):
    """GPU error <= max(2 x the restatement's error, 1e-5) in rotation (rad) and translation (scaled units): correspondences can flip
    between fp32 and fp64 near convergence.  The errors of icp_plane from the same start are printed next to them, not compared."""
    c = _case(fg, 2500, 700, overlap=1.0, noise=0.0)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05)
    reg.set_target_normals(k=16)
    reg.set_source_normals(k=16)
    tn, sn = reg.target_normals(), reg.source_normals()
    R0, t0 = off_pose(c, 3.0, 0.02)
    start = reg.icp_gicp(R0, t0, max_iter=0)
    assert start.iterations == 0 and start.rank == 0 and np.array_equal(start.R, R0) and np.array_equal(start.t, t0)
    assert _bits(start.sse) == _bits(reg.compute_sse_error(R0, t0)) and start.correspondences == 700
    got = reg.icp_gicp(R0, t0, max_iter=30, conv_thr=1e-6)
    assert got.rank == 6 and 1 <= got.iterations <= 30
    assert got.gicp_rmse < start.gicp_rmse and got.gicp_rmse == got.plane_rmse
    assert _bits(got.sse) == _bits(reg.compute_sse_error(got.R, got.t))
    assert abs(np.linalg.det(got.R.astype(f64)) - 1) <= 1e-6
    Rn, tn_, itn, _ = numpy_icp_gicp(c["pct"], c["pcs"], tn, sn, R0, t0, 30, 1e-6, 1e-3)
    e_gpu = (rot_angle(got.R, c["R"]), float(np.linalg.norm(got.t.astype(f64) - c["t"])))
    e_np = (rot_angle(Rn, c["R"]), float(np.linalg.norm(tn_ - c["t"])))
    pl = reg.icp_plane(R0, t0, max_iter=30, conv_thr=1e-6)
    e_pl = (rot_angle(pl.R, c["R"]), float(np.linalg.norm(pl.t.astype(f64) - c["t"])))
    print(f"start: {rot_angle(R0, c['R']):.3g} rad, {np.linalg.norm(t0 - c['t']):.3g}; GPU gicp after {got.iterations} steps: {e_gpu[0]:.3g} rad, {e_gpu[1]:.3g}; "
          f"numpy restatement after {itn} steps: {e_np[0]:.3g} rad, {e_np[1]:.3g}; gicp rmse {start.gicp_rmse:.3g} -> {got.gicp_rmse:.3g}; "
          f"icp_plane from the same start after {pl.iterations} steps: {e_pl[0]:.3g} rad, {e_pl[1]:.3g}")
    assert e_gpu[0] <= max(2 * e_np[0], 1e-5) and e_gpu[1] <= max(2 * e_np[1], 1e-5)
    assert reg.icp_gicp(R0, t0, max_iter=30, conv_thr=1e-6).raw == got.raw  # the same bytes again
    reg.close()


# ---- 4. the solver and the CLI -------------------------------------------------------------------------------------------------------
def test_solver_refine_gicp_answers_in_the_callers_frame_and_leaves_the_solver_alone(fg, gpu_required):
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    s = fg.FastGoICP(tgt, src, 0.05, 1e-3)
    with pytest.raises(fg.FgoicpError) as e:
        s.refine_gicp()
    assert e.value.status == INVALID_ARG and "has not succeeded" in str(e.value)
    R, t = s.run()
    best = (s.get_best_error(), s.get_best_transform())
    ref = s.refine_gicp()
    assert isinstance(ref, fg.PlaneRefinement)
    assert ref.rank == 6 and ref.iterations >= 1 and ref.scaling_factor == s.preproc()["scale"] and ref.correspondences == len(src)
    normals = s.registration.target_normals()  # both sets were estimated by the call; invariant under the solver's centring and scale
    assert s.registration.source_normals().shape == (len(src), 3)
    d0, d1 = mean_plane_distance(tgt, src, normals, R, t), mean_plane_distance(tgt, src, normals, ref.R, ref.t)
    print(f"tiny: mean point-to-plane distance {d0:.4g} -> {d1:.4g} (files' units) after {ref.iterations} steps, gicp rmse {ref.gicp_rmse:.4g}")
    assert d1 <= d0
    assert _bits(s.get_best_error()) == _bits(best[0]) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(s.get_best_transform(), best[1]))
    R2, t2 = s.run()
    assert np.array_equal(_bits(R2), _bits(R)) and np.array_equal(_bits(t2), _bits(t))
    assert s.refine_gicp(max_distance=0.05).correspondences <= ref.correspondences
    with pytest.raises(fg.FgoicpError) as e:
        s.refine_gicp(epsilon=0.0)
    assert e.value.status == INVALID_ARG and "epsilon" in str(e.value)
    s.close()


def test_cli_writes_the_refined_table_with_gicp_rmse_and_leaves_the_other_keys_alone(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src[:600])
    for tag, extra in (("with", 'refine = "gicp"\nrefine_knn = 12\nrefine_max_iter = 20\nrefine_epsilon = 0.01\n'), ("plain", "")):
        (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{tag}_out.toml"\n'
                                              f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert ("Generalized-ICP refinement: " in p.stdout + p.stderr) == (tag == "with")
        assert "Point-to-plane refinement" not in p.stdout + p.stderr
    lines = lambda name: [ln for ln in (tmp_path / name).read_text().splitlines() if not ln.startswith("seconds")]
    with_, plain = lines("with_out.toml"), lines("plain_out.toml")
    cut = with_.index("[refined]")
    assert [ln for ln in with_[:cut] if ln] == [ln for ln in plain if ln] and "[refined]" not in plain
    keys = {ln.split(" = ")[0] for ln in with_[cut + 1:] if " = " in ln}
    assert {"rotation", "translation", "gicp_rmse", "iterations", "rank", "correspondences"} <= keys and "plane_rmse" not in keys
    rmse = float([ln for ln in with_[cut:] if ln.startswith("gicp_rmse")][0].split(" = ")[1])
    assert 0 < rmse < 0.1  # the files' units; a Mahalanobis residual: at most 1 / sqrt(2 epsilon) = 7 times the Euclidean one
