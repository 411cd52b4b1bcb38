"""GPU: point-to-plane refinement with device-estimated target normals — the exact k-nearest-neighbour sets of the target's own tree
(target_knn_kernel) against a numpy brute force, the normals against numpy.linalg.eigh, the normal equations (refine_moments_kernel,
moment_fold_kernel of csrc/device/fixed_sum.hpp) against an fp64 numpy sum over the alignment report, the loop against a numpy restatement of it, the solver
entry point and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
INVALID_ARG = 1
BOX = (0.156, 0.152, 0.118)
SIZES = ((2500, 700), (1100, 300))  # two super-leaves of 64 leaves = 2048 points (the second holds 15 leaves and 49 empty ones), nt no multiple of the 32-point leaf; and one super-leaf
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _case(fg, nt, ns, overlap=0.7, noise=1e-3):
    """pre-processed pair + the ground-truth pose in the scaled frame; computed once per size"""
    key = (nt, ns, overlap, noise)
    if key not in _CACHE:
        tgt, src, R_gt, t_gt = fg.synth.make_pair(nt, ns, BOX, seed=900 + nt, overlap=overlap, noise=noise, angle_deg=20.0)
        pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
        t_s = f64(scale) * (t_gt + off_t.astype(f64) - R_gt @ off_s.astype(f64))
        _CACHE[key] = dict(pct=pct, pcs=pcs, bounds=bounds, R=R_gt, t=t_s)
    return _CACHE[key]


def brute_knn(tgt, k):
    """the k smallest of (bits(fp32 dist_sq), index) per target point, by brute force; shared through the cache"""
    key = ("knn", tgt.tobytes(), k)
    if key not in _CACHE:
        full = ("d2", tgt.tobytes())
        if full not in _CACHE:
            d2 = npr.dist_sq(tgt[:, None, :], tgt[None, :, :]).astype(f32)
            _CACHE[full] = (_bits(d2).astype(np.uint64) << np.uint64(32)) | np.arange(len(tgt), dtype=np.uint64)[None, :]
        keys = np.sort(_CACHE[full], axis=1)[:, :k]
        _CACHE[key] = ((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32).view(f32))
    return _CACHE[key]


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def rot_angle(A, B):
    return float(np.arccos(np.clip((np.trace(np.asarray(A, f64) @ np.asarray(B, f64).T) - 1) / 2, -1, 1)))


def off_pose(c, deg, shift, seed=5):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    return (rodrigues(np.deg2rad(deg) * ax) @ c["R"]).astype(f32), (c["t"] + shift * d).astype(f32)


# ---- 1. the neighbour sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,ns", SIZES)
def test_knn_equals_the_brute_force_in_indices_and_bits(fg, gpu_required, nt, ns):
    c = _case(fg, nt, ns)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05)
    for k in (4, 10, 32):
        idx, d2 = reg.target_knn(k)
        widx, wd2 = brute_knn(c["pct"], k)
        assert np.array_equal(idx, widx), (k, int((idx != widx).any(axis=1).sum()))
        assert np.array_equal(_bits(d2), _bits(wd2)), k
        assert np.array_equal(idx[:, 0], np.arange(nt)) and not d2[:, 0].any()  # the point itself comes first
    lib = reg._lib
    for bad in (3, 33, 0, -1):
        assert lib.fgoicp_target_knn(reg._h, bad, None, None) == INVALID_ARG and "fgoicp_target_knn" in lib.fgoicp_last_error().decode()
        assert lib.fgoicp_ctx_set_target_normals(reg._h, None, bad) == INVALID_ARG
    # either output alone
    i2 = np.empty((nt, 4), np.uint32)
    assert lib.fgoicp_target_knn(reg._h, 4, i2.ctypes.data_as(fg._lib.c_uint32_p), None) == 0 and np.array_equal(i2, brute_knn(c["pct"], 4)[0])
    reg.close()


def test_knn_with_duplicated_points_breaks_ties_by_index_and_small_targets_work(fg, gpu_required):
    c = _case(fg, 1100, 300)
    tgt = c["pct"].copy()
    rng = np.random.default_rng(3)
    src_rows = rng.choice(1100, 64, replace=False)
    dst_rows = rng.choice(np.setdiff1d(np.arange(1100), src_rows), 64, replace=False)
    tgt[dst_rows] = tgt[src_rows]  # 64 duplicated points: equal distances at the cut of their neighbours
    reg = fg.Registration(tgt, c["pcs"], c["bounds"], 0.05)
    for k in (4, 10, 32):
        idx, d2 = reg.target_knn(k)
        widx, wd2 = brute_knn(tgt, k)
        assert np.array_equal(idx, widx) and np.array_equal(_bits(d2), _bits(wd2)), k
    lo = np.minimum(src_rows, dst_rows)
    assert np.array_equal(reg.target_knn(4)[0][np.maximum(src_rows, dst_rows), 0], lo)  # the twin with the lower index is first for both
    reg.close()
    # nt = 33: two leaves, k = 32 takes all but one point; k > nt is refused
    small = c["pct"][:33].copy()
    reg = fg.Registration(small, c["pcs"], c["bounds"], 0.05)
    idx, d2 = reg.target_knn(32)
    widx, wd2 = brute_knn(small, 32)
    assert np.array_equal(idx, widx) and np.array_equal(_bits(d2), _bits(wd2))
    reg.close()
    reg = fg.Registration(c["pct"][:20].copy(), c["pcs"], c["bounds"], 0.05)
    assert reg._lib.fgoicp_target_knn(reg._h, 21, None, None) == INVALID_ARG
    assert reg._lib.fgoicp_ctx_set_target_normals(reg._h, None, 21) == INVALID_ARG
    assert np.array_equal(reg.target_knn(20)[0], brute_knn(c["pct"][:20].copy(), 20)[0])
    reg.close()


# ---- 2. the normals ------------------------------------------------------------------------------------------------------------------
def eigh_normals(tgt, idx):
    p = tgt[idx].astype(f64)  # (nt, k, 3)
    d = p - p.mean(axis=1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    return v[:, :, 0], w


@pytest.mark.parametrize("nt,ns,k", [(2500, 700, 10), (2500, 700, 16), (1100, 300, 8)])
def test_estimated_normals_match_eigh_of_the_same_neighbourhoods(fg, gpu_required, nt, ns, k):
    """angle <= 1e-5 rad for every point whose two smallest eigenvalues are separated by 5 % of the largest; at most 2 % of the cloud is
    left out by that condition"""
    c = _case(fg, nt, ns)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05)
    with pytest.raises(fg.FgoicpError) as e:
        reg.target_normals()
    assert e.value.status == INVALID_ARG and "not set" in str(e.value)
    reg.set_target_normals(k=k)
    n = reg.target_normals()
    want, w = eigh_normals(c["pct"], brute_knn(c["pct"], k)[0])
    good = (w[:, 1] - w[:, 0]) / w[:, 2] >= 0.05
    assert np.abs(np.linalg.norm(n.astype(f64), axis=1) - 1).max() <= 2e-7
    cosv = np.abs((n.astype(f64) * want).sum(axis=1))
    sinv = np.linalg.norm(np.cross(n.astype(f64), want), axis=1)
    ang = np.arctan2(sinv, cosv)
    print(f"nt {nt} k {k}: largest angle {ang[good].max():.3g} rad over {int(good.sum())} points, left out {100 * (1 - good.mean()):.2f} %")
    assert (1 - good.mean()) <= 0.02
    assert ang[good].max() <= 1e-5
    reg.close()


def test_given_normals_come_back_normalised_and_bad_ones_are_refused(fg, gpu_required):
    c = _case(fg, 1100, 300)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=fg.FLAG_BRUTE_FORCE_NN)  # given normals need no tree
    rng = np.random.default_rng(1)
    raw = (rng.normal(size=(1100, 3)) * rng.uniform(0.1, 50, (1100, 1))).astype(f32)
    reg.set_target_normals(raw, k=0)  # k is ignored
    got = reg.target_normals()
    r64 = raw.astype(f64)
    want = r64 / np.sqrt(r64[:, 0] * r64[:, 0] + r64[:, 1] * r64[:, 1] + r64[:, 2] * r64[:, 2])[:, None]
    assert np.array_equal(got, want.astype(f32))
    for bad in (0.0, np.nan, np.inf):
        spoiled = raw.copy()
        spoiled[77] = bad
        with pytest.raises(fg.FgoicpError) as e:
            reg.set_target_normals(spoiled)
        assert e.value.status == INVALID_ARG and "normal 77" in str(e.value)
    assert np.array_equal(reg.target_normals(), got)  # a refused call leaves the normals alone
    with pytest.raises(fg.FgoicpError):  # estimating needs the tree
        reg.set_target_normals(k=8)
    reg.close()


# ---- 3. the normal equations ---------------------------------------------------------------------------------------------------------
def numpy_moments(c, reg, a, normals, R, t, max_dist2):
    """the counted set from the report's arrays and the 28 sums in fp64 over it, with the per-term sum of |summand|"""
    nt = len(c["pct"])
    m = a.inlier & (a.dist2 <= f32(max_dist2)) & (a.indices < nt)
    j = np.where(m, a.indices, 0)
    m &= normals[j].any(axis=1)
    x = (npr.rot_apply(np.asarray(R, f32), c["pcs"]) + np.asarray(t, f32)[None, :]).astype(f32)[m].astype(f64)
    q, n = c["pct"][a.indices[m]].astype(f64), normals[a.indices[m]].astype(f64)
    r = (n * (x - q)).sum(axis=1)
    J = np.hstack([np.cross(x, n), n])
    terms = [J[:, i] * J[:, k] for i in range(6) for k in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r]
    return int(m.sum()), np.array([s.sum() for s in terms]), np.array([np.abs(s).sum() for s in terms])


@pytest.mark.parametrize("nt,ns", SIZES)
def test_moments_match_numpy_on_the_report_and_leave_the_context_alone(fg, gpu_required, nt, ns):
    c = _case(fg, nt, ns)
    for trimmed in (False, True):
        reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
        if trimmed:
            reg.set_inliers(int(0.8 * ns))
        with pytest.raises(fg.FgoicpError) as e:
            reg.plane_moments(c["R"], c["t"])
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals" in str(e.value)
        with pytest.raises(fg.FgoicpError) as e:
            reg.icp_plane(c["R"], c["t"])
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals" in str(e.value)
        for pose in ((c["R"].astype(f32), c["t"].astype(f32)), off_pose(c, 5.0, 0.0)):
            R, t = pose
            reg.set_target_normals(k=10)
            normals = reg.target_normals()
            before = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t))
            a = before[2]
            for max_d2 in (np.inf, float(np.sort(a.dist2)[ns // 2])):
                got = reg.plane_moments(R, t, max_d2)
                n, want, mag = numpy_moments(c, reg, a, normals, R, t, max_d2)
                assert got.correspondences == n and got.points == ns and n > 0
                err = np.abs(got.m - want)
                print(f"nt {nt} trimmed {trimmed} max_d2 {max_d2:.3g}: N {n}, largest error / bound {float((err / (16 * 2.0 ** -24 * mag + 1e-300)).max()):.3g}")
                assert (err <= 16 * 2.0 ** -24 * mag).all()
                assert reg.plane_moments(R, t, max_d2).raw == got.raw  # two calls: the same bytes
                assert np.array_equal(got.JtJ, got.JtJ.T) and got.sum_r2 == got.m[27]
            after = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t))
            assert _bits(before[0]) == _bits(after[0])
            assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1])) and np.array_equal(_bits(before[1][2]), _bits(after[1][2]))
            for name in ("indices", "inlier", "target_hit"):
                assert np.array_equal(getattr(before[2], name), getattr(after[2], name)), name
            assert np.array_equal(_bits(before[2].dist2), _bits(after[2].dist2)) and _bits(before[2].sse) == _bits(after[2].sse)
        reg.close()


def test_a_shorter_struct_is_not_overrun_and_points_without_a_normal_are_not_counted(fg, gpu_required):
    c = _case(fg, 1100, 300)
    tgt, src = c["pct"].copy(), c["pcs"].copy()
    tgt[[3, 400, 401, 777, 1099]] = tgt[3]  # five equal points: with k = 4 their neighbourhoods have no extent, hence no normal
    R, t = c["R"].astype(f32), c["t"].astype(f32)
    src[:4] = ((tgt[3].astype(f64) - t) @ R.astype(f64)).astype(f32)  # four source points that land on them
    reg = fg.Registration(tgt, src, c["bounds"], 0.05)
    reg.set_target_normals(k=4)
    normals = reg.target_normals()
    assert not normals[[3, 400, 401, 777, 1099]].any() and int((~normals.any(axis=1)).sum()) == 5
    a = reg.alignment(R, t)
    assert set(a.indices[:4]) == {3}  # the tie rule: the lowest index
    full = reg.plane_moments(R, t)
    cc = dict(c, pct=tgt, pcs=src)
    n, want, mag = numpy_moments(cc, reg, a, normals, R, t, np.inf)
    assert full.correspondences == n == 300 - int(np.isin(a.indices, [3, 400, 401, 777, 1099]).sum()) <= 296
    assert (np.abs(full.m - want) <= 16 * 2.0 ** -24 * mag).all()
    Rg = fg.to_glm(R)
    fp = fg._lib.c_float_p
    for cls, call in ((fg._lib.PlaneMoments, lambda o: reg._lib.fgoicp_plane_moments(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), o)),
                      (fg._lib.PlaneResult, lambda o: reg._lib.fgoicp_icp_plane(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), 0, 1e-6, float("inf"), o))):
        buf = (C.c_ubyte * 512)(*([0xA5] * 512))
        out = C.cast(buf, C.POINTER(cls))
        out.contents.struct_size = 40
        assert call(out) == 0
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 40
        out.contents.struct_size = 0
        assert call(out) == INVALID_ARG and "struct_size" in reg._lib.fgoicp_last_error().decode()
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 0
    reg.close()


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------------------
def numpy_icp_plane(tgt, src, normals, R, t, max_iter, thr):
    """the same loop in float64 with a brute-force search: evaluate, solve in the span of the eigenvalues above 1e-9 of the largest,
    update by Rodrigues; stop after a step shorter than thr, after a rank-deficient first step, or after max_iter steps"""
    tgt, src, normals, R, t = (np.asarray(v, f64) for v in (tgt, src, normals, R, t))
    it = 0
    while True:
        x = src @ R.T + t
        j = ((x[:, None, :] - tgt[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
        keep = normals[j].any(axis=1)
        xk, q, n = x[keep], tgt[j[keep]], normals[j[keep]]
        r = (n * (xk - q)).sum(axis=1)
        mse = float((r * r).mean())
        if it >= max_iter:
            return R, t, it, mse
        J = np.hstack([np.cross(xk, n), n])
        w, V = np.linalg.eigh(J.T @ J)
        ok = w > 1e-9 * w.max()
        xi = -(V[:, ok] / w[ok]) @ (V[:, ok].T @ (J.T @ r))
        Q = rodrigues(xi[:3])
        R, t = Q @ R, Q @ t + xi[3:]
        it += 1
        if np.linalg.norm(xi[:3]) + np.linalg.norm(xi[3:]) < thr or (it == 1 and ok.sum() < 6):
            max_iter = it  # one more evaluation at the pose returned


def test_loop_converges_like_its_numpy_restatement(fg, gpu_required):
    """GPU error <= max(2 x the restatement's error, 1e-5) in rotation (rad) and translation (scaled units): correspondences can flip
    between fp32 and fp64 near convergence"""
    c = _case(fg, 2500, 700, overlap=1.0, noise=0.0)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05)
    reg.set_target_normals(k=16)
    normals = reg.target_normals()
    R0, t0 = off_pose(c, 3.0, 0.02)
    start = reg.icp_plane(R0, t0, max_iter=0)
    assert start.iterations == 0 and start.rank == 0 and np.array_equal(start.R, R0) and np.array_equal(start.t, t0)
    assert _bits(start.sse) == _bits(reg.compute_sse_error(R0, t0)) and start.correspondences == 700
    got = reg.icp_plane(R0, t0, max_iter=30, conv_thr=1e-6)
    assert got.rank == 6 and 1 <= got.iterations <= 30
    assert got.plane_rmse < start.plane_rmse
    assert _bits(got.sse) == _bits(reg.compute_sse_error(got.R, got.t))
    assert abs(np.linalg.det(got.R.astype(f64)) - 1) <= 1e-6
    Rn, tn, itn, _ = numpy_icp_plane(c["pct"], c["pcs"], normals, R0, t0, 30, 1e-6)
    e_gpu = (rot_angle(got.R, c["R"]), float(np.linalg.norm(got.t.astype(f64) - c["t"])))
    e_np = (rot_angle(Rn, c["R"]), float(np.linalg.norm(tn - c["t"])))
    print(f"start: {rot_angle(R0, c['R']):.3g} rad, {np.linalg.norm(t0 - c['t']):.3g}; GPU after {got.iterations} steps: {e_gpu[0]:.3g} rad, {e_gpu[1]:.3g}; "
          f"numpy restatement after {itn} steps: {e_np[0]:.3g} rad, {e_np[1]:.3g}; plane rmse {start.plane_rmse:.3g} -> {got.plane_rmse:.3g}")
    assert e_gpu[0] <= max(2 * e_np[0], 1e-5) and e_gpu[1] <= max(2 * e_np[1], 1e-5)
    assert reg.icp_plane(R0, t0, max_iter=30, conv_thr=1e-6).raw == got.raw  # the same bytes again
    reg.close()


def test_planar_target_gives_rank_three_and_moves_only_off_the_plane(fg, gpu_required):
    g = np.linspace(-0.8, 0.8, 32)
    tgt = np.array([[x, y, 0.0] for x in g for y in g], f32)  # nt = 1024
    rng = np.random.default_rng(2)
    src = np.concatenate([rng.uniform(-0.5, 0.5, (300, 2)), np.zeros((300, 1))], axis=1).astype(f32)
    reg = fg.Registration(tgt, src, np.array([[-1, 1], [-1, 1], [-0.5, 0.5]], f32), 0.05)
    reg.set_target_normals(k=8)
    n = reg.target_normals()
    assert np.array_equal(np.abs(n), np.tile(f32([0, 0, 1]), (1024, 1)))
    R0 = rodrigues(np.array([0.02, -0.015, 0.01])).astype(f32)
    t0 = f32([0.01, -0.02, 0.03])
    got = reg.icp_plane(R0, t0, max_iter=30, conv_thr=1e-6)
    assert got.rank == 3 and got.iterations == 1 and got.correspondences == 300
    dR = got.R.astype(f64) @ R0.astype(f64).T
    w = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2
    v = got.t.astype(f64) - dR @ t0.astype(f64)
    print(f"planar target: step w {w}, v {v}, plane rmse {got.plane_rmse:.3g}")
    assert abs(w[2]) <= 1e-6 and max(abs(v[0]), abs(v[1])) <= 1e-6 and abs(v[2]) > 1e-3  # tilt and height only
    assert got.plane_rmse <= 0.05 * reg.icp_plane(R0, t0, max_iter=0).plane_rmse  # what one linearised step leaves is of second order in the tilt
    reg.close()


# ---- 5. the solver and the CLI -------------------------------------------------------------------------------------------------------
def mean_plane_distance(tgt, src, normals, R, t):
    x = np.asarray(src, f64) @ np.asarray(R, f64).T + np.asarray(t, f64)
    j = ((x[:, None, :] - tgt[None, :, :].astype(f64)) ** 2).sum(axis=2).argmin(axis=1)
    return float(np.abs((normals[j].astype(f64) * (x - tgt[j].astype(f64))).sum(axis=1)).mean())


def test_solver_refine_plane_answers_in_the_callers_frame_and_leaves_the_solver_alone(fg, gpu_required):
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    s = fg.FastGoICP(tgt, src, 0.05, 1e-3)
    with pytest.raises(fg.FgoicpError) as e:
        s.refine_plane()
    assert e.value.status == INVALID_ARG and "has not succeeded" in str(e.value)
    R, t = s.run()
    best = (s.get_best_error(), s.get_best_transform())
    ref = s.refine_plane()
    assert ref.rank == 6 and ref.iterations >= 1 and ref.scaling_factor == s.preproc()["scale"] and ref.correspondences == len(src)
    normals = s.registration.target_normals()  # invariant under the solver's centring and scale
    d0, d1 = mean_plane_distance(tgt, src, normals, R, t), mean_plane_distance(tgt, src, normals, ref.R, ref.t)
    print(f"tiny: mean point-to-plane distance {d0:.4g} -> {d1:.4g} (files' units) after {ref.iterations} steps, plane rmse {ref.plane_rmse:.4g}")
    assert d1 < d0
    assert _bits(s.get_best_error()) == _bits(best[0]) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(s.get_best_transform(), best[1]))
    R2, t2 = s.run()
    assert np.array_equal(_bits(R2), _bits(R)) and np.array_equal(_bits(t2), _bits(t))
    assert s.refine_plane(max_distance=0.05).correspondences <= ref.correspondences
    s.close()


def _write_txt(path, pts):
    with open(path, "w") as f:
        f.write(f"{len(pts)}\n")
        for x, y, z in pts:
            f.write(f"{x:.9g} {y:.9g} {z:.9g}\n")


def test_cli_writes_the_refined_table_and_leaves_the_other_keys_alone(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src[:600])
    for tag, extra in (("with", 'refine = "plane"\nrefine_knn = 12\nrefine_max_iter = 20\n'), ("plain", "")):
        (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{tag}_out.toml"\n'
                                              f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert ("Point-to-plane refinement" in p.stdout + p.stderr) == (tag == "with")
    lines = lambda name: [ln for ln in (tmp_path / name).read_text().splitlines() if not ln.startswith("seconds")]
    with_, plain = lines("with_out.toml"), lines("plain_out.toml")
    cut = with_.index("[refined]")
    assert [ln for ln in with_[:cut] if ln] == [ln for ln in plain if ln] and "[refined]" not in plain
    keys = {ln.split(" = ")[0] for ln in with_[cut + 1:] if " = " in ln}
    assert {"rotation", "translation", "plane_rmse", "iterations", "rank", "correspondences"} <= keys
    rmse = float([ln for ln in with_[cut:] if ln.startswith("plane_rmse")][0].split(" = ")[1])
    assert 0 < rmse < 0.01  # the files' units: the surface is 0.15 across
