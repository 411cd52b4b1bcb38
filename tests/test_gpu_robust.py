"""GPU: robust losses for the point-to-plane and Generalized-ICP refinements — the per-point residuals, weights and
counted set of refine_moments_kernel (weighted) against numpy on the alignment report, the weighted normal equations against fp64 sums of the device's
own weights times numpy's terms, the automatic scale, the edges (every weight zero, one point, one slot into a new block, a trimmed
context), the loop against the plain loop and a numpy restatement on a source with 20 % stray points, the solver entry point and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as npr
from tests.test_gpu_gicp import TRIU6, gicp_summands
from tests.test_gpu_plane import BOX, SIZES, _bits, _case, _write_txt, off_pose, rodrigues, rot_angle
from tests.test_robust_host import LOSSES, numpy_weight

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
INVALID_ARG = 1
BOUND = 16 * 2.0 ** -24  # x sum |summand|: the project's bound for these sums (tests/test_gpu_plane.py, tests/test_gpu_gicp.py)
EPS = 1e-3
MODELS = ("plane", "gicp")
_SHARED = {}


def _bits64(a):
    return np.ascontiguousarray(a, f64).view(np.uint64)


def numpy_pairs(c, a, tn, sn, R, t, max_dist2, model, eps=EPS):
    """the counted set from the report's arrays (with the source-normal condition for "gicp") and, per counted pair in fp64: the 28
    unweighted terms, the residual s and the sum of |summand| behind it — for "plane" the three products of r = n.(x - q); for "gicp" the
    nine products of d^T M d, brought to the residual's units by a square root (s = sqrt(d^T M d) >= |d| / sqrt(2) since S <= 2 I, so the
    root amplifies a relative error of the sum by at most sqrt(cond(M)) / 2: orders of magnitude inside the bound)"""
    nt = len(c["pct"])
    m = a.inlier & (a.dist2 <= f32(max_dist2)) & (a.indices < nt)
    j = np.where(m, a.indices, 0)
    m &= tn[j].any(axis=1)
    if model == "gicp":
        m &= sn.any(axis=1)
    x = (npr.rot_apply(np.asarray(R, f32), c["pcs"]) + np.asarray(t, f32)[None, :]).astype(f32)[m].astype(f64)
    q, n = c["pct"][a.indices[m]].astype(f64), tn[a.indices[m]].astype(f64)
    if model == "plane":
        r = (n * (x - q)).sum(axis=1)
        J = np.hstack([np.cross(x, n), n])
        terms = np.stack([J[:, i] * J[:, k] for i in range(6) for k in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r], axis=1)
        return m, terms, r, np.abs(n * (x - q)).sum(axis=1)
    terms = gicp_summands(x, q, n, sn[m].astype(f64), np.asarray(R, f32), eps)
    mm = sn[m].astype(f64) @ np.asarray(R, f64).T
    M = np.linalg.inv(2 * np.eye(3)[None] - (1 - eps) * (n[:, :, None] * n[:, None, :] + mm[:, :, None] * mm[:, None, :]))
    d = x - q
    mag = np.abs(d[:, :, None] * M * d[:, None, :]).sum(axis=(1, 2))
    return m, terms, np.sqrt(np.maximum(terms[:, 27], 0.0)), np.sqrt(mag)


def _ctx(fg, c, trimmed, k=10, source_normals=True):
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(int(0.8 * len(c["pcs"])))
    reg.set_target_normals(k=k)
    if source_normals:
        reg.set_source_normals(k=k)
    return reg


# ---- 4. the residuals, 5. the moments, 6. the scale ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,ns", SIZES)
def test_residuals_weights_moments_and_scale_match_numpy_and_leave_the_context_alone(fg, gpu_required, nt, ns, model):
    c = _case(fg, nt, ns)
    worst_res = worst_m = 0.0
    for trimmed in (False, True):
        reg = _ctx(fg, c, trimmed)
        tn, sn = reg.target_normals(), reg.source_normals()
        for R, t in ((c["R"].astype(f32), c["t"].astype(f32)), off_pose(c, 5.0, 0.0)):
            before = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t))
            a = before[2]
            for max_d2 in (np.inf, float(np.sort(a.dist2)[ns // 2])):
                mask, terms, s_np, s_mag = numpy_pairs(c, a, tn, sn, R, t, max_d2, model)
                n = int(mask.sum())
                assert n > 0
                # the scale: the lower median of the device's own residuals, one product
                res0, w0, cnt0 = reg.robust_residuals(R, t, model, None, 0.0, max_d2, EPS)
                assert np.array_equal(cnt0, mask) and np.array_equal(w0, mask.astype(f64))
                scale = reg.robust_scale(R, t, model, max_d2, EPS)
                assert _bits64(scale) == _bits64(f64(1.4826) * np.sort(np.abs(res0[cnt0]))[(n - 1) // 2])
                # loss none: the plain call's bits
                plain = reg.plane_moments(R, t, max_d2) if model == "plane" else reg.gicp_moments(R, t, max_d2, EPS)
                none = reg.robust_moments(R, t, model, None, 0.0, max_d2, EPS)
                assert np.array_equal(_bits64(none.m), _bits64(plain.m)) and none.correspondences == plain.correspondences == n
                assert none.weight_sum == float(n) and none.loss == "none" and none.points == ns
                for loss in LOSSES:
                    for sc in (scale, 0.25 * scale):
                        res, w, cnt = reg.robust_residuals(R, t, model, loss, sc, max_d2, EPS)
                        assert np.array_equal(cnt, mask), (loss, int((cnt != mask).sum()))
                        assert not res[~cnt].any() and not w[~cnt].any()  # uncounted rows: 0, 0, 0
                        assert np.array_equal(_bits64(res), _bits64(res0))  # the residual does not depend on the loss
                        ratio = float((np.abs(res[cnt] - s_np) / (BOUND * s_mag + 1e-300)).max())
                        worst_res = max(worst_res, ratio)
                        assert (np.abs(res[cnt] - s_np) <= BOUND * s_mag).all(), ratio
                        assert np.array_equal(_bits64(w[cnt]), _bits64(numpy_weight(loss, res[cnt], sc))), loss  # the formula on the DEVICE's residual
                        got = reg.robust_moments(R, t, model, loss, sc, max_d2, EPS)
                        assert got.correspondences == n and got.points == ns and got.loss == loss and got.scale == sc
                        wt = w[cnt][:, None] * terms
                        want, mag = wt.sum(axis=0), np.abs(wt).sum(axis=0)
                        err = np.abs(got.m - want)
                        ratio = float((err / (BOUND * mag + 1e-300)).max())
                        worst_m = max(worst_m, ratio)
                        assert (err <= BOUND * mag).all(), (loss, ratio)
                        assert abs(got.weight_sum - w[cnt].sum()) <= BOUND * w[cnt].sum()
                        assert reg.robust_moments(R, t, model, loss, sc, max_d2, EPS).raw == got.raw  # two calls: the same bytes
                        assert np.array_equal(got.JtJ, got.JtJ.T)
            after = (reg.compute_sse_error(R, t), fg.IterativeClosestPoint3D(reg, None, None, 20, 1e-4, R, t).run(), reg.alignment(R, t))
            assert _bits(before[0]) == _bits(after[0])
            assert _bits(before[1][0]) == _bits(after[1][0]) and np.array_equal(_bits(before[1][1]), _bits(after[1][1])) and np.array_equal(_bits(before[1][2]), _bits(after[1][2]))
            for name in ("indices", "inlier", "target_hit"):
                assert np.array_equal(getattr(before[2], name), getattr(after[2], name)), name
            assert np.array_equal(_bits(before[2].dist2), _bits(after[2].dist2)) and _bits(before[2].sse) == _bits(after[2].sse)
        reg.close()
    print(f"nt {nt} {model}: largest residual error / bound {worst_res:.3g}, largest moment error / bound {worst_m:.3g}")


def test_refusals_come_before_any_device_work_and_a_shorter_struct_is_not_overrun(fg, gpu_required):
    c = _case(fg, 1100, 300)
    R, t = c["R"].astype(f32), c["t"].astype(f32)
    reg = fg.Registration(c["pct"], c["pcs"], c["bounds"], 0.05)
    calls = (lambda **k: reg.robust_moments(R, t, **k), lambda **k: reg.robust_residuals(R, t, **k),
             lambda **k: reg.robust_scale(R, t, **{a: b for a, b in k.items() if a not in ("loss", "scale")}),
             lambda **k: (reg.icp_gicp if k.get("model") == "gicp" else reg.icp_plane)(R, t, loss=k.get("loss"), loss_scale=k.get("scale")))
    for call in calls:
        with pytest.raises(fg.FgoicpError) as e:
            call(model="plane", loss="huber", scale=0.1)
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_target_normals" in str(e.value)
    reg.set_target_normals(k=10)
    for call in calls:
        with pytest.raises(fg.FgoicpError) as e:
            call(model="gicp", loss="huber", scale=0.1)
        assert e.value.status == INVALID_ARG and "fgoicp_ctx_set_source_normals" in str(e.value)
    reg.set_source_normals(k=10)
    for bad in (dict(model=2), dict(model=-1), dict(loss=5), dict(loss=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=np.nan), dict(scale=np.inf),
                dict(max_dist2=-1.0), dict(max_dist2=np.nan), dict(model="gicp", epsilon=0.0), dict(model="gicp", epsilon=2.0)):
        for call in (reg.robust_moments, reg.robust_residuals):
            with pytest.raises(fg.FgoicpError) as e:
                call(R, t, **{**dict(model="plane", loss="tukey", scale=0.1), **bad})
            assert e.value.status == INVALID_ARG, bad
    assert reg.robust_moments(R, t, "plane", None, -5.0).weight_sum == 300.0  # loss none ignores the scale
    with pytest.raises(fg.FgoicpError):
        reg.robust_scale(R, t, 3)
    Rg = fg.to_glm(R)
    fp = fg._lib.c_float_p
    for cls, call in ((fg._lib.RobustMoments, lambda o: reg._lib.fgoicp_robust_moments(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), 1, 1e-3, 4, 0.1, o)),
                      (fg._lib.RobustResult, lambda o: reg._lib.fgoicp_icp_robust(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), 0, 1e-6, float("inf"), 0, 1e-3, 1, 0.1, o))):
        buf = (C.c_ubyte * 512)(*([0xA5] * 512))
        out = C.cast(buf, C.POINTER(cls))
        out.contents.struct_size = 40
        assert call(out) == 0
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 40
        out.contents.struct_size = 0
        assert call(out) == INVALID_ARG and "struct_size" in reg._lib.fgoicp_last_error().decode()
        assert bytes(buf)[40:] == bytes([0xA5] * 472) and out.contents.struct_size == 0
    # any of the three arrays may be NULL
    res = np.empty(300, f64)
    assert reg._lib.fgoicp_robust_residuals(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), 0, 1e-3, 1, 0.1, res.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert np.array_equal(_bits64(res), _bits64(reg.robust_residuals(R, t, "plane", "huber", 0.1)[0]))
    assert reg._lib.fgoicp_robust_residuals(reg._h, Rg.ctypes.data_as(fp), t.ctypes.data_as(fp), float("inf"), 0, 1e-3, 1, 0.1, None, None, None) == 0
    reg.close()


def test_the_scale_is_refused_where_the_median_residual_is_zero(fg, gpu_required):
    c = _case(fg, 1100, 300)
    R, t = c["R"].astype(f32), c["t"].astype(f32)
    src = np.ascontiguousarray(c["pct"][100:400])  # a source placed exactly on target points, at the identity
    reg = fg.Registration(c["pct"], src, c["bounds"], 0.05)
    reg.set_target_normals(k=10)
    reg.set_source_normals(k=10)
    I, z = np.eye(3, dtype=f32), np.zeros(3, f32)
    for model in MODELS:
        res, _, cnt = reg.robust_residuals(I, z, model)
        assert cnt.sum() > 150 and not res.any()
        with pytest.raises(fg.FgoicpError) as e:
            reg.robust_scale(I, z, model)
        assert e.value.status == INVALID_ARG and "pass a scale" in str(e.value)
        with pytest.raises(fg.FgoicpError) as e:
            (reg.icp_plane if model == "plane" else reg.icp_gicp)(I, z, loss="tukey")
        assert e.value.status == INVALID_ARG and "pass a scale" in str(e.value)
        given = (reg.icp_plane if model == "plane" else reg.icp_gicp)(I, z, loss="tukey", loss_scale=0.01)  # a given scale works
        assert given.weight_sum == float(given.correspondences) and not given.scale_estimated and given.loss_scale == 0.01
    reg.close()


# ---- 7. the edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_every_weight_zero_ends_the_loop_at_the_start_pose(fg, gpu_required, model):
    c = _case(fg, 1100, 300)
    reg = _ctx(fg, c, False)
    R0, t0 = off_pose(c, 2.0, 0.01)
    m = reg.robust_moments(R0, t0, model, "tukey", 1e-12)
    assert m.weight_sum == 0.0 and m.correspondences == 300 and not m.m.any()
    got = (reg.icp_plane if model == "plane" else reg.icp_gicp)(R0, t0, max_iter=30, loss="tukey", loss_scale=1e-12)
    assert got.weight_sum == 0.0 and got.iterations <= 1 and got.rank == 0 and got.plane_rmse == 0.0 and got.correspondences == 300
    assert np.array_equal(_bits(got.R), _bits(R0)) and np.array_equal(_bits(got.t), _bits(t0))
    assert _bits(got.sse) == _bits(reg.compute_sse_error(R0, t0)) and got.loss == "tukey" and got.loss_scale == 1e-12 and not got.scale_estimated
    reg.close()


@pytest.mark.parametrize("ns", [1, 257])
def test_one_point_and_one_slot_into_a_new_block(fg, gpu_required, ns):
    c = _case(fg, 1100, 300)
    cc = dict(c, pcs=np.ascontiguousarray(c["pcs"][:ns]) if ns <= 300 else np.ascontiguousarray(np.concatenate([c["pcs"], c["pcs"][:ns - 300] + f32(0.003)])[:ns]))
    assert len(cc["pcs"]) == ns
    reg = fg.Registration(cc["pct"], cc["pcs"], cc["bounds"], 0.05)
    reg.set_target_normals(k=10)
    rng = np.random.default_rng(ns)
    reg.set_source_normals(rng.normal(size=(ns, 3)).astype(f32))  # given: one point has no neighbourhood to estimate from
    tn, sn = reg.target_normals(), reg.source_normals()
    R, t = off_pose(c, 2.0, 0.01)
    a = reg.alignment(R, t)
    for model in MODELS:
        mask, terms, s_np, s_mag = numpy_pairs(cc, a, tn, sn, R, t, np.inf, model)
        assert mask.all()
        scale = 1.4826 * float(np.sort(np.abs(s_np))[(ns - 1) // 2])
        for loss in LOSSES:
            res, w, cnt = reg.robust_residuals(R, t, model, loss, scale)
            assert cnt.all() and (np.abs(res - s_np) <= BOUND * s_mag).all()
            assert np.array_equal(_bits64(w), _bits64(numpy_weight(loss, res, scale)))
            got = reg.robust_moments(R, t, model, loss, scale)
            wt = w[:, None] * terms
            assert got.correspondences == ns and (np.abs(got.m - wt.sum(axis=0)) <= BOUND * np.abs(wt).sum(axis=0)).all()
            assert abs(got.weight_sum - w.sum()) <= BOUND * w.sum()
        plain = reg.plane_moments(R, t) if model == "plane" else reg.gicp_moments(R, t, np.inf, EPS)
        assert np.array_equal(_bits64(reg.robust_moments(R, t, model).m), _bits64(plain.m))
        assert _bits64(reg.robust_scale(R, t, model)) == _bits64(f64(1.4826) * np.sort(np.abs(reg.robust_residuals(R, t, model)[0]))[(ns - 1) // 2])
        loop = (reg.icp_plane if model == "plane" else reg.icp_gicp)(R, t, max_iter=3, loss="cauchy")
        assert loop.correspondences == ns and loop.scale_estimated and 0.0 < loop.weight_sum <= ns
    reg.close()


@pytest.mark.parametrize("model", MODELS)
def test_a_trimmed_context_selects_its_inliers_anew_in_every_iteration_and_loss_none_is_the_plain_loop(fg, gpu_required, model):
    """the loop's first two poses are the steps of robust_moments at the start and at the first pose — each evaluated on the report of
    its own pose, whose inlier sets differ; and with loss none the loop is the plain loop"""
    c = _case(fg, 2500, 700)
    reg = _ctx(fg, c, True)
    R0, t0 = off_pose(c, 5.0, 0.02)
    loop = reg.icp_plane if model == "plane" else reg.icp_gicp
    scale = reg.robust_scale(R0, t0, model)
    pose, masks = (R0, t0), []
    for it in (1, 2):
        m = reg.robust_moments(pose[0], pose[1], model, "huber", scale)
        masks.append(reg.alignment(pose[0], pose[1]).inlier.copy())
        xi, rank = fg.plane_step_from_moments(m.correspondences, m.m)
        assert rank == 6
        pose = fg.plane_apply_step(pose[0], pose[1], xi)
        got = loop(R0, t0, max_iter=it, conv_thr=0.0, loss="huber", loss_scale=scale)
        assert got.iterations == it and np.array_equal(_bits(got.R), _bits(pose[0])) and np.array_equal(_bits(got.t), _bits(pose[1]))
        at = reg.robust_moments(pose[0], pose[1], model, "huber", scale)
        assert got.correspondences == at.correspondences and got.weight_sum == at.weight_sum
        assert got.plane_rmse_scaled == np.sqrt(at.m[27] / at.weight_sum)
    assert (masks[0] != masks[1]).any() and masks[0].sum() == masks[1].sum() == int(0.8 * 700)
    est = loop(R0, t0, max_iter=2, conv_thr=0.0, loss="huber")
    assert est.scale_estimated and est.loss_scale_scaled == scale and np.array_equal(_bits(est.R), _bits(pose[0]))
    # loss none through the C call: the plain loop's pose, counts and sse
    plain = loop(R0, t0, max_iter=30, conv_thr=1e-6)
    raw = fg._lib.RobustResult()
    fp = fg._lib.c_float_p
    Rg = fg.to_glm(R0)
    assert reg._lib.fgoicp_icp_robust(reg._h, Rg.ctypes.data_as(fp), t0.ctypes.data_as(fp), 30, 1e-6, float("inf"), MODELS.index(model), EPS, 0, 0.0, C.byref(raw)) == 0
    none = fg.RobustRefinement(raw, MODELS.index(model))
    assert np.array_equal(_bits(none.R), _bits(plain.R)) and np.array_equal(_bits(none.t), _bits(plain.t))
    assert (none.iterations, none.rank, none.correspondences) == (plain.iterations, plain.rank, plain.correspondences) and _bits(none.sse) == _bits(plain.sse)
    assert none.weight_sum == float(plain.correspondences) and none.plane_rmse_scaled == plain.plane_rmse_scaled and not none.scale_estimated
    reg.close()


# ---- 8. the point of it ---------------------------------------------------------------------------------------------------------------
def numpy_icp_robust(tgt, src, tn, sn, R, t, max_iter, thr, model, loss, scale, eps=EPS):
    """the robust loop in float64 with a brute-force search (numpy_icp_plane / numpy_icp_gicp of the plain tests, every pair's terms times
    its weight at the fixed scale)"""
    tgt, src, tn, sn, R, t = (np.asarray(v, f64) for v in (tgt, src, tn, sn, R, t))
    t2 = (tgt * tgt).sum(axis=1)
    it = 0
    while True:
        x = src @ R.T + t
        j = (t2[None, :] - 2.0 * (x @ tgt.T)).argmin(axis=1)
        keep = tn[j].any(axis=1) & (sn.any(axis=1) if model == "gicp" else True)
        xk, q, n = x[keep], tgt[j[keep]], tn[j[keep]]
        if model == "plane":
            r = (n * (xk - q)).sum(axis=1)
            J = np.hstack([np.cross(xk, n), n])
            w = numpy_weight(loss, r, scale)
            A, b = (J * w[:, None]).T @ J, (J * w[:, None]).T @ r
        else:
            terms = gicp_summands(xk, q, n, sn[keep], R, eps)
            w = numpy_weight(loss, np.sqrt(np.maximum(terms[:, 27], 0.0)), scale)
            s = (w[:, None] * terms).sum(axis=0)
            A = np.zeros((6, 6))
            A[TRIU6] = s[:21]
            A, b = np.triu(A) + np.triu(A, 1).T, s[21:27]
        if it >= max_iter:
            return R, t, it
        ev, V = np.linalg.eigh(A)
        ok = ev > 1e-9 * ev.max()
        xi = -(V[:, ok] / ev[ok]) @ (V[:, ok].T @ b)
        Q = rodrigues(xi[:3])
        R, t = Q @ R, Q @ t + xi[3:]
        it += 1
        if np.linalg.norm(xi[:3]) + np.linalg.norm(xi[3:]) < thr or (it == 1 and ok.sum() < 6):
            max_iter = it  # one more evaluation at the pose returned


def _stray_case(fg):
    """the 2500 / 700 pair with 20 % stray source points, its context with k = 16 normals, the plain loops of the device and of the
    restatement from the 2 degree / 0.01 start — shared by the eight cases below and left unchanged"""
    if "stray" not in _SHARED:
        tgt, src, R_gt, t_gt = fg.synth.make_pair(2500, 700, BOX, seed=3400, overlap=1.0, noise=1e-3, angle_deg=20.0, outlier_frac=0.2)
        pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
        c = dict(pct=pct, pcs=pcs, bounds=bounds, R=R_gt, t=f64(scale) * (t_gt + off_t.astype(f64) - R_gt @ off_s.astype(f64)))
        reg = fg.Registration(pct, pcs, bounds, 0.05)
        reg.set_target_normals(k=16)
        reg.set_source_normals(k=16)
        tn, sn = reg.target_normals(), reg.source_normals()
        R0, t0 = off_pose(c, 2.0, 0.01)
        err = lambda R, t: (rot_angle(R, c["R"]), float(np.linalg.norm(np.asarray(t, f64) - c["t"])))
        plain = {}
        for model in MODELS:
            dev = (reg.icp_plane if model == "plane" else reg.icp_gicp)(R0, t0, max_iter=50, conv_thr=1e-6)
            Rn, tn_, _ = numpy_icp_robust(pct, pcs, tn, sn, R0, t0, 50, 1e-6, model, "none", 1.0)
            plain[model] = (err(dev.R, dev.t), err(Rn, tn_), dev)
        _SHARED["stray"] = dict(c=c, reg=reg, tn=tn, sn=sn, R0=R0, t0=t0, err=err, plain=plain)
    return _SHARED["stray"]


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("model", MODELS)
def test_the_robust_loop_ends_four_times_nearer_the_truth_than_the_plain_loop(fg, gpu_required, model, loss):
    """20 % stray source points, no trimming, estimated scale.  Rotation and translation error of the robust loop are each at most a
    quarter of the plain loop's on the same context (in the fp64 reference the tightest ratio is 8.8: GICP, Huber, rotation), and each
    at most max(2 x the numpy restatement's error with the device's normals and scale, 0.25 x the restatement's plain error)."""
    s = _stray_case(fg)
    reg, c, R0, t0 = s["reg"], s["c"], s["R0"], s["t0"]
    loop = reg.icp_plane if model == "plane" else reg.icp_gicp
    got = loop(R0, t0, max_iter=50, conv_thr=1e-6, loss=loss)
    assert got.scale_estimated and got.loss == loss and got.scaling_factor == 1.0
    assert _bits64(got.loss_scale) == _bits64(reg.robust_scale(R0, t0, model))
    e_dev = s["err"](got.R, got.t)
    e_plain_dev, e_plain_np, plain = s["plain"][model]
    Rn, tn_, itn = numpy_icp_robust(c["pct"], c["pcs"], s["tn"], s["sn"], R0, t0, 50, 1e-6, model, loss, got.loss_scale)
    e_np = s["err"](Rn, tn_)
    print(f"{model} {loss}: scale {got.loss_scale:.4g}, weight {got.weight_sum:.1f} of {got.correspondences}, {got.iterations} steps (plain: {plain.iterations}); "
          f"rotation rad / translation — device {e_dev[0]:.3g} / {e_dev[1]:.3g}, plain device {e_plain_dev[0]:.3g} / {e_plain_dev[1]:.3g}, "
          f"restatement {e_np[0]:.3g} / {e_np[1]:.3g} after {itn} steps, plain restatement {e_plain_np[0]:.3g} / {e_plain_np[1]:.3g}")
    for k in (0, 1):
        assert e_dev[k] <= 0.25 * e_plain_dev[k], (k, e_dev[k], e_plain_dev[k])
        assert e_dev[k] <= max(2 * e_np[k], 0.25 * e_plain_np[k]), (k, e_dev[k], e_np[k], e_plain_np[k])
    assert got.rank == 6 and 0.0 < got.weight_sum < got.correspondences == 700
    assert loop(R0, t0, max_iter=50, conv_thr=1e-6, loss=loss).raw == got.raw  # the same bytes on a second call
    assert _bits(got.sse) == _bits(reg.compute_sse_error(got.R, got.t))
    if loss == "tukey":
        _, w, cnt = reg.robust_residuals(got.R, got.t, model, loss, got.loss_scale)
        print(f"{model} tukey: {int((w[cnt] == 0).sum())} zero weights")
        assert (w[cnt] == 0).sum() >= 70  # at least half of the 140 stray points are cut off entirely (the fp64 reference: 144 and 139 zero weights)


# ---- 9. the solver and the CLI -------------------------------------------------------------------------------------------------------
def test_solver_refine_with_a_loss_answers_in_the_callers_frame_and_leaves_the_solver_alone(fg, gpu_required):
    tgt, src, R_gt, t_gt = fg.synth.workload("tiny", angle_deg=25.0, outlier_frac=0.1)
    s = fg.FastGoICP(tgt, src, 0.05, 1e-3)
    with pytest.raises(fg.FgoicpError) as e:
        s.refine_plane(loss="tukey")
    assert e.value.status == INVALID_ARG and "has not succeeded" in str(e.value)
    R, t = s.run()
    best = (s.get_best_error(), s.get_best_transform())
    scale = s.preproc()["scale"]
    ref = s.refine_plane(loss="tukey")
    assert ref.rank == 6 and ref.iterations >= 1 and ref.scaling_factor == scale and ref.correspondences == len(src)
    assert ref.scale_estimated and ref.loss == "tukey" and 0 < ref.weight_sum < len(src) and ref.model == "plane"
    assert ref.loss_scale == ref.loss_scale_scaled / f64(scale)
    err = lambda Rr, tr: (rot_angle(Rr, R_gt), float(np.linalg.norm(np.asarray(tr, f64) - t_gt)))
    plain = s.refine_plane()
    print(f"tiny with 10 % stray points: search {err(R, t)}, plain refinement {err(plain.R, plain.t)}, tukey {err(ref.R, ref.t)} (files' units), "
          f"scale {ref.loss_scale:.4g}, weight {ref.weight_sum:.1f} of {ref.correspondences}")
    # the callers' frame: the same loop on the solver's context from the best transform taken into its frame, its translation restored by
    # hand (the start differs from the solver's own by a float32 rounding of t: 1e-4 of the box is orders above what that moves the fixed point)
    pp = s.preproc()
    t_s = ((t.astype(f64) - R.astype(f64) @ pp["offset_pcs"].astype(f64) + pp["offset_pct"].astype(f64)) * f64(scale)).astype(f32)
    inner = s.registration.icp_plane(R, t_s, loss="tukey")
    t_back = inner.t.astype(f64) / f64(scale) + inner.R.astype(f64) @ pp["offset_pcs"].astype(f64) - pp["offset_pct"].astype(f64)
    assert rot_angle(inner.R, ref.R) <= 1e-4 and np.abs(t_back - ref.t).max() <= 1e-4 * max(BOX)
    assert abs(inner.loss_scale - ref.loss_scale_scaled) <= 1e-4 * ref.loss_scale_scaled  # a bare context: its own units
    # loss_scale is in the files' units: the estimated scale handed back gives the same bytes but the flag
    again = s.refine_plane(loss="tukey", loss_scale=ref.loss_scale)
    assert not again.scale_estimated and abs(again.loss_scale_scaled - ref.loss_scale_scaled) <= 4 * np.finfo(f64).eps * ref.loss_scale_scaled
    assert rot_angle(again.R, ref.R) <= 1e-5 and np.abs(again.t - ref.t).max() <= 1e-5 * max(BOX)
    half = s.refine_plane(loss="tukey", loss_scale=0.5 * ref.loss_scale)
    assert abs(half.loss_scale_scaled - 0.5 * ref.loss_scale_scaled) <= 4 * np.finfo(f64).eps * ref.loss_scale_scaled and half.weight_sum < ref.weight_sum
    g = s.refine_gicp(loss="cauchy")
    assert g.model == "gicp" and g.gicp_rmse == g.plane_rmse and g.scale_estimated and g.rank == 6
    assert _bits(s.get_best_error()) == _bits(best[0]) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(s.get_best_transform(), best[1]))
    R2, t2 = s.run()
    assert np.array_equal(_bits(R2), _bits(R)) and np.array_equal(_bits(t2), _bits(t))
    s.close()


def test_the_facade_runs_the_robust_refinement_through_the_c_abi(fg, gpu_required, tmp_path):
    """include/fgoicp/fgoicp.hpp refine_robust (tests/host_harness/robust_facade_check.cpp) after FastGoICP::run(), next to refine_plane"""
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0, outlier_frac=0.1)
    lib_dir = os.path.join(REPO, "fast-go-icp_amd", "lib")
    exe = str(tmp_path / "robust_facade_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "host_harness", "robust_facade_check.cpp"), "-o", exe, "-L" + lib_dir, "-lfgoicp_amd", "-Wl,-rpath," + lib_dir], check=True)
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src)
    p = subprocess.run([exe, str(tmp_path / "tgt.txt"), str(tmp_path / "src.txt"), "0.05"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    import json
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["loss"] == 4 and rec["scale_estimated"] == 1 and rec["rank"] == 6 and rec["correspondences"] == len(src) and rec["iterations"] >= 1
    assert 0 < rec["weight_sum"] < len(src) and 0 < rec["loss_scale"] < 0.1 * max(BOX) and 0 < rec["rmse"] <= rec["loss_scale"]  # Tukey: no residual beyond the scale carries weight


def test_cli_writes_the_loss_keys_only_when_a_loss_is_set(fg, gpu_required, tmp_path):
    exe = os.path.join(REPO, "fast-go-icp_amd", "lib", "fast-go-icp")
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0, outlier_frac=0.1)
    _write_txt(tmp_path / "tgt.txt", tgt)
    _write_txt(tmp_path / "src.txt", src[:600])
    runs = (("plain", 'refine = "plane"\nrefine_loss = "none"\nrefine_loss_scale = 0.01\n'), ("tukey", 'refine = "plane"\nrefine_loss = "tukey"\n'),
            ("given", 'refine = "gicp"\nrefine_loss = "huber"\nrefine_loss_scale = 0.002\n'))
    logs = {}
    for tag, extra in runs:
        (tmp_path / f"{tag}.toml").write_text(f'[io]\ntarget = "{tmp_path}/tgt.txt"\nsource = "{tmp_path}/src.txt"\noutput = "{tmp_path}/{tag}_out.toml"\n'
                                              f'[params]\nlut_resolution = 0.05\nmse_threshold = 0.001\nseed = 3\n{extra}')
        p = subprocess.run([exe, "-c", str(tmp_path / f"{tag}.toml")], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        logs[tag] = [ln for ln in (p.stdout + p.stderr).splitlines() if "refinement:" in ln]
        assert len(logs[tag]) == 1
    lines = lambda name: [ln for ln in (tmp_path / name).read_text().splitlines() if not ln.startswith("seconds")]
    out = {tag: lines(f"{tag}_out.toml") for tag, _ in runs}
    keys = lambda ls: [ln.split(" = ")[0] for ln in ls[ls.index("[refined]") + 1:] if " = " in ln]
    assert " loss" not in logs["plain"][0] and not any(ln.startswith(("loss", "weight_sum")) for ln in out["plain"])  # "none": today's bytes
    assert keys(out["plain"]) == ["rotation", "translation", "plane_rmse", "iterations", "rank", "correspondences"]
    assert keys(out["tukey"]) == keys(out["plain"]) + ["loss", "loss_scale", "weight_sum"]
    assert keys(out["given"]) == ["rotation", "translation", "gicp_rmse", "iterations", "rank", "correspondences", "loss", "loss_scale", "weight_sum"]
    for tag in ("tukey", "given"):  # every line in front of [refined] is the plain run's
        cut = out[tag].index("[refined]")
        assert out[tag][:cut] == out["plain"][:out["plain"].index("[refined]")]
    val = lambda tag, key: [ln for ln in out[tag] if ln.startswith(key + " = ")][0].split(" = ")[1]
    assert val("tukey", "loss") == '"tukey"' and val("given", "loss") == '"huber"'
    assert float(val("given", "loss_scale")) == pytest.approx(0.002, rel=1e-6) and 0 < float(val("tukey", "loss_scale")) < 0.01
    assert 0 < float(val("tukey", "weight_sum")) < 600 and 0 < float(val("given", "weight_sum")) <= 600
    import re
    assert re.search(r"Point-to-plane refinement: \d+ iterations, rank \d, \d+ correspondences, plane RMSE \S+, tukey loss, scale \S+ \(estimated\), weight \S+ of \d+$", logs["tukey"][0]), logs["tukey"][0]
    assert re.search(r"Generalized-ICP refinement: .*plane-to-plane RMSE \S+, huber loss, scale 0\.002 \(given\), weight \S+ of \d+$", logs["given"][0]), logs["given"][0]
