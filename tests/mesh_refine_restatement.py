"""numpy restatement of fgoicp_mesh_pair_terms, fgoicp_mesh_moments and fgoicp_mesh_refine (include/fgoicp_amd.h): IEEE fp64 on the fp32
values, one rounding per operation in the order the header writes them.  Built on tests/mesh_distance_restatement.py (every face for every
point, no tree) and tests/mesh_restatement.py.  tests/test_mesh_refine_host.py checks the host function against it,
tests/test_gpu_mesh_refine.py the device."""
import numpy as np

from oracle.np_restatement import fixed_order_sum
from tests import mesh_distance_restatement as md
from tests.test_robust_host import numpy_weight

f32, f64 = np.float32, np.float64


def moved(P, R, t):
    """x[a] = (float)((((double)R[a][0] px + (double)R[a][1] py) + (double)R[a][2] pz) + (double)t[a]) — (n, 3) float32"""
    p = np.asarray(P, f32).astype(f64)
    Rm, tv = np.asarray(R, f32).astype(f64).reshape(3, 3), np.asarray(t, f32).astype(f64).reshape(3)
    return np.stack([((Rm[a, 0] * p[:, 0] + Rm[a, 1] * p[:, 1]) + Rm[a, 2] * p[:, 2]) + tv[a] for a in range(3)], 1).astype(f32)


def jacobian(x, g):
    """J = [(x cross g)^T, g^T], (n, 6)"""
    return np.stack([x[:, 1] * g[:, 2] - x[:, 2] * g[:, 1], x[:, 2] * g[:, 0] - x[:, 0] * g[:, 2], x[:, 0] * g[:, 1] - x[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]], 1)


def terms28(x, g, s, w=None):
    """the upper triangle of J^T J row by row, J^T s, s s — (n, 28) — each times w when w is given"""
    J = jacobian(x, g)
    v = np.stack([J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * s for a in range(6)] + [s * s], 1)
    return v if w is None else v * np.asarray(w, f64)[:, None]


def pair_terms(x, a, b, c, loss=None, scale=None):
    """x, a, b, c: (n, 3) values of fp32 numbers.  dict(closest (n, 3) float64, dist2, region, g, s, w, v (n, 28))"""
    x, a, b, c = (np.atleast_2d(np.asarray(q, f32)).astype(f64) for q in (x, a, b, c))
    closest, d2, region, _ = md.point_triangle(x, a, b, c)
    d = x - closest
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    off = (region != 0) & (d2 > 0.0)
    with np.errstate(all="ignore"):
        g = np.where(off[:, None], d / np.sqrt(d2)[:, None], n / np.sqrt(n2)[:, None])
    s = md.dot(g, d)
    weighted = loss not in (None, "none")
    w = numpy_weight(loss, s, scale) if weighted else np.ones_like(s)
    return dict(closest=closest, dist2=d2, region=region, g=g, s=s, w=w, v=terms28(x, g, s, w if weighted else None))


def per_point(V, T, P, R, t, max_distance=None, loss=None, scale=None):
    """every per-point output of fgoicp_mesh_moments, caller order, by the search that tests every face"""
    x = moved(P, R, t)
    d2, face, closest32, region, _, info = md.mesh_distance(V, T, x)
    X, Tn = np.asarray(V, f32), np.asarray(T, np.int64)
    o = pair_terms(x, X[Tn[face, 0]], X[Tn[face, 1]], X[Tn[face, 2]], loss, scale)
    assert np.array_equal(o["dist2"], d2) and np.array_equal(o["region"], region)
    thr = f64(np.float32(max_distance)) * f64(np.float32(max_distance)) if max_distance is not None and max_distance > 0 else f64(np.inf)
    counted = d2 <= thr
    o.update(x=x, face=face, closest32=closest32, counted=counted, max_dist2=thr, info=info, residual=np.where(counted, o["s"], 0.0), weight=np.where(counted, o["w"], 0.0))
    return o


def rows30(v28, w, dist2, counted):
    """what every slot hands the reduction: its 28 terms, its weight, its dist2; +0.0 thirty times when it is not counted"""
    rows = np.concatenate([v28, np.asarray(w, f64)[:, None], np.asarray(dist2, f64)[:, None]], 1)
    return np.where(np.asarray(counted, bool)[:, None], rows, 0.0)


def moments(V, T, P, R, t, max_distance=None, loss=None, scale=None, order=None):
    """dict(correspondences, m (28,), weight_sum, sum_dist2) added in the device's fixed order over the slots `order` (None: caller order)"""
    o = per_point(V, T, P, R, t, max_distance, loss, scale)
    rows = rows30(o["v"], o["w"], o["dist2"], o["counted"])
    sums = fixed_order_sum(rows if order is None else rows[np.asarray(order, np.int64)])
    return dict(correspondences=int(o["counted"].sum()), m=sums[:28], weight_sum=sums[28], sum_dist2=sums[29], per_point=o)


def mad_scale(residual, counted):
    a = np.sort(np.abs(np.asarray(residual, f64)[np.asarray(counted, bool)]))
    return f64(1.4826) * a[(len(a) - 1) // 2]


def refine(fg, V, T, P, R, t, max_iter=30, conv_thr=1e-6, max_distance=None, loss=None, scale=None):
    """the loop of fgoicp_mesh_refine over moments() with the library's host step functions (no device): dict(R, t, iterations, rank,
    correspondences, mesh_rmse, rms_distance, weight_sum, loss_scale)"""
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32).reshape(3)
    if loss not in (None, "none") and not (scale is not None and scale > 0):
        o = per_point(V, T, P, R, t, max_distance)
        scale = mad_scale(o["s"], o["counted"])
    iterations, rank, stop = 0, 0, False
    while True:
        m = moments(V, T, P, R, t, max_distance, loss, scale)
        if stop or iterations >= max_iter or m["correspondences"] == 0 or m["weight_sum"] == 0.0:
            break
        xi, rank = fg.plane_step_from_moments(m["correspondences"], m["m"])
        R, t = fg.plane_apply_step(R, t, xi)
        iterations += 1
        step = np.sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) + np.sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])
        stop = bool(step < f64(np.float32(conv_thr))) or (iterations == 1 and rank < 6)
    n = m["correspondences"]
    return dict(R=R, t=t, iterations=iterations, rank=rank, correspondences=n, weight_sum=m["weight_sum"], loss_scale=scale,
                mesh_rmse=float(np.sqrt(m["m"][27] / m["weight_sum"])) if m["weight_sum"] > 0.0 else 0.0, rms_distance=float(np.sqrt(m["sum_dist2"] / f64(n))) if n else 0.0)
