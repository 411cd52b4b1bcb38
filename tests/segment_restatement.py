"""The numpy restatement of fgoicp_segment_planes, written from the definition in include/fgoicp_amd.h (not a test file: the helper of
tests/test_segment_host.py and tests/test_gpu_segment.py).  Everything is numpy float64 on the float32 coordinates converted to float64,
one operation per numpy call in the order the header writes them; the draws are numpy uint64, which wraps mod 2^64; the refit's sums are
oracle.np_restatement.fixed_order_sum as it stands, its eigenvector numpy.linalg.eigh."""
import numpy as np

from oracle import np_restatement as npr

f32, f64, u64 = np.float32, np.float64, np.uint64
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    z = np.asarray(z, u64)
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def draws(seed, peel, K, m):
    """(K, 3) positions in [0, m)"""
    with np.errstate(over="ignore"):
        h = np.arange(K, dtype=u64)
        out = np.empty((K, 3), np.int64)
        for s in range(3):
            c = (u64(peel) * u64(K) + h) * u64(3) + u64(s + 1)
            u = mix64(u64(seed) + u64(GOLDEN) * c)
            out[:, s] = (((u >> u64(32)) * u64(m)) >> u64(32)).astype(np.int64)
    return out


def hypotheses(P, K, seed=0, peel=0, cand=None):
    """(sample (K, 3) caller indices, plane (K, 4) float64, degenerate (K,) bool); a degenerate hypothesis has the plane +0.0"""
    cand = np.arange(len(P)) if cand is None else np.asarray(cand, np.int64)
    idx = cand[draws(seed, peel, K, len(cand))]
    X = P.astype(f64)
    a, b, c = X[idx[:, 0]], X[idx[:, 1]], X[idx[:, 2]]
    e1, e2 = b - a, c - a
    Nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    Ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    Nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    L2 = (Nx * Nx + Ny * Ny) + Nz * Nz
    deg = (idx[:, 0] == idx[:, 1]) | (idx[:, 0] == idx[:, 2]) | (idx[:, 1] == idx[:, 2]) | ~(L2 > 0) | ~np.isfinite(L2)
    with np.errstate(all="ignore"):
        ln = np.sqrt(L2)
        nx, ny, nz = Nx / ln, Ny / ln, Nz / ln
        d = -((nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2])
    plane = np.stack([nx, ny, nz, d], 1)
    plane[deg] = 0.0
    return idx, plane, deg


def residual(P, plane):
    """r_i under one plane (4,), float64 (n,)"""
    X = P.astype(f64)
    return ((plane[0] * X[:, 0] + plane[1] * X[:, 1]) + plane[2] * X[:, 2]) + plane[3]


def inliers(P, plane, T, free):
    return free & (np.abs(residual(P, plane)) <= f64(T))


def counts(P, plane, deg, T, free, chunk=1 << 22):
    """count_h for every hypothesis, in row chunks of the K x m matrix"""
    X = P.astype(f64)[free]
    K = len(plane)
    out = np.zeros(K, np.int64)
    step = max(1, chunk // max(1, len(X)))
    for a in range(0, K, step):
        p = plane[a:a + step]
        r = ((p[:, 0:1] * X[None, :, 0] + p[:, 1:2] * X[None, :, 1]) + p[:, 2:3] * X[None, :, 2]) + p[:, 3:4]
        out[a:a + step] = (np.abs(r) <= f64(T)).sum(1)
    out[deg] = 0
    return out


def moments(P, mask, pivot):
    """(sum_u (3,), sum_uu (6,)) of the masked points in the device's fixed order: the term of caller index i at position i"""
    U = P.astype(f64) - pivot
    t = np.zeros((len(P), 9))
    u = U[mask]
    t[mask] = np.stack([u[:, 0], u[:, 1], u[:, 2], u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2], u[:, 2] * u[:, 2]], 1)
    s = npr.fixed_order_sum(t, 256)
    return s[:3], s[3:]


def covariance(count, sum_u, sum_uu):
    mean = sum_u / f64(count)
    xx, xy, xz, yy, yz, zz = sum_uu / f64(count)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - np.outer(mean, mean), mean


def fit_eigh(count, pivot, sum_u, sum_uu, toward=None):
    """(plane (4,), eigenvalues ascending) by numpy.linalg.eigh on the same moments"""
    C, mean = covariance(count, np.asarray(sum_u, f64), np.asarray(sum_uu, f64))
    w, V = np.linalg.eigh(C)
    nv = V[:, 0]
    if toward is not None and nv @ np.asarray(toward, f64)[:3] < 0:
        nv = -nv
    q = np.asarray(pivot, f64) + mean
    return np.array([nv[0], nv[1], nv[2], -((nv[0] * q[0] + nv[1] * q[1]) + nv[2] * q[2])]), w


def fit_bound(w):
    """the derived bound of the refit against eigh: 1e3 ulp amplified by the largest eigenvalue over the gap below the second"""
    return 1e3 * 2.0 ** -52 * w[2] / (w[1] - w[0])


def segment(P, T, K, seed=0, max_planes=1, min_inliers=0, refit=True, final_planes=None):
    """The whole definition.  final_planes: the refitted planes a device call returned — the refit's eigenvector is the one step numpy cannot
    restate to the bit, so the labels are evaluated under the returned doubles and the returned plane is compared with `eigh_plane` within
    the derived bound.  Without it the eigh plane is final.  Returns dict(label, models, count_vectors)."""
    T = f64(f32(T))
    n = len(P)
    label = np.full(n, -1, np.int32)
    models, vectors = [], []
    for j in range(max_planes):
        free = label < 0
        cand = np.flatnonzero(free)
        if len(cand) < 3:
            break
        idx, plane, deg = hypotheses(P, K, seed, j, cand)
        cnt = counts(P, plane, deg, T, free)
        vectors.append(cnt)
        win = int(np.argmax(cnt))  # argmax: the first of equal counts, the lowest h
        if cnt[win] < max(min_inliers, 3):
            break
        m = dict(candidates=len(cand), sample=idx[win].astype(np.uint32), hypothesis=win, hypothesis_inliers=int(cnt[win]), hypothesis_plane=plane[win].copy(),
                 pivot=P[idx[win, 0]].astype(f64), sum_u=np.zeros(3), sum_uu=np.zeros(6), ties=int((cnt == cnt[win]).sum()))
        final = plane[win].copy()
        if refit:
            mask = inliers(P, plane[win], T, free)
            assert int(mask.sum()) == cnt[win]
            m["sum_u"], m["sum_uu"] = moments(P, mask, m["pivot"])
            m["eigh_plane"], m["eigenvalues"] = fit_eigh(cnt[win], m["pivot"], m["sum_u"], m["sum_uu"], plane[win])
            final = m["eigh_plane"] if final_planes is None else np.asarray(final_planes[j], f64)
        m["plane"] = final
        on = inliers(P, final, T, free)
        m["inliers"] = int(on.sum())
        label[on] = j
        models.append(m)
    return dict(label=label, models=models, count_vectors=vectors)
