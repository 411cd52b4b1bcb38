"""Python mirror of the reference's operator classes for the hot path — same names, argument
meaning and return order as fgoicp/registration.hpp and fgoicp/icp3d.hpp — over the C ABI of
libfgoicp_amd.so.  Every call runs on the MI355X; nothing here computes on the CPU."""
import ctypes as C

import numpy as np

from . import _lib
from .nodes import RotNode, from_glm, pack_tnodes, to_glm


def _fp(a):
    return a.ctypes.data_as(_lib.c_float_p)


def _cloud(pc):
    a = np.ascontiguousarray(pc, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("point cloud must be (n, 3)")
    return a


class StreamPool:
    """Kept for signature compatibility with icp::StreamPool (fgoicp/common.hpp:138-164); the
    context owns its HIP stream, a batch is one fused launch instead of 32 per-stream launches."""

    def __init__(self, size=32):
        self.size = size


def cloud_stats(points):
    """fgoicp_cloud_stats: count, centroid, bounding box, largest centred coordinate, RMS radius of a raw cloud (host side)."""
    p = _cloud(points)
    st = _lib.CloudStats()
    _lib.check(_lib.load().fgoicp_cloud_stats(_fp(p), len(p), C.byref(st)), "fgoicp_cloud_stats")
    return dict(n=int(st.n), centroid=np.array(st.centroid, np.float32), min=np.array(st.min, np.float32), max=np.array(st.max, np.float32),
                max_abs_centred=float(st.max_abs_centred), rms_radius=float(st.rms_radius))


def voxel_downsample(points, voxel_size, origin=None, device=0, return_map=False):
    """fgoicp_voxel_downsample: one point per occupied cell of a grid of `voxel_size` — the centroid of the cell's members, rows in ascending
    (z, y, x) cell order — as an (m, 3) float32 array.  origin: 3 floats, None = the cloud's per-axis minimum.  return_map=True returns
    (points, voxel_of_point (n,) uint32, counts (m,) uint32, info) with info = dict(points, voxels, max_points_per_voxel, origin, voxel_size)."""
    p = _cloud(points)
    o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    n = len(p)
    out = np.empty((n, 3), np.float32)
    vop = np.empty(n, np.uint32) if return_map else None
    cnt = np.empty(n, np.uint32) if return_map else None
    u32 = lambda a: None if a is None else a.ctypes.data_as(_lib.c_uint32_p)
    info = _lib.VoxelInfo()
    _lib.check(_lib.load().fgoicp_voxel_downsample(_fp(p) if n else None, n, float(voxel_size), None if o is None else _fp(o), int(device), _fp(out), n, u32(vop), u32(cnt),
                                                   C.byref(info)), "fgoicp_voxel_downsample")
    m = int(info.voxels)
    out = out[:m].copy()
    if not return_map:
        return out
    return out, vop, cnt[:m].copy(), dict(points=int(info.points), voxels=m, max_points_per_voxel=int(info.max_points_per_voxel),
                                          origin=np.array(info.origin, np.float32), voxel_size=float(info.voxel_size))


def _remove_outliers(points, mode, k, param, device, return_map):
    p = _cloud(points)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    n = len(p)
    out = np.empty((n, 3), np.float32)
    idx = np.empty(n, np.uint32) if return_map else None
    keep = np.empty(n, np.uint8) if return_map else None
    mean_dist = np.empty(n, np.float64) if return_map else None
    kth = np.empty(n, np.float32) if return_map else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    info = _lib.OutlierInfo()
    _lib.check(_lib.load().fgoicp_remove_outliers(_fp(p) if n else None, n, mode, int(k), float(param), int(device), _fp(out), n, ptr(idx, _lib.c_uint32_p),
                                                  ptr(keep, _lib.c_uint8_p), ptr(mean_dist, _lib.c_double_p), ptr(kth, _lib.c_float_p), C.byref(info)),
               "fgoicp_remove_outliers")
    m = int(info.kept)
    out = out[:m].copy()
    if not return_map:
        return out
    return out, keep.astype(bool), idx[:m].copy(), mean_dist, kth, dict(points=int(info.points), kept=m, mode=int(info.mode), k=int(info.k), mean=float(info.mean),
                                                                        stddev=float(info.stddev), threshold=float(info.threshold), radius2=float(info.radius2))


def remove_statistical_outliers(points, k=20, std_ratio=2.0, device=0, return_map=False):
    """fgoicp_remove_outliers, FGOICP_OUTLIER_STATISTICAL: keeps the points whose mean distance to their k nearest points (themselves included)
    is at most mean + std_ratio * stddev of that statistic over the cloud — the kept points in caller order as an (m, 3) float32 array.
    return_map=True returns (kept, keep_mask (n,) bool, kept_index (m,) uint32, mean_dist (n,) float64, kth_dist2 (n,) float32, info) with
    info = dict(points, kept, mode, k, mean, stddev, threshold, radius2)."""
    return _remove_outliers(points, _lib.OUTLIER_STATISTICAL, k, std_ratio, device, return_map)


def remove_radius_outliers(points, k, radius, device=0, return_map=False):
    """fgoicp_remove_outliers, FGOICP_OUTLIER_RADIUS: keeps the points with at least k points of the cloud (themselves included) within `radius`;
    the returns are those of remove_statistical_outliers."""
    return _remove_outliers(points, _lib.OUTLIER_RADIUS, k, radius, device, return_map)


def farthest_point_sample(points, m, start_index=0, device=0, return_map=False):
    """fgoicp_farthest_point_sample: exactly m points of the cloud, each the farthest from those picked before it (ties to the lowest index),
    from points[start_index] on, in pick order, as an (m, 3) float32 array; every prefix is the sampling of that size.  return_map=True returns
    (samples, sample_index (m,) uint32, pick_dist2 (m,) float32, min_dist2 (n,) float32, owner (n,) uint32, info) with
    info = dict(points, samples, start_index, next_index, cover_dist2).  m DEPENDENT steps over the n points."""
    p = _cloud(points)
    for name, v in (("m", m), ("start_index", start_index)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer")
    n = len(p)
    if not 1 <= m <= n:
        raise ValueError(f"m must lie in [1, {n}], the number of points")
    if not 0 <= start_index < n:
        raise ValueError(f"start_index must lie in [0, {n})")
    m = int(m)
    out = np.empty((m, 3), np.float32)
    idx = np.empty(m, np.uint32) if return_map else None
    pick = np.empty(m, np.float32) if return_map else None
    mind = np.empty(n, np.float32) if return_map else None
    owner = np.empty(n, np.uint32) if return_map else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    info = _lib.FpsInfo()
    _lib.check(_lib.load().fgoicp_farthest_point_sample(_fp(p), n, m, int(start_index), int(device), _fp(out), ptr(idx, _lib.c_uint32_p), ptr(pick, _lib.c_float_p),
                                                        ptr(mind, _lib.c_float_p), ptr(owner, _lib.c_uint32_p), C.byref(info)), "fgoicp_farthest_point_sample")
    if not return_map:
        return out
    return out, idx, pick, mind, owner, dict(points=int(info.points), samples=int(info.samples), start_index=int(info.start_index), next_index=int(info.next_index),
                                             cover_dist2=np.float32(info.cover_dist2))


def _mesh(vertices, triangles):
    v = _cloud(vertices)
    t = np.asarray(triangles)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError("triangles must be an (nf, 3) array of integers")
    if t.size and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
        raise ValueError("a triangle index must lie in [0, 2^32)")
    return v, np.ascontiguousarray(t, dtype=np.uint32)


def sample_mesh(vertices, triangles, m, seed=0, device=0, return_map=False):
    """fgoicp_mesh_sample: m points on the surface of the triangle mesh (vertices (nv, 3) float32, triangles (nf, 3) vertex indices), spread
    over the faces in proportion to their area, as an (m, 3) float32 array.  Sample k is a function of (mesh, seed, k): two calls return the
    same bytes and every prefix is the sampling of that size.  return_map=True returns (points, normals (m, 3) float32 — the unit normal of
    each sample's face, along the winding —, face (m,) uint32, uv (m, 2) float64, face_area (nf,) float64, info) with
    info = dict(vertices, triangles, samples, zero_area, unweighted, weight_total, max_area, area)."""
    v, t = _mesh(vertices, triangles)
    for name, x in (("m", m), ("seed", seed)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"{name} must be an integer")
    if m < 1:
        raise ValueError("m must be at least 1")
    m, nv, nf = int(m), len(v), len(t)
    out = np.empty((m, 3), np.float32)
    nrm = np.empty((m, 3), np.float32) if return_map else None
    face = np.empty(m, np.uint32) if return_map else None
    uv = np.empty((m, 2), np.float64) if return_map else None
    area = np.empty(nf, np.float64) if return_map else None
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    info = _lib.MeshInfo()
    _lib.check(_lib.load().fgoicp_mesh_sample(_fp(v) if nv else None, nv, ptr(t, _lib.c_uint32_p) if nf else None, nf, m, int(seed) & 0xFFFFFFFFFFFFFFFF, int(device), _fp(out),
                                              ptr(nrm, _lib.c_float_p), ptr(face, _lib.c_uint32_p), ptr(uv, _lib.c_double_p), ptr(area, _lib.c_double_p), C.byref(info)),
               "fgoicp_mesh_sample")
    if not return_map:
        return out
    return out, nrm, face, uv, area, dict(vertices=int(info.vertices), triangles=int(info.triangles), samples=int(info.samples), zero_area=int(info.zero_area),
                                          unweighted=int(info.unweighted), weight_total=int(info.weight_total), max_area=float(info.max_area), area=float(info.area))


def sample_mesh_even(vertices, triangles, m, init_factor=5, seed=0, device=0, return_map=False):
    """The Poisson-disk recipe: sample_mesh draws init_factor * m surface samples and farthest_point_sample (start_index 0) thins them to
    exactly m, evenly spread, in pick order.  return_map=True returns (points, normals (m, 3), face (m,), sample_index (m,) uint32 — the row
    of the underlying init_factor * m samples each point is —, info of sample_mesh), normals and faces carried along through sample_index."""
    for name, x in (("m", m), ("init_factor", init_factor)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"{name} must be an integer")
    if m < 1 or init_factor < 1:
        raise ValueError("m and init_factor must be at least 1")
    m = int(m)
    if not return_map:
        return farthest_point_sample(sample_mesh(vertices, triangles, m * int(init_factor), seed=seed, device=device), m, device=device)
    pts, nrm, face, _, _, info = sample_mesh(vertices, triangles, m * int(init_factor), seed=seed, device=device, return_map=True)
    out, idx = farthest_point_sample(pts, m, device=device, return_map=True)[:2]
    return out, nrm[idx], face[idx], idx, info


def mesh_distance(vertices, triangles, points, device=0, return_map=False, brute=False):
    """fgoicp_mesh_distance: the distance from every point to the SURFACE of the triangle mesh (vertices (nv, 3) float32, triangles (nf, 3)
    vertex indices) as an (nq,) float64 array, sqrt(dist2).  return_map=True returns (dist, face (nq,) uint32 — the nearest face, the lowest
    index among equally near ones —, closest (nq, 3) float32, region (nq,) uint8 — 0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex
    a / b / c —, side (nq,) int8 — the side of the winning face's plane, weak where region != 0 —, info) with info = dict(flags, vertices,
    triangles, queries, faces, zero_area, tree_depth, leaf_faces, max_dist2, max_dist2_index, dist2 (nq,) float64).  brute=True tests every
    face for every point without the tree and returns the same bytes."""
    v, t = _mesh(vertices, triangles)
    q = _cloud(points)
    nv, nf, nq = len(v), len(t), len(q)
    dist2 = np.empty(nq, np.float64)
    face = np.empty(nq, np.uint32) if return_map else None
    closest = np.empty((nq, 3), np.float32) if return_map else None
    region = np.empty(nq, np.uint8) if return_map else None
    side = np.empty(nq, np.int8) if return_map else None
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    info = _lib.MeshDistanceInfo()
    _lib.check(_lib.load().fgoicp_mesh_distance(_fp(v) if nv else None, nv, ptr(t, _lib.c_uint32_p) if nf else None, nf, _fp(q) if nq else None, nq,
                                                _lib.MESH_DISTANCE_BRUTE if brute else 0, int(device), ptr(face, _lib.c_uint32_p), ptr(closest, _lib.c_float_p),
                                                ptr(dist2, _lib.c_double_p), ptr(region, _lib.c_uint8_p), ptr(side, C.POINTER(C.c_int8)), C.byref(info)), "fgoicp_mesh_distance")
    dist = np.sqrt(dist2)
    if not return_map:
        return dist
    return dist, face, closest, region, side, dict(flags=int(info.flags), vertices=int(info.vertices), triangles=int(info.triangles), queries=int(info.queries),
                                                   faces=int(info.faces), zero_area=int(info.zero_area), tree_depth=int(info.tree_depth), leaf_faces=int(info.leaf_faces),
                                                   max_dist2=float(info.max_dist2), max_dist2_index=int(info.max_dist2_index), dist2=dist2)


def mesh_deviation(vertices, triangles, source, R, t, device=0, return_map=False, brute=False):
    """mesh_distance of R p + t for every source point p: the deviation of a registered scan from the model's surface — what follows
    FastGoICP.run() or refine_plane() against a mesh's samples.  The moved points are formed in fp64 on the host, per axis
    (R[a, 0]*x + R[a, 1]*y) + R[a, 2]*z + t[a], and rounded to fp32 once."""
    p = _cloud(source).astype(np.float64)
    Rm, tv = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    moved = np.stack([((Rm[a, 0] * p[:, 0] + Rm[a, 1] * p[:, 1]) + Rm[a, 2] * p[:, 2]) + tv[a] for a in range(3)], 1).astype(np.float32)
    return mesh_distance(vertices, triangles, moved, device=device, return_map=return_map, brute=brute)


def point_triangle(p, a, b, c):
    """fgoicp_point_triangle (host only): the closest point of the triangle (a, b, c) to p in the arithmetic the kernel runs —
    (closest (3,) float32, dist2 float64, region int, side int)."""
    x = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (p, a, b, c)]
    closest = np.empty(3, np.float32)
    d2, region, side = C.c_double(), C.c_int(), C.c_int()
    _lib.check(_lib.load().fgoicp_point_triangle(_fp(x[0]), _fp(x[1]), _fp(x[2]), _fp(x[3]), _fp(closest), C.byref(d2), C.byref(region), C.byref(side)), "fgoicp_point_triangle")
    return closest, np.float64(d2.value), int(region.value), int(side.value)


def _loss_args(loss, scale):
    """(code, scale as a float; None -> 0)"""
    return _loss_code(loss), 0.0 if scale is None else float(scale)


def mesh_pair_terms(x, a, b, c, loss=None, scale=None):
    """fgoicp_mesh_pair_terms (host only): what the moved point x contributes against the triangle (a, b, c) in the arithmetic the kernel
    runs — dict(closest (3,) float64, dist2, region, g (3,) float64 — the direction —, s — the residual —, w — its weight —, v (28,)
    float64 — the terms, times w when a loss is set)."""
    p = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (x, a, b, c)]
    code, sc = _loss_args(loss, scale)
    closest, g, v = np.empty(3, np.float64), np.empty(3, np.float64), np.empty(28, np.float64)
    d2, s, w, region = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    dp = lambda arr: arr.ctypes.data_as(_lib.c_double_p)
    _lib.check(_lib.load().fgoicp_mesh_pair_terms(_fp(p[0]), _fp(p[1]), _fp(p[2]), _fp(p[3]), code, sc, dp(closest), C.byref(d2), C.byref(region), dp(g), C.byref(s), C.byref(w),
                                                  dp(v)), "fgoicp_mesh_pair_terms")
    return dict(closest=closest, dist2=np.float64(d2.value), region=int(region.value), g=g, s=np.float64(s.value), w=np.float64(w.value), v=v)


class MeshMomentsResult:
    """EXTENSION (fgoicp_mesh_moments): m (28,) float64 in the layout of PlaneMomentsResult (JtJ, Jtr, sum_r2), points, correspondences,
    weight_sum, sum_dist2, max_dist2 (the fp64 threshold compared with; inf: none), loss (name), scale, flags, vertices, triangles, faces,
    zero_area, tree_depth, leaf_faces; rms_distance = sqrt(sum_dist2 / correspondences).  With return_map=True also, per source point in
    caller order: face, closest (float32), dist2, region, direction, residual, weight, counted (bool), and order — slot k of the sums holds
    the caller's point order[k]."""

    def __init__(self, raw, per_point=None):
        self.m = np.array(raw.m, np.float64)
        self.points, self.correspondences = int(raw.points), int(raw.correspondences)
        self.JtJ = np.zeros((6, 6))
        self.JtJ[np.triu_indices(6)] = self.m[:21]
        self.JtJ = self.JtJ + np.triu(self.JtJ, 1).T
        self.Jtr, self.sum_r2 = self.m[21:27].copy(), float(self.m[27])
        self.weight_sum, self.sum_dist2, self.max_dist2 = float(raw.weight_sum), float(raw.sum_dist2), float(raw.max_dist2)
        self.rms_distance = float(np.sqrt(np.float64(raw.sum_dist2) / np.float64(self.correspondences))) if self.correspondences else 0.0
        self.loss, self.scale, self.flags = LOSS_NAMES.get(int(raw.loss), int(raw.loss)), float(raw.scale), int(raw.flags)
        self.vertices, self.triangles, self.faces, self.zero_area = int(raw.vertices), int(raw.triangles), int(raw.faces), int(raw.zero_area)
        self.tree_depth, self.leaf_faces = int(raw.tree_depth), int(raw.leaf_faces)
        self.raw = bytes(raw)  # the struct as the library filled it (two results of the same inputs are the same bytes)
        for key, value in (per_point or {}).items():
            setattr(self, key, value)


def mesh_moments(vertices, triangles, source, R, t, max_distance=None, loss=None, loss_scale=None, device=0, return_map=False, brute=False):
    """fgoicp_mesh_moments: ONE evaluation of the point-to-mesh normal equations at the pose (R (3, 3), t (3,)) in the mesh's frame — every
    source point moved, its nearest triangle found (the search of mesh_distance), residual and direction taken from the exact closest
    point — as a MeshMomentsResult.  max_distance (None or <= 0: none) leaves out the points farther from the surface; loss / loss_scale as
    robust_weight.  plane_step_from_moments(r.correspondences, r.m) and plane_apply_step give the step and the pose it leads to."""
    v, tr = _mesh(vertices, triangles)
    p = _cloud(source)
    nv, nf, ns = len(v), len(tr), len(p)
    Rg, tt = to_glm(R), np.ascontiguousarray(t, np.float32).reshape(3)
    code, sc = _loss_args(loss, loss_scale)
    per = None
    if return_map:
        per = dict(face=np.empty(ns, np.uint32), closest=np.empty((ns, 3), np.float32), dist2=np.empty(ns, np.float64), region=np.empty(ns, np.uint8),
                   direction=np.empty((ns, 3), np.float64), residual=np.empty(ns, np.float64), weight=np.empty(ns, np.float64), counted=np.empty(ns, np.uint8),
                   order=np.empty(ns, np.uint32))
    ptr = lambda key, ty: None if per is None else per[key].ctypes.data_as(ty)
    raw = _lib.MeshMoments()
    _lib.check(_lib.load().fgoicp_mesh_moments(_fp(v) if nv else None, nv, tr.ctypes.data_as(_lib.c_uint32_p) if nf else None, nf, _fp(p) if ns else None, ns, _fp(Rg), _fp(tt),
                                               0.0 if max_distance is None else float(max_distance), code, sc, _lib.MESH_DISTANCE_BRUTE if brute else 0, int(device),
                                               ptr("face", _lib.c_uint32_p), ptr("closest", _lib.c_float_p), ptr("dist2", _lib.c_double_p), ptr("region", _lib.c_uint8_p),
                                               ptr("direction", _lib.c_double_p), ptr("residual", _lib.c_double_p), ptr("weight", _lib.c_double_p),
                                               ptr("counted", _lib.c_uint8_p), ptr("order", _lib.c_uint32_p), C.byref(raw)), "fgoicp_mesh_moments")
    if per is not None:
        per["counted"] = per["counted"].astype(bool)
    return MeshMomentsResult(raw, per)


class MeshRefinement:
    """EXTENSION (fgoicp_mesh_refine): R (3, 3), t (3,) — the refined pose in the mesh's frame; iterations; rank of the last solve (6: well
    posed); points; correspondences counted at the returned pose; mesh_rmse = sqrt(sum w s^2 / sum w) there; rms_distance =
    sqrt(sum dist2 / correspondences) there — the rms of mesh_deviation at (R, t) when no max_distance is set; weight_sum; loss (name);
    loss_scale — the scale the loop ran with; scale_estimated; triangles, faces, zero_area of the mesh."""

    def __init__(self, raw):
        self.R, self.t = from_glm(np.array(raw.R, np.float32)), np.array(raw.t, np.float32)
        self.iterations, self.rank, self.points, self.correspondences = int(raw.iterations), int(raw.rank), int(raw.points), int(raw.correspondences)
        self.weight_sum, self.mesh_rmse, self.rms_distance = float(raw.weight_sum), float(raw.mesh_rmse), float(raw.rms_distance)
        self.loss, self.loss_scale, self.scale_estimated = LOSS_NAMES.get(int(raw.loss), int(raw.loss)), float(raw.loss_scale), bool(raw.scale_estimated)
        self.triangles, self.faces, self.zero_area = int(raw.triangles), int(raw.faces), int(raw.zero_area)
        self.raw = bytes(raw)


def refine_to_mesh(vertices, triangles, source, R, t, max_iter=30, conv_thr=1e-6, max_distance=None, loss=None, loss_scale=None, device=0, brute=False):
    """fgoicp_mesh_refine: the pose near (R, t) that minimises the deviation map — the squared distances from the moved source points to the
    SURFACE of the mesh — by Gauss-Newton steps over mesh_moments, as a MeshRefinement.  The tree is built and the points are sorted once;
    an iteration is one kernel launch.  loss_scale None or <= 0 with a loss: estimated at the start pose.

    After a registration against a mesh's samples the caller writes (poses in the frame of the files, which is the mesh's):

        R, t = solver.run()                    # or fine = solver.refine_plane(); R, t = fine.R, fine.t
        fine = fg.refine_to_mesh(V, T, source, R, t)
        dist = fg.mesh_deviation(V, T, source, fine.R, fine.t)   # its rms is fine.rms_distance"""
    v, tr = _mesh(vertices, triangles)
    p = _cloud(source)
    nv, nf, ns = len(v), len(tr), len(p)
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer")
    Rg, tt = to_glm(R), np.ascontiguousarray(t, np.float32).reshape(3)
    code, sc = _loss_args(loss, loss_scale)
    raw = _lib.MeshRefineResult()
    _lib.check(_lib.load().fgoicp_mesh_refine(_fp(v) if nv else None, nv, tr.ctypes.data_as(_lib.c_uint32_p) if nf else None, nf, _fp(p) if ns else None, ns, _fp(Rg), _fp(tt),
                                              int(max_iter), float(conv_thr), 0.0 if max_distance is None else float(max_distance), code, sc,
                                              _lib.MESH_DISTANCE_BRUTE if brute else 0, int(device), C.byref(raw)), "fgoicp_mesh_refine")
    return MeshRefinement(raw)


def cluster_dbscan(points, eps, min_points=10, keep_min_size=0, device=0, return_map=False):
    """fgoicp_cluster_dbscan: density clustering of the cloud (a point is core when at least min_points points, itself included, lie within
    eps; clusters are the connected components of the core points, numbered by their lowest index; a border point joins its nearest core
    neighbour's cluster; the rest is noise) — returns the points of the largest cluster (keep_min_size=0) or of every cluster of at least
    keep_min_size points, in caller order, as an (m, 3) float32 array.  return_map=True returns (kept, label (n,) int32 with -1 = noise,
    neighbours (n,) uint32, cluster_size (clusters,) uint64, kept_index (m,) uint32, info) with info = dict(points, core_points, border_points,
    noise_points, clusters, largest_label, largest_size, kept, keep_min_size, min_points, eps2, rounds)."""
    p = _cloud(points)
    for name, v in (("min_points", min_points), ("keep_min_size", keep_min_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an integer")
    if keep_min_size < 0:
        raise ValueError("keep_min_size must not be negative")
    if not -2 ** 31 <= min_points < 2 ** 31:
        raise ValueError("min_points does not fit an int")
    n = len(p)
    out = np.empty((n, 3), np.float32)
    idx = np.empty(n, np.uint32) if return_map else None
    label = np.empty(n, np.int32) if return_map else None
    nbr = np.empty(n, np.uint32) if return_map else None
    size = np.empty(n, np.uint64) if return_map else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    info = _lib.ClusterInfo()
    _lib.check(_lib.load().fgoicp_cluster_dbscan(_fp(p) if n else None, n, float(eps), int(min_points), int(keep_min_size), int(device), _fp(out), n, ptr(idx, _lib.c_uint32_p),
                                                 ptr(label, C.POINTER(C.c_int32)), ptr(nbr, _lib.c_uint32_p), ptr(size, C.POINTER(C.c_uint64)), n, C.byref(info)),
               "fgoicp_cluster_dbscan")
    m = int(info.kept)
    out = out[:m].copy()
    if not return_map:
        return out
    d = {name: int(getattr(info, name)) for name, _ in _lib.ClusterInfo._fields_ if name not in ("struct_size", "eps2")}
    d["eps2"] = np.float32(info.eps2)
    return out, label, nbr, size[:int(info.clusters)].copy(), idx[:m].copy(), d


SEGMENT_TILE = 1024   # points per block of the scoring kernel (csrc/device/segment_score.hpp kSegTile)
SEGMENT_CHUNK = 256   # hypotheses the scoring kernel stages per pass over its tile (kSegChunk)


def _whole(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer")
    if not lo <= v <= hi:
        raise ValueError(f"{name} must lie in [{lo}, {hi}]")
    return int(v)


def segment_planes(points, distance_threshold, iterations=1000, seed=0, max_planes=1, min_inliers=0, refit=True, keep="rest", device=0, return_map=False):
    """fgoicp_segment_planes: up to max_planes planes peeled off the cloud by RANSAC — `iterations` three-point hypotheses per peel, drawn
    from `seed` by a counter-based generator, all scored on the device in one pass in fp64; the winner is refitted to its inliers (refit) and
    the points within distance_threshold of it get the plane's number.  Returns the points on no plane (keep="rest": the support plane
    removed) or those on one (keep="planes"), in caller order, as an (m, 3) float32 array.  return_map=True returns (kept, label (n,) int32
    with -1 = on no plane, kept_index (m,) uint32, models, info) with models a list of dict(candidates, sample (3,), hypothesis,
    hypothesis_inliers, inliers, hypothesis_plane (4,), plane (4,), pivot (3,), sum_u (3,), sum_uu (6,)) and info = dict(points, planes,
    on_planes, kept, iterations, max_planes, refit, keep_planes, min_inliers, seed, distance_threshold)."""
    p = _cloud(points)
    iterations = _whole("iterations", iterations, -2 ** 31, 2 ** 31 - 1)  # the call judges the ranges of the definition
    max_planes = _whole("max_planes", max_planes, -2 ** 31, 2 ** 31 - 1)
    seed = _whole("seed", seed, 0, 2 ** 64 - 1)
    min_inliers = _whole("min_inliers", min_inliers, 0, 2 ** 63 - 1)
    if keep not in ("rest", "planes"):
        raise ValueError('keep must be "rest" or "planes"')
    n = len(p)
    cap = min(max(max_planes, 1), 16)
    out = np.empty((n, 3), np.float32)
    idx = np.empty(n, np.uint32) if return_map else None
    label = np.empty(n, np.int32) if return_map else None
    models = (_lib.SegmentModel * cap)() if return_map else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    info = _lib.SegmentInfo()
    _lib.check(_lib.load().fgoicp_segment_planes(_fp(p) if n else None, n, float(distance_threshold), iterations, seed, max_planes, min_inliers, 1 if refit else 0,
                                                 1 if keep == "planes" else 0, int(device), _fp(out), n, ptr(idx, _lib.c_uint32_p), ptr(label, C.POINTER(C.c_int32)),
                                                 models, cap, C.sizeof(_lib.SegmentModel), C.byref(info)), "fgoicp_segment_planes")
    m = int(info.kept)
    out = out[:m].copy()
    if not return_map:
        return out
    found = []
    for j in range(int(info.planes)):
        mod = models[j]
        found.append(dict(candidates=int(mod.candidates), sample=np.array(mod.sample, np.uint32), hypothesis=int(mod.hypothesis),
                          hypothesis_inliers=int(mod.hypothesis_inliers), inliers=int(mod.inliers), hypothesis_plane=np.array(mod.hypothesis_plane, np.float64),
                          plane=np.array(mod.plane, np.float64), pivot=np.array(mod.pivot, np.float64), sum_u=np.array(mod.sum_u, np.float64),
                          sum_uu=np.array(mod.sum_uu, np.float64)))
    d = {name: int(getattr(info, name)) for name, _ in _lib.SegmentInfo._fields_ if name not in ("struct_size", "distance_threshold")}
    d["distance_threshold"] = float(info.distance_threshold)
    return out, label, idx[:m].copy(), found, d


def segment_hypotheses(points, iterations, seed=0, peel=0, candidates=None):
    """fgoicp_segment_hypotheses (host only): the table of one peel of segment_planes — (sample (K, 3) uint32 caller indices, plane (K, 4)
    float64 nx ny nz d, degenerate (K,) bool).  candidates: the ascending caller indices the peel draws from, None = every point."""
    p = _cloud(points)
    K = _whole("iterations", iterations, 1, 65536)
    seed = _whole("seed", seed, 0, 2 ** 64 - 1)
    peel = _whole("peel", peel, 0, 15)
    cand = None if candidates is None else np.ascontiguousarray(candidates, dtype=np.uint32).reshape(-1)
    sample = np.empty((K, 3), np.uint32)
    plane = np.empty((K, 4), np.float64)
    deg = np.empty(K, np.uint8)
    _lib.check(_lib.load().fgoicp_segment_hypotheses(_fp(p) if len(p) else None, len(p), None if cand is None else cand.ctypes.data_as(_lib.c_uint32_p),
                                                     len(p) if cand is None else len(cand), K, seed, peel, sample.ctypes.data_as(_lib.c_uint32_p),
                                                     plane.ctypes.data_as(_lib.c_double_p), deg.ctypes.data_as(_lib.c_uint8_p)), "fgoicp_segment_hypotheses")
    return sample, plane, deg.astype(bool)


def segment_fit_from_moments(count, pivot, sum_u, sum_uu, toward=None):
    """fgoicp_segment_fit_from_moments (host only): the refit of segment_planes — `count` points u = p - pivot with sums sum_u (3,) and sum_uu
    (6,: xx xy xz yy yz zz) -> the plane (4,) float64 through pivot + mean whose normal is the eigenvector of the smallest eigenvalue of the
    covariance, flipped towards the normal of `toward` (4,) when given."""
    count = _whole("count", count, 0, 2 ** 64 - 1)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    a, su, suu = (np.ascontiguousarray(x, dtype=np.float64).reshape(k) for x, k in ((pivot, 3), (sum_u, 3), (sum_uu, 6)))
    tw = None if toward is None else np.ascontiguousarray(toward, dtype=np.float64).reshape(4)
    plane = np.empty(4, np.float64)
    _lib.check(_lib.load().fgoicp_segment_fit_from_moments(count, dp(a), dp(su), dp(suu), None if tw is None else dp(tw), dp(plane)), "fgoicp_segment_fit_from_moments")
    return plane


class Alignment:
    """EXTENSION: the alignment report of fgoicp_alignment / fgoicp_solver_alignment / fgoicp_batch_alignment.  Arrays in the caller's point
    order: indices (ns,) uint32 — nearest target point of every source point; dist2 (ns,) float32 — its squared distance in the frame the
    search ran in; inlier (ns,) bool; target_hit (nt,) bool — neighbour of an inlier.  Summary: points, inliers, targets_hit, sse (the bits
    of compute_sse_error(R, t)), max_inlier_dist2, scaling_factor (1 for a bare Registration, the solver's scale otherwise)."""

    def __init__(self, indices, dist2, inlier, target_hit, summary):
        self.indices, self.dist2, self.inlier, self.target_hit = indices, dist2, inlier.view(np.bool_), target_hit.view(np.bool_)
        self.points, self.inliers, self.targets_hit = int(summary.points), int(summary.inliers), int(summary.targets_hit)
        self.sse, self.max_inlier_dist2 = np.float32(summary.sse), np.float32(summary.max_inlier_dist2)
        self.scaling_factor = np.float32(summary.scaling_factor)

    @property
    def fitness(self):
        """inliers / points (Open3D's evaluate_registration names it so; without a distance threshold every untrimmed point is an inlier)"""
        return self.inliers / self.points

    @property
    def inlier_rmse(self):
        """root mean squared inlier distance in the callers' units"""
        return float(np.sqrt(np.float64(self.sse) / self.inliers) / np.float64(self.scaling_factor))

    @property
    def distances(self):
        """(ns,) float64: distance of every source point to its neighbour in the callers' units, sqrt(dist2) / scaling_factor"""
        return np.sqrt(self.dist2.astype(np.float64)) / np.float64(self.scaling_factor)


def _alignment(call, where, ns, nt):
    """call(corr, d2, inlier, hit, summary) -> status; the marshalling shared by the three entry points"""
    idx = np.empty(ns, np.uint32); d2 = np.empty(ns, np.float32); inl = np.empty(ns, np.uint8); hit = np.empty(nt, np.uint8)
    sm = _lib.AlignmentSummary()
    _lib.check(call(idx.ctypes.data_as(_lib.c_uint32_p), _fp(d2), inl.ctypes.data_as(_lib.c_uint8_p), hit.ctypes.data_as(_lib.c_uint8_p), C.byref(sm)), where)
    return Alignment(idx, d2, inl, hit, sm)


class Information:
    """EXTENSION: the information matrix of fgoicp_information / fgoicp_solver_information / fgoicp_batch_information — matrix (6, 6) float64,
    sum G^T G over the counted correspondences with G = [-[q]x | I], twist order (wx, wy, wz, vx, vy, vz), q the target points (a bare
    Registration: as it holds them; a solver or a batch: as the caller passed them in).  correspondences: the inliers of the Alignment
    within the distance threshold; sum_q (3,), sum_qq (6,: xx xy xz yy yz zz) the moments the matrix is made of; sum_dist2 and max_dist2 in
    the frame the search ran in (scaling_factor converts)."""

    def __init__(self, raw):
        self.matrix = np.array(raw.info, np.float64).reshape(6, 6)
        self.points, self.correspondences = int(raw.points), int(raw.correspondences)
        self.sum_q, self.sum_qq = np.array(raw.sum_q, np.float64), np.array(raw.sum_qq, np.float64)
        self.sum_dist2 = float(raw.sum_dist2)
        self.max_dist2, self.scaling_factor = np.float32(raw.max_dist2), np.float32(raw.scaling_factor)
        self.raw = bytes(raw)  # the struct as the library filled it (two results of the same inputs are the same bytes)

    @property
    def fitness(self):
        """correspondences / points (Open3D's evaluate_registration at this distance threshold)"""
        return self.correspondences / self.points

    @property
    def inlier_rmse(self):
        """root mean squared distance of the counted correspondences in the callers' units (0 when nothing is counted)"""
        if not self.correspondences:
            return 0.0
        return float(np.sqrt(self.sum_dist2 / self.correspondences) / np.float64(self.scaling_factor))


def _information(call, where):
    """call(out) -> status; the marshalling shared by the three entry points"""
    raw = _lib.Information()
    _lib.check(call(C.byref(raw)), where)
    return Information(raw)


def information_from_moments(n, sum_q, sum_qq, offset=None, scale=1.0):
    """fgoicp_information_from_moments (host only): moments of n points q_s -> (matrix (6, 6), sum_q, sum_qq) of q = q_s / scale + offset."""
    q = np.ascontiguousarray(sum_q, np.float64).reshape(3); qq = np.ascontiguousarray(sum_qq, np.float64).reshape(6)
    off = None if offset is None else np.ascontiguousarray(offset, np.float32).reshape(3)
    info = np.empty(36, np.float64); qo = np.empty(3, np.float64); qqo = np.empty(6, np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.load().fgoicp_information_from_moments(int(n), dp(q), dp(qq), None if off is None else _fp(off), float(scale), dp(info), dp(qo), dp(qqo)),
               "fgoicp_information_from_moments")
    return info.reshape(6, 6), qo, qqo


class PlaneMomentsResult:
    """EXTENSION (fgoicp_plane_moments): the point-to-plane normal equations at one pose — JtJ (6, 6) float64 = sum J^T J, Jtr (6,) = sum
    J^T r, sum_r2, over `correspondences` counted points, with J = [(x cross n)^T, n^T], r = n.(x - q), twist order (wx, wy, wz, vx, vy, vz);
    m (28,): the sums as the library returned them (upper triangle row by row, J^T r, r^2)."""

    def __init__(self, raw):
        self.m = np.array(raw.m, np.float64)
        self.points, self.correspondences = int(raw.points), int(raw.correspondences)
        self.JtJ = np.zeros((6, 6))
        self.JtJ[np.triu_indices(6)] = self.m[:21]
        self.JtJ = self.JtJ + np.triu(self.JtJ, 1).T
        self.Jtr, self.sum_r2 = self.m[21:27].copy(), float(self.m[27])
        self.max_dist2 = np.float32(raw.max_dist2)
        self.raw = bytes(raw)  # the struct as the library filled it (two results of the same inputs are the same bytes)


class PlaneRefinement:
    """EXTENSION (fgoicp_icp_plane / fgoicp_solver_refine_plane): R (3, 3), t (3,) — the refined pose (a solver's: t in the callers' frame);
    iterations; rank of the last solve (6: well posed); correspondences counted at the returned pose; plane_rmse — root mean squared
    point-to-plane residual there, in the callers' units; sse — compute_sse_error(R, t) there, bit for bit, in the frame the search ran in."""

    def __init__(self, raw):
        self.R, self.t = from_glm(np.array(raw.R, np.float32)), np.array(raw.t, np.float32)
        self.iterations, self.rank, self.correspondences = int(raw.iterations), int(raw.rank), int(raw.correspondences)
        self.scaling_factor = np.float32(raw.scaling_factor)
        self.plane_rmse_scaled = float(raw.plane_rmse)
        self.plane_rmse = float(raw.plane_rmse / np.float64(raw.scaling_factor))
        self.sse = np.float32(raw.sse)
        self.raw = bytes(raw)


def plane_step_from_moments(n, m28):
    """fgoicp_plane_step_from_moments (host only): -> (xi (6,) float64 = (w, v), rank) of (sum J^T J) xi = -sum J^T r."""
    m = np.ascontiguousarray(m28, np.float64).reshape(28)
    xi = np.empty(6, np.float64); rank = C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.load().fgoicp_plane_step_from_moments(int(n), dp(m), dp(xi), C.byref(rank)), "fgoicp_plane_step_from_moments")
    return xi, rank.value


def plane_apply_step(R, t, xi):
    """fgoicp_plane_apply_step (host only): -> (R', t') = (Rod(w) R, Rod(w) t + v), R' the rotation nearest to the float32 product."""
    Rg = to_glm(R); tt = np.ascontiguousarray(t, np.float32).reshape(3); x = np.ascontiguousarray(xi, np.float64).reshape(6)
    Ro = np.empty(9, np.float32); to = np.empty(3, np.float32)
    _lib.check(_lib.load().fgoicp_plane_apply_step(_fp(Rg), _fp(tt), x.ctypes.data_as(C.POINTER(C.c_double)), _fp(Ro), _fp(to)), "fgoicp_plane_apply_step")
    return from_glm(Ro), to


class GicpRefinement(PlaneRefinement):
    """EXTENSION (fgoicp_icp_gicp / fgoicp_solver_refine_gicp): a PlaneRefinement whose residual is the plane-to-plane one — gicp_rmse =
    sqrt(sum d^T M d / N) at the returned pose in the callers' units (the value the library leaves in plane_rmse)."""

    def __init__(self, raw):
        super().__init__(raw)
        self.gicp_rmse_scaled, self.gicp_rmse = self.plane_rmse_scaled, self.plane_rmse


def _loss_code(loss):
    """None / a name of _lib.LOSSES / its code -> the code"""
    if loss is None:
        return _lib.LOSS_NONE
    if isinstance(loss, str):
        if loss not in _lib.LOSSES:
            raise ValueError(f"loss must be None or one of {sorted(_lib.LOSSES)}, not {loss!r}")
        return _lib.LOSSES[loss]
    return int(loss)


def _model_code(model):
    return {"plane": _lib.MODEL_PLANE, "gicp": _lib.MODEL_GICP}.get(model, model)


LOSS_NAMES = {v: k for k, v in _lib.LOSSES.items()}


def robust_weight(loss, s, scale):
    """fgoicp_robust_weight (host only): the IRLS weight w(s) of the loss ("huber", "cauchy", "geman_mcclure", "tukey", "none" or a
    code) at the scale -> float (fp64; the arithmetic the device kernel runs)."""
    w = C.c_double()
    _lib.check(_lib.load().fgoicp_robust_weight(_loss_code(loss), float(s), float(scale), C.byref(w)), "fgoicp_robust_weight")
    return w.value


class RobustMomentsResult(PlaneMomentsResult):
    """EXTENSION (fgoicp_robust_moments): a PlaneMomentsResult whose every term carries its pair's weight, plus weight_sum, loss (name)
    and scale."""

    def __init__(self, raw):
        super().__init__(raw)
        self.weight_sum, self.loss, self.scale = float(raw.weight_sum), LOSS_NAMES.get(int(raw.loss), int(raw.loss)), float(raw.scale)


class RobustRefinement(PlaneRefinement):
    """EXTENSION (fgoicp_icp_robust / fgoicp_solver_refine_robust): a PlaneRefinement (model "plane") or GicpRefinement ("gicp") of the
    robustly weighted loop.  plane_rmse / gicp_rmse hold sqrt(sum w s^2 / sum w) at the returned pose; weight_sum = sum w there; loss (name);
    loss_scale — the scale the loop ran with, in the callers' units; scale_estimated — whether the library estimated it."""

    def __init__(self, raw, model):
        self.R, self.t = from_glm(np.array(raw.R, np.float32)), np.array(raw.t, np.float32)
        self.iterations, self.rank, self.correspondences = int(raw.iterations), int(raw.rank), int(raw.correspondences)
        self.scaling_factor = np.float32(raw.scaling_factor)
        self.plane_rmse_scaled = float(raw.rmse)
        self.plane_rmse = float(raw.rmse / np.float64(raw.scaling_factor))
        if model == _lib.MODEL_GICP:
            self.gicp_rmse_scaled, self.gicp_rmse = self.plane_rmse_scaled, self.plane_rmse
        self.sse = np.float32(raw.sse)
        self.weight_sum = float(raw.weight_sum)
        self.loss = LOSS_NAMES.get(int(raw.loss), int(raw.loss))
        self.loss_scale_scaled = float(raw.scale)
        self.loss_scale = float(raw.scale / np.float64(raw.scaling_factor))
        self.scale_estimated = bool(raw.scale_estimated)
        self.model = "gicp" if model == _lib.MODEL_GICP else "plane"
        self.raw = bytes(raw)


def gicp_terms(x, q, nq, np_, R, epsilon=1e-3):
    """fgoicp_gicp_terms (host only): one pair -> (M (3, 3) float64, v (28,) float64) — M = (C_q + R C_p R^T)^-1 of the regularised
    covariances, v the pair's terms of J^T M J (upper triangle row by row), J^T M d and d^T M d."""
    a = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (x, q, nq, np_)]
    Rg = to_glm(R)
    M6 = np.empty(6, np.float64); v = np.empty(28, np.float64)
    dp = lambda z: z.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.load().fgoicp_gicp_terms(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), _fp(Rg), float(epsilon), dp(M6), dp(v)), "fgoicp_gicp_terms")
    M = np.empty((3, 3), np.float64)
    M[np.triu_indices(3)] = M6
    return np.triu(M) + np.triu(M, 1).T, v


class Registration:
    """icp::Registration (fgoicp/registration.hpp:49-98) + its NearestNeighborLUT member."""

    def __init__(self, pct, pcs, target_bounds, lut_resolution, device=0, flags=0):
        self._lib = _lib.load()
        self.pct = _cloud(pct)
        self.pcs = _cloud(pcs)
        self.nt, self.ns = len(self.pct), len(self.pcs)
        b = np.asarray(target_bounds, dtype=np.float32).reshape(6)  # ((minx,maxx),(miny,maxy),(minz,maxz))
        self._h = C.c_void_p()
        _lib.check(self._lib.fgoicp_ctx_create(_fp(self.pct), self.nt, _fp(self.pcs), self.ns, _fp(b), float(lut_resolution),
                                               int(device), int(flags), C.byref(self._h)), "fgoicp_ctx_create")

    @classmethod
    def _borrow(cls, handle, owner):
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = C.c_void_p(handle)
        self._owner = owner  # keeps the solver alive; this object must not destroy the ctx
        self.ns = self._lib.fgoicp_ctx_ns(self._h)
        self.nt = self._lib.fgoicp_ctx_nt(self._h)
        return self

    def close(self):
        if getattr(self, "_h", None) and not hasattr(self, "_owner"):
            self._lib.fgoicp_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- NearestNeighborLUT ---------------------------------------------------------------
    def lut_dims(self):
        d = (C.c_int * 3)()
        _lib.check(self._lib.fgoicp_lut_dims(self._h, d), "fgoicp_lut_dims")
        return tuple(d)

    def set_coop_split(self, min_points_untrimmed=None, min_points_trimmed=None):
        """fgoicp_ctx_set_coop_split: from how many source points a cooperative refinement splits its scans over the ranks (None = never)"""
        never = (1 << 64) - 1
        _lib.check(self._lib.fgoicp_ctx_set_coop_split(self._h, never if min_points_untrimmed is None else int(min_points_untrimmed),
                                                       never if min_points_trimmed is None else int(min_points_trimmed)), "fgoicp_ctx_set_coop_split")

    def info(self):
        """fgoicp_ctx_get_info: LUT size and layout, source density per LUT face voxel, points per work item (what the context
        derived from the clouds' statistics).  lut_layout: 1 z-pairs, 2 yz-quad runs, 4 apron-bricked yz-quads, 6 z-pair apron bricks."""
        i = _lib.CtxInfo()
        i.struct_size = C.sizeof(_lib.CtxInfo)
        _lib.check(self._lib.fgoicp_ctx_get_info(self._h, C.byref(i)), "fgoicp_ctx_get_info")
        return dict(lut_dims=tuple(i.lut_dims), lut_layout=i.lut_layout, lut_nodes=i.lut_nodes, lut_bytes=i.lut_bytes,
                    source_points_per_face_voxel=i.source_points_per_face_voxel, points_per_item=i.points_per_item,
                    items_per_evaluation=i.items_per_evaluation, max_subcubes_per_window=i.max_subcubes_per_window,
                    source_order=i.source_order, tree_order=i.tree_order, chunks_per_item_with_thresholds=i.chunks_per_item_with_thresholds)

    def lut_read(self):
        dx, dy, dz = self.lut_dims()
        out = np.empty(dx * dy * dz, dtype=np.float32)
        _lib.check(self._lib.fgoicp_lut_read(self._h, _fp(out), out.size), "fgoicp_lut_read")
        return out.reshape(dz, dy, dx)

    def lut_nodes(self, xyz):
        """Single LUT nodes by index (n, 3) int (x, y, z) — for LUTs too large to read back whole."""
        q = np.ascontiguousarray(xyz, dtype=np.int32).reshape(-1, 3)
        out = np.empty(len(q), dtype=np.float32)
        _lib.check(self._lib.fgoicp_lut_nodes(self._h, q.ctypes.data_as(_lib.c_int_p), len(q), _fp(out)), "fgoicp_lut_nodes")
        return out

    def lut_search(self, queries):
        q = _cloud(queries)
        out = np.empty(len(q), dtype=np.float32)
        _lib.check(self._lib.fgoicp_lut_search(self._h, _fp(q), len(q), _fp(out)), "fgoicp_lut_search")
        return out

    # -- Registration::compute_sse_error, both overloads ---------------------------------------
    def compute_sse_error(self, *args):
        """(R, t) -> float sse                               registration.hpp:96
        (rnode, tnodes, fix_rot[, stream_pool]) -> (lb, ub)  registration.hpp:97 (lower first)"""
        if isinstance(args[0], RotNode):
            rnode, tnodes, fix_rot = args[0], args[1], args[2]
            return self.compute_bounds(rnode.q.R, rnode.span, tnodes, fix_rot)
        R, t = args
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        out = C.c_float()
        _lib.check(self._lib.fgoicp_sse(self._h, _fp(Rg), _fp(tt), C.byref(out)), "fgoicp_sse")
        return np.float32(out.value)

    def alignment(self, R, t):
        """EXTENSION (fgoicp_alignment): the Alignment of R*pcs + t against the target — exact correspondences, squared distances, the
        inlier mask (trimmed contexts: the set_inliers(k) smallest, ties to the lowest index) and the targets the inliers land on."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        return _alignment(lambda *a: self._lib.fgoicp_alignment(self._h, _fp(Rg), _fp(tt), *a), "fgoicp_alignment", self.ns, self.nt)

    def information(self, R, t, max_dist2=np.inf):
        """EXTENSION (fgoicp_information): the Information of R*pcs + t against the target over the Alignment's inliers with
        dist2 <= max_dist2 (inf: all of them), in the frame of the clouds this object holds."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        return _information(lambda out: self._lib.fgoicp_information(self._h, _fp(Rg), _fp(tt), float(max_dist2), out), "fgoicp_information")

    def set_target_normals(self, normals=None, k=16):
        """EXTENSION (fgoicp_ctx_set_target_normals): normals (nt, 3) are normalised and uploaded; None: estimated on the device from
        every target point's k nearest target points (4 <= k <= 32).  The sign of an estimated normal is arbitrary (nothing depends on it)."""
        if normals is None:
            _lib.check(self._lib.fgoicp_ctx_set_target_normals(self._h, None, int(k)), "fgoicp_ctx_set_target_normals")
            return
        n = _cloud(normals)
        if len(n) != self.nt:
            raise ValueError("normals must be (nt, 3)")
        _lib.check(self._lib.fgoicp_ctx_set_target_normals(self._h, _fp(n), int(k)), "fgoicp_ctx_set_target_normals")

    def target_normals(self):
        """fgoicp_target_normals: (nt, 3) float32 unit normals in the caller's order (zero rows: degenerate neighbourhoods)."""
        out = np.empty((self.nt, 3), np.float32)
        _lib.check(self._lib.fgoicp_target_normals(self._h, _fp(out)), "fgoicp_target_normals")
        return out

    def target_knn(self, k):
        """fgoicp_target_knn: (indices (nt, k) uint32, dist2 (nt, k) float32) — every target point's k nearest target points, itself
        included, sorted by (squared distance, index)."""
        idx = np.empty((self.nt, int(k)), np.uint32); d2 = np.empty((self.nt, int(k)), np.float32)
        _lib.check(self._lib.fgoicp_target_knn(self._h, int(k), idx.ctypes.data_as(_lib.c_uint32_p), _fp(d2)), "fgoicp_target_knn")
        return idx, d2

    def plane_moments(self, R, t, max_dist2=np.inf):
        """EXTENSION (fgoicp_plane_moments): the PlaneMomentsResult of R*pcs + t against the target and its normals."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.PlaneMoments()
        _lib.check(self._lib.fgoicp_plane_moments(self._h, _fp(Rg), _fp(tt), float(max_dist2), C.byref(raw)), "fgoicp_plane_moments")
        return PlaneMomentsResult(raw)

    def robust_moments(self, R, t, model="plane", loss=None, scale=0.0, max_dist2=np.inf, epsilon=1e-3):
        """EXTENSION (fgoicp_robust_moments): plane_moments (model "plane") or gicp_moments ("gicp") with every pair's terms times its
        weight w(s) -> RobustMomentsResult.  loss None / "none": the plain sums, bit for bit."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.RobustMoments()
        _lib.check(self._lib.fgoicp_robust_moments(self._h, _fp(Rg), _fp(tt), float(max_dist2), _model_code(model), float(epsilon), _loss_code(loss), float(scale),
                                                   C.byref(raw)), "fgoicp_robust_moments")
        return RobustMomentsResult(raw)

    def robust_residuals(self, R, t, model="plane", loss=None, scale=0.0, max_dist2=np.inf, epsilon=1e-3):
        """EXTENSION (fgoicp_robust_residuals): per source point in the caller's order -> (residual (ns,) float64, weight (ns,) float64,
        counted (ns,) bool); an uncounted point has 0, 0, False."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        res = np.empty(self.ns, np.float64); w = np.empty(self.ns, np.float64); cnt = np.empty(self.ns, np.uint8)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(self._lib.fgoicp_robust_residuals(self._h, _fp(Rg), _fp(tt), float(max_dist2), _model_code(model), float(epsilon), _loss_code(loss), float(scale),
                                                     dp(res), dp(w), cnt.ctypes.data_as(_lib.c_uint8_p)), "fgoicp_robust_residuals")
        return res, w, cnt.astype(bool)

    def robust_scale(self, R, t, model="plane", max_dist2=np.inf, epsilon=1e-3):
        """EXTENSION (fgoicp_robust_scale): 1.4826 x the lower median of |residual| over the counted -> float."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        s = C.c_double()
        _lib.check(self._lib.fgoicp_robust_scale(self._h, _fp(Rg), _fp(tt), float(max_dist2), _model_code(model), float(epsilon), C.byref(s)), "fgoicp_robust_scale")
        return s.value

    def _icp_robust(self, model, R, t, max_iter, conv_thr, max_dist2, epsilon, loss, loss_scale):
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.RobustResult()
        _lib.check(self._lib.fgoicp_icp_robust(self._h, _fp(Rg), _fp(tt), int(max_iter), float(conv_thr), float(max_dist2), model, float(epsilon), _loss_code(loss),
                                               0.0 if loss_scale is None else float(loss_scale), C.byref(raw)), "fgoicp_icp_robust")
        return RobustRefinement(raw, model)

    def icp_plane(self, R, t, max_iter=30, conv_thr=1e-6, max_dist2=np.inf, loss=None, loss_scale=None):
        """EXTENSION (fgoicp_icp_plane): point-to-plane ICP from (R, t) -> PlaneRefinement.  max_iter = 0 evaluates the start.
        loss "huber" / "cauchy" / "geman_mcclure" / "tukey" (fgoicp_icp_robust): the robustly weighted loop -> RobustRefinement;
        loss_scale None: estimated at (R, t)."""
        if loss is not None:
            return self._icp_robust(_lib.MODEL_PLANE, R, t, max_iter, conv_thr, max_dist2, 1e-3, loss, loss_scale)
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.PlaneResult()
        _lib.check(self._lib.fgoicp_icp_plane(self._h, _fp(Rg), _fp(tt), int(max_iter), float(conv_thr), float(max_dist2), C.byref(raw)), "fgoicp_icp_plane")
        return PlaneRefinement(raw)

    def set_source_normals(self, normals=None, k=16):
        """EXTENSION (fgoicp_ctx_set_source_normals): normals (ns, 3) are normalised and uploaded; None: estimated on the device from
        every source point's k nearest source points (4 <= k <= 32).  The sign of an estimated normal is arbitrary (nothing depends on it)."""
        if normals is None:
            _lib.check(self._lib.fgoicp_ctx_set_source_normals(self._h, None, int(k)), "fgoicp_ctx_set_source_normals")
            return
        n = _cloud(normals)
        if len(n) != self.ns:
            raise ValueError("normals must be (ns, 3)")
        _lib.check(self._lib.fgoicp_ctx_set_source_normals(self._h, _fp(n), int(k)), "fgoicp_ctx_set_source_normals")

    def source_normals(self):
        """fgoicp_source_normals: (ns, 3) float32 unit normals in the caller's order (zero rows: degenerate neighbourhoods)."""
        out = np.empty((self.ns, 3), np.float32)
        _lib.check(self._lib.fgoicp_source_normals(self._h, _fp(out)), "fgoicp_source_normals")
        return out

    def gicp_moments(self, R, t, max_dist2=np.inf, epsilon=1e-3):
        """EXTENSION (fgoicp_gicp_moments): the Generalized-ICP normal equations of R*pcs + t as a PlaneMomentsResult — JtJ = sum J^T M J,
        Jtr = sum J^T M d, sum_r2 = sum d^T M d, with J = [-[x]x | I] and M the inverse of the summed regularised covariances."""
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.PlaneMoments()
        _lib.check(self._lib.fgoicp_gicp_moments(self._h, _fp(Rg), _fp(tt), float(max_dist2), float(epsilon), C.byref(raw)), "fgoicp_gicp_moments")
        return PlaneMomentsResult(raw)

    def icp_gicp(self, R, t, max_iter=30, conv_thr=1e-6, max_dist2=np.inf, epsilon=1e-3, loss=None, loss_scale=None):
        """EXTENSION (fgoicp_icp_gicp): Generalized ICP from (R, t) -> GicpRefinement.  max_iter = 0 evaluates the start.  loss and
        loss_scale as icp_plane's."""
        if loss is not None:
            return self._icp_robust(_lib.MODEL_GICP, R, t, max_iter, conv_thr, max_dist2, epsilon, loss, loss_scale)
        Rg = to_glm(R)
        tt = np.ascontiguousarray(t, dtype=np.float32).reshape(3)
        raw = _lib.PlaneResult()
        _lib.check(self._lib.fgoicp_icp_gicp(self._h, _fp(Rg), _fp(tt), int(max_iter), float(conv_thr), float(max_dist2), float(epsilon), C.byref(raw)), "fgoicp_icp_gicp")
        return GicpRefinement(raw)

    def compute_bounds(self, R, rot_span, tnodes, fix_rot):
        Rg = to_glm(R)
        tn = pack_tnodes(tnodes)
        B = len(tn)
        lb = np.empty(B, dtype=np.float32)
        ub = np.empty(B, dtype=np.float32)
        _lib.check(self._lib.fgoicp_bounds_batch(self._h, _fp(Rg), float(rot_span), _fp(tn), B, int(bool(fix_rot)), _fp(lb), _fp(ub)),
                   "fgoicp_bounds_batch")
        return lb, ub

    def compute_bounds_multi(self, Rs, rot_spans, fix_rots, tnode_groups):
        """G rotation nodes in one submission; returns lists of (lb, ub) per group."""
        G = len(Rs)
        Rg = np.concatenate([to_glm(R) for R in Rs]).astype(np.float32) if G else np.zeros(0, np.float32)
        spans = np.asarray(rot_spans, dtype=np.float32)
        fr = np.asarray([int(bool(f)) for f in fix_rots], dtype=np.int32)
        packed = [pack_tnodes(t) for t in tnode_groups]
        offs = np.zeros(G + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in packed])
        tn = np.concatenate(packed) if G else np.zeros((0, 4), np.float32)
        lb = np.empty(len(tn), dtype=np.float32)
        ub = np.empty(len(tn), dtype=np.float32)
        _lib.check(self._lib.fgoicp_bounds_multi(self._h, G, _fp(Rg), _fp(spans), fr.ctypes.data_as(_lib.c_int_p),
                                                 offs.ctypes.data_as(_lib.c_int_p), _fp(np.ascontiguousarray(tn)), _fp(lb), _fp(ub)),
                   "fgoicp_bounds_multi")
        return [(lb[offs[g]:offs[g + 1]], ub[offs[g]:offs[g + 1]]) for g in range(G)]

    def compute_bounds_cut(self, Rs, rot_spans, fix_rots, tnode_groups, cut_above, twin=None, slot=0, ub_below_span=None):
        """fgoicp_bounds_submit_cut + fgoicp_bounds_collect: as compute_bounds_multi, but a subcube of group g whose lower bound is
        >= cut_above[g] comes back as lb = ub = cut_above[g] (np.inf: exact).  twin: optional array over all subcubes (-1 = none).
        ub_below_span (fgoicp_bounds_submit_leaf): per group, subcubes with a translation span below it are terminal — such a row comes
        back as lb = ub = cut_above[g] once its UPPER bound is >= cut_above[g]."""
        G = len(Rs)
        Rg = np.concatenate([to_glm(R) for R in Rs]).astype(np.float32) if G else np.zeros(0, np.float32)
        spans = np.asarray(rot_spans, dtype=np.float32)
        fr = np.asarray([int(bool(f)) for f in fix_rots], dtype=np.int32)
        packed = [pack_tnodes(t) for t in tnode_groups]
        offs = np.zeros(G + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in packed])
        tn = np.ascontiguousarray(np.concatenate(packed) if G else np.zeros((0, 4), np.float32))
        cut = None if cut_above is None else np.ascontiguousarray(cut_above, dtype=np.float32)
        assert cut is None or len(cut) == G
        tw = None if twin is None else np.ascontiguousarray(twin, dtype=np.int32)
        lb = np.empty(len(tn), dtype=np.float32)
        ub = np.empty(len(tn), dtype=np.float32)
        args = (self._h, int(slot), G, _fp(Rg), _fp(spans), fr.ctypes.data_as(_lib.c_int_p), offs.ctypes.data_as(_lib.c_int_p),
                _fp(tn), None if tw is None else tw.ctypes.data_as(_lib.c_int_p), None if cut is None else _fp(cut))
        if ub_below_span is None:
            _lib.check(self._lib.fgoicp_bounds_submit_cut(*args), "fgoicp_bounds_submit_cut")
        else:
            leaf = np.ascontiguousarray(ub_below_span, dtype=np.float32)
            assert len(leaf) == G
            _lib.check(self._lib.fgoicp_bounds_submit_leaf(*args, _fp(leaf)), "fgoicp_bounds_submit_leaf")
        _lib.check(self._lib.fgoicp_bounds_collect(self._h, int(slot), _fp(lb), _fp(ub)), "fgoicp_bounds_collect")
        return [(lb[offs[g]:offs[g + 1]], ub[offs[g]:offs[g + 1]]) for g in range(G)]

    def cut_stats(self, reset=False):
        """(work items of the submissions that carried thresholds, work items the early exit did not evaluate) since the last reset"""
        a = C.c_uint64(); b = C.c_uint64()
        _lib.check(self._lib.fgoicp_ctx_cut_stats(self._h, C.byref(a), C.byref(b), int(reset)), "fgoicp_ctx_cut_stats")
        return a.value, b.value

    def procrustes(self, working):
        """One IterativeClosestPoint3D::procrustes() step (icp3d.cu:140-172) on `working` (ns, 3)."""
        w = _cloud(working)
        assert len(w) == self.ns
        R = np.empty(9, np.float32); t = np.empty(3, np.float32); cen = np.empty(6, np.float32); ABt = np.empty(9, np.float32)
        idx = np.empty(self.ns, np.int32)
        _lib.check(self._lib.fgoicp_procrustes(self._h, _fp(w), _fp(R), _fp(t), _fp(cen), _fp(ABt), idx.ctypes.data_as(_lib.c_int_p)),
                   "fgoicp_procrustes")
        return from_glm(R), t, cen, ABt, idx

    def set_inliers(self, k):
        """EXTENSION (trimmed Go-ICP): every sum over source points runs over the k smallest terms; 0 = off."""
        _lib.check(self._lib.fgoicp_ctx_set_inliers(self._h, int(k)), "fgoicp_ctx_set_inliers")

    def point_distances(self, R, rot_span, tnode, fix_rot):
        """Trimmed mode, diagnostic: e_i = max(distance_i, 0) of registration.cu:48-52 for one subcube, caller order."""
        tn = pack_tnodes(np.asarray(tnode, np.float32).reshape(1, 4))
        out = np.empty(self.ns, dtype=np.float32)
        _lib.check(self._lib.fgoicp_bounds_point_distances(self._h, _fp(to_glm(R)), float(rot_span), _fp(tn), int(bool(fix_rot)), _fp(out)),
                   "fgoicp_bounds_point_distances")
        return out

    def test_sort_fault(self, nth_tick):
        """TEST HOOK: spoil the nth sorted tick from now (0 = off) so that the on-device permutation check has something to find."""
        _lib.check(self._lib.fgoicp_ctx_test_sort_fault(self._h, int(nth_tick)), "fgoicp_ctx_test_sort_fault")

    def sort_fallbacks(self):
        """(sorted ticks, ticks repeated after a failed permutation check)"""
        a = C.c_uint64(); b = C.c_uint64()
        _lib.check(self._lib.fgoicp_ctx_sort_fallbacks(self._h, C.byref(a), C.byref(b)), "fgoicp_ctx_sort_fallbacks")
        return a.value, b.value

    def trim_stats(self, reset=False):
        """trimmed bounds: (rows selected, rows done again in two passes after the sampled bracket failed its check, bracket members)"""
        out = (C.c_uint64 * 3)()
        _lib.check(self._lib.fgoicp_ctx_trim_stats(self._h, out, int(reset)), "fgoicp_ctx_trim_stats")
        return int(out[0]), int(out[1]), int(out[2])

    def set_profile(self, enabled):
        _lib.check(self._lib.fgoicp_ctx_set_profile(self._h, int(bool(enabled))), "fgoicp_ctx_set_profile")

    def profile(self, reset=False):
        ms = C.c_double(); launches = C.c_uint64(); sub = C.c_uint64(); ev = C.c_uint64(); sel = C.c_double()
        _lib.check(self._lib.fgoicp_ctx_profile_evaluations(self._h, C.byref(ev)), "fgoicp_ctx_profile_evaluations")
        _lib.check(self._lib.fgoicp_ctx_profile_select_ms(self._h, C.byref(sel)), "fgoicp_ctx_profile_select_ms")
        _lib.check(self._lib.fgoicp_ctx_profile(self._h, C.byref(ms), C.byref(launches), C.byref(sub), int(reset)), "fgoicp_ctx_profile")
        return {"kernel_ms": ms.value, "launches": launches.value, "subcubes": sub.value, "evaluations": ev.value, "select_ms": sel.value}


def icp_batch(reg, Rs, ts, max_iter=100, convergence_threshold=0.005):
    """n IterativeClosestPoint3D runs at once (fgoicp_icp_batch): -> (sse (n,), R (n,3,3), t (n,3), iterations (n,))"""
    n = len(Rs)
    R0 = np.concatenate([to_glm(R) for R in Rs]).astype(np.float32) if n else np.zeros(0, np.float32)
    t0 = np.ascontiguousarray(np.asarray(ts, np.float32).reshape(-1))
    sse = np.empty(n, np.float32); Ro = np.empty(9 * n, np.float32); to = np.empty(3 * n, np.float32); it = np.empty(n, np.int32)
    _lib.check(reg._lib.fgoicp_icp_batch(reg._h, n, _fp(R0), _fp(t0), int(max_iter), float(convergence_threshold), _fp(sse), _fp(Ro), _fp(to),
                                         it.ctypes.data_as(_lib.c_int_p)), "fgoicp_icp_batch")
    return sse, np.stack([from_glm(Ro[9 * i:9 * i + 9]) for i in range(n)]) if n else np.zeros((0, 3, 3), np.float32), to.reshape(n, 3), it


class IterativeClosestPoint3D:
    """icp::IterativeClosestPoint3D (fgoicp/icp3d.hpp:9-41): ctor arguments as the reference's
    (the clouds live in `reg`), run() -> (sse, R, t)."""

    def __init__(self, reg, pct=None, pcs=None, max_iter=100, convergence_threshold=0.05, R=None, t=None):
        self.reg = reg
        self.max_iter = int(max_iter)
        self.thr = float(convergence_threshold)
        self.R = np.eye(3, dtype=np.float32) if R is None else np.asarray(R, dtype=np.float32)
        self.t = np.zeros(3, dtype=np.float32) if t is None else np.asarray(t, dtype=np.float32)
        self.iterations = 0

    def run(self):
        lib = self.reg._lib
        sse = C.c_float(); iters = C.c_int()
        R = np.empty(9, np.float32); t = np.empty(3, np.float32)
        _lib.check(lib.fgoicp_icp(self.reg._h, _fp(to_glm(self.R)), _fp(np.ascontiguousarray(self.t, np.float32)), self.max_iter, self.thr,
                                  C.byref(sse), _fp(R), _fp(t), C.byref(iters)), "fgoicp_icp")
        self.iterations = iters.value
        return np.float32(sse.value), from_glm(R), t
