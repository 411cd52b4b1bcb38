"""The stable compaction shared by fgoicp_remove_outliers, fgoicp_cluster_dbscan and fgoicp_segment_planes (csrc/device/one_shot.hpp: the scan
of the flags, the count from its last row, the scatter, the copies out of `kept` rows), pinned through the three public calls on clouds whose
kept mask is known by construction — no restatement of the filters is needed.

Point i sits at x = i on the x axis; a point that is to go is "isolated": moved to x = i + 1000 (r + 1), r its rank among the isolated ones, so
that nothing lies within 1.5 of it.  The outlier call (radius mode, k = 2, radius 1.5) and the cluster call (eps 1.5, min_points 2,
keep_min_size 1) then keep exactly the points that still have a neighbour at distance 1; "none kept" is the plain chain under a radius
(eps) of 1e-3.  For the segment call the points lie on the plane z = 0 with y = i^2 mod 5 (three points on the x axis span no plane), the
others at z = 5: one peel of 64 hypotheses at distance 0.1 finds z = 0 whenever at least three points lie on it and they are the majority;
keep="planes" keeps them, keep="rest" the others.  The mask shapes that leave fewer than three points on the plane (or none off it that
RANSAC could tell from a second plane) are left out by construction, below in segment_cases.

Sizes: one wave, the block edge of the 256-thread scatter on both sides, two full blocks plus one point.  Masks: all, none, all but the last
point, only the last two — the count is read from the LAST row of the scan and the LAST flag, so both values of each are covered."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
OK, TOO_LARGE = 0, 5
SIZES = [3, 64, 255, 256, 257, 513]
SEED = 17


def masks(n):
    all_, none = np.ones(n, bool), np.zeros(n, bool)
    but_last, last_two = all_.copy(), none.copy()
    but_last[-1] = False
    last_two[-2:] = True
    return {"all": all_, "none": none, "all but the last": but_last, "the last two": last_two}


def chain(mask):
    """the points of `mask` one unit apart on the x axis, the others isolated"""
    x = np.arange(len(mask), dtype=np.float64)
    gone = np.flatnonzero(~mask)
    x[gone] += 1000.0 * (1 + np.arange(len(gone)))
    p = np.zeros((len(mask), 3), f32)
    p[:, 0] = x
    return p


def sheet(on_plane):
    n = len(on_plane)
    i = np.arange(n)
    return np.ascontiguousarray(np.stack([i, (i * i) % 5, np.where(on_plane, 0, 5)], 1).astype(f32))


def segment_cases(n):
    """(name, cloud, mask, keep): on the plane = the mask (keep="planes") or its complement (keep="rest"); only where at least three points lie on
    the plane and more than off it"""
    out = []
    for name, mask in masks(n).items():
        for keep, on_plane in (("planes", mask), ("rest", ~mask)):
            if on_plane.sum() >= 3 and 2 * on_plane.sum() > n:
                out.append((name, sheet(on_plane), mask, keep))
    return out


def check_rows(p, mask, kept, idx, count):
    assert kept.dtype == f32 and kept.tobytes() == p[mask].tobytes()
    assert idx.dtype == np.uint32 and np.array_equal(idx, np.flatnonzero(mask))
    assert count == int(mask.sum())


def _buffers(capacity):
    cap = max(capacity, 1)
    return np.empty((cap, 3), f32), np.empty(cap, np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_outlier_rows(fg, gpu_required, n):
    L, lib = fg._lib, fg._lib.load()
    for name, mask in masks(n).items():
        p, radius = (chain(np.ones(n, bool)), 1e-3) if name == "none" else (chain(mask), 1.5)
        kept, keep, idx, _, _, info = fg.remove_radius_outliers(p, 2, radius, return_map=True)
        check_rows(p, mask, kept, idx, info["kept"])
        assert np.array_equal(keep, mask), name
        if mask.any():
            out, ix = _buffers(int(mask.sum()) - 1)
            raw = L.OutlierInfo()
            rc = lib.fgoicp_remove_outliers(p.ctypes.data_as(L.c_float_p), n, L.OUTLIER_RADIUS, 2, C.c_float(radius), 0, out.ctypes.data_as(L.c_float_p), int(mask.sum()) - 1,
                                            ix.ctypes.data_as(L.c_uint32_p), None, None, None, C.byref(raw))
            assert rc == TOO_LARGE and raw.kept == mask.sum() and raw.points == n, name


@pytest.mark.parametrize("n", SIZES)
def test_cluster_rows(fg, gpu_required, n):
    L, lib = fg._lib, fg._lib.load()
    for name, mask in masks(n).items():
        p, eps = (chain(np.ones(n, bool)), 1e-3) if name == "none" else (chain(mask), 1.5)
        kept, label, _, _, idx, info = fg.cluster_dbscan(p, eps, min_points=2, keep_min_size=1, return_map=True)
        check_rows(p, mask, kept, idx, info["kept"])
        assert np.array_equal(label >= 0, mask), name
        if mask.any():
            out, ix = _buffers(int(mask.sum()) - 1)
            raw = L.ClusterInfo()
            rc = lib.fgoicp_cluster_dbscan(p.ctypes.data_as(L.c_float_p), n, C.c_float(eps), 2, 1, 0, out.ctypes.data_as(L.c_float_p), int(mask.sum()) - 1,
                                           ix.ctypes.data_as(L.c_uint32_p), None, None, None, 0, C.byref(raw))
            assert rc == TOO_LARGE and raw.kept == mask.sum() and raw.points == n, name


@pytest.mark.parametrize("n", SIZES)
def test_segment_rows(fg, gpu_required, n):
    L, lib = fg._lib, fg._lib.load()
    cases = segment_cases(n)
    want = [("all", "planes"), ("none", "rest"), ("all but the last", "planes"), ("the last two", "rest")]  # n = 3: the last two would leave one or two points on the plane
    assert [(c[0], c[3]) for c in cases] == (want[:2] if n == 3 else want)
    for name, p, mask, keep in cases:
        kept, label, idx, models, info = fg.segment_planes(p, 0.1, iterations=64, seed=SEED, keep=keep, return_map=True)
        check_rows(p, mask, kept, idx, info["kept"])
        assert info["planes"] == 1 and np.array_equal(label >= 0, mask if keep == "planes" else ~mask), (name, keep)
        if mask.any():
            out, ix = _buffers(int(mask.sum()) - 1)
            raw = L.SegmentInfo()
            rc = lib.fgoicp_segment_planes(p.ctypes.data_as(L.c_float_p), n, C.c_float(0.1), 64, SEED, 1, 0, 1, 1 if keep == "planes" else 0, 0, out.ctypes.data_as(L.c_float_p),
                                           int(mask.sum()) - 1, ix.ctypes.data_as(L.c_uint32_p), None, None, 0, C.sizeof(L.SegmentModel), C.byref(raw))
            assert rc == TOO_LARGE and raw.kept == mask.sum() and raw.points == n, (name, keep)
