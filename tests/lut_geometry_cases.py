"""Grids, clouds and queries shared by tests/test_lut_geometry_host.py (CPU) and tests/test_gpu_lut_geometry.py (GPU): the distance LUT at
the shapes where its addressing changes — one-node and two-node axes, every remainder of the apron bricks, the apron copy's 10-bit index
limit, the longest axis, the 24-bit row limit of the narrow texel addressing, and the cell shift of the tick sort.  No device code here:
numpy, the oracle and oracle/np_restatement.py only.

A case is built backwards from the lookups it must make.  The wanted query positions Q (LUT frame) come first — spread over the whole box
and half a voxel beyond it, bunched around all eight corners, two of them clamped on every axis at once — and the source cloud is
R^T (Q - centre) for the case's rotation node, so that R * src + centre lands on Q again (up to fp32 rounding, ~1e-3 of a voxel; the
margins below are a quarter voxel).  Translation nodes then push the cloud to both ends of every axis.

Bounds and resolution are binary fractions (resolution 2^-k, bounds multiples of a quarter voxel, everything below 1 in magnitude), so
(max - min) / resolution is exactly d - 0.5 in fp32 and its ceiling is the wanted node count d on both sides."""
import numpy as np

from oracle import np_restatement as npr

f32 = np.float32
REL = 1e-6  # the suite's bar for sums over points (tests/test_gpu_ops.py)

# class -> grids (x, y, z)
GRID_CLASSES = {
    "single_node": [(1, 1, 1)],
    "one_node_axis": [(1, 12, 20), (20, 1, 12), (12, 20, 1)],
    "two_node_axes": [(2, 2, 2), (2, 5, 3)],
    "apron_remainder": [(4, 3, 5), (5, 4, 3), (6, 5, 4), (3, 6, 2)],  # px mod 3 = 0, 1, 2, 2; py odd, even, odd, even
    "apron_10_bit_limit": [(1021, 9, 13), (1022, 9, 13), (9, 1021, 13), (9, 1022, 13), (9, 13, 1021), (9, 13, 1022)],
    "largest_axis": [(4094, 4, 4)],
    "row_limit_24_bit": [(1, 4094, 2046), (1, 4094, 2047)],  # py * pz = 2^23: narrow addressing; one slice more: wide
    "sort_cell_shift": [(32, 5, 7), (33, 5, 7), (64, 5, 7), (65, 5, 7)],
}
GRIDS = [g for grids in GRID_CLASSES.values() for g in grids]
ONE_PER_CLASS = [grids[-1] for grids in GRID_CLASSES.values()]
SMALL_GRIDS = [g for c in ("single_node", "one_node_axis", "two_node_axes", "apron_remainder") for g in GRID_CLASSES[c]]
ADDRESSING_GRIDS = GRID_CLASSES["row_limit_24_bit"]
WIDE_GRID = (1, 4094, 2047)
NS = 300  # source points of the default cloud
NT = 24   # target points (the oracle builds the LUT by brute force: 8.4 M nodes x 24 points stay within a second)


def grid_id(dims):
    return "x".join(str(d) for d in dims)


def class_of(dims):
    return next(c for c, grids in GRID_CLASSES.items() if tuple(dims) in grids)


def face_voxels(dims):
    dx, dy, dz = dims
    return dx * dy + dy * dz + dx * dz


def threshold_ns(dims):
    """(ns just below, ns at) half a source point per voxel of the LUT's three faces: the rule between the quad copies and the z-pair copy"""
    at = -(-face_voxels(dims) // 2)  # ceil(0.5 * faces)
    return at - 1, at


def expected_layout_and_item(dims, ns):
    """DESIGN.md section 4, restated: (layout, points per work item) the shipped build derives from the grid and the cloud."""
    density = ns / face_voxels(dims)
    layout = 1 if density >= 0.5 else (2 if max(dims) + 2 > 1023 else 4)
    return layout, (2048 if density >= 1.0 else 1024 if density >= 0.5 else 512 if density >= 0.25 else 256)


def geometry(dims):
    """(bounds (3, 2) float32, resolution float32) whose ceil(extent / resolution) is dims, exactly"""
    d = np.asarray(dims, np.int64)
    res = 2.0 ** -max(2, int(np.ceil(np.log2(d.max()))))
    lo = -res * (d // 2) - res / 4
    hi = lo + (d - 0.5) * res
    bounds = np.stack([lo, hi], 1).astype(f32)
    assert np.array_equal(bounds.astype(np.float64), np.stack([lo, hi], 1)) and npr.lut_dims(bounds, res) == tuple(dims)
    return bounds, f32(res)


def rot_node():
    from fgoicp_amd.nodes import RotNode
    return RotNode(0.1875, -0.0625, 0.125, 0.03125)  # ~27 degrees; sin of the uncertainty angle 0.085


def make_case(dims, ns=NS):
    dims = tuple(int(v) for v in dims)
    bounds, res = geometry(dims)
    res64 = float(res)
    lo, hi = bounds[:, 0].astype(np.float64), bounds[:, 1].astype(np.float64)
    ext, centre = hi - lo, 0.5 * (lo + hi)
    rng = np.random.default_rng(dims[0] * 10 ** 8 + dims[1] * 10 ** 4 + dims[2])
    d = np.asarray(dims)
    # target: most points inside the bounds, a third of them up to one extent outside
    tgt = np.concatenate([rng.uniform(lo, hi, (NT - 8, 3)), centre + rng.choice([-1.0, 1.0], (8, 3)) * rng.uniform(0.5, 1.5, (8, 3)) * ext]).astype(f32)
    # wanted queries, most important first (a cloud of fewer points keeps a prefix)
    first, last = lo + 0.5 * res64, hi  # centre of texel 0; from here on floor(u - 0.5) is d - 1
    clamped = np.stack([lo - 0.75 * res64, hi + 0.75 * res64])
    corners = []
    for c in range(8):
        at = np.where([(c >> a) & 1 for a in range(3)], last, first)
        corners.append(at + rng.uniform(-1.25, 1.25, (6, 3)) * res64)
    idx = np.stack([rng.integers(0, d[a], 32) for a in range(3)], 1)
    on_nodes = lo + idx[:16] * res64
    on_centres = lo + (idx[16:] + 0.5) * res64
    spread = rng.uniform(lo - res64, hi + res64, (max(ns, 96) - 82, 3))
    Q = np.concatenate([clamped] + corners + [on_nodes, on_centres, spread])[:ns]
    rn = rot_node()
    R = rn.q.R.astype(np.float64)
    src = ((Q - centre) @ R).astype(f32)  # rows R^T (Q - centre)
    # translation nodes: the centre, a sub-voxel shift, half an extent to both ends of every axis, a whole extent along the diagonal both ways
    shifts = [np.zeros(3), np.full(3, 0.37 * res64)]
    for a in range(3):
        for sgn in (-0.5, 0.5):
            s = np.zeros(3); s[a] = sgn * ext[a]
            shifts.append(s)
    shifts += [ext.copy(), -ext]
    spans = np.resize([0.0, 0.02, 0.1, 0.005], len(shifts))
    tnodes = np.concatenate([centre + np.asarray(shifts), spans[:, None]], 1).astype(f32)
    return dict(dims=dims, bounds=bounds, res=res, tgt=tgt, src=src, rn=rn, tnodes=tnodes, centre=centre.astype(f32))


def lower_texels(case, tnode4):
    """(ns, 3) int: floor(u - 0.5) per axis, clamped to [-1, d - 1] (the footprint's lower texel), in the restatement's arithmetic"""
    b, res = case["bounds"], case["res"]
    rp = npr.rot_apply(case["rn"].q.R, case["src"])
    q = (rp + np.asarray(tnode4[:3], f32)[None, :]).astype(f32)
    scale = f32(1.0) / f32(res)
    out = np.empty((len(q), 3), np.int64)
    for a in range(3):
        u = ((q[:, a] + (-b[a, 0])).astype(f32) * scale).astype(f32)
        out[:, a] = np.clip(np.floor((u - f32(0.5)).astype(f32)), -1, case["dims"][a] - 1)
    return out


def lookup_queries(case):
    """queries of lut_search: inside, exactly on nodes, on texel centres, on the ties of the 1.8 fixed-point weight, within half a voxel
    outside each face, far outside"""
    bounds, res, dims = case["bounds"], float(case["res"]), np.asarray(case["dims"])
    lo, hi = bounds[:, 0].astype(np.float64), bounds[:, 1].astype(np.float64)
    rng = np.random.default_rng(int(dims.sum()) + 17)
    ints = lambda n: np.stack([rng.integers(0, dims[a], n) for a in range(3)], 1)
    ends = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)]) * (dims - 1)
    inside = rng.uniform(lo, hi, (400, 3))
    nodes = lo + np.concatenate([ints(64), ends]) * res
    centres = lo + (np.concatenate([ints(64), ends]) + 0.5) * res
    ties = lo + (ints(128) + 0.5 + (2 * rng.integers(0, 256, (128, 3)) + 1) / 512.0) * res  # weight (2k + 1) / 512: w * 256 + 0.5 is an integer
    faces = []
    for a in range(3):
        for side in (0, 1):
            q = rng.uniform(lo, hi, (32, 3))
            q[:, a] = lo[a] - rng.uniform(0, 0.5, 32) * res if side == 0 else hi[a] + rng.uniform(0, 0.5, 32) * res
            faces.append(q)
    far = np.array([[1e6, -1e6, 0.0], [-3e38, 3e38, 1.0], [1e3, 1e3, 1e3], [-1e3, -1e3, -1e3], [1e3, -1e3, 0.0]])
    q = np.concatenate([inside, nodes, centres, ties] + faces + [far]).astype(f32)
    exact = np.concatenate([nodes, centres, ties])
    assert np.array_equal(exact.astype(f32).astype(np.float64), exact)  # these positions are fp32 numbers: the weights are 0.5, 0 and the ties
    return q


def restated_sums(e, span):
    """fp64 sums of the per-point terms of both bounds from the per-point values e (fp32): (lb, ub)"""
    e = np.asarray(e, f32)
    l = (e - f32(npr.SQRT3 * f32(span))).astype(f32)
    lb = np.where(l > 0, (l * l).astype(f32), f32(0))
    return lb.astype(np.float64).sum(), (e * e).astype(f32).astype(np.float64).sum()


def close_rel(a, b, rel=REL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b)))
