"""What a context, a solver, a batch and the one-shot calls hold on the device goes with them: fg.live_resources() — the device allocations,
pinned allocations, streams and events held by the library's owning handles (csrc/device/owned.hpp) — is back where it was once the object
is closed, whatever was called on it in between, and after a creation that is refused half-way.  Also pinned here: what creation decides
from the clouds' statistics (Registration.info()), as literals recorded from the commit before creation was cut into stages."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
BOX = np.array([[-1.0, 1.0]] * 3, f32)
RES = 0.05


def _cloud(seed, n):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-0.9, 0.9, (n, 3)).astype(f32))


@pytest.fixture(scope="module")
def clouds(gpu_required):
    return _cloud(1, 257), _cloud(2, 511)  # target, source


def _baseline(fg):
    gc.collect()  # objects of earlier tests that are still waiting for their finaliser
    return fg.live_resources()


def _held(fg, base):
    now = fg.live_resources()
    assert all(n > b for n, b in zip(now, base)), (base, now)
    return now


def _tnodes(seed, B, span):
    t = np.random.default_rng(seed).uniform(-0.5, 0.5, (B, 3)).astype(f32)
    return np.concatenate([t, np.full((B, 1), span, f32)], axis=1)


@pytest.mark.parametrize("flags", ["plain", "brute", "profile"])
def test_a_context_returns_what_it_held(fg, clouds, flags):
    tgt, src = clouds
    base = _baseline(fg)
    reg = fg.Registration(tgt, src, BOX, RES, flags={"plain": 0, "brute": fg.FLAG_BRUTE_FORCE_NN, "profile": fg.FLAG_PROFILE}[flags])
    now = _held(fg, base)
    if flags == "profile":
        assert now[3] - base[3] >= 4 * 1024  # the profile's event pairs
    assert np.isfinite(reg.compute_sse_error(np.eye(3, dtype=f32), np.zeros(3, f32)))
    reg.close()
    assert fg.live_resources() == base


def test_a_profile_switched_on_later_is_returned_too(fg, clouds):
    tgt, src = clouds
    base = _baseline(fg)
    reg = fg.Registration(tgt, src, BOX, RES)
    before = _held(fg, base)
    reg.set_profile(True)
    after = fg.live_resources()
    assert after[3] == before[3] + 4 * 1024 and after[:3] == before[:3]
    reg.compute_bounds(np.eye(3, dtype=f32), 0.5, _tnodes(3, 8, 0.25), False)
    assert reg.profile()["launches"] >= 1
    reg.set_profile(False)
    reg.set_profile(True)  # the events are created once
    assert fg.live_resources() == after
    reg.close()
    assert fg.live_resources() == base


def test_a_trimmed_context_returns_what_it_held(fg, clouds):
    tgt, src = clouds
    base = _baseline(fg)
    reg = fg.Registration(tgt, src, BOX, RES)
    before = _held(fg, base)
    reg.set_inliers(400)
    trimmed = fg.live_resources()
    assert trimmed[0] > before[0] and trimmed[1] > before[1] and trimmed[2:] == before[2:]
    reg.set_inliers(300)  # the buffers are there: nothing is allocated again
    assert fg.live_resources() == trimmed
    R = np.eye(3, dtype=f32)
    (lb, ub), = reg.compute_bounds_cut([R], [0.5], [False], [_tnodes(4, 16, 0.25)], [np.inf])
    assert np.all(np.isfinite(lb)) and np.all(lb <= ub)
    assert len(reg.trim_stats()) == 3
    assert fg.live_resources() == trimmed
    reg.close()
    assert fg.live_resources() == base


def test_a_context_returns_what_its_lazy_allocators_added(fg, clouds):
    tgt, src = clouds
    base = _baseline(fg)
    reg = fg.Registration(tgt, src, BOX, RES)
    created = _held(fg, base)
    R, t = np.eye(3, dtype=f32), np.zeros(3, f32)
    assert reg.alignment(R, t).points == len(src)
    reg.information(R, t)
    reg.set_target_normals()
    reg.plane_moments(R, t)
    reg.set_source_normals()
    reg.gicp_moments(R, t)
    rng = np.random.default_rng(5)
    sse, _, _, _ = fg.icp_batch(reg, [fg.synth.random_rotation(rng, 10.0).astype(f32) for _ in range(5)], np.zeros((5, 3), f32), max_iter=5)
    assert np.all(np.isfinite(sse))
    grown = fg.live_resources()
    assert grown[0] > created[0] and grown[1:] == created[1:]  # the report, the normals, the moment rows: device arrays only
    reg.alignment(R, t)
    reg.gicp_moments(R, t)
    assert fg.live_resources() == grown  # ... each allocated once
    reg.close()
    assert fg.live_resources() == base


def test_a_solver_run_returns_what_it_held(fg, gpu_required):
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    base = _baseline(fg)
    s = fg.FastGoICP(tgt, src, 0.05, 1e-3)
    _held(fg, base)
    s.run()
    assert np.isfinite(s.get_best_error())
    s.close()
    assert fg.live_resources() == base


def test_a_batch_with_a_trimmed_pair_returns_what_it_held(fg, gpu_required):
    """A limit of the Python surface: the batch creates its stream, its staging buffers and every pair's context inside run() and releases
    them before run() returns, so "above the baseline while it lives" cannot be observed from here; what is checked is that a FastGoICPBatch
    holds nothing before its run and that everything the run held — two contexts, one of them trimmed, the e-row arena — is back afterwards."""
    tgt, src, _, _ = fg.synth.workload("tiny", angle_deg=25.0)
    base = _baseline(fg)
    b = fg.FastGoICPBatch([(tgt, src, 0.05, 1e-3), (tgt, src, 0.05, 1e-3, 0.1)])
    assert fg.live_resources() == base
    out = b.run()
    assert all(o is not None for o in out), [b.status(i) for i in range(2)]
    b.close()
    assert fg.live_resources() == base


def test_the_one_shot_calls_return_what_they_held(fg, gpu_required):
    pts = _cloud(6, 511)
    base = _baseline(fg)
    assert len(fg.voxel_downsample(pts, 0.2)) > 0
    assert fg.live_resources() == base
    assert len(fg.remove_statistical_outliers(pts, k=8, std_ratio=2.0)) > 0
    assert fg.live_resources() == base
    fg.remove_radius_outliers(pts, 4, 0.5)
    assert fg.live_resources() == base
    assert len(fg.farthest_point_sample(pts, 32)) == 32
    assert fg.live_resources() == base
    fg.cluster_dbscan(pts, 0.3, min_points=4)
    assert fg.live_resources() == base
    fg.segment_planes(pts, 0.05, iterations=64)
    assert fg.live_resources() == base


def test_a_creation_refused_after_its_first_device_resource_leaves_nothing(fg, clouds):
    """bounds of +-1 at resolution 1e-4: LUT dims of 20000 > 4094, found once the device is selected and the main stream exists"""
    tgt, src = clouds
    base = _baseline(fg)
    with pytest.raises(fg.FgoicpError) as e:
        fg.Registration(tgt, src, BOX, 1e-4)
    assert e.value.status == 1  # FGOICP_ERR_INVALID_ARG
    assert "fgoicp_ctx_create: LUT dims out of range (20000,20000,20000)" in str(e.value)
    assert fg.live_resources() == base


def test_twenty_rounds_of_create_and_close_end_at_the_baseline(fg, gpu_required):
    tgt, src = _cloud(7, 64), _cloud(8, 96)
    base = _baseline(fg)
    for _ in range(20):
        reg = fg.Registration(tgt, src, BOX, 0.1)
        reg.close()
    assert fg.live_resources() == base


# Registration.info() of a 257-point target and n uniform source points in [-0.9, 0.9]^3, LUT over [-1, 1]^3 at resolution 0.05 (40^3 nodes,
# 4800 face voxels): 0.11, 0.85 and 4.2 source points per face voxel.  Recorded on an MI355X from the commit before creation was cut
# into stages; the stages must decide the same.
INFO_AT_PARENT = {
    511: dict(lut_layout=4, points_per_item=256, max_subcubes_per_window=131072, chunks_per_item_with_thresholds=2, source_order=2, tree_order=1,
              lut_dims=(40, 40, 40), lut_bytes=1876896),
    4096: dict(lut_layout=1, points_per_item=1024, max_subcubes_per_window=131072, chunks_per_item_with_thresholds=1, source_order=2, tree_order=1,
               lut_dims=(40, 40, 40), lut_bytes=889056),
    20000: dict(lut_layout=1, points_per_item=2048, max_subcubes_per_window=131072, chunks_per_item_with_thresholds=1, source_order=2, tree_order=1,
                lut_dims=(40, 40, 40), lut_bytes=889056),
}
INFO_FIELDS = ["lut_layout", "points_per_item", "max_subcubes_per_window", "chunks_per_item_with_thresholds", "source_order", "tree_order", "lut_dims", "lut_bytes"]


@pytest.mark.parametrize("ns", sorted(INFO_AT_PARENT))
def test_creation_decides_what_it_decided_before(fg, clouds, ns):
    reg = fg.Registration(clouds[0], _cloud(100 + ns, ns), BOX, RES)
    info = reg.info()
    reg.close()
    assert {k: info[k] for k in INFO_FIELDS} == INFO_AT_PARENT[ns]


def test_the_three_shapes_take_three_item_sizes():
    assert len({v["points_per_item"] for v in INFO_AT_PARENT.values()}) == 3
