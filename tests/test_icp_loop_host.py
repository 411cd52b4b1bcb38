"""The ICP loop's host state (csrc/host/icp_loop.hpp: the loop test, the composition, the choice between the last two iterations, the write-out)
without a GPU: tests/host_harness drives it with the oracle's own procrustes / move_working / compute_sse_error, and the result is compared with
the oracle's IterativeClosestPoint3D::run() on the same inputs.  Both sides apply the same operators in the same order, math3.hpp's products spell
the oracle's host_mul and the harness is built with -ffp-contract=off: the comparison is bit for bit."""
import numpy as np
import pytest

from tests import host_harness as hh

f32 = np.float32
# (thr, start angle, max_iter): the runs of tests/test_gpu_ops.py::test_icp_loop_variants_are_bit_identical, and a loop whose body never runs
CASES = [(0.05, 40.0, 100), (0.005, 15.0, 100), (0.0005, 3.0, 100), (0.0, 25.0, 3), (0.005, 20.0, 1), (1e-7, 2.0, 40), (0.005, 15.0, 0)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def clouds(fg):
    tgt, src, R_gt, t_gt = fg.synth.workload("tiny", angle_deg=30.0)
    pct, pcs, off_t, off_s, scale, bounds = fg.synth.preprocess(tgt, src)
    return pct, pcs, bounds


@pytest.mark.parametrize("trimmed", [False, True])
@pytest.mark.parametrize("thr,ang,max_iter", CASES)
def test_icp_loop_over_the_oracles_operators_is_the_oracles_run(fg, oracle, clouds, thr, ang, max_iter, trimmed):
    pct, pcs, bounds = clouds
    inliers = len(pcs) * 8 // 10 if trimmed else 0
    R0 = fg.synth.random_rotation(np.random.default_rng(int(ang)), ang).astype(f32)
    t0 = np.array([0.01, -0.02, 0.005], f32)
    orc = oracle.Registration(pct, pcs, bounds, 0.05, build_lut=False)
    orc.set_inliers(inliers)
    sse_o, R_o, t_o, it_o = orc.icp(R0, t0, max_iter, thr)
    sse, R, t, it = hh.icp_loop(pct, pcs, bounds, 0.05, R0, t0, max_iter, thr, inliers=inliers)
    assert it == it_o
    assert _bits(sse) == _bits(sse_o) and np.array_equal(_bits(R), _bits(R_o)) and np.array_equal(_bits(t), _bits(t_o))
    if max_iter == 0:
        assert it == 0 and float(sse) == pytest.approx(1e10)  # icp3d.cu:94, :106: the initial error, the start pose
        assert np.array_equal(R, R0) and np.array_equal(t, t0)
    if max_iter in (1, 3):
        assert it == max_iter


def test_a_step_that_makes_things_worse_returns_the_state_before_it():
    """Quarter turns about z, x and y (exact in fp32) with tn = (1, 0, 0) and the errors 5, 3, 4, thr = 0: the third step raises the error, the
    loop ends after it, and the result is the second iteration's — a branch real clouds may never reach."""
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    Rx = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
    Ry = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], f32)
    tn = np.array([1, 0, 0], f32)
    R0, t0 = np.eye(3, dtype=f32), np.array([0.5, -0.25, 2.0], f32)
    none = np.zeros((0, 3), f32)
    sse, R, t, it = hh.icp_loop(none, none, np.zeros(6, f32), 1.0, R0, t0, 10, 0.0, script=[(Rz, tn, 5.0), (Rx, tn, 3.0), (Ry, tn, 4.0)])
    assert it == 3 and sse == f32(3.0)
    R2 = Rx @ Rz @ R0
    t2 = Rx @ (Rz @ t0 + tn) + tn
    assert np.array_equal(R, R2) and np.array_equal(t, t2)
    # ... and a loop that ends on its best iteration returns that one
    sse, R, t, it = hh.icp_loop(none, none, np.zeros(6, f32), 1.0, R0, t0, 2, 0.0, script=[(Rz, tn, 5.0), (Rx, tn, 3.0)])
    assert it == 2 and sse == f32(3.0) and np.array_equal(R, R2) and np.array_equal(t, t2)
