"""GPU: fgoicp_icp_plane, fgoicp_icp_gicp, fgoicp_icp_robust, fgoicp_robust_moments, fgoicp_robust_residuals and fgoicp_robust_scale
return the bytes recorded in tests/golden/refine_bits.npz (recorded by tests/golden/make_refine_bits.py on an MI355X before the three
moment kernels became refine_moments_kernel and the two loops refine_loop).  The inputs are those of tests/golden/moments_bits.npz; the
calls are the recorder's own (record_context), so a replay cannot drift from what was recorded.  Recorded twice on the recording commit,
every entry came out the same both times: none is left out."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONTEXTS = [(tag, trimmed) for tag in ("2500_700", "1100_300") for trimmed in (False, True)]
PER_CONTEXT = 88  # 18 plain loops + 2 nothing counted; per model: 1 scale + 5 losses x (2 loops + 1 moments + 3 arrays) + 3 edges


def _recorder():
    spec = importlib.util.spec_from_file_location("make_refine_bits", os.path.join(GOLDEN, "make_refine_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_holds_every_recorded_entry():
    want = np.load(os.path.join(GOLDEN, "refine_bits.npz"))
    assert len(want.files) == PER_CONTEXT * len(CONTEXTS)
    for tag, trimmed in CONTEXTS:
        assert sum(k.startswith(f"{tag}_{'trim' if trimmed else 'full'}_") for k in want.files) == PER_CONTEXT


@pytest.mark.parametrize("tag,trimmed", CONTEXTS, ids=[f"{tag}-{'trimmed' if trimmed else 'untrimmed'}" for tag, trimmed in CONTEXTS])
def test_loops_and_robust_evaluations_give_the_recorded_bytes(fg, gpu_required, tag, trimmed):
    """per pair and context: both plain loops at max_iter 0 / 1 / 30 with and without a cut, the robust loop per model and loss at a given
    and an estimated scale, the robust moments, the three per-point arrays, the scale, nothing counted, every weight zero"""
    want = np.load(os.path.join(GOLDEN, "refine_bits.npz"))
    got = _recorder().record_context(np.load(os.path.join(GOLDEN, "moments_bits.npz")), tag, trimmed)
    assert len(got) == PER_CONTEXT
    differ = [k for k, v in got.items() if k not in want.files or want[k].dtype != np.asarray(v).dtype or want[k].tobytes() != np.asarray(v).tobytes()]
    assert not differ, differ
