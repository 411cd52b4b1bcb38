"""GPU: fgoicp_plane_moments and fgoicp_gicp_moments return the bytes recorded in tests/golden/moments_bits.npz (recorded by
tests/golden/make_moments_bits.py before the three moment kernels came to share csrc/device/fixed_sum.hpp).  The moved queries of
the two kernels (today the unweighted instantiations of refine_moments_kernel) stay on the device, so the fixed order of their fp64 additions is pinned by recorded bytes
rather than by oracle/np_restatement.py fixed_order_sum; the fixture holds every input, and nothing here is computed from the clouds'
generator."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moments_bits.npz")
f32 = np.float32


def _registration(fg, ref, tag, trimmed):
    pcs = ref[tag + "_pcs"]
    reg = fg.Registration(ref[tag + "_pct"], pcs, ref[tag + "_bounds"], float(ref["res"]), flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(int(0.8 * len(pcs)))
    return reg


@pytest.mark.parametrize("trimmed", [False, True], ids=["untrimmed", "trimmed"])
@pytest.mark.parametrize("tag", ["2500_700", "1100_300"])
def test_estimated_normals_give_the_recorded_bytes(fg, gpu_required, tag, trimmed):
    """both poses, max_dist2 = inf and the recorded median dist2, both epsilons: 8 point-to-plane and 16 Generalized-ICP structs"""
    ref = np.load(GOLDEN)
    reg = _registration(fg, ref, tag, trimmed)
    reg.set_target_normals(k=int(ref["k"]))
    reg.set_source_normals(k=int(ref["k"]))
    for pose in ("true", "off"):
        R, t = ref[f"{tag}_{pose}_R"], ref[f"{tag}_{pose}_t"]
        for cut in ("inf", "median"):
            key = f"{tag}_{'trim' if trimmed else 'full'}_{pose}_{cut}"
            max_d2 = float(ref[key + "_max_dist2"])
            assert np.isinf(max_d2) == (cut == "inf")
            assert reg.plane_moments(R, t, max_d2).raw == ref[key + "_plane"].tobytes(), key
            for eps in ref["epsilons"]:
                assert reg.gicp_moments(R, t, max_d2, float(eps)).raw == ref[f"{key}_gicp_{float(eps)}"].tobytes(), (key, float(eps))
    reg.close()


def test_given_normals_give_the_recorded_bytes(fg, gpu_required):
    ref = np.load(GOLDEN)
    tag = "1100_300"
    reg = _registration(fg, ref, tag, False)
    reg.set_target_normals(ref["given_tn"].astype(f32), k=0)
    reg.set_source_normals(ref["given_sn"].astype(f32), k=0)
    R, t = ref[tag + "_off_R"], ref[tag + "_off_t"]
    assert reg.plane_moments(R, t).raw == ref["given_plane"].tobytes()
    assert reg.gicp_moments(R, t, np.inf, float(ref["epsilons"][0])).raw == ref["given_gicp"].tobytes()
    reg.close()
