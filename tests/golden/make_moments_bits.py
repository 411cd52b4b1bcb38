"""Records tests/golden/moments_bits.npz: the bytes that fgoicp_plane_moments and fgoicp_gicp_moments return.

The moved queries of plane_moments_kernel and gicp_moments_kernel (today the unweighted instantiations of refine_moments_kernel) never
leave the device, so their fixed-order fp64 sums cannot be restated from the caller's side the way oracle/np_restatement.py::fixed_order_sum
restates fgoicp_information's.  The tolerance of tests/test_gpu_plane.py and tests/test_gpu_gicp.py (16 x 2^-24 x sum |term|) would not
notice a changed order of additions either.  This fixture pins the bytes instead: tests/test_gpu_moments_bits.py asks the current build
for the same structs.

Cases: the plane tests' two sizes, (nt, ns) = (2500, 700) and (1100, 300); untrimmed, and trimmed at 0.8 ns (with FGOICP_FLAG_CURVE_ORDER,
as those tests run it); at the true pose and at the tests' 5 degrees off pose; max_dist2 = inf and the median dist2 of the report; normals
estimated with k = 10; epsilon 1e-3 and 0.1 for the GICP sums.  One more case has given rather than estimated normals in both clouds.
The fixture holds the inputs as well: the clouds, the LUT bounds, the poses, k, the epsilons, every max_dist2 and the given normals
(unnormalised: the library normalises them).

The committed file was recorded on an MI355X from commit cfdd306 (the last one in which align_info_kernel, plane_moments_kernel and
gicp_moments_kernel each carry their own copy of the reduction), with the shipped build of that commit's tree:

    python tests/golden/make_moments_bits.py [OUT]

Do not regenerate it from a later tree: a fixture recorded from the code it checks makes the test circular.  The file is toolchain
output; if a ROCm update changes what the kernels compute, that is a finding to investigate, not a reason to re-record.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402
from tests.test_gpu_plane import SIZES, _case, off_pose  # noqa: E402  (the plane tests' clouds and poses)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "moments_bits.npz")
K = 10
EPSILONS = (1e-3, 0.1)
RES = 0.05
f32 = np.float32


def case_key(nt, ns, trimmed, pose, cut):
    return f"{nt}_{ns}_{'trim' if trimmed else 'full'}_{pose}_{'median' if cut else 'inf'}"


def registration(pct, pcs, bounds, ns, trimmed):
    reg = fg.Registration(pct, pcs, bounds, RES, flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(int(0.8 * ns))
    return reg


def as_u8(raw):
    return np.frombuffer(raw, np.uint8).copy()


def main(out_path):
    out = {"k": np.int32(K), "epsilons": np.array(EPSILONS, np.float64), "res": np.float64(RES)}
    n_structs = 0
    for nt, ns in SIZES:
        c = _case(fg, nt, ns)
        tag = f"{nt}_{ns}"
        out[tag + "_pct"], out[tag + "_pcs"], out[tag + "_bounds"] = c["pct"], c["pcs"], c["bounds"]
        poses = {"true": (c["R"].astype(f32), c["t"].astype(f32)), "off": off_pose(c, 5.0, 0.0)}
        for name, (R, t) in poses.items():
            out[f"{tag}_{name}_R"], out[f"{tag}_{name}_t"] = R, t
        for trimmed in (False, True):
            reg = registration(c["pct"], c["pcs"], c["bounds"], ns, trimmed)
            reg.set_target_normals(k=K)
            reg.set_source_normals(k=K)
            for name, (R, t) in poses.items():
                median = float(np.sort(reg.alignment(R, t).dist2)[ns // 2])
                for cut in (False, True):
                    key = case_key(nt, ns, trimmed, name, cut)
                    max_d2 = median if cut else np.inf
                    out[key + "_max_dist2"] = np.float64(max_d2)
                    p = reg.plane_moments(R, t, max_d2)
                    assert 0 < p.correspondences <= ns and reg.plane_moments(R, t, max_d2).raw == p.raw
                    out[key + "_plane"] = as_u8(p.raw)
                    for eps in EPSILONS:
                        g = reg.gicp_moments(R, t, max_d2, eps)
                        assert 0 < g.correspondences <= ns and reg.gicp_moments(R, t, max_d2, eps).raw == g.raw
                        out[f"{key}_gicp_{eps}"] = as_u8(g.raw)
                    n_structs += 1 + len(EPSILONS)
            reg.close()
    # given normals in both clouds: the smaller size, untrimmed, the off pose, no cut
    nt, ns = SIZES[1]
    c = _case(fg, nt, ns)
    rng = np.random.default_rng(11)
    out["given_tn"] = (rng.normal(size=(nt, 3)) * rng.uniform(0.1, 50, (nt, 1))).astype(f32)
    out["given_sn"] = (rng.normal(size=(ns, 3)) * rng.uniform(0.1, 50, (ns, 1))).astype(f32)
    reg = registration(c["pct"], c["pcs"], c["bounds"], ns, False)
    reg.set_target_normals(out["given_tn"], k=0)
    reg.set_source_normals(out["given_sn"], k=0)
    R, t = off_pose(c, 5.0, 0.0)
    out["given_plane"] = as_u8(reg.plane_moments(R, t).raw)
    out["given_gicp"] = as_u8(reg.gicp_moments(R, t, np.inf, EPSILONS[0]).raw)
    reg.close()
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path}: {n_structs + 2} structs, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
