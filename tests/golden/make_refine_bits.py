"""Records tests/golden/refine_bits.npz: the bytes that the refinement loops and the robust evaluations return.

tests/golden/moments_bits.npz pins the two plain evaluations; this fixture does the same for what stands on them — fgoicp_icp_plane,
fgoicp_icp_gicp, fgoicp_icp_robust, fgoicp_robust_moments, fgoicp_robust_residuals and fgoicp_robust_scale.  The path has no atomics and a
fixed order of additions, so two runs give the same bytes; tests/test_gpu_refine_bits.py asks the current build for them.

Inputs: moments_bits.npz — both pairs, the "off" pose, normals estimated at its k, untrimmed and trimmed at 0.8 ns (as
tests/test_gpu_moments_bits.py builds the contexts).  Recorded per pair and context (names: the KEYS of each section below):
  loops     fgoicp_icp_plane and fgoicp_icp_gicp (both epsilons) at max_iter 0, 1, 30, max_dist2 inf and the fixture's median
  scale     fgoicp_robust_scale per model at the start pose: a recorded result, and the "given" scale of everything below
  robust    fgoicp_icp_robust per model and loss (none and the four weights), scale given and estimated (0), max_iter 30
  moments   fgoicp_robust_moments per model and loss at that scale
  residual  the three arrays of fgoicp_robust_residuals per model and loss at that scale
  edges     nothing counted (max_dist2 = 0: both plain loops, the robust loop per model) and every weight 0 (Tukey at 1e-12, below the
            smallest residual: the robust loop and the robust moments per model)
The Generalized-ICP robust calls use the first epsilon.  The fixture holds results only.

The committed file was recorded on an MI355X from commit 36a3b9c (the last one in which plane_moments_kernel, gicp_moments_kernel and
robust_moments_kernel are three texts and the plain and the robust loop two), with the shipped build of that commit's tree:

    python tests/golden/make_refine_bits.py [OUT]

Do not regenerate it from a later tree: a fixture recorded from the code it checks makes the test circular.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import fgoicp_amd as fg  # noqa: E402

IN = os.path.join(HERE, "moments_bits.npz")
OUT = os.path.join(HERE, "refine_bits.npz")
TAGS = ("2500_700", "1100_300")
MODELS = ("plane", "gicp")
LOSSES = ("none", "huber", "cauchy", "geman_mcclure", "tukey")
ITERS = (0, 1, 30)
ZERO_WEIGHT_SCALE = 1e-12


def as_u8(raw):
    return np.frombuffer(raw, np.uint8).copy()


def context(ref, tag, trimmed):
    pcs = ref[tag + "_pcs"]
    reg = fg.Registration(ref[tag + "_pct"], pcs, ref[tag + "_bounds"], float(ref["res"]), flags=fg.FLAG_CURVE_ORDER if trimmed else 0)
    if trimmed:
        reg.set_inliers(int(0.8 * len(pcs)))
    reg.set_target_normals(k=int(ref["k"]))
    reg.set_source_normals(k=int(ref["k"]))
    return reg


def icp_robust(reg, model, R, t, loss, scale, max_dist2=np.inf, eps=1e-3):
    """fgoicp_icp_robust itself, loss "none" included (icp_plane / icp_gicp go there for every loss that is not None)"""
    call = reg.icp_plane if model == "plane" else reg.icp_gicp
    kw = {} if model == "plane" else {"epsilon": eps}
    return call(R, t, max_iter=30, max_dist2=max_dist2, loss=loss, loss_scale=scale, **kw)


def record_context(ref, tag, trimmed):
    """the entries of one pair and context, in a dict; the calls tests/test_gpu_refine_bits.py replays"""
    out = {}
    eps0 = float(ref["epsilons"][0])
    R, t = ref[tag + "_off_R"], ref[tag + "_off_t"]
    reg = context(ref, tag, trimmed)
    ctx = f"{tag}_{'trim' if trimmed else 'full'}"
    for cut in ("inf", "median"):
        max_d2 = float(ref[f"{ctx}_off_{cut}_max_dist2"])
        for it in ITERS:
            out[f"{ctx}_{cut}_plane_{it}"] = as_u8(reg.icp_plane(R, t, max_iter=it, max_dist2=max_d2).raw)
            for eps in ref["epsilons"]:
                out[f"{ctx}_{cut}_gicp_{float(eps)}_{it}"] = as_u8(reg.icp_gicp(R, t, max_iter=it, max_dist2=max_d2, epsilon=float(eps)).raw)
    out[f"{ctx}_plane_none"] = as_u8(reg.icp_plane(R, t, max_iter=30, max_dist2=0.0).raw)
    out[f"{ctx}_gicp_none"] = as_u8(reg.icp_gicp(R, t, max_iter=30, max_dist2=0.0, epsilon=eps0).raw)
    for model in MODELS:
        scale = reg.robust_scale(R, t, model, np.inf, eps0)
        out[f"{ctx}_{model}_scale"] = np.float64(scale)
        for loss in LOSSES:
            key = f"{ctx}_{model}_{loss}"
            out[key + "_given"] = as_u8(icp_robust(reg, model, R, t, loss, scale, eps=eps0).raw)
            out[key + "_estimated"] = as_u8(icp_robust(reg, model, R, t, loss, 0.0, eps=eps0).raw)
            out[key + "_moments"] = as_u8(reg.robust_moments(R, t, model, loss, scale, np.inf, eps0).raw)
            res, w, cnt = reg.robust_residuals(R, t, model, loss, scale, np.inf, eps0)
            out[key + "_residual"], out[key + "_weight"], out[key + "_counted"] = res, w, cnt.astype(np.uint8)
        got = icp_robust(reg, model, R, t, "huber", scale, max_dist2=0.0, eps=eps0)
        assert got.correspondences == 0, "max_dist2 = 0 must count nothing"
        out[f"{ctx}_{model}_robust_none"] = as_u8(got.raw)
        m = reg.robust_moments(R, t, model, "tukey", ZERO_WEIGHT_SCALE, np.inf, eps0)
        got = icp_robust(reg, model, R, t, "tukey", ZERO_WEIGHT_SCALE, eps=eps0)
        assert m.weight_sum == 0.0 and m.correspondences > 0 and got.weight_sum == 0.0, "Tukey at 1e-12 must weigh every pair 0"
        out[f"{ctx}_{model}_zero_weight_moments"], out[f"{ctx}_{model}_zero_weight_loop"] = as_u8(m.raw), as_u8(got.raw)
    reg.close()
    return out


def record(ref):
    out = {}
    for tag in TAGS:
        for trimmed in (False, True):
            out.update(record_context(ref, tag, trimmed))
    return out


def main(out_path):
    ref = np.load(IN)
    first, second = record(ref), record(ref)
    differ = [k for k in first if np.asarray(first[k]).tobytes() != np.asarray(second[k]).tobytes()]
    print(f"two recordings: {len(first)} entries, {len(differ)} differ {differ}")
    np.savez_compressed(out_path, **{k: v for k, v in first.items() if k not in differ})
    print(f"wrote {out_path}: {len(first) - len(differ)} entries, {os.path.getsize(out_path)} bytes")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else OUT))
