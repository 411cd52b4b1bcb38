"""Records tests/golden/item_kernel_bits.npz: the bit reference of bounds_item_kernel (csrc/device/bounds_item.hpp).

Round 3's bounds_sorted_kernel family used to be the reference that tests/test_gpu_ops.py::test_item_kernel_keeps_every_bit compared the
item kernel against, in the development build (FGOICP_BOUNDS_ITEM=0).  That family has been retired; its outputs on the test's exact
submissions are kept here as data instead.  For every case of the test (workloads tiny, small/0.02 and small/0.013 at 256- / 1024-point
work items; LUT layouts 1, 2 and 4; trimmed and untrimmed; weight quantisation on and off; the twelve twins of the test's submission) the
script evaluates the submission with FGOICP_BOUNDS_ITEM=0 (round 3's kernel) and =1 (the item kernel) and refuses to write if the two
differ in any bit.  The fixture holds the inputs as well: the clouds, the LUT bounds and the submission arrays.

The committed file was recorded on an MI355X from commit 7505b37 (the last one that has round 3's kernel), with the development build of
that commit's tree:

    FGOICP_LIB=<that tree>/fast-go-icp_amd/lib/libfgoicp_amd_dev.so python tests/golden/make_item_kernel_bits.py [OUT]

Do not regenerate it from a later tree: there FGOICP_BOUNDS_ITEM selects nothing, both runs are the item kernel, and a fixture recorded
from it makes the test circular.  The file is toolchain output; if a ROCm update changes what the item kernel computes, that is a finding
to investigate, not a reason to re-record.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import fgoicp_amd as fg  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "item_kernel_bits.npz")
CASES = [("tiny", 0.05, 256), ("small", 0.02, 256), ("small", 0.013, 1024)]  # workload, LUT resolution, points per work item
LAYOUTS = (1, 2, 4)


def case_key(workload, res, chunk, noquant, layout, trim):
    return f"{workload}_{res}_{chunk}_{'noquant' if noquant else 'quant'}_z{layout}_{'trim' if trim else 'full'}"


def clouds(workload):
    """The test's clouds: pre-processed, the source three points short of a whole number of passes."""
    tgt, src, _, _ = fg.synth.workload(workload, angle_deg=30.0)
    pct, pcs, _, _, _, bounds = fg.synth.preprocess(tgt, src)
    return pct, np.ascontiguousarray(pcs[:len(pcs) - 3]), bounds


def submission():
    """Four groups of two rotation nodes (fix_rot and not), 60 translation nodes, twelve twins between groups 0 and 1."""
    rng = np.random.default_rng(21)

    def tnodes(B, span):
        t = rng.uniform(-0.6, 0.6, size=(B, 3)).astype(np.float32)
        return np.concatenate([t, np.full((B, 1), span, np.float32)], axis=1)
    rn = [fg.RotNode(0.125, -0.25, 0.375, 0.25), fg.RotNode(-0.375, 0.125, 0.25, 0.125)]
    ta, tb, tc, td = tnodes(20, 0.25), tnodes(24, 0.25), tnodes(9, 0.125), tnodes(7, 0.125)
    tb[3:15] = ta[5:17]
    twin = np.full(60, -1, np.int32)
    for k in range(12):
        twin[5 + k], twin[20 + 3 + k] = 20 + 3 + k, 5 + k
    return dict(R9=np.concatenate([fg.nodes.to_glm(n.q.R) for n in (rn[0], rn[0], rn[1], rn[1])]).astype(np.float32),
                spans=np.array([rn[0].span, rn[0].span, rn[1].span, rn[1].span], np.float32),
                fix=np.array([1, 0, 1, 0], np.int32), offs=np.array([0, 20, 44, 53, 60], np.int32),
                tn=np.ascontiguousarray(np.concatenate([ta, tb, tc, td]), np.float32), twin=twin)


def evaluate(pct, pcs, bounds, res, noquant, trim, sub):
    """One fgoicp_bounds_submit_twins of the submission on a fresh context (the knobs are read when it is created)."""
    lib = fg._lib.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    reg = fg.Registration(pct, pcs, bounds, res, flags=fg.FLAG_NO_WEIGHT_QUANT if noquant else 0)
    if trim:
        reg.set_inliers(int(0.8 * len(pcs)))
    lb, ub = np.zeros(60, np.float32), np.zeros(60, np.float32)
    assert lib.fgoicp_bounds_submit_twins(reg._h, 0, 4, sub["R9"].ctypes.data_as(fp), sub["spans"].ctypes.data_as(fp), sub["fix"].ctypes.data_as(ip),
                                          sub["offs"].ctypes.data_as(ip), sub["tn"].ctypes.data_as(fp), sub["twin"].ctypes.data_as(ip)) == 0
    assert lib.fgoicp_bounds_collect(reg._h, 0, lb.ctypes.data_as(fp), ub.ctypes.data_as(fp)) == 0
    reg.close()
    return lb, ub


def main(out_path):
    assert fg.dev_knobs(), "needs the development build (FGOICP_LIB=.../libfgoicp_amd_dev.so): FGOICP_BOUNDS_ITEM selects the kernel"
    sub = submission()
    out = {k: v for k, v in sub.items()}
    os.environ["FGOICP_SMALL_TICK"] = "0"
    for workload in sorted({w for w, _, _ in CASES}):
        out[workload + "_pct"], out[workload + "_pcs"], out[workload + "_bounds"] = clouds(workload)
    for workload, res, chunk in CASES:
        os.environ["FGOICP_CHUNK_PTS"] = str(chunk)
        pct, pcs, bounds = out[workload + "_pct"], out[workload + "_pcs"], out[workload + "_bounds"]
        for noquant in (False, True):
            for layout in LAYOUTS:
                os.environ["FGOICP_LUT_ZPAIR"] = str(layout)
                for trim in (False, True):
                    got = {}
                    for item in ("0", "1"):
                        os.environ["FGOICP_BOUNDS_ITEM"] = item
                        got[item] = evaluate(pct, pcs, bounds, res, noquant, trim, sub)
                    key = case_key(workload, res, chunk, noquant, layout, trim)
                    for a, b in zip(got["0"], got["1"]):
                        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                            sys.exit(f"{key}: FGOICP_BOUNDS_ITEM=0 and =1 differ; nothing written")
                    assert float(got["1"][1].max()) > 0
                    out[key + "_lb"], out[key + "_ub"] = got["1"]
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path}: {len(CASES) * 2 * len(LAYOUTS) * 2} cases, both kernels bit-identical in each")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
