// TEST-ONLY: the product's host driver (fast-go-icp_amd/csrc/host/driver.hpp) over the CPU oracle's operators PLUS the optional operator
// entry for terminal rows (Ops::bounds_submit_leaf, fgoicp_bounds_submit_leaf): the oracle evaluates every subcube in full and then answers
// by the device's contract — a terminal row (translation span below its group's ub_below_span) is {T, T} once its UPPER bound is >= T,
// every other row once its lower bound is.  The driver must not be able to tell (tests/test_leaf_cut_host.py).  Never part of libfgoicp_amd.so.
#include "oracle_ops.hpp"

using namespace host_harness;

namespace {
struct LeafOps : OracleOps {
    unsigned long long rows = 0;       // rows that came through bounds_submit_leaf with thresholds
    unsigned long long cut_lb = 0;     // ... answered {T, T} with lb >= T (the lower-bound rule would have said the same)
    unsigned long long cut_leaf = 0;   // ... answered {T, T} although lb < T: terminal rows decided by their upper bound alone
    int bounds_submit_leaf(int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4, const int* twin,
                           const float* cut_above, const float* ub_below_span) {
        const int rc = OracleOps::bounds_submit(slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, nullptr);  // exact rows
        if (rc || !cut_above) return rc;
        float *lb = slot_lb[slot].data(), *ub = slot_ub[slot].data();
        for (int g = 0; g < G; ++g) {
            const float T = cut_above[g];
            for (int i = offsets[g]; i < offsets[g + 1]; ++i) {
                const bool terminal = ub_below_span && tn4[4 * i + 3] < ub_below_span[g];
                ++rows;
                if (lb[i] >= T) ++cut_lb;
                else if (terminal && ub[i] >= T) ++cut_leaf;
                else continue;
                lb[i] = ub[i] = T;
            }
        }
        return 0;
    }
};
struct LeafHarness {
    std::unique_ptr<Harness> base;  // pre-processing, the oracle's Registration (its driver over OracleOps is not run)
    LeafOps ops;
    std::unique_ptr<GoIcpDriver<LeafOps>> drv;
};
}  // namespace

extern "C" {

// schedule / round_width as harness_create (tests/host_harness/harness.cpp); thresholds = 0: the driver hands the operator none (exact answers)
void* leaf_harness_create(const float* tgt, size_t nt, const float* src, size_t ns, float lut_res, float mse_thr, int schedule, int round_width, int thresholds) {
    auto h = std::make_unique<LeafHarness>();
    h->base.reset(make_harness(tgt, nt, src, ns, lut_res, mse_thr, schedule, round_width, 0.0f, 1, 0));
    static_cast<OracleOps&>(h->ops) = h->base->ops;
    const int sched = (schedule == 2 || schedule == 4) ? 1 : (schedule == 3 || schedule == 5) ? 0 : schedule;
    h->drv.reset(new GoIcpDriver<LeafOps>(h->ops, ns, mse_thr, sched, round_width));
    h->drv->set_use_cut(thresholds != 0);
    return h.release();
}
void leaf_harness_destroy(void* p) { delete static_cast<LeafHarness*>(p); }
int leaf_harness_run(void* p, float* R9, float* t3, float* best_sse, unsigned long long* stats7, unsigned long long* rows3) {
    auto* h = static_cast<LeafHarness*>(p);
    const int rc = h->drv->run();
    if (rc) return rc;
    Mat3f R; Vec3f t;
    h->drv->best_transform(R, t);
    std::memcpy(R9, R.m, sizeof(R.m));
    const Vec3f tr = t / h->base->scale + R * h->base->off_s - h->base->off_t;  // fgoicp.hpp:87-90, as harness_run
    t3[0] = tr.x; t3[1] = tr.y; t3[2] = tr.z;
    *best_sse = h->drv->best_sse();
    const DriverStats& s = h->drv->stats();
    stats7[0] = s.trans_cubes; stats7[1] = s.bounds_calls; stats7[2] = s.rot_cubes; stats7[3] = s.icp_runs; stats7[4] = s.icp_iters;
    stats7[5] = s.inner_bnb; stats7[6] = s.rounds;
    rows3[0] = h->ops.rows; rows3[1] = h->ops.cut_lb; rows3[2] = h->ops.cut_leaf;
    return 0;
}

}  // extern "C"
