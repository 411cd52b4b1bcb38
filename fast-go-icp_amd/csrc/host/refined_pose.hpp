// The information matrix at a REFINED pose, in the callers' frame (io.information of the command-line tool after params.refine;
// fgoicp_batch_refined_information): ONE text for both, over the public ABI only, built with -ffp-contract=off on either side, so that the
// two write the same bytes.
//   1. the restored translation of fgoicp_solver_refine_* is taken back into the solver's frame, in fp32:
//          t_s = (t - R offset_pcs + offset_pct) * scale         (R9 in glm order; offs6 = {offset_pcs, offset_pct} as fgoicp_solver_preproc)
//   2. fgoicp_information on the context there, the distance threshold d of the callers' units as (d * scale)^2 (d <= 0: none);
//   3. fgoicp_information_from_moments turns the context-frame sums into the callers' frame (c = -offset_pct, the centroid subtracted).
#pragma once
#include <cmath>

#include "../../../include/fgoicp_amd.h"

namespace fgoicp {
inline void refined_solver_translation(const float* R9, const float* t3, const float* offs6, float scale, float* ts3) {
    for (int r = 0; r < 3; ++r) ts3[r] = (t3[r] - (R9[r] * offs6[0] + R9[3 + r] * offs6[1] + R9[6 + r] * offs6[2]) + offs6[3 + r]) * scale;
}
// inf->struct_size must be set (sizeof(fgoicp_information_t)).  Returns the status of the first call that fails.
inline int refined_information(fgoicp_ctx* ctx, const float* R9, const float* t3, const float* offs6, float scale, float d, fgoicp_information_t* inf) {
    float ts[3];
    refined_solver_translation(R9, t3, offs6, scale, ts);
    const float ds = d * scale;
    int rc = fgoicp_information(ctx, R9, ts, d > 0.0f ? ds * ds : INFINITY, inf);
    if (rc) return rc;
    const float c3[3] = {-offs6[3], -offs6[4], -offs6[5]};
    rc = fgoicp_information_from_moments(inf->correspondences, inf->sum_q, inf->sum_qq, c3, scale, inf->info, inf->sum_q, inf->sum_qq);
    if (rc) return rc;
    inf->scaling_factor = scale;
    return FGOICP_OK;
}
}  // namespace fgoicp
