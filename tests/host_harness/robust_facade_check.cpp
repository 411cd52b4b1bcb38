// Test-only: the robust-loss methods of the header-only C++ façades (include/fgoicp/*.hpp) over the C ABI alone.  Without arguments: the
// host half — fgoicp_robust_weight and the struct sizes the façade sets — and the methods' signatures, no device.  With two raw clouds
// (the reference's TXT format) and a LUT resolution: FastGoICP::run(), then refine_robust (point-to-plane, Tukey, estimated scale) next
// to refine_plane, printed as one JSON object.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../include/fgoicp/fgoicp.hpp"
#include "../../include/fgoicp/registration.hpp"

static icp::PointCloud read_txt(const std::string& path) {
    std::ifstream f(path);
    size_t n = 0;
    f >> n;
    icp::PointCloud pc(n);
    for (size_t i = 0; i < n; ++i) f >> pc[i].x >> pc[i].y >> pc[i].z;
    return pc;
}

int main(int argc, char** argv) {
    // the signatures, as a caller spells them
    icp::RobustRefinement (icp::FastGoICP::*solver_call)(int, int, double, int, size_t, float, float, double) const = &icp::FastGoICP::refine_robust;
    icp::RobustRefinement (icp::Registration::*ctx_call)(icp::mat3, icp::vec3, int, int, double, size_t, float, float, double) const = &icp::Registration::icp_robust;
    if (!solver_call || !ctx_call) return 3;
    if (argc < 4) {
        double w = -1.0;
        if (fgoicp_robust_weight(FGOICP_LOSS_TUKEY, 0.5, 1.0, &w) != FGOICP_OK || w != 0.5625) return 4;       // (1 - 1/4)^2
        if (fgoicp_robust_weight(FGOICP_LOSS_HUBER, -4.0, 1.0, &w) != FGOICP_OK || w != 0.25) return 5;
        if (fgoicp_robust_weight(FGOICP_LOSS_CAUCHY, 1.0, 1.0, &w) != FGOICP_OK || w != 0.5) return 6;
        if (fgoicp_robust_weight(FGOICP_LOSS_GEMAN_MCCLURE, 1.0, 1.0, &w) != FGOICP_OK || w != 0.25) return 7;
        if (fgoicp_robust_weight(7, 1.0, 1.0, &w) != FGOICP_ERR_INVALID_ARG || w != 0.25) return 8;            // refused: w untouched
        icp::RobustRefinement r;
        std::printf("HOST OK %zu %zu\n", sizeof(r.result), sizeof(fgoicp_robust_moments_t));
        return 0;
    }
    icp::FastGoICP solver(read_txt(argv[1]), read_txt(argv[2]), std::stof(argv[3]), 1e-3f);
    solver.run();
    const icp::PlaneRefinement plain = solver.refine_plane();
    const icp::RobustRefinement rob = solver.refine_robust(FGOICP_MODEL_PLANE, FGOICP_LOSS_TUKEY);
    std::cout.flush();
    std::printf("{\"plain_iterations\": %d, \"iterations\": %d, \"rank\": %d, \"correspondences\": %llu, \"weight_sum\": %.17g, \"rmse\": %.17g, \"loss_scale\": %.17g, "
                "\"scale_estimated\": %d, \"loss\": %d, \"t\": [%.9g, %.9g, %.9g]}\n",
                plain.result.iterations, rob.result.iterations, rob.result.rank, (unsigned long long)rob.result.correspondences, rob.weight_sum(), rob.rmse(), rob.loss_scale(),
                rob.scale_estimated() ? 1 : 0, rob.result.loss, rob.t().x, rob.t().y, rob.t().z);
    return 0;
}
