// TEST-ONLY: the params.refine = "mesh" side of the CLI's parser and of its result writer (fast-go-icp_amd/csrc/cli/config.hpp).
//   mesh_refine_config_check config FILE.toml   prints the refine keys as the configuration parser reads them
//   mesh_refine_config_check write FILE.toml    writes a planted result with a mesh [refined] table through write_result_toml
#include <cstdio>
#include <cstring>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    try {
        if (!std::strcmp(argv[1], "config")) {
            cli::Config c(argv[2]);
            std::printf("REFINE [%s] KNN %d MAX_ITER %d DISTANCE %.9g EPSILON %.9g LOSS [%s] %d SCALE %.9g DEVIATION [%s]\n", c.params.refine.c_str(), c.params.refine_knn,
                        c.params.refine_max_iter, (double)c.params.refine_distance, c.params.refine_epsilon, c.params.refine_loss.c_str(), c.params.refine_loss_code(),
                        c.params.refine_loss_scale, c.io.deviation.c_str());
            return 0;
        }
        if (std::strcmp(argv[1], "write")) return 3;
        icp::mat3 R;
        const float eye[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        std::memcpy(R.data(), eye, sizeof(eye));
        fgoicp_run_stats st{};
        fgoicp_plane_result_t refined{};
        std::memcpy(refined.R, eye, sizeof(eye));
        refined.t[0] = 0.5f; refined.t[1] = -0.25f; refined.t[2] = 2.0f;
        refined.iterations = 4; refined.rank = 6; refined.correspondences = 600; refined.plane_rmse = 0.125; refined.scaling_factor = 1.0f;
        fgoicp_robust_result_t robust{};
        robust.scale = 0.75; robust.scaling_factor = 1.0f; robust.weight_sum = 480.5;
        const double rms_distance = 0.25;
        cli::write_result_toml(argv[2], R, icp::vec3{0.0f, 0.0f, 0.0f}, 1.0f, 600, 0.5, st, &refined, "mesh_rmse", &robust, "tukey", &rms_distance);
        std::printf("WRITTEN\n");
        return 0;
    } catch (const std::exception& e) {
        std::printf("REFUSED %s\n", e.what());
        return 2;
    }
}
