// TEST-ONLY: the CLI side of the Generalized-ICP refinement without a GPU — the `params.refine*` keys (fast-go-icp_amd/csrc/cli/config.hpp)
// and the [refined] table of the result file, driven through a C interface (tests/test_gicp_host.py).
#include <cstdio>
#include <cstring>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

extern "C" {

struct GicpConfigOut {
    char refine[64], error[512];
    int refine_knn, refine_max_iter;
    float refine_distance;
    double refine_epsilon;
};

// 0: parsed; 2: the config was refused (out->error says why); 1: anything else
int gicp_parse_config(const char* path, GicpConfigOut* out) {
    try {
        cli::Config c(path);
        std::snprintf(out->refine, sizeof(out->refine), "%s", c.params.refine.c_str());
        out->refine_knn = c.params.refine_knn;
        out->refine_max_iter = c.params.refine_max_iter;
        out->refine_distance = c.params.refine_distance;
        out->refine_epsilon = c.params.refine_epsilon;
        return 0;
    } catch (const std::invalid_argument& e) {
        std::snprintf(out->error, sizeof(out->error), "%s", e.what());
        return 2;
    } catch (const std::exception&) {
        return 1;
    }
}

int gicp_write_result(const char* path, const fgoicp_plane_result_t* refined, const char* rmse_key) {
    try {
        icp::mat3 R;
        const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(R.data(), eye, sizeof(eye));
        if (rmse_key) cli::write_result_toml(path, R, icp::vec3{1.f, 2.f, 3.f}, 0.5f, 10, 1.25, fgoicp_run_stats{}, refined, rmse_key);
        else cli::write_result_toml(path, R, icp::vec3{1.f, 2.f, 3.f}, 0.5f, 10, 1.25, fgoicp_run_stats{}, refined);
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

}  // extern "C"
