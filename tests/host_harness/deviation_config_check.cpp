// TEST-ONLY: the io.deviation side of the CLI's parsers and writers (fast-go-icp_amd/csrc/cli/config.hpp).
//   deviation_config_check config FILE.toml   prints io.deviation as the configuration parser reads it ("" when absent)
//   deviation_config_check write FILE.txt     writes a planted three-point map with write_deviation_txt and prints its summary
#include <cstdio>
#include <cstring>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    try {
        if (!std::strcmp(argv[1], "config")) {
            cli::Config c(argv[2]);
            std::printf("DEVIATION [%s] ALIGNMENT [%s]\n", c.io.deviation.c_str(), c.io.alignment.c_str());
            return 0;
        }
        if (std::strcmp(argv[1], "write")) return 3;
        const std::vector<icp::vec3> src = {{1.0f, 2.0f, 3.0f}, {-0.5f, 0.25f, 1e-3f}, {4.0f, 5.0f, 6.0f}};
        const uint32_t face[3] = {7, 0, 4000000000u};
        const double dist2[3] = {0.25, 0.0, 4.0};
        const int8_t side[3] = {-1, 0, 1};
        const uint8_t region[3] = {0, 5, 2};
        fgoicp_mesh_distance_info_t mi{};
        mi.queries = 3; mi.triangles = 12; mi.zero_area = 1;
        const cli::DeviationSummary s = cli::summarize_deviation(mi, dist2, side);
        cli::write_deviation_txt(argv[2], src, face, dist2, side, region, s);
        std::printf("SUMMARY %llu %llu %llu %.17g %.17g %.17g %llu %llu %llu\n", (unsigned long long)s.points, (unsigned long long)s.triangles, (unsigned long long)s.zero_area, s.mean,
                    s.rms, s.max, (unsigned long long)s.negative, (unsigned long long)s.on_plane, (unsigned long long)s.positive);
        return 0;
    } catch (const std::exception& e) {
        std::printf("REFUSED %s\n", e.what());
        return 2;
    }
}
