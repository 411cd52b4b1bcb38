// TEST-ONLY: the host side of the information matrix without a GPU — the CLI's `io.information` / `params.information_distance` keys
// (fast-go-icp_amd/csrc/cli/config.hpp), what the parser prints, and the file writer, driven through a C interface
// (tests/test_information_host.py).
#include <cstdio>
#include <cstring>
#include <sstream>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

extern "C" {

struct InfoConfigOut {
    char target[512], source[512], output[512], visualization[512], alignment[512], information[512], printed[2048];
    float information_distance;
};

int info_parse_config(const char* path, InfoConfigOut* out) {
    try {
        cli::Config c(path);
        std::snprintf(out->target, sizeof(out->target), "%s", c.io.target.c_str());
        std::snprintf(out->source, sizeof(out->source), "%s", c.io.source.c_str());
        std::snprintf(out->output, sizeof(out->output), "%s", c.io.output.c_str());
        std::snprintf(out->visualization, sizeof(out->visualization), "%s", c.io.visualization.c_str());
        std::snprintf(out->alignment, sizeof(out->alignment), "%s", c.io.alignment.c_str());
        std::snprintf(out->information, sizeof(out->information), "%s", c.io.information.c_str());
        std::ostringstream os;
        os << c;  // the summary the CLI prints
        std::snprintf(out->printed, sizeof(out->printed), "%s", os.str().c_str());
        out->information_distance = c.params.information_distance;
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

int info_write(const char* path, unsigned long long points, unsigned long long correspondences, double sum_dist2, const double* info36, float scaling_factor,
               float distance) {
    try {
        fgoicp_information_t s{};
        s.struct_size = sizeof(s);
        s.points = points;
        s.correspondences = correspondences;
        s.sum_dist2 = sum_dist2;
        std::memcpy(s.info, info36, sizeof(s.info));
        s.scaling_factor = scaling_factor;
        cli::write_information_txt(path, s, distance);
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

}  // extern "C"
