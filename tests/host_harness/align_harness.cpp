// TEST-ONLY: the host side of the alignment report without a GPU — the CLI's `io.alignment` key (fast-go-icp_amd/csrc/cli/config.hpp) and its
// file writer, driven with canned arrays through a C interface (tests/test_alignment_host.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

extern "C" {

struct AlignConfigOut {
    char target[512], source[512], output[512], visualization[512], alignment[512];
};

int align_parse_config(const char* path, AlignConfigOut* out) {
    try {
        cli::Config c(path);
        std::snprintf(out->target, sizeof(out->target), "%s", c.io.target.c_str());
        std::snprintf(out->source, sizeof(out->source), "%s", c.io.source.c_str());
        std::snprintf(out->output, sizeof(out->output), "%s", c.io.output.c_str());
        std::snprintf(out->visualization, sizeof(out->visualization), "%s", c.io.visualization.c_str());
        std::snprintf(out->alignment, sizeof(out->alignment), "%s", c.io.alignment.c_str());
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

int align_write(const char* path, const float* src_xyz, size_t ns, const uint32_t* idx, const float* dist2, const uint8_t* inlier, unsigned long long inliers,
                unsigned long long targets_hit, float sse, float max_inlier_dist2, float scaling_factor) {
    try {
        std::vector<icp::vec3> src(ns);
        for (size_t i = 0; i < ns; ++i) src[i] = icp::vec3(src_xyz[3 * i], src_xyz[3 * i + 1], src_xyz[3 * i + 2]);
        fgoicp_alignment_summary s{};
        s.struct_size = sizeof(s);
        s.points = ns;
        s.inliers = inliers;
        s.targets_hit = targets_hit;
        s.sse = sse;
        s.max_inlier_dist2 = max_inlier_dist2;
        s.scaling_factor = scaling_factor;
        cli::write_alignment_txt(path, src, idx, dist2, inlier, s);
        return 0;
    } catch (const std::exception&) {
        return 1;
    }
}

}  // extern "C"
