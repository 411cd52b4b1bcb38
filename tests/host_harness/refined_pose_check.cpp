// TEST-ONLY: the hoisted information-pose helper (fast-go-icp_amd/csrc/host/refined_pose.hpp) against the expression it replaced in the
// command-line tool, on fixed inputs, bit for bit.  Stand-alone: the two ABI calls the helper makes are recorded by stand-ins here.
// Built with -ffp-contract=off, as the library and the tool are (tests/test_batch_refine_host.py).  Exit status 0 = the same bits.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../fast-go-icp_amd/csrc/host/refined_pose.hpp"

namespace {
struct Seen {
    float R[9], ts[3], max_dist2, c3[3], scale;
    int info_calls = 0, moment_calls = 0;
} seen;
}  // namespace

extern "C" int fgoicp_information(fgoicp_ctx*, const float* R9, const float* t3, float max_dist2, fgoicp_information_t* out) {
    std::memcpy(seen.R, R9, sizeof(seen.R));
    std::memcpy(seen.ts, t3, sizeof(seen.ts));
    seen.max_dist2 = max_dist2;
    ++seen.info_calls;
    out->correspondences = 7;
    for (int k = 0; k < 3; ++k) out->sum_q[k] = 0.25 * (k + 1);
    for (int k = 0; k < 6; ++k) out->sum_qq[k] = 0.125 * (k + 1);
    out->scaling_factor = 1.0f;
    return FGOICP_OK;
}
extern "C" int fgoicp_information_from_moments(uint64_t n, const double* sum_q3, const double* sum_qq6, const float* offset3, float scale, double* info36, double* sum_q3_out,
                                               double* sum_qq6_out) {
    if (n != 7 || sum_q3 != sum_q3_out || sum_qq6 != sum_qq6_out || !info36) return FGOICP_ERR_INVALID_ARG;  // in place, as the tool called it
    std::memcpy(seen.c3, offset3, sizeof(seen.c3));
    seen.scale = scale;
    ++seen.moment_calls;
    return FGOICP_OK;
}

static bool same(const void* a, const void* b, size_t n, const char* what) {
    if (std::memcmp(a, b, n) == 0) return true;
    std::fprintf(stderr, "refined_pose_check: %s differs\n", what);
    return false;
}

int main() {
    // rotations in glm order, restored translations, offsets {offset_pcs, offset_pct} and scales with long mantissas
    const float Rs[2][9] = {{0.9362934f, 0.2896295f, -0.1986693f, -0.2750958f, 0.9564251f, 0.0978434f, 0.2183507f, -0.0369570f, 0.9751703f},
                            {0.3320391f, -0.7071068f, 0.6242871f, 0.9111111f, 0.4082483f, -0.0567891f, -0.2447219f, 0.5773503f, 0.7790123f}};
    const float ts[2][3] = {{0.123456789f, -7.654321f, 3.1415927f}, {-1001.3337f, 0.000123f, 17.25001f}};
    const float offs[2][6] = {{-0.31f, 0.777777f, -12.5f, 4.000001f, -0.0625f, 9.87654f}, {100.1f, -200.2f, 300.3f, -0.001f, 0.002f, -0.003f}};
    const float scales[3] = {0.37123f, 1.0f, 0.0049731f};
    const float dists[4] = {0.0f, -1.0f, 0.05f, 3.3333333f};
    bool ok = true;
    int cases = 0;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int c = 0; c < 2; ++c)
                for (float scale : scales)
                    for (float d : dists) {
                        // the expression as the tool's write_information had it
                        const float* Q = Rs[a];
                        float want_ts[3];
                        for (int r = 0; r < 3; ++r) want_ts[r] = (ts[b][r] - (Q[r] * offs[c][0] + Q[3 + r] * offs[c][1] + Q[6 + r] * offs[c][2]) + offs[c][3 + r]) * scale;
                        const float ds = d * scale;
                        const float want_d2 = d > 0.0f ? ds * ds : INFINITY;
                        const float want_c3[3] = {-offs[c][3], -offs[c][4], -offs[c][5]};
                        fgoicp_information_t inf{};
                        inf.struct_size = sizeof(inf);
                        seen = Seen();
                        if (fgoicp::refined_information(nullptr, Rs[a], ts[b], offs[c], scale, d, &inf) != FGOICP_OK) { std::fprintf(stderr, "refined_pose_check: the helper failed\n"); return 1; }
                        ok &= seen.info_calls == 1 && seen.moment_calls == 1;
                        ok &= same(seen.R, Rs[a], sizeof(seen.R), "R") && same(seen.ts, want_ts, sizeof(want_ts), "the solver-frame translation");
                        ok &= same(&seen.max_dist2, &want_d2, sizeof(float), "the squared threshold") && same(seen.c3, want_c3, sizeof(want_c3), "the centroid");
                        ok &= same(&seen.scale, &scale, sizeof(float), "the scale") && same(&inf.scaling_factor, &scale, sizeof(float), "scaling_factor");
                        ++cases;
                    }
    std::fprintf(stderr, "refined_pose_check: %d cases %s\n", cases, ok ? "matched" : "DIFFER");
    return ok ? 0 : 1;
}
