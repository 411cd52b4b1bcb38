// TEST-ONLY, stand-alone (its own main; tests/test_gicp_host.py builds it with -fsanitize=address,undefined and runs it): the host half
// of the Generalized-ICP refinement on a sum whose exact solution is known.  200 pairs with q_i = x_i + (w x x_i + v), every coordinate a
// multiple of 2^-8 and the twist (w, v) of 2^-10, so that q_i is exact in fp32: then d_i = -J_i (w, v) exactly, the normal equations
// sum J^T M J xi = -sum J^T M d have the solution xi = (w, v) whatever the M_i are, and the step must return it to 1e-9.
// The two entry points below are the library's (csrc/host/solver.cpp) over the same headers; the library itself links the HIP runtime.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../fast-go-icp_amd/csrc/host/gicp.hpp"
#include "../../fast-go-icp_amd/csrc/host/plane.hpp"

static std::string g_error;
namespace fgoicp {
void set_error(const std::string& s) { g_error = s; }
}  // namespace fgoicp

extern "C" int fgoicp_gicp_terms(const float* x3, const float* q3, const float* nq3, const float* np3, const float* R9, double epsilon, double* M6, double* v28) {
    return fgoicp::gicp_terms_entry(x3, q3, nq3, np3, R9, epsilon, M6, v28);
}
extern "C" int fgoicp_plane_step_from_moments(uint64_t n, const double* m28, double* xi6, int* rank) {
    if (!m28 || !xi6 || !rank) { fgoicp::set_error("fgoicp_plane_step_from_moments: m28, xi6 and rank must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (n == 0) { fgoicp::set_error("fgoicp_plane_step_from_moments: n = 0: nothing was counted, there is no step"); return FGOICP_ERR_INVALID_ARG; }
    if (!fgoicp::plane_moments_finite(m28)) { fgoicp::set_error("fgoicp_plane_step_from_moments: a moment is not finite"); return FGOICP_ERR_INVALID_ARG; }
    fgoicp::plane_step(m28, xi6, rank);
    return FGOICP_OK;
}

static uint32_t g_state = 12345u;
static double uniform() {  // [0, 1)
    g_state = g_state * 1664525u + 1013904223u;
    return (double)(g_state >> 8) / 16777216.0;
}
static void unit(float* n) {
    double v[3], len;
    do {
        for (int a = 0; a < 3; ++a) v[a] = 2.0 * uniform() - 1.0;
        len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    } while (len < 0.1 || len > 1.0);
    for (int a = 0; a < 3; ++a) n[a] = (float)(v[a] / len);
}

int main() {
    const double twist[6] = {3.0 / 1024, -2.0 / 1024, 1.0 / 1024, -4.0 / 1024, 5.0 / 1024, 2.0 / 1024};
    const float c = 0.8f, s = 0.6f;  // a rotation about z up to fp32 rounding, glm order
    const float R9[9] = {c, s, 0.f, -s, c, 0.f, 0.f, 0.f, 1.f};
    int bad = 0;
    for (double eps : {1.0, 0.1, 1e-3}) {
        double m[28] = {};
        const int pairs = 200;
        for (int i = 0; i < pairs; ++i) {
            float x[3], q[3], nq[3], np[3];
            for (int a = 0; a < 3; ++a) x[a] = (float)(std::floor(512.0 * uniform()) - 256.0) / 256.0f;
            const double w[3] = {twist[0], twist[1], twist[2]};
            const double wx[3] = {w[1] * x[2] - w[2] * x[1], w[2] * x[0] - w[0] * x[2], w[0] * x[1] - w[1] * x[0]};
            for (int a = 0; a < 3; ++a) {
                const double qa = (double)x[a] + wx[a] + twist[3 + a];
                q[a] = (float)qa;
                if ((double)q[a] != qa) { std::fprintf(stderr, "gicp_twist_check: q is not exact in fp32\n"); return 2; }
            }
            unit(nq);
            unit(np);
            double v[28], M6[6];
            if (fgoicp_gicp_terms(x, q, nq, np, R9, eps, M6, v) != FGOICP_OK) { std::fprintf(stderr, "gicp_twist_check: %s\n", g_error.c_str()); return 2; }
            for (int k = 0; k < 28; ++k) m[k] += v[k];
        }
        double xi[6];
        int rank = 0;
        if (fgoicp_plane_step_from_moments(pairs, m, xi, &rank) != FGOICP_OK) { std::fprintf(stderr, "gicp_twist_check: %s\n", g_error.c_str()); return 2; }
        double worst = 0.0;
        for (int k = 0; k < 6; ++k) worst = std::fmax(worst, std::fabs(xi[k] - twist[k]));
        std::fprintf(stderr, "gicp_twist_check: epsilon %g: rank %d, largest deviation from the twist %.3g\n", eps, rank, worst);
        if (rank != 6 || !(worst <= 1e-9)) ++bad;
    }
    // the refusals run under the sanitizers too
    float z[3] = {0.f, 0.f, 1.f};
    double v[28];
    if (fgoicp_gicp_terms(nullptr, z, z, z, R9, 1e-3, nullptr, v) != FGOICP_ERR_INVALID_ARG) ++bad;
    if (fgoicp_gicp_terms(z, z, z, z, R9, 0.0, nullptr, v) != FGOICP_ERR_INVALID_ARG) ++bad;
    if (fgoicp_gicp_terms(z, z, z, z, R9, 1e-3, nullptr, nullptr) != FGOICP_OK) ++bad;
    if (bad) { std::fprintf(stderr, "gicp_twist_check: %d checks failed\n", bad); return 1; }
    std::fprintf(stderr, "gicp_twist_check: all checks passed\n");
    return 0;
}
