// The host half of the plane segmentation (fgoicp_segment_planes, fgoicp_segment_hypotheses, fgoicp_segment_fit_from_moments; DESIGN.md
// section 18): the counter-based draws, the table of one peel's hypothesis planes and the refit from the inliers' moments, all in fp64 with
// every operation rounded on its own (the build passes -ffp-contract=off).  No device, no HIP headers.  The device call builds its tables
// and refits its planes with these functions: there is one text.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../../include/fgoicp_amd.h"

namespace fgoicp {
void set_error(const std::string& s);

constexpr int kSegMaxIterations = 65536, kSegMaxPlanes = 16;

// the splitmix64 finaliser; also the hash of fgoicp_mesh_sample's draws, which run on the device (mesh.hip)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t seg_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// draw s (0, 1, 2) of hypothesis h of peel j among m candidates: a position in [0, m); everything mod 2^64, m < 2^31 keeps the product below 2^63
inline uint64_t seg_draw(uint64_t seed, uint64_t peel, uint64_t K, uint64_t h, uint64_t s, uint64_t m) {
    const uint64_t u = seg_mix64(seed + 0x9E3779B97F4A7C15ull * ((peel * K + h) * 3ull + s + 1ull));
    return ((u >> 32) * m) >> 32;
}

// One peel's table.  cand: the m candidate caller indices in ascending order, NULL = 0 .. m - 1.  Per hypothesis: sample (3 caller indices),
// plane (nx, ny, nz, d), degenerate (0 / 1).  A degenerate hypothesis reports the plane as four +0.0.
inline void segment_hypotheses(const float* xyz, const uint32_t* cand, size_t m, int K, uint64_t seed, int peel, uint32_t* sample_K3, double* plane_K4,
                               unsigned char* degenerate_K) {
    for (int h = 0; h < K; ++h) {
        uint32_t idx[3];
        for (int s = 0; s < 3; ++s) {
            const uint64_t at = seg_draw(seed, (uint64_t)peel, (uint64_t)K, (uint64_t)h, (uint64_t)s, (uint64_t)m);
            idx[s] = cand ? cand[at] : (uint32_t)at;
        }
        const float *pa = xyz + 3 * (size_t)idx[0], *pb = xyz + 3 * (size_t)idx[1], *pc = xyz + 3 * (size_t)idx[2];
        const double ax = pa[0], ay = pa[1], az = pa[2];
        const double e1x = (double)pb[0] - ax, e1y = (double)pb[1] - ay, e1z = (double)pb[2] - az;
        const double e2x = (double)pc[0] - ax, e2y = (double)pc[1] - ay, e2z = (double)pc[2] - az;
        const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
        const double L2 = (Nx * Nx + Ny * Ny) + Nz * Nz;
        const bool deg = idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2] || !(L2 > 0.0) || !std::isfinite(L2);
        double p[4] = {0.0, 0.0, 0.0, 0.0};
        if (!deg) {
            const double len = std::sqrt(L2);
            p[0] = Nx / len; p[1] = Ny / len; p[2] = Nz / len;
            p[3] = -((p[0] * ax + p[1] * ay) + p[2] * az);
        }
        if (sample_K3) for (int s = 0; s < 3; ++s) sample_K3[3 * (size_t)h + s] = idx[s];
        if (plane_K4) for (int k = 0; k < 4; ++k) plane_K4[4 * (size_t)h + k] = p[k];
        if (degenerate_K) degenerate_K[h] = deg ? 1 : 0;
    }
}

// Eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi sweeps, as sym6_jacobi (plane.hpp): A = V diag(w) V^T
inline void sym3_jacobi(double A[3][3], double V[3][3], double w[3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, all = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                all += A[i][j] * A[i][j];
                if (i != j) off += A[i][j] * A[i][j];
            }
        if (!(off > 1e-30 * all)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {  // A <- A G (columns p, q)
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {  // A <- G^T A (rows p, q)
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// The refit: count points u = p - pivot with sums sum_u and sum_uu (xx xy xz yy yz zz) -> the plane through pivot + mean whose normal is
// the unit eigenvector of the smallest eigenvalue of C = sum_uu / count - mean mean^T, flipped so that its dot product with toward's
// normal is >= 0 (toward = NULL: as the iteration leaves it).
inline void segment_fit(uint64_t count, const double* pivot, const double* su, const double* suu, const double* toward, double* plane) {
    const double cnt = (double)count;
    const double mean[3] = {su[0] / cnt, su[1] / cnt, su[2] / cnt};
    double A[3][3], V[3][3], w[3];
    const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) A[a][b] = suu[at[a][b]] / cnt - mean[a] * mean[b];
    sym3_jacobi(A, V, w);
    int lo = 0;
    for (int i = 1; i < 3; ++i)
        if (w[i] < w[lo]) lo = i;
    double nv[3] = {V[0][lo], V[1][lo], V[2][lo]};
    const double len = std::sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    for (int a = 0; a < 3; ++a) nv[a] /= len;
    if (toward && (nv[0] * toward[0] + nv[1] * toward[1]) + nv[2] * toward[2] < 0.0)
        for (int a = 0; a < 3; ++a) nv[a] = -nv[a];
    const double q[3] = {pivot[0] + mean[0], pivot[1] + mean[1], pivot[2] + mean[2]};
    plane[0] = nv[0]; plane[1] = nv[1]; plane[2] = nv[2];
    plane[3] = -((nv[0] * q[0] + nv[1] * q[1]) + nv[2] * q[2]);
}

// fgoicp_segment_hypotheses: the refusals and the call
inline int segment_hypotheses_entry(const float* xyz, size_t n, const uint32_t* cand, size_t m, int iterations, uint64_t seed, int peel, uint32_t* sample_K3,
                                    double* plane_K4, unsigned char* degenerate_K) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_segment_hypotheses: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!xyz || n == 0) return refuse("the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
    if (m == 0 || m > n || (!cand && m != n)) return refuse("m must lie in [1, n], and equal n without a candidate list");
    if (iterations < 1 || iterations > kSegMaxIterations) return refuse("iterations must lie in [1, 65536]");
    if (peel < 0 || peel >= kSegMaxPlanes) return refuse("peel must lie in [0, 16)");
    for (size_t c = 0; cand && c < m; ++c)
        if (cand[c] >= n || (c && cand[c] <= cand[c - 1])) return refuse("the candidates must be ascending indices below n");
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse("point " + std::to_string(i) + " has a non-finite coordinate");
    segment_hypotheses(xyz, cand, m, iterations, seed, peel, sample_K3, plane_K4, degenerate_K);
    return FGOICP_OK;
}

// fgoicp_segment_fit_from_moments: the refusals and the call
inline int segment_fit_entry(uint64_t count, const double* pivot3, const double* sum_u3, const double* sum_uu6, const double* toward4, double* plane4) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_segment_fit_from_moments: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!pivot3 || !sum_u3 || !sum_uu6 || !plane4) return refuse("pivot3, sum_u3, sum_uu6 and plane4 must not be null");
    if (count < 3) return refuse("fewer than 3 points have no plane");
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(pivot3[k]) && std::isfinite(sum_u3[k]);
    for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(sum_uu6[k]);
    for (int k = 0; toward4 && k < 3; ++k) finite = finite && std::isfinite(toward4[k]);
    if (!finite) return refuse("a moment is not finite");
    double out[4];
    segment_fit(count, pivot3, sum_u3, sum_uu6, toward4, out);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(out[k])) return refuse("the moments give no finite plane");
    for (int k = 0; k < 4; ++k) plane4[k] = out[k];
    return FGOICP_OK;
}

}  // namespace fgoicp
