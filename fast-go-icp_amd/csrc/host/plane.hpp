// The host half of the point-to-plane refinement (fgoicp_plane_step_from_moments, fgoicp_plane_apply_step, fgoicp_icp_plane,
// fgoicp_solver_refine_plane): the solve of the 6 x 6 normal equations and the pose update, in fp64.  No device, no HIP headers
// (DESIGN.md section 12).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../../include/fgoicp_amd.h"
#include "math3.hpp"

namespace fgoicp {
void set_error(const std::string& s);

// what the device leaves (launch_refine_moments): the 28 sums — the upper triangle of sum J^T J row by row (21), sum J^T r (6),
// sum r^2 — with J = [ (x cross n)^T, n^T ], r = n.(x - q), twist order (wx, wy, wz, vx, vy, vz)
constexpr int kPlaneMoments = 28;

// Eigen-decomposition of a symmetric 6 x 6 matrix by cyclic Jacobi sweeps: A = V diag(w) V^T, the columns of V the eigenvectors.  The
// sweeps end when the off-diagonal part is below 1e-30 of the whole in squared Frobenius norm (quadratic convergence: 6-8 sweeps).
inline void sym6_jacobi(double A[6][6], double V[6][6], double w[6]) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, all = 0.0;
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                all += A[i][j] * A[i][j];
                if (i != j) off += A[i][j] * A[i][j];
            }
        if (!(off > 1e-30 * all)) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) {  // A <- A G (columns p, q)
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {  // A <- G^T A (rows p, q)
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 6; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 6; ++i) w[i] = A[i][i];
}

// xi = the minimum-norm solution of (sum J^T J) xi = -sum J^T r in the span of the eigenvectors whose eigenvalue exceeds 1e-9 x the
// largest; rank = how many those are (a planar target: 3; nothing counted, or a zero matrix: 0 and xi = 0).
constexpr double kPlaneRankTol = 1e-9;
inline void plane_step(const double* m, double* xi, int* rank) {
    double A[6][6], V[6][6], w[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = m[k++];
    sym6_jacobi(A, V, w);
    double wmax = 0.0;
    for (int i = 0; i < 6; ++i) wmax = w[i] > wmax ? w[i] : wmax;
    for (int a = 0; a < 6; ++a) xi[a] = 0.0;
    int r = 0;
    for (int i = 0; i < 6 && wmax > 0.0; ++i) {
        if (!(w[i] > kPlaneRankTol * wmax)) continue;
        ++r;
        double proj = 0.0;
        for (int a = 0; a < 6; ++a) proj += V[a][i] * m[21 + a];
        for (int a = 0; a < 6; ++a) xi[a] -= V[a][i] * (proj / w[i]);
    }
    *rank = r;
}
inline bool plane_moments_finite(const double* m) {
    for (int k = 0; k < kPlaneMoments; ++k)
        if (!std::isfinite(m[k])) return false;
    return true;
}

// The pose update of a step xi = (w, v): R' = Rod(w) R, t' = Rod(w) t + v, Rod = Rodrigues' formula, everything in fp64 from the fp32
// pose; R' is rounded to fp32 once and then passes through closest_orthogonal_approximation (the rotation nearest to it), so a chain of
// updates stays a rotation.
inline void plane_rodrigues(const double* w, double Q[3][3]) {
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    // sin(th) / th and (1 - cos(th)) / th^2, by their series below 1e-4 (the next terms are below 1e-17 relative)
    const double a = th < 1e-4 ? 1.0 - th * th / 6.0 : std::sin(th) / th;
    const double b = th < 1e-4 ? 0.5 - th * th / 24.0 : (1.0 - std::cos(th)) / (th * th);
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int l = 0; l < 3; ++l) kk += K[i][l] * K[l][j];
            Q[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * kk;
        }
}
inline void plane_apply_step(const Mat3f& R, const Vec3f& t, const double* xi, Mat3f& R_out, Vec3f& t_out) {
    double Q[3][3];
    plane_rodrigues(xi, Q);
    Mat3f Mt;  // the transpose of the rounded product: closest_orthogonal_approximation(H) returns V D U^T for H = U S V^T, the rotation nearest to H^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Mt.at(i, j) = (float)(Q[i][0] * (double)R.at(j, 0) + Q[i][1] * (double)R.at(j, 1) + Q[i][2] * (double)R.at(j, 2));
    R_out = closest_orthogonal_approximation(Mt);
    const double tt[3] = {(double)t.x, (double)t.y, (double)t.z};
    float o[3];
    for (int i = 0; i < 3; ++i) o[i] = (float)(Q[i][0] * tt[0] + Q[i][1] * tt[1] + Q[i][2] * tt[2] + xi[3 + i]);
    t_out = Vec3f{o[0], o[1], o[2]};
}

// a result handed to a caller: no byte beyond the struct_size the caller set is written (0, or less than the size field itself: refused)
template <class T>
inline bool plane_size_ok(const T* out) { return out && out->struct_size >= sizeof(uint32_t) && out->struct_size <= 4096; }
template <class T>
inline int plane_out(const T& full, T* out, const char* where, const char* type) {
    if (!plane_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(" + type + ")"); return FGOICP_ERR_INVALID_ARG; }
    const uint32_t n = out->struct_size;
    std::memcpy(out, &full, n < sizeof(full) ? n : sizeof(full));
    out->struct_size = n;
    return FGOICP_OK;
}
}  // namespace fgoicp
