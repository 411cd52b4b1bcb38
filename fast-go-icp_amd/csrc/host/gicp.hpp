// The per-pair arithmetic of the Generalized-ICP refinement (fgoicp_gicp_terms, fgoicp_gicp_moments, fgoicp_icp_gicp):
// ONE text for refine_moments_kernel (kernels.hip) and the host entry point.  No device, no HIP headers: under hipcc the function is
// __host__ __device__, under a plain C++ compiler it is a host function.
#pragma once
#include <cmath>
#include <string>

#include "../../../include/fgoicp_amd.h"

#if defined(__HIPCC__)
#define FGOICP_GICP_HD __host__ __device__
#else
#define FGOICP_GICP_HD
#endif

namespace fgoicp {
void set_error(const std::string& s);

// epsilon must be finite and lie in (0, 1]
inline bool gicp_epsilon_ok(double eps) { return eps > 0.0 && eps <= 1.0; }

// One correspondence.  x: the moved source point, q: the target point, nq: its normal, np: the source point's normal (source frame),
// R9: the rotation in glm order (R9[col * 3 + row]) — all fp32 values, every operation below in fp64.
//   m  = R np
//   S  = 2 I - (1 - eps) (nq nq^T + m m^T)          the sum of the two regularised covariances I - (1 - eps) n n^T
//   M  = adj(S) / det(S)                             S >= 2 eps I: always invertible
//   d  = x - q,  J = [ -[x]x | I ]  (3 x 6, twist order wx wy wz vx vy vz)
//   v  = the upper triangle of J^T M J row by row (21), J^T M d (6), d^T M d (1)
// With B = [x]x M (column j = x cross M[:, j]): J^T M J = [[T, B], [B^T, M]], T[i][k] = (x cross B[i][:])_k, J^T M d = (x cross M d, M d).
// M6 (optional): M as xx xy xz yy yz zz.
FGOICP_GICP_HD inline void gicp_pair_terms(const double x[3], const double q[3], const double nq[3], const double np[3], const float* R9, double eps, double* M6,
                                           double* v) {
    double m[3];
    for (int r = 0; r < 3; ++r) m[r] = (double)R9[r] * np[0] + (double)R9[3 + r] * np[1] + (double)R9[6 + r] * np[2];
    const double a = 1.0 - eps;
    const double s00 = 2.0 - a * (nq[0] * nq[0] + m[0] * m[0]), s11 = 2.0 - a * (nq[1] * nq[1] + m[1] * m[1]), s22 = 2.0 - a * (nq[2] * nq[2] + m[2] * m[2]);
    const double s01 = -a * (nq[0] * nq[1] + m[0] * m[1]), s02 = -a * (nq[0] * nq[2] + m[0] * m[2]), s12 = -a * (nq[1] * nq[2] + m[1] * m[2]);
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const double det = s00 * c00 + s01 * c01 + s02 * c02;
    double M[3][3];
    M[0][0] = c00 / det; M[0][1] = M[1][0] = c01 / det; M[0][2] = M[2][0] = c02 / det;
    M[1][1] = c11 / det; M[1][2] = M[2][1] = c12 / det; M[2][2] = c22 / det;
    if (M6) { M6[0] = M[0][0]; M6[1] = M[0][1]; M6[2] = M[0][2]; M6[3] = M[1][1]; M6[4] = M[1][2]; M6[5] = M[2][2]; }
    if (!v) return;
    double B[3][3], T[3][3];
    for (int j = 0; j < 3; ++j) {
        B[0][j] = x[1] * M[2][j] - x[2] * M[1][j];
        B[1][j] = x[2] * M[0][j] - x[0] * M[2][j];
        B[2][j] = x[0] * M[1][j] - x[1] * M[0][j];
    }
    for (int i = 0; i < 3; ++i) {
        T[i][0] = x[1] * B[i][2] - x[2] * B[i][1];
        T[i][1] = x[2] * B[i][0] - x[0] * B[i][2];
        T[i][2] = x[0] * B[i][1] - x[1] * B[i][0];
    }
    const double d[3] = {x[0] - q[0], x[1] - q[1], x[2] - q[2]};
    double Md[3];
    for (int i = 0; i < 3; ++i) Md[i] = M[i][0] * d[0] + M[i][1] * d[1] + M[i][2] * d[2];
    v[0] = T[0][0]; v[1] = T[0][1]; v[2] = T[0][2]; v[3] = B[0][0]; v[4] = B[0][1]; v[5] = B[0][2];
    v[6] = T[1][1]; v[7] = T[1][2]; v[8] = B[1][0]; v[9] = B[1][1]; v[10] = B[1][2];
    v[11] = T[2][2]; v[12] = B[2][0]; v[13] = B[2][1]; v[14] = B[2][2];
    v[15] = M[0][0]; v[16] = M[0][1]; v[17] = M[0][2];
    v[18] = M[1][1]; v[19] = M[1][2];
    v[20] = M[2][2];
    v[21] = x[1] * Md[2] - x[2] * Md[1];
    v[22] = x[2] * Md[0] - x[0] * Md[2];
    v[23] = x[0] * Md[1] - x[1] * Md[0];
    v[24] = Md[0]; v[25] = Md[1]; v[26] = Md[2];
    v[27] = d[0] * Md[0] + d[1] * Md[1] + d[2] * Md[2];
}

// fgoicp_gicp_terms: the refusals and the call
inline int gicp_terms_entry(const float* x3, const float* q3, const float* nq3, const float* np3, const float* R9, double eps, double* M6, double* v28) {
    if (!x3 || !q3 || !nq3 || !np3 || !R9) { set_error("fgoicp_gicp_terms: x, q, nq, np and R must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!gicp_epsilon_ok(eps)) { set_error("fgoicp_gicp_terms: epsilon must be finite and lie in (0, 1]"); return FGOICP_ERR_INVALID_ARG; }
    const double x[3] = {x3[0], x3[1], x3[2]}, q[3] = {q3[0], q3[1], q3[2]}, nq[3] = {nq3[0], nq3[1], nq3[2]}, np[3] = {np3[0], np3[1], np3[2]};
    gicp_pair_terms(x, q, nq, np, R9, eps, M6, v28);
    return FGOICP_OK;
}
}  // namespace fgoicp
