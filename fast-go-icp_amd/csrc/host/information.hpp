// The host half of fgoicp_information / fgoicp_solver_information / fgoicp_batch_information / fgoicp_information_from_moments: the
// change of frame of the ten moments and the assembly of the 6 x 6 matrix, in fp64.  No device, no HIP headers.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../../include/fgoicp_amd.h"

namespace fgoicp {
void set_error(const std::string& s);

// what the device leaves (launch_align_info): the counted correspondences and their sums, in the frame of the clouds the context holds
struct InfoMoments {
    uint64_t n = 0;
    double sum_q[3] = {0, 0, 0};
    double sum_qq[6] = {0, 0, 0, 0, 0, 0};  // xx xy xz yy yz zz
    double sum_d2 = 0.0;
};

// The context holds q_s = (q - c) * s; the moments of q = q_s / s + c:
//   sum q     = sum q_s / s + N c
//   sum q q^T = sum q_s q_s^T / s^2 + (c sum q_s^T + sum q_s c^T) / s + N c c^T
// and Info = [ (tr sum qq) I - sum qq , [sum q]x ; -[sum q]x , N I ], twist order (wx, wy, wz, vx, vy, vz), row-major.
// offset3 = nullptr, scale = 1: no change of frame.  Every output may be null.
// (one definition, csrc/host/solver.cpp, so that every caller runs the same instructions: the three entry points agree bit for bit)
void information_from_moments(uint64_t n, const double* sq_s, const double* sqq_s, const float* offset3, float scale, double* info36, double* sum_q3_out,
                              double* sum_qq6_out);

// the threshold a solver or a batch takes is a distance in the callers' units; the device compares squared distances in the context's
// frame.  This arithmetic, in fp32, is part of the interface (include/fgoicp_amd.h).
inline float information_max_dist2(float max_distance, float scale) {
    const float ds = max_distance * scale;
    return ds * ds;
}

// `full` from the device's moments: offset3 / scale as above (a bare context: nullptr, 1), max_dist2 the threshold the device compared with
inline void information_fill(fgoicp_information_t& full, uint64_t points, const InfoMoments& m, const float* offset3, float scale, float max_dist2) {
    std::memset(&full, 0, sizeof(full));  // the padding too: two results of the same inputs are the same bytes
    full.struct_size = (uint32_t)sizeof(full);
    full.points = points;
    full.correspondences = m.n;
    full.sum_dist2 = m.sum_d2;
    information_from_moments(m.n, m.sum_q, m.sum_qq, offset3, scale, full.info, full.sum_q, full.sum_qq);
    full.max_dist2 = max_dist2;
    full.scaling_factor = scale;
}

inline bool information_size_ok(const fgoicp_information_t* out) { return out && out->struct_size >= sizeof(uint32_t) && out->struct_size <= 4096; }
// a result handed to a caller: no byte beyond the struct_size the caller set is written
inline int information_out(const fgoicp_information_t& full, fgoicp_information_t* out, const char* where) {
    if (!information_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(fgoicp_information_t)"); return FGOICP_ERR_INVALID_ARG; }
    const uint32_t n = out->struct_size;
    std::memcpy(out, &full, n < sizeof(full) ? n : sizeof(full));
    out->struct_size = n;
    return FGOICP_OK;
}
}  // namespace fgoicp
