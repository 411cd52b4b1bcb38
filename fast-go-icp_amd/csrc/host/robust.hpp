// The robust losses of the point-to-plane and Generalized-ICP refinements (fgoicp_robust_weight, fgoicp_robust_moments,
// fgoicp_robust_residuals, fgoicp_robust_scale, fgoicp_icp_robust): ONE text of the weight for refine_moments_kernel
// (kernels.hip) and the host entry point, and the host half of the scale.  No device, no HIP headers: under hipcc the weight is
// __host__ __device__, under a plain C++ compiler it is a host function.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/fgoicp_amd.h"

#if defined(__HIPCC__)
#define FGOICP_ROBUST_HD __host__ __device__
#else
#define FGOICP_ROBUST_HD
#endif

namespace fgoicp {
void set_error(const std::string& s);

inline bool robust_loss_ok(int loss) { return loss >= FGOICP_LOSS_NONE && loss <= FGOICP_LOSS_TUKEY; }
inline bool robust_model_ok(int model) { return model == FGOICP_MODEL_PLANE || model == FGOICP_MODEL_GICP; }
// a scale must be finite and positive
inline bool robust_scale_ok(double c) { return c > 0.0 && std::isfinite(c); }

// The IRLS weight w(s) = rho'(s) / s of a residual s at scale c > 0: fp64, only + - * /, one rounding per operation (the build has
// -ffp-contract=off), so the host, the kernel and a numpy float64 restatement agree in every bit.  The switch is wave-uniform on the device.
FGOICP_ROBUST_HD inline double robust_weight(int loss, double s, double c) {
    const double a = s < 0.0 ? -s : s;
    switch (loss) {
        case FGOICP_LOSS_HUBER: return a <= c ? 1.0 : c / a;
        case FGOICP_LOSS_CAUCHY: {
            const double u = s / c;
            return 1.0 / (1.0 + u * u);
        }
        case FGOICP_LOSS_GEMAN_MCCLURE: {
            const double c2 = c * c, g = c2 / (c2 + s * s);
            return g * g;
        }
        case FGOICP_LOSS_TUKEY: {
            if (!(a <= c)) return 0.0;
            const double v = 1.0 - (s / c) * (s / c);
            return v * v;
        }
        default: return 1.0;
    }
}

// fgoicp_robust_weight: the refusals and the call; *w is written on success only
inline int robust_weight_entry(int loss, double s, double scale, double* w) {
    if (!w) { set_error("fgoicp_robust_weight: w must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_loss_ok(loss)) { set_error("fgoicp_robust_weight: unknown loss " + std::to_string(loss)); return FGOICP_ERR_INVALID_ARG; }
    if (!std::isfinite(s)) { set_error("fgoicp_robust_weight: s must be finite"); return FGOICP_ERR_INVALID_ARG; }
    if (loss != FGOICP_LOSS_NONE && !robust_scale_ok(scale)) { set_error("fgoicp_robust_weight: the scale must be finite and > 0"); return FGOICP_ERR_INVALID_ARG; }
    *w = robust_weight(loss, s, scale);
    return FGOICP_OK;
}

// what the device leaves (launch_refine_moments): the counted correspondences, the 28 sums of plane.hpp (weighted or not), the sum of the weights
constexpr int kRobustMoments = 29;
struct RefineMoments {
    uint64_t n = 0;
    double m[kRobustMoments] = {};  // m[28]: sum w
};

// 1.4826 x the lower median of |s| over the counted: sorted(|s|)[(N - 1) / 2], one fp64 product.  false: nothing counted
inline bool robust_mad_scale(const double* residual, const unsigned char* counted, size_t n, double* scale) {
    std::vector<double> a;
    a.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (counted[i]) a.push_back(std::fabs(residual[i]));
    if (a.empty()) return false;
    const size_t k = (a.size() - 1) / 2;
    std::nth_element(a.begin(), a.begin() + (std::ptrdiff_t)k, a.end());
    *scale = 1.4826 * a[k];
    return true;
}
}  // namespace fgoicp
