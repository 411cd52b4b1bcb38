// The scans' fp32 squared distance (device code only), shared by every kernel file: one text, one rounding order.
#pragma once
#include <hip/hip_runtime.h>

namespace fgoicp {

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// distance_squared, fgoicp/registration.cu:154-160 / :250-256
__device__ __forceinline__ float dist_sq(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fma_(dz, dz, fma_(dy, dy, dx * dx));
}

}  // namespace fgoicp
