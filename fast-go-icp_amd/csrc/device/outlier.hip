// Outlier removal (fgoicp_remove_outliers; include/fgoicp_amd.h has the definition, DESIGN.md section 14 the pipeline).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
//
//   host      the refusals (they need no device), then the exact search tree over the cloud itself (bvh_build_host)
//   knn       outlier_knn_kernel (kernels.hip): per point mean_dist (fp64) and kth_dist2 (fp32) at the caller index
//   moments   STATISTICAL only: the tree sum of mean_dist, the host forms the mean; the same tree over (m - mean)^2, the host forms
//             stddev and threshold (on the host: the value the mask is compared with is the value the caller gets)
//   flags     keep[i] = mean_dist[i] <= threshold, or kth_dist2[i] <= radius2
//   rows      the stable compaction of one_shot.hpp by those flags: the kept points and their indices in caller order
//
// Every sum is a function of n alone, in the fixed order of fixed_sum.hpp with one term and no count: a block of 256 consecutive caller
// indices is joined by wave_xor_sum over each wave and waves_in_order over its four waves, one row per block; the fold's thread t adds
// rows t, t + 1024, ... in that order — any number of rows — then the same two steps over its 16 waves.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "bvh.hpp"
#include "kernels.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

constexpr int kOutBlock = 256;

// rows[block] = the sum over the block's caller indices of m[i] (squared == 0) or (m[i] - mean)^2 (squared != 0); indices >= n add 0
__global__ __launch_bounds__(kOutBlock) void outlier_rows_kernel(const double* __restrict__ m, uint32_t n, double mean, int squared, double* __restrict__ rows) {
    __shared__ double s_v[kOutBlock / 64];
    const size_t i = (size_t)blockIdx.x * kOutBlock + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        v = m[i];
        if (squared) {
            const double d = v - mean;
            v = d * d;
        }
    }
    v = wave_xor_sum(v);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) rows[blockIdx.x] = waves_in_order<kOutBlock / 64>(s_v);
}
// One block of 1024 threads, any number of rows.
__global__ __launch_bounds__(1024) void outlier_fold_kernel(const double* __restrict__ rows, uint32_t nrows, double* __restrict__ out) {
    __shared__ double s_v[16];
    double v = 0.0;
    for (uint32_t b = threadIdx.x; b < nrows; b += 1024u) v += rows[b];
    v = wave_xor_sum(v);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = waves_in_order<16>(s_v);
}

__global__ __launch_bounds__(kOutBlock) void outlier_flag_kernel(const double* __restrict__ mean_dist, const float* __restrict__ kth_dist2, uint32_t n, int radius_mode,
                                                                double threshold, float radius2, uint8_t* __restrict__ keep, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * kOutBlock + threadIdx.x;
    if (i >= n) return;
    const bool k = radius_mode ? kth_dist2[i] <= radius2 : mean_dist[i] <= threshold;
    keep[i] = k ? 1 : 0;
    flag[i] = k ? 1u : 0u;
}

int remove_outliers_impl(const float* xyz, size_t n, int mode, int k, float param, int device, float* out_xyz, size_t capacity, uint32_t* kept_index, uint8_t* keep_n,
                         double* mean_dist_n, float* kth_dist2_n, fgoicp_outlier_info_t* out) {
    const char* const call = "fgoicp_remove_outliers";
    auto refuse = [call](const std::string& what) { return fgoicp::refuse(call, what); };
    if (const int rc = refuse_cloud_head(call, xyz, n)) return rc;
    if (mode != FGOICP_OUTLIER_STATISTICAL && mode != FGOICP_OUTLIER_RADIUS) return refuse("mode must be 0 (statistical) or 1 (radius)");
    if (k < kOutlierKnnMin || k > kKnnMax || (size_t)k > n) return refuse("k must lie in [2, 32] and be at most the number of points");
    const bool radius_mode = mode == FGOICP_OUTLIER_RADIUS;
    if (radius_mode ? !(std::isfinite(param) && param > 0.0f) : !(std::isfinite(param) && param >= 0.0f))
        return refuse(radius_mode ? "the radius must be a positive finite number" : "std_ratio must be a finite number >= 0");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_outlier_info_t, radius2), "fgoicp_outlier_info_t")) return rc;
    if (const int rc = refuse_first_non_finite(call, xyz, n)) return rc;
    if (const int rc = select_device(call, device)) return rc;

    const BvhHost tree = bvh_build_host_xyz(xyz, n);

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n;
    const uint32_t nrows = (uint32_t)((n + kOutBlock - 1) / kOutBlock);
    size_t scan_bytes = 0;
    ONECHK(call, rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    float *d_xyz, *d_kth, *d_out;
    BvhDevice bvh;
    BvhView view;
    double *d_mean, *d_rows, *d_sum;
    uint8_t* d_keep;
    uint32_t *d_flag, *d_row, *d_idx;
    char* tmp;
    Arena plan;
    plan.take(d_xyz, 3 * n); bvh_take(plan, tree, &bvh); plan.take(d_mean, n); plan.take(d_kth, n);
    plan.take(d_keep, n); plan.take(d_flag, n); plan.take(d_row, n); plan.take(d_out, 3 * n); plan.take(d_idx, n);
    plan.take(d_rows, nrows); plan.take(d_sum, 1); plan.take(tmp, scan_bytes);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);

    const dim3 block(kOutBlock), per_point(nrows);
    ONECHK(call, hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    ONECHK(call, bvh_upload_async(tree, bvh, d.stream, &view));
    launch_outlier_knn(view, (int)n, k, d_mean, d_kth, d.stream);

    double mean = 0.0, stddev = 0.0, threshold = 0.0;
    const float radius2 = radius_mode ? param * param : 0.0f;
    if (!radius_mode) {
        double sum = 0.0;
        hipLaunchKernelGGL(outlier_rows_kernel, per_point, block, 0, d.stream, d_mean, n32, 0.0, 0, d_rows);
        hipLaunchKernelGGL(outlier_fold_kernel, dim3(1), dim3(1024), 0, d.stream, d_rows, nrows, d_sum);
        ONECHK(call, hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
        mean = sum / (double)n;
        if (n > 1) {
            hipLaunchKernelGGL(outlier_rows_kernel, per_point, block, 0, d.stream, d_mean, n32, mean, 1, d_rows);
            hipLaunchKernelGGL(outlier_fold_kernel, dim3(1), dim3(1024), 0, d.stream, d_rows, nrows, d_sum);
            ONECHK(call, hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, d.stream));
            ONECHK(call, hipStreamSynchronize(d.stream));
            ONECHK(call, hipGetLastError());
            stddev = std::sqrt(sum / (double)(n - 1));
        }
        const double spread = (double)param * stddev;
        threshold = mean + spread;
    }
    hipLaunchKernelGGL(outlier_flag_kernel, per_point, block, 0, d.stream, d_mean, d_kth, n32, radius_mode ? 1 : 0, threshold, radius2, d_keep, d_flag);
    uint32_t h[2] = {0u, 0u};  // rows before the last point, the last point's flag
    if (const int rc = scan_flags_async(d, tmp, scan_bytes, d_flag, d_row, n, h)) return rc;
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    uint64_t kept = 0;
    if (const int rc = kept_rows(d, h, n, &kept)) return rc;

    fgoicp_outlier_info_t full{};
    full.points = n;
    full.kept = kept;
    full.mode = mode;
    full.k = k;
    full.mean = mean;
    full.stddev = stddev;
    full.threshold = threshold;
    full.radius2 = radius2;
    write_info(out, full);
    if ((out_xyz || kept_index) && capacity < kept) {
        set_error("fgoicp_remove_outliers: " + std::to_string(kept) + " points kept, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }

    if ((out_xyz || kept_index) && kept)
        if (const int rc = scatter_rows_async(d, d_xyz, d_flag, d_row, n, d_out, d_idx, kept, out_xyz, kept_index)) return rc;
    if (keep_n) ONECHK(call, hipMemcpyAsync(keep_n, d_keep, n, hipMemcpyDeviceToHost, d.stream));
    if (mean_dist_n) ONECHK(call, hipMemcpyAsync(mean_dist_n, d_mean, 8 * n, hipMemcpyDeviceToHost, d.stream));
    if (kth_dist2_n) ONECHK(call, hipMemcpyAsync(kth_dist2_n, d_kth, 4 * n, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_remove_outliers(const float* xyz, size_t n, int mode, int k, float param, int device, float* out_xyz, size_t capacity_points, uint32_t* kept_index,
                                      uint8_t* keep_n, double* mean_dist_n, float* kth_dist2_n, fgoicp_outlier_info_t* out) {
    return fgoicp::abi_guard("fgoicp_remove_outliers", [&] {
        return fgoicp::remove_outliers_impl(xyz, n, mode, k, param, device, out_xyz, capacity_points, kept_index, keep_n, mean_dist_n, kth_dist2_n, out);
    });
}
