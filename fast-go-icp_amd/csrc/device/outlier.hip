// Outlier removal (fgoicp_remove_outliers; include/fgoicp_amd.h has the definition, DESIGN.md section 14 the pipeline).
// One call = one stream + one device allocation of its own, both released before it returns; no fgoicp_ctx, no global state, no knobs.
//
//   host      the refusals (they need no device), then the exact search tree over the cloud itself (bvh_build_host)
//   knn       outlier_knn_kernel (kernels.hip): per point mean_dist (fp64) and kth_dist2 (fp32) at the caller index
//   moments   STATISTICAL only: the tree sum of mean_dist, the host forms the mean; the same tree over (m - mean)^2, the host forms
//             stddev and threshold (on the host: the value the mask is compared with is the value the caller gets)
//   flags     keep[i] = mean_dist[i] <= threshold, or kth_dist2[i] <= radius2
//   scan      rocPRIM exclusive scan of the flags: the output row of every kept point
//   scatter   out_xyz[row] = the point's three floats, kept_index[row] = i: stable, the rows are in caller order
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

#include "../../../include/fgoicp_amd.h"
#include "../host/abi_guard.hpp"
#include "bvh.hpp"
#include "kernels.hpp"

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

// row[i] = the exclusive scan of the flags: the number of kept points before i
__global__ __launch_bounds__(kOutBlock) void outlier_scatter_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ row,
                                                                   uint32_t n, float* __restrict__ out_xyz, uint32_t* __restrict__ kept_index) {
    const size_t i = (size_t)blockIdx.x * kOutBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float* p = xyz + 3 * i;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out_xyz + 3 * (size_t)row[i];
    o[0] = x; o[1] = y; o[2] = z;
    kept_index[row[i]] = (uint32_t)i;
}

struct OutDevice {  // what the call owns on the device
    hipStream_t stream = nullptr;
    void* arena = nullptr;
    ~OutDevice() {  // (an early return may leave copies into the caller's arrays in flight)
        if (stream) (void)hipStreamSynchronize(stream);
        if (arena) (void)hipFree(arena);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#define OUTCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) {                                                                            \
            set_error(std::string("fgoicp_remove_outliers: " #expr " failed: ") + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;                             \
        }                                                                                                  \
    } while (0)

int remove_outliers_impl(const float* xyz, size_t n, int mode, int k, float param, int device, float* out_xyz, size_t capacity, uint32_t* kept_index, uint8_t* keep_n,
                         double* mean_dist_n, float* kth_dist2_n, fgoicp_outlier_info_t* out) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_remove_outliers: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!xyz || n == 0) return refuse("the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
    if (mode != FGOICP_OUTLIER_STATISTICAL && mode != FGOICP_OUTLIER_RADIUS) return refuse("mode must be 0 (statistical) or 1 (radius)");
    if (k < kOutlierKnnMin || k > kKnnMax || (size_t)k > n) return refuse("k must lie in [2, 32] and be at most the number of points");
    const bool radius_mode = mode == FGOICP_OUTLIER_RADIUS;
    if (radius_mode ? !(std::isfinite(param) && param > 0.0f) : !(std::isfinite(param) && param >= 0.0f))
        return refuse(radius_mode ? "the radius must be a positive finite number" : "std_ratio must be a finite number >= 0");
    if (!out || out->struct_size < offsetof(fgoicp_outlier_info_t, radius2) || out->struct_size > 4096)
        return refuse("out must not be null and out->struct_size = sizeof(fgoicp_outlier_info_t)");
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse("point " + std::to_string(i) + " has a non-finite coordinate");

    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string("fgoicp_remove_outliers: no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                  "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return refuse("device ordinal out of range");
    OUTCHK(hipSetDevice(device));

    BvhHost tree;
    {
        std::vector<float4> p4(n);
        for (size_t i = 0; i < n; ++i) p4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
        tree = bvh_build_host(p4.data(), n);
    }

    OutDevice d;
    OUTCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n;
    const uint32_t nrows = (uint32_t)((n + kOutBlock - 1) / kOutBlock);
    size_t scan_bytes = 0;
    OUTCHK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    // the arena: every array starts on a 256-byte boundary
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t box_bytes = tree.box.size() * sizeof(float4), pts_bytes = tree.pts.size() * sizeof(float4), slab_bytes = tree.slab.size() * sizeof(float4);
    const size_t at_xyz = take(12 * n), at_box = take(box_bytes), at_pts = take(pts_bytes), at_slab = take(slab_bytes), at_mean = take(8 * n), at_kth = take(4 * n);
    const size_t at_keep = take(n), at_flag = take(4 * n), at_row = take(4 * n), at_out = take(12 * n), at_idx = take(4 * n);
    const size_t at_rows = take(8 * (size_t)nrows), at_sum = take(8), at_tmp = take(scan_bytes);
    OUTCHK(hipMalloc(&d.arena, total));
    char* base = static_cast<char*>(d.arena);
    float* d_xyz = reinterpret_cast<float*>(base + at_xyz);
    BvhView view{reinterpret_cast<const float4*>(base + at_box), reinterpret_cast<const float4*>(base + at_pts),
                 slab_bytes ? reinterpret_cast<const float4*>(base + at_slab) : nullptr, tree.depth, tree.first_leaf};
    double* d_mean = reinterpret_cast<double*>(base + at_mean);
    float* d_kth = reinterpret_cast<float*>(base + at_kth);
    uint8_t* d_keep = reinterpret_cast<uint8_t*>(base + at_keep);
    uint32_t *d_flag = reinterpret_cast<uint32_t*>(base + at_flag), *d_row = reinterpret_cast<uint32_t*>(base + at_row), *d_idx = reinterpret_cast<uint32_t*>(base + at_idx);
    float* d_out = reinterpret_cast<float*>(base + at_out);
    double *d_rows = reinterpret_cast<double*>(base + at_rows), *d_sum = reinterpret_cast<double*>(base + at_sum);
    void* tmp = base + at_tmp;

    const dim3 block(kOutBlock), per_point(nrows);
    OUTCHK(hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    OUTCHK(hipMemcpyAsync(base + at_box, tree.box.data(), box_bytes, hipMemcpyHostToDevice, d.stream));
    OUTCHK(hipMemcpyAsync(base + at_pts, tree.pts.data(), pts_bytes, hipMemcpyHostToDevice, d.stream));
    if (slab_bytes) OUTCHK(hipMemcpyAsync(base + at_slab, tree.slab.data(), slab_bytes, hipMemcpyHostToDevice, d.stream));
    launch_outlier_knn(view, (int)n, k, d_mean, d_kth, d.stream);

    double mean = 0.0, stddev = 0.0, threshold = 0.0;
    const float radius2 = radius_mode ? param * param : 0.0f;
    if (!radius_mode) {
        double sum = 0.0;
        hipLaunchKernelGGL(outlier_rows_kernel, per_point, block, 0, d.stream, d_mean, n32, 0.0, 0, d_rows);
        hipLaunchKernelGGL(outlier_fold_kernel, dim3(1), dim3(1024), 0, d.stream, d_rows, nrows, d_sum);
        OUTCHK(hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, d.stream));
        OUTCHK(hipStreamSynchronize(d.stream));
        OUTCHK(hipGetLastError());
        mean = sum / (double)n;
        if (n > 1) {
            hipLaunchKernelGGL(outlier_rows_kernel, per_point, block, 0, d.stream, d_mean, n32, mean, 1, d_rows);
            hipLaunchKernelGGL(outlier_fold_kernel, dim3(1), dim3(1024), 0, d.stream, d_rows, nrows, d_sum);
            OUTCHK(hipMemcpyAsync(&sum, d_sum, 8, hipMemcpyDeviceToHost, d.stream));
            OUTCHK(hipStreamSynchronize(d.stream));
            OUTCHK(hipGetLastError());
            stddev = std::sqrt(sum / (double)(n - 1));
        }
        const double spread = (double)param * stddev;
        threshold = mean + spread;
    }
    hipLaunchKernelGGL(outlier_flag_kernel, per_point, block, 0, d.stream, d_mean, d_kth, n32, radius_mode ? 1 : 0, threshold, radius2, d_keep, d_flag);
    OUTCHK(rocprim::exclusive_scan(tmp, scan_bytes, d_flag, d_row, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    uint32_t h[2] = {0u, 0u};  // rows before the last point, the last point's flag
    OUTCHK(hipMemcpyAsync(&h[0], d_row + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    OUTCHK(hipMemcpyAsync(&h[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    OUTCHK(hipStreamSynchronize(d.stream));
    OUTCHK(hipGetLastError());
    const uint64_t kept = (uint64_t)h[0] + h[1];
    if (kept > n || h[1] > 1u) {
        set_error("fgoicp_remove_outliers: the device returned an inconsistent row count");
        return FGOICP_ERR_HIP;
    }

    fgoicp_outlier_info_t full{};
    full.points = n;
    full.kept = kept;
    full.mode = mode;
    full.k = k;
    full.mean = mean;
    full.stddev = stddev;
    full.threshold = threshold;
    full.radius2 = radius2;
    full.struct_size = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
    std::memcpy(out, &full, full.struct_size);
    if ((out_xyz || kept_index) && capacity < kept) {
        set_error("fgoicp_remove_outliers: " + std::to_string(kept) + " points kept, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }

    if ((out_xyz || kept_index) && kept) {
        hipLaunchKernelGGL(outlier_scatter_kernel, per_point, block, 0, d.stream, d_xyz, d_flag, d_row, n32, d_out, d_idx);
        if (out_xyz) OUTCHK(hipMemcpyAsync(out_xyz, d_out, 12 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
        if (kept_index) OUTCHK(hipMemcpyAsync(kept_index, d_idx, 4 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
    }
    if (keep_n) OUTCHK(hipMemcpyAsync(keep_n, d_keep, n, hipMemcpyDeviceToHost, d.stream));
    if (mean_dist_n) OUTCHK(hipMemcpyAsync(mean_dist_n, d_mean, 8 * n, hipMemcpyDeviceToHost, d.stream));
    if (kth_dist2_n) OUTCHK(hipMemcpyAsync(kth_dist2_n, d_kth, 4 * n, hipMemcpyDeviceToHost, d.stream));
    OUTCHK(hipStreamSynchronize(d.stream));
    OUTCHK(hipGetLastError());
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
