// Plane segmentation by RANSAC (fgoicp_segment_planes; include/fgoicp_amd.h has the definition, DESIGN.md section 18 the launch chain).
// One call = one stream + one device allocation of its own, both released before it returns; no fgoicp_ctx, no global state, no knobs.
//
//   host      the refusals (they need no device); label[i] = -1
//   peel j    host: the candidates from the labels, the table of K planes (segment_hypotheses, host/segment.hpp), 32 bytes each, uploaded
//             score    segment_score_kernel (segment_score.hpp): count[h] for every hypothesis, one pass over the cloud
//             host: 4 bytes per hypothesis come back; the winner is the largest count, the lowest h among equals
//             moments  segment_moments_kernel under the winning plane: per block one MomentRow<9> (block_moment_row), folded by
//                      moment_fold_kernel<9> — the fixed order of fixed_sum.hpp, the term of caller index i at position i
//             host: the refit (segment_fit)
//             label    segment_label_kernel under the final plane: label[i] = j, and the number of points it labelled
//             the labels come back when another peel needs its candidates
//   rows      flag[i] from the label, rocPRIM exclusive scan, scatter — stable, the rows are in caller order (as cluster.hip)
// All plane arithmetic is fp64, every operation on its own (-ffp-contract=off).  The only atomics are integer adds.  No floating-point
// atomics, no cooperative launch, no grid barrier, no spin-wait.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../include/fgoicp_amd.h"
#include "../host/abi_guard.hpp"
#include "../host/segment.hpp"
#include "fixed_sum.hpp"
#include "segment_score.hpp"

namespace fgoicp {
namespace {

static_assert(kSegChunk <= kSegBlock, "thread t adds up hypothesis t of the chunk");
static_assert(sizeof(SegPlane) == 32, "the table is 32 bytes per hypothesis");
constexpr int kSegTerms = 9;  // sum_u (3), sum_uu (6: xx xy xz yy yz zz)

__global__ __launch_bounds__(kSegBlock) void segment_init_kernel(int32_t* __restrict__ label, uint32_t n) {
    const size_t i = (size_t)blockIdx.x * kSegBlock + threadIdx.x;
    if (i < n) label[i] = -1;
}

// One thread per caller index: the terms of the candidates within T of the plane, +0.0 for everyone else
__global__ __launch_bounds__(kSegBlock) void segment_moments_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ label, uint32_t n, SegPlane pl, double T,
                                                                   double ax, double ay, double az, MomentRow<kSegTerms>* __restrict__ rows) {
    const size_t i = (size_t)blockIdx.x * kSegBlock + threadIdx.x;
    double v[kSegTerms];
#pragma unroll
    for (int k = 0; k < kSegTerms; ++k) v[k] = 0.0;
    unsigned cnt = 0u;
    if (i < n && label[i] < 0) {
        const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
        const double r = ((pl.nx * x + pl.ny * y) + pl.nz * z) + pl.d;
        if (fabs(r) <= T) {
            const double ux = x - ax, uy = y - ay, uz = z - az;
            v[0] = ux; v[1] = uy; v[2] = uz;
            v[3] = ux * ux; v[4] = ux * uy; v[5] = ux * uz;
            v[6] = uy * uy; v[7] = uy * uz; v[8] = uz * uz;
            cnt = 1u;
        }
    }
    block_moment_row<kSegBlock / 64>(v, cnt, &rows[blockIdx.x]);
}

// label[i] = j for the candidates within T of the final plane; *labelled += their number, once per wave
__global__ __launch_bounds__(kSegBlock) void segment_label_kernel(const float* __restrict__ xyz, int32_t* __restrict__ label, uint32_t n, SegPlane pl, double T, int32_t j,
                                                                 unsigned long long* __restrict__ labelled) {
    const size_t i = (size_t)blockIdx.x * kSegBlock + threadIdx.x;
    bool in = false;
    if (i < n && label[i] < 0) {
        const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
        const double r = ((pl.nx * x + pl.ny * y) + pl.nz * z) + pl.d;
        in = fabs(r) <= T;
        if (in) label[i] = j;
    }
    const unsigned long long mask = __ballot(in);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(labelled, (unsigned long long)__popcll(mask));
}

__global__ __launch_bounds__(kSegBlock) void segment_flag_kernel(const int32_t* __restrict__ label, uint32_t n, int keep_planes, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * kSegBlock + threadIdx.x;
    if (i < n) flag[i] = ((label[i] >= 0) == (keep_planes != 0)) ? 1u : 0u;
}

// row[i] = the exclusive scan of the flags: the number of kept points before i
__global__ __launch_bounds__(kSegBlock) void segment_scatter_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ row,
                                                                   uint32_t n, float* __restrict__ out_xyz, uint32_t* __restrict__ kept_index) {
    const size_t i = (size_t)blockIdx.x * kSegBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float* p = xyz + 3 * i;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out_xyz + 3 * (size_t)row[i];
    o[0] = x; o[1] = y; o[2] = z;
    kept_index[row[i]] = (uint32_t)i;
}

struct SegDevice {  // what the call owns on the device
    hipStream_t stream = nullptr;
    void* arena = nullptr;
    ~SegDevice() {  // (an early return may leave copies into the caller's arrays in flight)
        if (stream) (void)hipStreamSynchronize(stream);
        if (arena) (void)hipFree(arena);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#define SEGCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            set_error(std::string("fgoicp_segment_planes: " #expr " failed: ") + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;                            \
        }                                                                                                 \
    } while (0)

int segment_planes_impl(const float* xyz, size_t n, float distance_threshold, int iterations, uint64_t seed, int max_planes, size_t min_inliers, int refit, int keep_planes,
                        int device, float* out_xyz, size_t capacity, uint32_t* kept_index, int32_t* label_n, fgoicp_segment_model_t* models, size_t capacity_models,
                        size_t model_size, fgoicp_segment_info_t* out) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_segment_planes: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!xyz || n == 0) return refuse("the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
    if (!(std::isfinite(distance_threshold) && distance_threshold > 0.0f)) return refuse("distance_threshold must be a positive finite number");
    if (iterations < 1 || iterations > kSegMaxIterations) return refuse("iterations must lie in [1, 65536]");
    if (max_planes < 1 || max_planes > kSegMaxPlanes) return refuse("max_planes must lie in [1, 16]");
    if (!out || out->struct_size < offsetof(fgoicp_segment_info_t, distance_threshold) + sizeof(out->distance_threshold) || out->struct_size > 4096)
        return refuse("out must not be null and out->struct_size = sizeof(fgoicp_segment_info_t)");
    if (models && model_size == 0) return refuse("model_size must be sizeof(fgoicp_segment_model_t), not 0");
    if (device < 0) return refuse("device ordinal out of range");
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse("point " + std::to_string(i) + " has a non-finite coordinate");

    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string("fgoicp_segment_planes: no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                  "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device >= ndev) return refuse("device ordinal out of range");  // (a negative one was refused above, where no count is needed)
    SEGCHK(hipSetDevice(device));

    SegDevice d;
    SEGCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n, K = (uint32_t)iterations;
    const double T = (double)distance_threshold;
    const bool want_rows = out_xyz || kept_index;
    size_t scan_bytes = 0;
    SEGCHK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    const uint32_t nrows = (uint32_t)((n + kSegBlock - 1) / kSegBlock), tiles = (uint32_t)((n + kSegTile - 1) / kSegTile);
    // the arena: every array starts on a 256-byte boundary
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t at_xyz = take(12 * n), at_label = take(4 * n), at_flag = take(4 * n), at_row = take(4 * n), at_out = take(12 * n), at_idx = take(4 * n);
    const size_t at_planes = take(sizeof(SegPlane) * (size_t)K), at_counts = take(4 * (size_t)K), at_rows = take(sizeof(MomentRow<kSegTerms>) * (size_t)nrows);
    const size_t at_sums = take(8 * (1 + kSegTerms)), at_ctr = take(8), at_tmp = take(scan_bytes);
    SEGCHK(hipMalloc(&d.arena, total));
    char* base = static_cast<char*>(d.arena);
    float *d_xyz = reinterpret_cast<float*>(base + at_xyz), *d_out = reinterpret_cast<float*>(base + at_out);
    int32_t* d_label = reinterpret_cast<int32_t*>(base + at_label);
    uint32_t *d_flag = reinterpret_cast<uint32_t*>(base + at_flag), *d_row = reinterpret_cast<uint32_t*>(base + at_row), *d_idx = reinterpret_cast<uint32_t*>(base + at_idx);
    SegPlane* d_planes = reinterpret_cast<SegPlane*>(base + at_planes);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(base + at_counts);
    MomentRow<kSegTerms>* d_rows = reinterpret_cast<MomentRow<kSegTerms>*>(base + at_rows);
    unsigned long long *d_sums = reinterpret_cast<unsigned long long*>(base + at_sums), *d_ctr = reinterpret_cast<unsigned long long*>(base + at_ctr);
    void* tmp = base + at_tmp;

    const dim3 block(kSegBlock), per_point(nrows);
    SEGCHK(hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(segment_init_kernel, per_point, block, 0, d.stream, d_label, n32);

    std::vector<int32_t> label(n, -1);  // the host's copy: the candidates of the next peel
    std::vector<uint32_t> cand, sample(3 * (size_t)K), counts(K);
    std::vector<double> plane(4 * (size_t)K);
    std::vector<unsigned char> degenerate(K);
    std::vector<SegPlane> table(K);
    std::vector<fgoicp_segment_model_t> found;
    uint64_t on_planes = 0;
    const uint64_t need = min_inliers > 3 ? (uint64_t)min_inliers : 3u;
    for (int j = 0; j < max_planes; ++j) {
        cand.clear();
        for (size_t i = 0; i < n; ++i)
            if (label[i] < 0) cand.push_back((uint32_t)i);
        const size_t m = cand.size();
        if (m < 3) break;
        segment_hypotheses(xyz, cand.data(), m, iterations, seed, j, sample.data(), plane.data(), degenerate.data());
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (uint32_t h = 0; h < K; ++h)  // a degenerate hypothesis: a NaN plane fails every comparison
            table[h] = degenerate[h] ? SegPlane{nan, nan, nan, nan} : SegPlane{plane[4 * (size_t)h], plane[4 * (size_t)h + 1], plane[4 * (size_t)h + 2], plane[4 * (size_t)h + 3]};
        SEGCHK(hipMemcpyAsync(d_planes, table.data(), sizeof(SegPlane) * (size_t)K, hipMemcpyHostToDevice, d.stream));
        SEGCHK(hipMemsetAsync(d_counts, 0, 4 * (size_t)K, d.stream));
        hipLaunchKernelGGL(segment_score_kernel, dim3(tiles, segment_score_grid_y(tiles, K)), block, 0, d.stream, d_xyz, d_label, n32, d_planes, K, T, d_counts);
        SEGCHK(hipMemcpyAsync(counts.data(), d_counts, 4 * (size_t)K, hipMemcpyDeviceToHost, d.stream));
        SEGCHK(hipStreamSynchronize(d.stream));
        SEGCHK(hipGetLastError());
        uint32_t win = 0;
        for (uint32_t h = 1; h < K; ++h)
            if (counts[h] > counts[win]) win = h;  // strictly: a tie stays with the lowest h
        if (counts[win] > m) {
            set_error("fgoicp_segment_planes: the device returned an inconsistent inlier count");
            return FGOICP_ERR_HIP;
        }
        if (counts[win] < need) break;

        fgoicp_segment_model_t mod{};
        mod.candidates = m;
        for (int s = 0; s < 3; ++s) mod.sample[s] = sample[3 * (size_t)win + s];
        mod.hypothesis = win;
        mod.hypothesis_inliers = counts[win];
        for (int k = 0; k < 4; ++k) mod.hypothesis_plane[k] = mod.plane[k] = plane[4 * (size_t)win + k];
        for (int a = 0; a < 3; ++a) mod.pivot[a] = (double)xyz[3 * (size_t)mod.sample[0] + a];
        if (refit) {
            unsigned long long sums[1 + kSegTerms];
            hipLaunchKernelGGL(segment_moments_kernel, per_point, block, 0, d.stream, d_xyz, d_label, n32, table[win], T, mod.pivot[0], mod.pivot[1], mod.pivot[2], d_rows);
            hipLaunchKernelGGL(moment_fold_kernel<kSegTerms>, dim3(1), dim3(1024), 0, d.stream, d_rows, (int)nrows, d_sums);
            SEGCHK(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, d.stream));
            SEGCHK(hipStreamSynchronize(d.stream));
            SEGCHK(hipGetLastError());
            if (sums[0] != mod.hypothesis_inliers) {
                set_error("fgoicp_segment_planes: the moments counted " + std::to_string(sums[0]) + " inliers, the scores " + std::to_string(mod.hypothesis_inliers));
                return FGOICP_ERR_HIP;
            }
            std::memcpy(mod.sum_u, sums + 1, sizeof(mod.sum_u));
            std::memcpy(mod.sum_uu, sums + 4, sizeof(mod.sum_uu));
            const int rc = segment_fit_entry(mod.hypothesis_inliers, mod.pivot, mod.sum_u, mod.sum_uu, mod.hypothesis_plane, mod.plane);
            if (rc != FGOICP_OK) {
                set_error(std::string("fgoicp_segment_planes: the refit of plane ") + std::to_string(j) + " failed: " + fgoicp_last_error());
                return FGOICP_ERR_HIP;
            }
        }
        unsigned long long labelled = 0;
        SEGCHK(hipMemsetAsync(d_ctr, 0, 8, d.stream));
        hipLaunchKernelGGL(segment_label_kernel, per_point, block, 0, d.stream, d_xyz, d_label, n32, SegPlane{mod.plane[0], mod.plane[1], mod.plane[2], mod.plane[3]}, T,
                           (int32_t)j, d_ctr);
        SEGCHK(hipMemcpyAsync(&labelled, d_ctr, 8, hipMemcpyDeviceToHost, d.stream));
        if (j + 1 < max_planes) SEGCHK(hipMemcpyAsync(label.data(), d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
        SEGCHK(hipStreamSynchronize(d.stream));
        SEGCHK(hipGetLastError());
        if (labelled > m || (!refit && labelled != mod.hypothesis_inliers)) {
            set_error("fgoicp_segment_planes: the device returned an inconsistent label count");
            return FGOICP_ERR_HIP;
        }
        mod.inliers = labelled;
        on_planes += labelled;
        found.push_back(mod);
    }

    const uint64_t kept = keep_planes ? on_planes : (uint64_t)n - on_planes;
    fgoicp_segment_info_t full{};
    full.points = n;
    full.planes = found.size();
    full.on_planes = on_planes;
    full.kept = kept;
    full.iterations = iterations;
    full.max_planes = max_planes;
    full.refit = refit ? 1 : 0;
    full.keep_planes = keep_planes ? 1 : 0;
    full.min_inliers = min_inliers;
    full.seed = seed;
    full.distance_threshold = T;
    full.struct_size = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
    std::memcpy(out, &full, full.struct_size);
    if (want_rows && capacity < kept) {
        set_error("fgoicp_segment_planes: " + std::to_string(kept) + " points kept, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }
    if (models && capacity_models < found.size()) {
        set_error("fgoicp_segment_planes: " + std::to_string(found.size()) + " planes, capacity_models is " + std::to_string(capacity_models));
        return FGOICP_ERR_TOO_LARGE;
    }

    if (want_rows && kept) {
        uint32_t h[2] = {0u, 0u};  // rows before the last point, the last point's flag
        hipLaunchKernelGGL(segment_flag_kernel, per_point, block, 0, d.stream, d_label, n32, keep_planes, d_flag);
        SEGCHK(rocprim::exclusive_scan(tmp, scan_bytes, d_flag, d_row, 0u, n, rocprim::plus<uint32_t>(), d.stream));
        SEGCHK(hipMemcpyAsync(&h[0], d_row + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
        SEGCHK(hipMemcpyAsync(&h[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
        SEGCHK(hipStreamSynchronize(d.stream));
        SEGCHK(hipGetLastError());
        if ((uint64_t)h[0] + h[1] != kept) {  // checked before the scatter: its rows then lie below kept <= n
            set_error("fgoicp_segment_planes: the device returned an inconsistent row count");
            return FGOICP_ERR_HIP;
        }
        hipLaunchKernelGGL(segment_scatter_kernel, per_point, block, 0, d.stream, d_xyz, d_flag, d_row, n32, d_out, d_idx);
        if (out_xyz) SEGCHK(hipMemcpyAsync(out_xyz, d_out, 12 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
        if (kept_index) SEGCHK(hipMemcpyAsync(kept_index, d_idx, 4 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
    }
    if (label_n) SEGCHK(hipMemcpyAsync(label_n, d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
    SEGCHK(hipStreamSynchronize(d.stream));
    SEGCHK(hipGetLastError());
    const size_t each = model_size < sizeof(fgoicp_segment_model_t) ? model_size : sizeof(fgoicp_segment_model_t);
    for (size_t j = 0; models && j < found.size(); ++j) std::memcpy(reinterpret_cast<char*>(models) + j * model_size, &found[j], each);
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_segment_planes(const float* xyz, size_t n, float distance_threshold, int iterations, uint64_t seed, int max_planes, size_t min_inliers, int refit,
                                     int keep_planes, int device, float* out_xyz, size_t capacity_points, uint32_t* kept_index, int32_t* label_n,
                                     fgoicp_segment_model_t* models, size_t capacity_models, size_t model_size, fgoicp_segment_info_t* out) {
    return fgoicp::abi_guard("fgoicp_segment_planes", [&] {
        return fgoicp::segment_planes_impl(xyz, n, distance_threshold, iterations, seed, max_planes, min_inliers, refit, keep_planes, device, out_xyz, capacity_points,
                                           kept_index, label_n, models, capacity_models, model_size, out);
    });
}
