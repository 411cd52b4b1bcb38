// Plane segmentation by RANSAC (fgoicp_segment_planes; include/fgoicp_amd.h has the definition, DESIGN.md section 18 the launch chain).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
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
//   rows      flag[i] from the label; the stable compaction of one_shot.hpp
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

#include "../host/segment.hpp"
#include "fixed_sum.hpp"
#include "one_shot.hpp"
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

int segment_planes_impl(const float* xyz, size_t n, float distance_threshold, int iterations, uint64_t seed, int max_planes, size_t min_inliers, int refit, int keep_planes,
                        int device, float* out_xyz, size_t capacity, uint32_t* kept_index, int32_t* label_n, fgoicp_segment_model_t* models, size_t capacity_models,
                        size_t model_size, fgoicp_segment_info_t* out) {
    const char* const call = "fgoicp_segment_planes";
    auto refuse = [call](const std::string& what) { return fgoicp::refuse(call, what); };
    if (const int rc = refuse_cloud_head(call, xyz, n)) return rc;
    if (!(std::isfinite(distance_threshold) && distance_threshold > 0.0f)) return refuse("distance_threshold must be a positive finite number");
    if (iterations < 1 || iterations > kSegMaxIterations) return refuse("iterations must lie in [1, 65536]");
    if (max_planes < 1 || max_planes > kSegMaxPlanes) return refuse("max_planes must lie in [1, 16]");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_segment_info_t, distance_threshold) + sizeof(out->distance_threshold), "fgoicp_segment_info_t")) return rc;
    if (models && model_size == 0) return refuse("model_size must be sizeof(fgoicp_segment_model_t), not 0");
    if (device < 0) return refuse("device ordinal out of range");  // before the device count is asked for
    if (const int rc = refuse_first_non_finite(call, xyz, n)) return rc;
    if (const int rc = select_device(call, device)) return rc;

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n, K = (uint32_t)iterations;
    const double T = (double)distance_threshold;
    const bool want_rows = out_xyz || kept_index;
    size_t scan_bytes = 0;
    ONECHK(call, rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    const uint32_t nrows = (uint32_t)((n + kSegBlock - 1) / kSegBlock), tiles = (uint32_t)((n + kSegTile - 1) / kSegTile);
    float *d_xyz, *d_out;
    int32_t* d_label;
    uint32_t *d_flag, *d_row, *d_idx, *d_counts;
    SegPlane* d_planes;
    MomentRow<kSegTerms>* d_rows;
    unsigned long long *d_sums, *d_ctr;
    char* tmp;
    Arena plan;
    plan.take(d_xyz, 3 * n); plan.take(d_label, n); plan.take(d_flag, n); plan.take(d_row, n); plan.take(d_out, 3 * n); plan.take(d_idx, n);
    plan.take(d_planes, K); plan.take(d_counts, K); plan.take(d_rows, nrows); plan.take(d_sums, 1 + kSegTerms); plan.take(d_ctr, 1); plan.take(tmp, scan_bytes);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);

    const dim3 block(kSegBlock), per_point(nrows);
    ONECHK(call, hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
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
        ONECHK(call, hipMemcpyAsync(d_planes, table.data(), sizeof(SegPlane) * (size_t)K, hipMemcpyHostToDevice, d.stream));
        ONECHK(call, hipMemsetAsync(d_counts, 0, 4 * (size_t)K, d.stream));
        hipLaunchKernelGGL(segment_score_kernel, dim3(tiles, segment_score_grid_y(tiles, K)), block, 0, d.stream, d_xyz, d_label, n32, d_planes, K, T, d_counts);
        ONECHK(call, hipMemcpyAsync(counts.data(), d_counts, 4 * (size_t)K, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
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
            ONECHK(call, hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, d.stream));
            ONECHK(call, hipStreamSynchronize(d.stream));
            ONECHK(call, hipGetLastError());
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
        ONECHK(call, hipMemsetAsync(d_ctr, 0, 8, d.stream));
        hipLaunchKernelGGL(segment_label_kernel, per_point, block, 0, d.stream, d_xyz, d_label, n32, SegPlane{mod.plane[0], mod.plane[1], mod.plane[2], mod.plane[3]}, T,
                           (int32_t)j, d_ctr);
        ONECHK(call, hipMemcpyAsync(&labelled, d_ctr, 8, hipMemcpyDeviceToHost, d.stream));
        if (j + 1 < max_planes) ONECHK(call, hipMemcpyAsync(label.data(), d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
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
    write_info(out, full);
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
        if (const int rc = scan_flags_async(d, tmp, scan_bytes, d_flag, d_row, n, h)) return rc;
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
        uint64_t rows = 0;
        if (const int rc = kept_rows(d, h, n, &rows)) return rc;
        if (rows != kept) {
            set_error("fgoicp_segment_planes: the device returned an inconsistent row count");
            return FGOICP_ERR_HIP;
        }
        if (const int rc = scatter_rows_async(d, d_xyz, d_flag, d_row, n, d_out, d_idx, kept, out_xyz, kept_index)) return rc;
    }
    if (label_n) ONECHK(call, hipMemcpyAsync(label_n, d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
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
