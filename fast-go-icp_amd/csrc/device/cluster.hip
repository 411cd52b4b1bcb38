// Density clustering (fgoicp_cluster_dbscan; include/fgoicp_amd.h has the definition, DESIGN.md section 17 the pipeline).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
//
//   host        the refusals (they need no device), then the exact search tree over the cloud itself (bvh_build_host)
//   count       cluster_count_kernel (kernels.hip): per point neighbours and core at the caller index, and the number of core points
//   components  parent[i] = i, then rounds of launch_cluster_round (hook, compress) until one hooks nothing; the host reads one word per round
//   labels      flag the roots (core[i] && parent[i] == i), rocPRIM exclusive scan over caller index: the dense number of every root, in
//               ascending order of the lowest core index — the defined order
//   border      cluster_border_kernel: every point's label
//   sizes       integer atomic adds per label, one per wave and label; the same pass counts border and noise points.  The host picks the largest
//   keep        flag[i] = the point's cluster is kept; the stable compaction of one_shot.hpp
// Every per-point array is in CALLER order: the walks' leaf functor sees a candidate as its point, whose w is the caller index, and a
// candidate is wave-uniform, so a gather per candidate is one word per wave whichever order the array has.
// Nothing is summed in floating point; the only atomics are integer min, add and a flag, whose results do not depend on their order.
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

constexpr int kCluBlock = 256;

__global__ __launch_bounds__(kCluBlock) void cluster_init_kernel(uint32_t* __restrict__ parent, uint32_t n) {
    const size_t i = (size_t)blockIdx.x * kCluBlock + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kCluBlock) void cluster_root_flag_kernel(const uint32_t* __restrict__ core, const uint32_t* __restrict__ parent, uint32_t n,
                                                                     uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * kCluBlock + threadIdx.x;
    if (i < n) flag[i] = (core[i] != 0u && parent[i] == (uint32_t)i) ? 1u : 0u;
}

// size[c] += the points labelled c; counters[1] += the border points, counters[2] += the noise points.  A wave adds once per distinct label
// among its 64 points (mostly one): the sums are integers, exact in any order.
__global__ __launch_bounds__(kCluBlock) void cluster_size_kernel(const int32_t* __restrict__ label, const uint32_t* __restrict__ core, uint32_t n,
                                                                unsigned long long* __restrict__ size, unsigned long long* __restrict__ counters) {
    const size_t i = (size_t)blockIdx.x * kCluBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t l = i < n ? label[i] : -2;
    const unsigned long long border = __ballot(l >= 0 && core[i] == 0u), noise = __ballot(l == -1);
    if (lane == 0 && border) atomicAdd(counters + 1, (unsigned long long)__popcll(border));
    if (lane == 0 && noise) atomicAdd(counters + 2, (unsigned long long)__popcll(noise));
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t ll = __shfl(l, lead);
        const unsigned long long same = __ballot(l == ll);
        if (lane == lead) atomicAdd(size + ll, (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

// flag[i] = the point's cluster is kept: the largest one (min_size == 0), or every one of at least min_size points
__global__ __launch_bounds__(kCluBlock) void cluster_keep_kernel(const int32_t* __restrict__ label, const unsigned long long* __restrict__ size, uint32_t n, int32_t largest,
                                                                unsigned long long min_size, uint32_t* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * kCluBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t l = label[i];
    flag[i] = (l >= 0 && (min_size == 0ull ? l == largest : size[l] >= min_size)) ? 1u : 0u;
}

int cluster_dbscan_impl(const float* xyz, size_t n, float eps, int min_points, size_t keep_min_size, int device, float* out_xyz, size_t capacity, uint32_t* kept_index,
                        int32_t* label_n, uint32_t* neighbours_n, uint64_t* cluster_size, size_t capacity_clusters, fgoicp_cluster_info_t* out) {
    const char* const call = "fgoicp_cluster_dbscan";
    auto refuse = [call](const std::string& what) { return fgoicp::refuse(call, what); };
    if (const int rc = refuse_cloud_head(call, xyz, n)) return rc;
    if (!(std::isfinite(eps) && eps > 0.0f)) return refuse("eps must be a positive finite number");
    if (min_points < 1) return refuse("min_points must be at least 1");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_cluster_info_t, rounds) + sizeof(out->rounds), "fgoicp_cluster_info_t")) return rc;
    if (device < 0) return refuse("device ordinal out of range");  // before the device count is asked for
    if (const int rc = refuse_first_non_finite(call, xyz, n)) return rc;
    if (const int rc = select_device(call, device)) return rc;

    const BvhHost tree = bvh_build_host_xyz(xyz, n);

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n;
    const float eps2 = eps * eps;
    size_t scan_bytes = 0;
    ONECHK(call, rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    float *d_xyz, *d_out;
    BvhDevice bvh;
    BvhView view;
    uint32_t *d_nbr, *d_core, *d_parent, *d_flag, *d_row, *d_idx;
    int32_t* d_label;
    unsigned long long *d_size, *d_ctr;  // d_ctr: the core, border and noise points; then the rounds' changed word
    char* tmp;
    Arena plan;
    plan.take(d_xyz, 3 * n); bvh_take(plan, tree, &bvh); plan.take(d_nbr, n); plan.take(d_core, n);
    plan.take(d_parent, n); plan.take(d_flag, n); plan.take(d_row, n); plan.take(d_label, n); plan.take(d_size, n); plan.take(d_out, 3 * n); plan.take(d_idx, n);
    plan.take(d_ctr, 4); plan.take(tmp, scan_bytes);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);
    uint32_t* d_changed = reinterpret_cast<uint32_t*>(d_ctr + 3);

    const dim3 block(kCluBlock), per_point((uint32_t)((n + kCluBlock - 1) / kCluBlock));
    ONECHK(call, hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    ONECHK(call, bvh_upload_async(tree, bvh, d.stream, &view));
    ONECHK(call, hipMemsetAsync(d_ctr, 0, 4 * 8, d.stream));
    hipLaunchKernelGGL(cluster_init_kernel, per_point, block, 0, d.stream, d_parent, n32);
    launch_cluster_count(view, (int)n, eps2, (uint32_t)min_points, d_nbr, d_core, d_ctr, d.stream);
    unsigned long long core_points = 0;
    ONECHK(call, hipMemcpyAsync(&core_points, d_ctr, 8, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    if (core_points > n) {
        set_error("fgoicp_cluster_dbscan: the device returned an inconsistent core count");
        return FGOICP_ERR_HIP;
    }

    // components: rounds until one hooks nothing.  The cap is a safety stop: every round that hooks lowers at least one parent.
    uint32_t rounds = 0;
    while (core_points) {
        uint32_t changed = 0;
        ONECHK(call, hipMemsetAsync(d_changed, 0, 4, d.stream));
        launch_cluster_round(view, (int)n, eps2, d_core, d_parent, d_changed, d.stream);
        ONECHK(call, hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
        ++rounds;
        if (!changed) break;
        if (rounds >= core_points) {
            set_error("fgoicp_cluster_dbscan: the connected-components pass did not settle within " + std::to_string(core_points) + " rounds");
            return FGOICP_ERR_HIP;
        }
    }

    // labels, sizes
    hipLaunchKernelGGL(cluster_root_flag_kernel, per_point, block, 0, d.stream, d_core, d_parent, n32, d_flag);
    uint32_t h[2] = {0u, 0u};  // rows before the last point, the last point's flag
    if (const int rc = scan_flags_async(d, tmp, scan_bytes, d_flag, d_row, n, h)) return rc;
    launch_cluster_border(view, (int)n, eps2, d_core, d_parent, d_row, d_label, d.stream);
    ONECHK(call, hipMemsetAsync(d_size, 0, 8 * n, d.stream));
    hipLaunchKernelGGL(cluster_size_kernel, per_point, block, 0, d.stream, d_label, d_core, n32, d_size, d_ctr);
    unsigned long long ctr[3] = {0, 0, 0};
    ONECHK(call, hipMemcpyAsync(ctr, d_ctr, 3 * 8, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    uint64_t clusters = 0;
    if (const int rc = kept_rows(d, h, n, &clusters)) return rc;
    if (clusters > core_points || (clusters == 0) != (core_points == 0) || ctr[0] != core_points || ctr[0] + ctr[1] + ctr[2] != n) {
        set_error("fgoicp_cluster_dbscan: the device returned inconsistent counts");
        return FGOICP_ERR_HIP;
    }
    std::vector<unsigned long long> sizes((size_t)clusters);
    if (clusters) {
        ONECHK(call, hipMemcpyAsync(sizes.data(), d_size, 8 * (size_t)clusters, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
    }
    int64_t largest = -1;
    uint64_t largest_size = 0;
    for (size_t c = 0; c < sizes.size(); ++c)
        if (sizes[c] > largest_size) { largest = (int64_t)c; largest_size = sizes[c]; }  // strictly: a tie stays with the lowest label

    // keep
    uint64_t kept = 0;
    if (clusters) {
        hipLaunchKernelGGL(cluster_keep_kernel, per_point, block, 0, d.stream, d_label, d_size, n32, (int32_t)largest, (unsigned long long)keep_min_size, d_flag);
        if (const int rc = scan_flags_async(d, tmp, scan_bytes, d_flag, d_row, n, h)) return rc;
        ONECHK(call, hipStreamSynchronize(d.stream));
        ONECHK(call, hipGetLastError());
        if (const int rc = kept_rows(d, h, n, &kept)) return rc;
    }

    fgoicp_cluster_info_t full{};
    full.points = n;
    full.core_points = ctr[0];
    full.border_points = ctr[1];
    full.noise_points = ctr[2];
    full.clusters = clusters;
    full.largest_label = largest;
    full.largest_size = largest_size;
    full.kept = kept;
    full.keep_min_size = keep_min_size;
    full.min_points = min_points;
    full.eps2 = eps2;
    full.rounds = rounds;
    write_info(out, full);
    if ((out_xyz || kept_index) && capacity < kept) {
        set_error("fgoicp_cluster_dbscan: " + std::to_string(kept) + " points kept, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }
    if (cluster_size && capacity_clusters < clusters) {
        set_error("fgoicp_cluster_dbscan: " + std::to_string(clusters) + " clusters, capacity_clusters is " + std::to_string(capacity_clusters));
        return FGOICP_ERR_TOO_LARGE;
    }

    if ((out_xyz || kept_index) && kept)
        if (const int rc = scatter_rows_async(d, d_xyz, d_flag, d_row, n, d_out, d_idx, kept, out_xyz, kept_index)) return rc;
    if (label_n) ONECHK(call, hipMemcpyAsync(label_n, d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (neighbours_n) ONECHK(call, hipMemcpyAsync(neighbours_n, d_nbr, 4 * n, hipMemcpyDeviceToHost, d.stream));
    for (size_t c = 0; cluster_size && c < sizes.size(); ++c) cluster_size[c] = sizes[c];
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_cluster_dbscan(const float* xyz, size_t n, float eps, int min_points, size_t keep_min_size, int device, float* out_xyz, size_t capacity_points,
                                     uint32_t* kept_index, int32_t* label_n, uint32_t* neighbours_n, uint64_t* cluster_size, size_t capacity_clusters,
                                     fgoicp_cluster_info_t* out) {
    return fgoicp::abi_guard("fgoicp_cluster_dbscan", [&] {
        return fgoicp::cluster_dbscan_impl(xyz, n, eps, min_points, keep_min_size, device, out_xyz, capacity_points, kept_index, label_n, neighbours_n, cluster_size,
                                           capacity_clusters, out);
    });
}
