// Density clustering (fgoicp_cluster_dbscan; include/fgoicp_amd.h has the definition, DESIGN.md section 17 the pipeline).
// One call = one stream + one device allocation of its own, both released before it returns; no fgoicp_ctx, no global state, no knobs.
//
//   host        the refusals (they need no device), then the exact search tree over the cloud itself (bvh_build_host)
//   count       cluster_count_kernel (kernels.hip): per point neighbours and core at the caller index, and the number of core points
//   components  parent[i] = i, then rounds of launch_cluster_round (hook, compress) until one hooks nothing; the host reads one word per round
//   labels      flag the roots (core[i] && parent[i] == i), rocPRIM exclusive scan over caller index: the dense number of every root, in
//               ascending order of the lowest core index — the defined order
//   border      cluster_border_kernel: every point's label
//   sizes       integer atomic adds per label, one per wave and label; the same pass counts border and noise points.  The host picks the largest
//   keep        flag[i] = the point's cluster is kept; scan; scatter — stable, the rows are in caller order (as outlier.hip)
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

#include "../../../include/fgoicp_amd.h"
#include "../host/abi_guard.hpp"
#include "bvh.hpp"
#include "kernels.hpp"

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

// row[i] = the exclusive scan of the flags: the number of kept points before i
__global__ __launch_bounds__(kCluBlock) void cluster_scatter_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ row,
                                                                   uint32_t n, float* __restrict__ out_xyz, uint32_t* __restrict__ kept_index) {
    const size_t i = (size_t)blockIdx.x * kCluBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float* p = xyz + 3 * i;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out_xyz + 3 * (size_t)row[i];
    o[0] = x; o[1] = y; o[2] = z;
    kept_index[row[i]] = (uint32_t)i;
}

struct CluDevice {  // what the call owns on the device
    hipStream_t stream = nullptr;
    void* arena = nullptr;
    ~CluDevice() {  // (an early return may leave copies into the caller's arrays in flight)
        if (stream) (void)hipStreamSynchronize(stream);
        if (arena) (void)hipFree(arena);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#define CLUCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            set_error(std::string("fgoicp_cluster_dbscan: " #expr " failed: ") + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;                            \
        }                                                                                                 \
    } while (0)

int cluster_dbscan_impl(const float* xyz, size_t n, float eps, int min_points, size_t keep_min_size, int device, float* out_xyz, size_t capacity, uint32_t* kept_index,
                        int32_t* label_n, uint32_t* neighbours_n, uint64_t* cluster_size, size_t capacity_clusters, fgoicp_cluster_info_t* out) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_cluster_dbscan: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!xyz || n == 0) return refuse("the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
    if (!(std::isfinite(eps) && eps > 0.0f)) return refuse("eps must be a positive finite number");
    if (min_points < 1) return refuse("min_points must be at least 1");
    if (!out || out->struct_size < offsetof(fgoicp_cluster_info_t, rounds) + sizeof(out->rounds) || out->struct_size > 4096)
        return refuse("out must not be null and out->struct_size = sizeof(fgoicp_cluster_info_t)");
    if (device < 0) return refuse("device ordinal out of range");
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse("point " + std::to_string(i) + " has a non-finite coordinate");

    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string("fgoicp_cluster_dbscan: no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                  "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device >= ndev) return refuse("device ordinal out of range");  // (a negative one was refused above, where no count is needed)
    CLUCHK(hipSetDevice(device));

    BvhHost tree;
    {
        std::vector<float4> p4(n);
        for (size_t i = 0; i < n; ++i) p4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
        tree = bvh_build_host(p4.data(), n);
    }

    CluDevice d;
    CLUCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n;
    const float eps2 = eps * eps;
    size_t scan_bytes = 0;
    CLUCHK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    // the arena: every array starts on a 256-byte boundary
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t box_bytes = tree.box.size() * sizeof(float4), pts_bytes = tree.pts.size() * sizeof(float4), slab_bytes = tree.slab.size() * sizeof(float4);
    const size_t at_xyz = take(12 * n), at_box = take(box_bytes), at_pts = take(pts_bytes), at_slab = take(slab_bytes), at_nbr = take(4 * n), at_core = take(4 * n);
    const size_t at_parent = take(4 * n), at_flag = take(4 * n), at_row = take(4 * n), at_label = take(4 * n), at_size = take(8 * n), at_out = take(12 * n), at_idx = take(4 * n);
    const size_t at_ctr = take(4 * 8), at_tmp = take(scan_bytes);  // counters: core, border, noise points; then the rounds' changed word
    CLUCHK(hipMalloc(&d.arena, total));
    char* base = static_cast<char*>(d.arena);
    float* d_xyz = reinterpret_cast<float*>(base + at_xyz);
    BvhView view{reinterpret_cast<const float4*>(base + at_box), reinterpret_cast<const float4*>(base + at_pts),
                 slab_bytes ? reinterpret_cast<const float4*>(base + at_slab) : nullptr, tree.depth, tree.first_leaf};
    uint32_t *d_nbr = reinterpret_cast<uint32_t*>(base + at_nbr), *d_core = reinterpret_cast<uint32_t*>(base + at_core), *d_parent = reinterpret_cast<uint32_t*>(base + at_parent);
    uint32_t *d_flag = reinterpret_cast<uint32_t*>(base + at_flag), *d_row = reinterpret_cast<uint32_t*>(base + at_row), *d_idx = reinterpret_cast<uint32_t*>(base + at_idx);
    int32_t* d_label = reinterpret_cast<int32_t*>(base + at_label);
    unsigned long long *d_size = reinterpret_cast<unsigned long long*>(base + at_size), *d_ctr = reinterpret_cast<unsigned long long*>(base + at_ctr);
    uint32_t* d_changed = reinterpret_cast<uint32_t*>(d_ctr + 3);
    float* d_out = reinterpret_cast<float*>(base + at_out);
    void* tmp = base + at_tmp;

    const dim3 block(kCluBlock), per_point((uint32_t)((n + kCluBlock - 1) / kCluBlock));
    CLUCHK(hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    CLUCHK(hipMemcpyAsync(base + at_box, tree.box.data(), box_bytes, hipMemcpyHostToDevice, d.stream));
    CLUCHK(hipMemcpyAsync(base + at_pts, tree.pts.data(), pts_bytes, hipMemcpyHostToDevice, d.stream));
    if (slab_bytes) CLUCHK(hipMemcpyAsync(base + at_slab, tree.slab.data(), slab_bytes, hipMemcpyHostToDevice, d.stream));
    CLUCHK(hipMemsetAsync(d_ctr, 0, 4 * 8, d.stream));
    hipLaunchKernelGGL(cluster_init_kernel, per_point, block, 0, d.stream, d_parent, n32);
    launch_cluster_count(view, (int)n, eps2, (uint32_t)min_points, d_nbr, d_core, d_ctr, d.stream);
    unsigned long long core_points = 0;
    CLUCHK(hipMemcpyAsync(&core_points, d_ctr, 8, hipMemcpyDeviceToHost, d.stream));
    CLUCHK(hipStreamSynchronize(d.stream));
    CLUCHK(hipGetLastError());
    if (core_points > n) {
        set_error("fgoicp_cluster_dbscan: the device returned an inconsistent core count");
        return FGOICP_ERR_HIP;
    }

    // components: rounds until one hooks nothing.  The cap is a safety stop: every round that hooks lowers at least one parent.
    uint32_t rounds = 0;
    while (core_points) {
        uint32_t changed = 0;
        CLUCHK(hipMemsetAsync(d_changed, 0, 4, d.stream));
        launch_cluster_round(view, (int)n, eps2, d_core, d_parent, d_changed, d.stream);
        CLUCHK(hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, d.stream));
        CLUCHK(hipStreamSynchronize(d.stream));
        CLUCHK(hipGetLastError());
        ++rounds;
        if (!changed) break;
        if (rounds >= core_points) {
            set_error("fgoicp_cluster_dbscan: the connected-components pass did not settle within " + std::to_string(core_points) + " rounds");
            return FGOICP_ERR_HIP;
        }
    }

    // labels, sizes
    hipLaunchKernelGGL(cluster_root_flag_kernel, per_point, block, 0, d.stream, d_core, d_parent, n32, d_flag);
    CLUCHK(rocprim::exclusive_scan(tmp, scan_bytes, d_flag, d_row, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    uint32_t h[2] = {0u, 0u};  // rows before the last point, the last point's flag
    CLUCHK(hipMemcpyAsync(&h[0], d_row + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    CLUCHK(hipMemcpyAsync(&h[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    launch_cluster_border(view, (int)n, eps2, d_core, d_parent, d_row, d_label, d.stream);
    CLUCHK(hipMemsetAsync(d_size, 0, 8 * n, d.stream));
    hipLaunchKernelGGL(cluster_size_kernel, per_point, block, 0, d.stream, d_label, d_core, n32, d_size, d_ctr);
    unsigned long long ctr[3] = {0, 0, 0};
    CLUCHK(hipMemcpyAsync(ctr, d_ctr, 3 * 8, hipMemcpyDeviceToHost, d.stream));
    CLUCHK(hipStreamSynchronize(d.stream));
    CLUCHK(hipGetLastError());
    const uint64_t clusters = (uint64_t)h[0] + h[1];
    if (clusters > core_points || h[1] > 1u || (clusters == 0) != (core_points == 0) || ctr[0] != core_points || ctr[0] + ctr[1] + ctr[2] != n) {
        set_error("fgoicp_cluster_dbscan: the device returned inconsistent counts");
        return FGOICP_ERR_HIP;
    }
    std::vector<unsigned long long> sizes((size_t)clusters);
    if (clusters) {
        CLUCHK(hipMemcpyAsync(sizes.data(), d_size, 8 * (size_t)clusters, hipMemcpyDeviceToHost, d.stream));
        CLUCHK(hipStreamSynchronize(d.stream));
    }
    int64_t largest = -1;
    uint64_t largest_size = 0;
    for (size_t c = 0; c < sizes.size(); ++c)
        if (sizes[c] > largest_size) { largest = (int64_t)c; largest_size = sizes[c]; }  // strictly: a tie stays with the lowest label

    // keep
    uint64_t kept = 0;
    if (clusters) {
        hipLaunchKernelGGL(cluster_keep_kernel, per_point, block, 0, d.stream, d_label, d_size, n32, (int32_t)largest, (unsigned long long)keep_min_size, d_flag);
        CLUCHK(rocprim::exclusive_scan(tmp, scan_bytes, d_flag, d_row, 0u, n, rocprim::plus<uint32_t>(), d.stream));
        CLUCHK(hipMemcpyAsync(&h[0], d_row + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
        CLUCHK(hipMemcpyAsync(&h[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
        CLUCHK(hipStreamSynchronize(d.stream));
        CLUCHK(hipGetLastError());
        kept = (uint64_t)h[0] + h[1];
        if (kept > n || h[1] > 1u) {
            set_error("fgoicp_cluster_dbscan: the device returned an inconsistent row count");
            return FGOICP_ERR_HIP;
        }
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
    full.struct_size = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
    std::memcpy(out, &full, full.struct_size);
    if ((out_xyz || kept_index) && capacity < kept) {
        set_error("fgoicp_cluster_dbscan: " + std::to_string(kept) + " points kept, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }
    if (cluster_size && capacity_clusters < clusters) {
        set_error("fgoicp_cluster_dbscan: " + std::to_string(clusters) + " clusters, capacity_clusters is " + std::to_string(capacity_clusters));
        return FGOICP_ERR_TOO_LARGE;
    }

    if ((out_xyz || kept_index) && kept) {
        hipLaunchKernelGGL(cluster_scatter_kernel, per_point, block, 0, d.stream, d_xyz, d_flag, d_row, n32, d_out, d_idx);
        if (out_xyz) CLUCHK(hipMemcpyAsync(out_xyz, d_out, 12 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
        if (kept_index) CLUCHK(hipMemcpyAsync(kept_index, d_idx, 4 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
    }
    if (label_n) CLUCHK(hipMemcpyAsync(label_n, d_label, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (neighbours_n) CLUCHK(hipMemcpyAsync(neighbours_n, d_nbr, 4 * n, hipMemcpyDeviceToHost, d.stream));
    for (size_t c = 0; cluster_size && c < sizes.size(); ++c) cluster_size[c] = sizes[c];
    CLUCHK(hipStreamSynchronize(d.stream));
    CLUCHK(hipGetLastError());
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
