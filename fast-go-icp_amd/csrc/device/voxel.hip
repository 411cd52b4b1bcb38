// Voxel-grid downsampling (fgoicp_voxel_downsample; include/fgoicp_amd.h has the definition, DESIGN.md section 13 the pipeline).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
//
//   host    finite check, origin (given, or the per-axis minimum), every cell in [0, 2^21) — the refusals need no device
//   key     one thread per point: c = floor(((double)p - o) / v) per axis in IEEE fp64; sort key and caller index
//   sort    rocPRIM radix sort of (key, index), stable: indices start ascending, so every cell's members stay in caller order
//   heads   a sorted position is a head when its key differs from its predecessor's; the inclusive scan of the heads numbers the rows
//   rows    voxel_of_point[index] = row; the head positions are the rows' starts; counts and the tile counts of the long rows
//   sums    by run length L alone: L <= 64 one thread, L <= 4096 one wave, longer: tiles of 4096 members, one wave each, folded in tile order
//
// The SORT key packs the three cell numbers into as few bits as the cloud's extent needs, (cz << (bx + by)) | (cy << bx) | cx with
// bx, by, bz = the bit widths of the largest cell number per axis: it orders the points exactly as the key of the definition,
// (cz << 42) | (cy << 21) | cx, does (z-major, then y, then x) and the radix sort runs over bx + by + bz bits instead of 63.
//
// Every sum is a function of the input array alone: a thread or a lane adds its members in ascending sorted position, lanes are joined
// by the xor butterfly (both operands of every addition are the same pair whichever lane adds them: wave_xor_sum in fixed_sum.hpp),
// tiles are added first to last.  No floating-point atomics; the one atomic is an integer maximum.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "fixed_sum.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

constexpr int kVoxBlock = 256;
constexpr uint32_t kVoxThreadMax = 64;  // rows of up to this many points: one thread walks the run
constexpr uint32_t kVoxTile = 4096;     // rows of up to this many points: one wave; longer rows: tiles of this many points, one wave each
constexpr double kVoxCells = 2097152.0; // 2^21 cells per axis

struct VoxGrid {
    double o[3], v;
    int shift_y, shift_z;
};
struct VoxPartial {  // one tile of a long row
    double x, y, z;
    uint32_t row, tile;
};

__global__ __launch_bounds__(kVoxBlock) void voxel_key_kernel(const float* __restrict__ xyz, uint32_t n, VoxGrid g, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ idx) {
    const size_t i = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (i >= n) return;
    const float* p = xyz + 3 * i;
    const uint64_t cx = (uint64_t)floor(((double)p[0] - g.o[0]) / g.v);
    const uint64_t cy = (uint64_t)floor(((double)p[1] - g.o[1]) / g.v);
    const uint64_t cz = (uint64_t)floor(((double)p[2] - g.o[2]) / g.v);
    keys[i] = (cz << g.shift_z) | (cy << g.shift_y) | cx;
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kVoxBlock) void voxel_heads_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// row_incl = inclusive scan of head: the row of sorted position i is row_incl[i] - 1, and row_incl[n - 1] is the number of rows
__global__ __launch_bounds__(kVoxBlock) void voxel_rows_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ row_incl, uint32_t n, uint32_t* __restrict__ voxel_of_point,
                                                              uint32_t* __restrict__ start) {
    const size_t i = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = row_incl[i] - 1u;
    voxel_of_point[idx[i]] = row;
    if (head[i]) start[row] = (uint32_t)i;
    if (i == n - 1) start[row + 1u] = n;
}

// one thread per possible row (n of them; those at or beyond the number of rows write zeros for the scan that follows)
__global__ __launch_bounds__(kVoxBlock) void voxel_counts_kernel(const uint32_t* __restrict__ start, const uint32_t* __restrict__ row_incl, uint32_t n,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ tiles, uint32_t* __restrict__ max_count) {
    const size_t r = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    const uint32_t voxels = row_incl[n - 1];
    uint32_t len = 0u;
    if (r < voxels) len = start[r + 1] - start[r];
    if (r < n) {
        counts[r] = len;
        tiles[r] = len > kVoxTile ? (len + kVoxTile - 1u) / kVoxTile : 0u;
    }
    uint32_t mx = len;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(max_count, mx);
}

__device__ __forceinline__ void vox_store_centroid(float* __restrict__ out, uint32_t row, double x, double y, double z, uint32_t len) {
    const double c = (double)len;
    out[3 * (size_t)row] = (float)(x / c);
    out[3 * (size_t)row + 1] = (float)(y / c);
    out[3 * (size_t)row + 2] = (float)(z / c);
}

// rows of up to kVoxThreadMax points: one thread per row adds the members in sorted (= caller) order
__global__ __launch_bounds__(kVoxBlock) void voxel_centroid_thread_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ idx,
                                                                         const uint32_t* __restrict__ start, uint32_t voxels, float* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (r >= voxels) return;
    const uint32_t s = start[r], len = start[r + 1] - s;
    if (len > kVoxThreadMax) return;
    double x = 0.0, y = 0.0, z = 0.0;
    for (uint32_t j = 0; j < len; ++j) {
        const float* p = xyz + 3 * (size_t)idx[s + j];
        x += (double)p[0]; y += (double)p[1]; z += (double)p[2];
    }
    vox_store_centroid(out, (uint32_t)r, x, y, z, len);
}

// lane l adds members first + l, first + l + 64, ... of [first, last) in that order, then the butterfly
__device__ __forceinline__ void vox_wave_run(const float* __restrict__ xyz, const uint32_t* __restrict__ idx, uint32_t first, uint32_t last, int lane, double& x,
                                             double& y, double& z) {
    x = 0.0; y = 0.0; z = 0.0;
    for (uint32_t j = first + (uint32_t)lane; j < last; j += 64u) {
        const float* p = xyz + 3 * (size_t)idx[j];
        x += (double)p[0]; y += (double)p[1]; z += (double)p[2];
    }
    x = wave_xor_sum(x); y = wave_xor_sum(y); z = wave_xor_sum(z);
}

// rows of kVoxThreadMax + 1 .. kVoxTile points: one wave per row (waves of other rows leave at once)
__global__ __launch_bounds__(kVoxBlock) void voxel_centroid_wave_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ idx,
                                                                       const uint32_t* __restrict__ start, uint32_t voxels, float* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * (kVoxBlock / 64) + (threadIdx.x >> 6);
    if (r >= voxels) return;
    const uint32_t s = start[r], len = start[r + 1] - s;
    if (len <= kVoxThreadMax || len > kVoxTile) return;
    const int lane = threadIdx.x & 63;
    double x, y, z;
    vox_wave_run(xyz, idx, s, s + len, lane, x, y, z);
    if (lane == 0) vox_store_centroid(out, (uint32_t)r, x, y, z, len);
}

// longer rows: tile t of the launch is tile t - (tile_incl[row] - tiles of row) of the first row whose inclusive tile count exceeds t
__global__ __launch_bounds__(kVoxBlock) void voxel_centroid_tile_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ idx,
                                                                       const uint32_t* __restrict__ start, const uint32_t* __restrict__ tile_incl, uint32_t voxels,
                                                                       uint32_t total_tiles, VoxPartial* __restrict__ partials) {
    const size_t t = (size_t)blockIdx.x * (kVoxBlock / 64) + (threadIdx.x >> 6);
    if (t >= total_tiles) return;
    uint32_t lo = 0u, hi = voxels - 1u;  // tile_incl[voxels - 1] = total_tiles > t
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tile_incl[mid] > (uint32_t)t) hi = mid; else lo = mid + 1u;
    }
    const uint32_t s = start[lo], len = start[lo + 1] - s, row_tiles = (len + kVoxTile - 1u) / kVoxTile;
    const uint32_t k = (uint32_t)t - (tile_incl[lo] - row_tiles);
    const uint32_t first = s + k * kVoxTile, last = min(s + len, first + kVoxTile);
    const int lane = threadIdx.x & 63;
    double x, y, z;
    vox_wave_run(xyz, idx, first, last, lane, x, y, z);
    if (lane == 0) partials[t] = VoxPartial{x, y, z, lo, k};
}
// the thread of a row's first tile adds the row's partials in tile order
__global__ __launch_bounds__(kVoxBlock) void voxel_centroid_fold_kernel(const VoxPartial* __restrict__ partials, const uint32_t* __restrict__ start, uint32_t total_tiles,
                                                                       float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kVoxBlock + threadIdx.x;
    if (t >= total_tiles || partials[t].tile != 0u) return;
    const uint32_t row = partials[t].row, len = start[row + 1] - start[row], row_tiles = (len + kVoxTile - 1u) / kVoxTile;
    double x = 0.0, y = 0.0, z = 0.0;
    for (uint32_t k = 0; k < row_tiles; ++k) {
        x += partials[t + k].x; y += partials[t + k].y; z += partials[t + k].z;
    }
    vox_store_centroid(out, row, x, y, z, len);
}

int bit_width(uint32_t x) {
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

int voxel_downsample_impl(const float* xyz, size_t n, float voxel_size, const float* origin3, int device, float* out_xyz, size_t capacity, uint32_t* voxel_of_point,
                          uint32_t* count_per_voxel, fgoicp_voxel_info_t* out) {
    const char* const call = "fgoicp_voxel_downsample";
    auto refuse = [call](const std::string& what) { return fgoicp::refuse(call, what); };
    if (const int rc = refuse_cloud_head(call, xyz, n)) return rc;
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return refuse("voxel_size must be a positive finite number");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_voxel_info_t, max_points_per_voxel), "fgoicp_voxel_info_t")) return rc;
    float o[3] = {xyz[0], xyz[1], xyz[2]};
    for (size_t i = 0; i < n; ++i)  // the finite check and the per-axis minimum in one pass
        for (int a = 0; a < 3; ++a) {
            const float c = xyz[3 * i + a];
            if (!std::isfinite(c)) return refuse_non_finite(call, i);
            if (c < o[a]) o[a] = c;
        }
    if (origin3)
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(origin3[a])) return refuse("the origin is not finite");
            o[a] = origin3[a];
        }
    VoxGrid g{};
    g.v = (double)voxel_size;
    uint32_t cmax[3] = {0u, 0u, 0u};
    for (int a = 0; a < 3; ++a) g.o[a] = (double)o[a];
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double c = std::floor(((double)xyz[3 * i + a] - g.o[a]) / g.v);
            if (!(c >= 0.0 && c < kVoxCells))
                return refuse("point " + std::to_string(i) + " falls into a cell outside [0, 2^21): the voxel size is too small for the extent of the cloud (or the point lies below the given origin)");
            if ((uint32_t)c > cmax[a]) cmax[a] = (uint32_t)c;
        }
    g.shift_y = bit_width(cmax[0]);
    g.shift_z = g.shift_y + bit_width(cmax[1]);
    const unsigned end_bit = (unsigned)std::max(1, g.shift_z + bit_width(cmax[2]));

    if (const int rc = select_device(call, device)) return rc;

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n;
    const size_t max_tiles = n / (kVoxTile / 2) + 1;  // a row of L > kVoxTile points has ceil(L / kVoxTile) < 2 L / kVoxTile tiles
    size_t sort_bytes = 0, scan_bytes = 0;
    ONECHK(call, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, end_bit, d.stream));
    ONECHK(call, rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, n, rocprim::plus<uint32_t>(), d.stream));
    float *d_xyz, *d_out;
    uint64_t *keys_a, *keys_b;
    uint32_t *idx_a, *idx_b, *start, *vop, *counts, *tile_incl, *d_max;
    VoxPartial* partials;
    char* tmp;
    Arena plan;
    plan.take(d_xyz, 3 * n); plan.take(keys_a, n); plan.take(keys_b, n); plan.take(idx_a, n); plan.take(idx_b, n);
    plan.take(start, n + 1); plan.take(vop, n); plan.take(counts, n); plan.take(tile_incl, n); plan.take(d_out, 3 * n);
    plan.take(partials, max_tiles); plan.take(d_max, 1); plan.take(tmp, std::max(sort_bytes, scan_bytes));
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);
    // After the sort the first key buffer is free: its halves hold the head flags and their scan; the first index buffer then holds the
    // tile counts.
    uint32_t *head = reinterpret_cast<uint32_t*>(keys_a), *row_incl = head + n, *tiles = idx_a;

    const dim3 block(kVoxBlock), per_point((unsigned)((n + kVoxBlock - 1) / kVoxBlock));
    ONECHK(call, hipMemcpyAsync(d_xyz, xyz, 12 * n, hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemsetAsync(d_max, 0, 4, d.stream));
    hipLaunchKernelGGL(voxel_key_kernel, per_point, block, 0, d.stream, d_xyz, n32, g, keys_a, idx_a);
    ONECHK(call, rocprim::radix_sort_pairs(tmp, sort_bytes, keys_a, keys_b, idx_a, idx_b, n, 0u, end_bit, d.stream));
    hipLaunchKernelGGL(voxel_heads_kernel, per_point, block, 0, d.stream, keys_b, n32, head);
    ONECHK(call, rocprim::inclusive_scan(tmp, scan_bytes, head, row_incl, n, rocprim::plus<uint32_t>(), d.stream));
    hipLaunchKernelGGL(voxel_rows_kernel, per_point, block, 0, d.stream, idx_b, head, row_incl, n32, vop, start);
    hipLaunchKernelGGL(voxel_counts_kernel, per_point, block, 0, d.stream, start, row_incl, n32, counts, tiles, d_max);
    ONECHK(call, rocprim::inclusive_scan(tmp, scan_bytes, tiles, tile_incl, n, rocprim::plus<uint32_t>(), d.stream));
    uint32_t h[3] = {0u, 0u, 0u};  // rows, the longest row, tiles of the rows beyond kVoxTile
    ONECHK(call, hipMemcpyAsync(&h[0], row_incl + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipMemcpyAsync(&h[1], d_max, 4, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipMemcpyAsync(&h[2], tile_incl + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    const uint32_t voxels = h[0], longest = h[1], total_tiles = h[2];
    if (voxels == 0 || voxels > n32 || longest == 0 || total_tiles > max_tiles) {
        set_error("fgoicp_voxel_downsample: the device returned an inconsistent row count");
        return FGOICP_ERR_HIP;
    }

    fgoicp_voxel_info_t full{};
    full.points = n;
    full.voxels = voxels;
    full.max_points_per_voxel = longest;
    for (int a = 0; a < 3; ++a) full.origin[a] = o[a];
    full.voxel_size = voxel_size;
    write_info(out, full);
    if ((out_xyz || count_per_voxel) && capacity < voxels) {
        set_error("fgoicp_voxel_downsample: " + std::to_string(voxels) + " occupied voxels, capacity_points is " + std::to_string(capacity));
        return FGOICP_ERR_TOO_LARGE;
    }

    if (out_xyz) {
        const unsigned per_row = (voxels + kVoxBlock - 1) / kVoxBlock, per_wave = (voxels + kVoxBlock / 64 - 1) / (kVoxBlock / 64);
        hipLaunchKernelGGL(voxel_centroid_thread_kernel, dim3(per_row), block, 0, d.stream, d_xyz, idx_b, start, voxels, d_out);
        if (longest > kVoxThreadMax) hipLaunchKernelGGL(voxel_centroid_wave_kernel, dim3(per_wave), block, 0, d.stream, d_xyz, idx_b, start, voxels, d_out);
        if (total_tiles) {
            hipLaunchKernelGGL(voxel_centroid_tile_kernel, dim3((total_tiles + kVoxBlock / 64 - 1) / (kVoxBlock / 64)), block, 0, d.stream, d_xyz, idx_b, start, tile_incl,
                               voxels, total_tiles, partials);
            hipLaunchKernelGGL(voxel_centroid_fold_kernel, dim3((total_tiles + kVoxBlock - 1) / kVoxBlock), block, 0, d.stream, partials, start, total_tiles, d_out);
        }
        ONECHK(call, hipMemcpyAsync(out_xyz, d_out, 12 * (size_t)voxels, hipMemcpyDeviceToHost, d.stream));
    }
    if (voxel_of_point) ONECHK(call, hipMemcpyAsync(voxel_of_point, vop, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (count_per_voxel) ONECHK(call, hipMemcpyAsync(count_per_voxel, counts, 4 * (size_t)voxels, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_voxel_downsample(const float* xyz, size_t n, float voxel_size, const float* origin3_or_NULL, int device, float* out_xyz, size_t capacity_points,
                                       uint32_t* voxel_of_point_n, uint32_t* count_per_voxel, fgoicp_voxel_info_t* out) {
    return fgoicp::abi_guard("fgoicp_voxel_downsample", [&] {
        return fgoicp::voxel_downsample_impl(xyz, n, voxel_size, origin3_or_NULL, device, out_xyz, capacity_points, voxel_of_point_n, count_per_voxel, out);
    });
}
