// Farthest-point sampling (fgoicp_farthest_point_sample; include/fgoicp_amd.h has the definition, DESIGN.md section 16 the launch chain).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
//
//   host      the refusals (they need no device) and, in the same pass, the 16-byte records {x, y, z, D = +inf}
//   step t    fps_step_kernel, m launches queued back to back on the call's stream, nothing between them but the kernel boundary:
//               every block reduces the previous step's per-block keys to the winner c_t (t = 0: the start index),
//               block 0 records sample_index[t], pick_dist2[t] and the row of out_xyz,
//               every block loads p_c once, lowers D over its slice of the points and leaves its own largest key in the other half of
//               the double-buffered key array
//   finish    fps_finish_kernel: the last keys -> next_index and cover_dist2; D -> min_dist2 with the picked points' marker as +0.0
//
// The key of point i is one signed 64-bit integer: the bits of D in the high word, 0xFFFFFFFF - i in the low one.  D is a non-negative
// float or +inf, whose bits order as integers; a picked point holds D = -1 (the sign bit makes its key negative: below every other);
// the low word hands a tie to the lowest caller index.  Nothing is summed, so the outputs are a function of the input alone whatever
// the grid.  No grid barrier, no spin-wait, no cooperative launch, no atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "dist_sq.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

constexpr int kFpsBlock = 256;
constexpr uint32_t kFpsMaxBlocks = 1024;  // at most this many keys per step: their reduction stays one pass of 4 loads per thread
constexpr float kFpsPicked = -1.0f;       // D of a picked point

__device__ __forceinline__ long long fps_key(float d, uint32_t i) {
    return (long long)(((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xFFFFFFFFu - i));
}

// the largest key of the block, in every thread; s: one slot per wave (a second call needs another array)
__device__ __forceinline__ long long block_max_key(long long v, long long* s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)((unsigned long long)v >> 32), off, 64);
        const long long o = (long long)(((unsigned long long)hi << 32) | lo);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = s[0];
#pragma unroll
    for (int w = 1; w < kFpsBlock / 64; ++w) r = s[w] > r ? s[w] : r;
    return r;
}

__device__ __forceinline__ long long fps_reduce_keys(const long long* __restrict__ keys, uint32_t nkeys, long long* s) {
    long long k = LLONG_MIN;
    for (uint32_t b = threadIdx.x; b < nkeys; b += kFpsBlock) {
        const long long o = keys[b];
        k = o > k ? o : k;
    }
    return block_max_key(k, s);
}

// Step t.  prev: the nblocks keys step t - 1 left (not read when t == 0); part: where this step leaves its own.  The block that holds
// c stores the marker into rec[c].w while the others load rec[c]: a 4-byte store beside the 12 bytes they use.
template <bool OWNER>
__global__ __launch_bounds__(kFpsBlock) void fps_step_kernel(float4* __restrict__ rec, uint32_t n, uint32_t t, uint32_t start, const long long* __restrict__ prev,
                                                            long long* __restrict__ part, uint32_t* __restrict__ owner, float* __restrict__ out_xyz,
                                                            uint32_t* __restrict__ sample_index, float* __restrict__ pick_dist2) {
    __shared__ long long s_win[kFpsBlock / 64], s_max[kFpsBlock / 64];
    uint32_t c = start;
    float dc = INFINITY;
    if (t != 0u) {
        const long long k = fps_reduce_keys(prev, gridDim.x, s_win);
        c = 0xFFFFFFFFu - (uint32_t)(unsigned long long)k;
        dc = __uint_as_float((uint32_t)((unsigned long long)k >> 32));
    }
    if (c >= n) return;  // (every key carries the index of a point; the whole block takes the same way)
    const float4 pc = rec[c];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sample_index[t] = c;
        pick_dist2[t] = dc;
        float* o = out_xyz + 3 * (size_t)t;
        o[0] = pc.x; o[1] = pc.y; o[2] = pc.z;
    }
    long long best = LLONG_MIN;
    const uint32_t stride = gridDim.x * kFpsBlock;
    for (uint32_t i = blockIdx.x * kFpsBlock + threadIdx.x; i < n; i += stride) {  // n < 2^31 and stride <= 2^18: no wrap
        const float4 r = rec[i];
        float D = r.w;
        if (!(D < 0.0f)) {
            const float d = dist_sq(r.x, r.y, r.z, pc.x, pc.y, pc.z);
            const bool lower = d < D;
            if (lower) {
                D = d;
                if (OWNER) owner[i] = t;
            }
            if (i == c) D = kFpsPicked;
            if (lower || i == c) rec[i].w = D;
        }
        const long long k = fps_key(D, i);
        best = k > best ? k : best;
    }
    best = block_max_key(best, s_max);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

// min_dist2 (optional; then the grid covers the n points): the final D, +0.0 for a sample.  Block 0: info2 = {next_index, bits of cover_dist2}
// from the nkeys keys of the last step; all keys negative = every point is picked: {n, +0.0}.
__global__ __launch_bounds__(kFpsBlock) void fps_finish_kernel(const float4* __restrict__ rec, uint32_t n, const long long* __restrict__ last, uint32_t nkeys,
                                                              float* __restrict__ min_dist2, uint32_t* __restrict__ info2) {
    __shared__ long long s_win[kFpsBlock / 64];
    const size_t i = (size_t)blockIdx.x * kFpsBlock + threadIdx.x;
    if (min_dist2 && i < n) {
        const float D = rec[i].w;
        min_dist2[i] = D < 0.0f ? 0.0f : D;
    }
    if (blockIdx.x != 0) return;
    const long long k = fps_reduce_keys(last, nkeys, s_win);
    if (threadIdx.x == 0) {
        info2[0] = k < 0 ? n : 0xFFFFFFFFu - (uint32_t)(unsigned long long)k;
        info2[1] = k < 0 ? 0u : (uint32_t)((unsigned long long)k >> 32);
    }
}

int farthest_point_sample_impl(const float* xyz, size_t n, size_t m, size_t start_index, int device, float* out_xyz, uint32_t* sample_index, float* pick_dist2,
                               float* min_dist2_n, uint32_t* owner_n, fgoicp_fps_info_t* out) {
    const char* const call = "fgoicp_farthest_point_sample";
    if (const int rc = refuse_cloud_head(call, xyz, n)) return rc;
    if (m == 0 || m > n) return refuse(call, "the sample count must lie in [1, the number of points]");
    if (start_index >= n) return refuse(call, "start_index must be below the number of points");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_fps_info_t, cover_dist2), "fgoicp_fps_info_t")) return rc;
    std::vector<float4> rec(n);
    for (size_t i = 0; i < n; ++i) {  // the finite check and the records in one pass
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse_non_finite(call, i);
        rec[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], INFINITY);
    }
    if (const int rc = select_device(call, device)) return rc;

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n, m32 = (uint32_t)m;
    const uint32_t per_point = (uint32_t)((n + kFpsBlock - 1) / kFpsBlock);
    const uint32_t nblocks = per_point < kFpsMaxBlocks ? per_point : kFpsMaxBlocks;  // above 1024 x 256 points a block loops over its slice
    float4* d_rec;
    long long* d_keys;
    float *d_out, *d_pick, *d_min;  // d_min, d_owner: nullptr unless asked for
    uint32_t *d_idx, *d_owner, *d_info;
    Arena plan;
    plan.take(d_rec, n); plan.take(d_keys, 2 * (size_t)kFpsMaxBlocks); plan.take(d_out, 3 * m); plan.take(d_idx, m); plan.take(d_pick, m);
    plan.take(d_min, min_dist2_n ? n : 0); plan.take(d_owner, owner_n ? n : 0); plan.take(d_info, 2);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);

    ONECHK(call, hipMemcpyAsync(d_rec, rec.data(), 16 * n, hipMemcpyHostToDevice, d.stream));
    if (d_owner) ONECHK(call, hipMemsetAsync(d_owner, 0, 4 * n, d.stream));  // (a point at an infinite fp32 distance from every sample is never lowered)
    const dim3 block(kFpsBlock), grid(nblocks);
    for (uint32_t t = 0; t < m32; ++t) {  // the chain: step t reads the keys of step t - 1 and leaves its own in the other half
        const long long* prev = d_keys + (size_t)((t + 1u) & 1u) * kFpsMaxBlocks;
        long long* part = d_keys + (size_t)(t & 1u) * kFpsMaxBlocks;
        if (d_owner)
            hipLaunchKernelGGL(fps_step_kernel<true>, grid, block, 0, d.stream, d_rec, n32, t, (uint32_t)start_index, prev, part, d_owner, d_out, d_idx, d_pick);
        else
            hipLaunchKernelGGL(fps_step_kernel<false>, grid, block, 0, d.stream, d_rec, n32, t, (uint32_t)start_index, prev, part, d_owner, d_out, d_idx, d_pick);
    }
    hipLaunchKernelGGL(fps_finish_kernel, dim3(d_min ? per_point : 1u), block, 0, d.stream, d_rec, n32, d_keys + (size_t)((m32 - 1u) & 1u) * kFpsMaxBlocks, nblocks, d_min,
                       d_info);
    uint32_t h_info[2] = {0u, 0u};
    ONECHK(call, hipMemcpyAsync(h_info, d_info, 8, hipMemcpyDeviceToHost, d.stream));
    if (out_xyz) ONECHK(call, hipMemcpyAsync(out_xyz, d_out, 12 * m, hipMemcpyDeviceToHost, d.stream));
    if (sample_index) ONECHK(call, hipMemcpyAsync(sample_index, d_idx, 4 * m, hipMemcpyDeviceToHost, d.stream));
    if (pick_dist2) ONECHK(call, hipMemcpyAsync(pick_dist2, d_pick, 4 * m, hipMemcpyDeviceToHost, d.stream));
    if (min_dist2_n) ONECHK(call, hipMemcpyAsync(min_dist2_n, d_min, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (owner_n) ONECHK(call, hipMemcpyAsync(owner_n, d_owner, 4 * n, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    if (h_info[0] > n32 || (h_info[0] == n32) != (m == n)) {
        set_error("fgoicp_farthest_point_sample: the device returned an inconsistent next index");
        return FGOICP_ERR_HIP;
    }

    fgoicp_fps_info_t full{};
    full.points = n;
    full.samples = m;
    full.start_index = start_index;
    full.next_index = h_info[0];
    std::memcpy(&full.cover_dist2, &h_info[1], 4);
    write_info(out, full);
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_farthest_point_sample(const float* xyz, size_t n, size_t m, size_t start_index, int device, float* out_xyz_m3, uint32_t* sample_index_m,
                                            float* pick_dist2_m, float* min_dist2_n, uint32_t* owner_n, fgoicp_fps_info_t* out) {
    return fgoicp::abi_guard("fgoicp_farthest_point_sample", [&] {
        return fgoicp::farthest_point_sample_impl(xyz, n, m, start_index, device, out_xyz_m3, sample_index_m, pick_dist2_m, min_dist2_n, owner_n, out);
    });
}
