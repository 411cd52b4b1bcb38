// Farthest-point sampling (fgoicp_farthest_point_sample; include/fgoicp_amd.h has the definition, DESIGN.md section 16 the launch chain).
// One call = one stream + one device allocation of its own, both released before it returns; no fgoicp_ctx, no global state, no knobs.
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

#include "../../../include/fgoicp_amd.h"
#include "../host/abi_guard.hpp"
#include "dist_sq.hpp"

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

struct FpsDevice {  // what the call owns on the device
    hipStream_t stream = nullptr;
    void* arena = nullptr;
    ~FpsDevice() {  // (an early return may leave copies into the caller's arrays in flight)
        if (stream) (void)hipStreamSynchronize(stream);
        if (arena) (void)hipFree(arena);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

#define FPSCHK(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            set_error(std::string("fgoicp_farthest_point_sample: " #expr " failed: ") + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;                                   \
        }                                                                                                        \
    } while (0)

int farthest_point_sample_impl(const float* xyz, size_t n, size_t m, size_t start_index, int device, float* out_xyz, uint32_t* sample_index, float* pick_dist2,
                               float* min_dist2_n, uint32_t* owner_n, fgoicp_fps_info_t* out) {
    auto refuse = [](const std::string& what) { set_error("fgoicp_farthest_point_sample: " + what); return (int)FGOICP_ERR_INVALID_ARG; };
    if (!xyz || n == 0) return refuse("the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse("more than 2^31 - 1 points");
    if (m == 0 || m > n) return refuse("the sample count must lie in [1, the number of points]");
    if (start_index >= n) return refuse("start_index must be below the number of points");
    if (!out || out->struct_size < offsetof(fgoicp_fps_info_t, cover_dist2) || out->struct_size > 4096)
        return refuse("out must not be null and out->struct_size = sizeof(fgoicp_fps_info_t)");
    std::vector<float4> rec(n);
    for (size_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse("point " + std::to_string(i) + " has a non-finite coordinate");
        rec[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], INFINITY);
    }

    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string("fgoicp_farthest_point_sample: no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                  "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return refuse("device ordinal out of range");
    FPSCHK(hipSetDevice(device));

    FpsDevice d;
    FPSCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    const uint32_t n32 = (uint32_t)n, m32 = (uint32_t)m;
    const uint32_t per_point = (uint32_t)((n + kFpsBlock - 1) / kFpsBlock);
    const uint32_t nblocks = per_point < kFpsMaxBlocks ? per_point : kFpsMaxBlocks;  // above 1024 x 256 points a block loops over its slice
    // the arena: every array starts on a 256-byte boundary
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t at_rec = take(16 * n), at_keys = take(2 * 8 * (size_t)kFpsMaxBlocks), at_out = take(12 * m), at_idx = take(4 * m), at_pick = take(4 * m);
    const size_t at_min = take(min_dist2_n ? 4 * n : 0), at_owner = take(owner_n ? 4 * n : 0), at_info = take(8);
    FPSCHK(hipMalloc(&d.arena, total));
    char* base = static_cast<char*>(d.arena);
    float4* d_rec = reinterpret_cast<float4*>(base + at_rec);
    long long* d_keys = reinterpret_cast<long long*>(base + at_keys);
    float *d_out = reinterpret_cast<float*>(base + at_out), *d_pick = reinterpret_cast<float*>(base + at_pick);
    float* d_min = min_dist2_n ? reinterpret_cast<float*>(base + at_min) : nullptr;
    uint32_t *d_idx = reinterpret_cast<uint32_t*>(base + at_idx), *d_info = reinterpret_cast<uint32_t*>(base + at_info);
    uint32_t* d_owner = owner_n ? reinterpret_cast<uint32_t*>(base + at_owner) : nullptr;

    FPSCHK(hipMemcpyAsync(d_rec, rec.data(), 16 * n, hipMemcpyHostToDevice, d.stream));
    if (d_owner) FPSCHK(hipMemsetAsync(d_owner, 0, 4 * n, d.stream));  // (a point at an infinite fp32 distance from every sample is never lowered)
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
    FPSCHK(hipMemcpyAsync(h_info, d_info, 8, hipMemcpyDeviceToHost, d.stream));
    if (out_xyz) FPSCHK(hipMemcpyAsync(out_xyz, d_out, 12 * m, hipMemcpyDeviceToHost, d.stream));
    if (sample_index) FPSCHK(hipMemcpyAsync(sample_index, d_idx, 4 * m, hipMemcpyDeviceToHost, d.stream));
    if (pick_dist2) FPSCHK(hipMemcpyAsync(pick_dist2, d_pick, 4 * m, hipMemcpyDeviceToHost, d.stream));
    if (min_dist2_n) FPSCHK(hipMemcpyAsync(min_dist2_n, d_min, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (owner_n) FPSCHK(hipMemcpyAsync(owner_n, d_owner, 4 * n, hipMemcpyDeviceToHost, d.stream));
    FPSCHK(hipStreamSynchronize(d.stream));
    FPSCHK(hipGetLastError());
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
    full.struct_size = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
    std::memcpy(out, &full, full.struct_size);
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
