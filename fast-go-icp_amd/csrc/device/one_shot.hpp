// The frame of a one-shot call (voxel.hip, outlier.hip, fps.hip, cluster.hip, segment.hip, mesh.hip, mesh_distance.hip; DESIGN.md section 13, "The one-shot pattern").
// One call = one stream + one device allocation of its own, both released before it returns; no fgoicp_ctx, no global state, no knobs.
//   OneShot, ONECHK      what the call owns on the device; a failed HIP call ends it
//   refuse_*, select_device    the refusals every call shares (they need no device), then the device
//   write_info                 an extensible info struct back to the caller
//   Arena (arena.hpp)          every device array of the call in one allocation
//   scan_flags_async, kept_rows, scatter_rows_async   stable compaction by a flag per point: the kept rows in caller order
// Everything here has internal linkage: each of the seven translation units carries its own copy, the kernel included.
#pragma once
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
#include "arena.hpp"
#include "owned.hpp"

namespace fgoicp {
namespace {

struct OneShot {  // what the call owns on the device
    const char* name;  // "fgoicp_...": the head of every message
    Stream stream;  // declared first, released last: the arena goes while the stream still exists
    Dev<char> arena;
    explicit OneShot(const char* call) : name(call) {}
    ~OneShot() { stream.sync(); }  // before the arena is freed (an early return may leave copies into the caller's arrays in flight)
};

#define ONECHK(call, expr)                                                                 \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            set_error(std::string(call) + ": " #expr " failed: " + hipGetErrorString(e_)); \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;            \
        }                                                                                  \
    } while (0)

// ---- the refusals; every one returns FGOICP_OK (0) or the status to return, with the message set
int refuse(const char* call, const std::string& what) {
    set_error(std::string(call) + ": " + what);
    return FGOICP_ERR_INVALID_ARG;
}
int refuse_cloud_head(const char* call, const float* xyz, size_t n) {
    if (!xyz || n == 0) return refuse(call, "the cloud must not be null or empty");
    if (n >= ((size_t)1 << 31)) return refuse(call, "more than 2^31 - 1 points");
    return FGOICP_OK;
}
int refuse_non_finite(const char* call, size_t i) { return refuse(call, "point " + std::to_string(i) + " has a non-finite coordinate"); }
int refuse_first_non_finite(const char* call, const float* xyz, size_t n) {
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(xyz[3 * i + a])) return refuse_non_finite(call, i);
    return FGOICP_OK;
}
// floor: the bytes of the struct's first version (a caller built against it passes no more)
template <class Info>
int refuse_info(const char* call, const Info* out, size_t floor, const char* type) {
    if (!out || out->struct_size < floor || out->struct_size > 4096) return refuse(call, std::string("out must not be null and out->struct_size = sizeof(") + type + ")");
    return FGOICP_OK;
}
int select_device(const char* call, int device) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string(call) + ": no HIP device available (" + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") + "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return refuse(call, "device ordinal out of range");
    ONECHK(call, hipSetDevice(device));
    return FGOICP_OK;
}

// as many bytes as the caller's version of the struct holds
template <class Info>
void write_info(Info* out, Info& full) {
    full.struct_size = out->struct_size < sizeof(full) ? out->struct_size : (uint32_t)sizeof(full);
    std::memcpy(out, &full, full.struct_size);
}

// ---- stable compaction: flag[i] != 0 keeps point i; row[i] = the exclusive scan of the flags, the number of kept points before i.
// Templates on the flag word (deduced; uint32_t at every call), so that a file that compacts nothing — fps.hip, voxel.hip, mesh.hip, mesh_distance.hip — carries neither
// the scatter kernel nor rocPRIM's scan kernels.
constexpr int kRowsBlock = 256;

template <class Word>
__global__ __launch_bounds__(kRowsBlock) void scatter_rows_kernel(const float* __restrict__ xyz, const Word* __restrict__ flag, const Word* __restrict__ row, uint32_t n,
                                                                 float* __restrict__ out_xyz, uint32_t* __restrict__ kept_index) {
    const size_t i = (size_t)blockIdx.x * kRowsBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float* p = xyz + 3 * i;
    const float x = p[0], y = p[1], z = p[2];
    float* o = out_xyz + 3 * (size_t)row[i];
    o[0] = x; o[1] = y; o[2] = z;
    kept_index[row[i]] = (uint32_t)i;
}

// enqueues the scan and the read-backs of h = {rows before the last point, the last point's flag}; the caller synchronises (with whatever
// else it has enqueued) and then asks kept_rows
template <class Word>
int scan_flags_async(const OneShot& d, void* tmp, size_t scan_bytes, Word* d_flag, Word* d_row, size_t n, Word h[2]) {
    static_assert(sizeof(Word) == 4, "the read-backs copy 4 bytes");
    ONECHK(d.name, rocprim::exclusive_scan(tmp, scan_bytes, d_flag, d_row, 0u, n, rocprim::plus<uint32_t>(), d.stream));
    ONECHK(d.name, hipMemcpyAsync(&h[0], d_row + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    ONECHK(d.name, hipMemcpyAsync(&h[1], d_flag + (n - 1), 4, hipMemcpyDeviceToHost, d.stream));
    return FGOICP_OK;
}
// the number of flags set; checked before the scatter: its rows then lie below count <= n
template <class Word>
int kept_rows(const OneShot& d, const Word h[2], size_t n, uint64_t* count) {
    *count = (uint64_t)h[0] + h[1];
    if (*count > n || h[1] > 1u) {
        set_error(std::string(d.name) + ": the device returned an inconsistent row count");
        return FGOICP_ERR_HIP;
    }
    return FGOICP_OK;
}
// enqueues the scatter of the kept points into d_out, d_idx and the copies of the `kept` rows to whichever of out_xyz, kept_index is given
template <class Word>
int scatter_rows_async(const OneShot& d, const float* d_xyz, const Word* d_flag, const Word* d_row, size_t n, float* d_out, uint32_t* d_idx, uint64_t kept, float* out_xyz,
                       uint32_t* kept_index) {
    hipLaunchKernelGGL(scatter_rows_kernel<Word>, dim3((unsigned)((n + kRowsBlock - 1) / kRowsBlock)), dim3(kRowsBlock), 0, d.stream, d_xyz, d_flag, d_row, (uint32_t)n, d_out, d_idx);
    if (out_xyz) ONECHK(d.name, hipMemcpyAsync(out_xyz, d_out, 12 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
    if (kept_index) ONECHK(d.name, hipMemcpyAsync(kept_index, d_idx, 4 * (size_t)kept, hipMemcpyDeviceToHost, d.stream));
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp
