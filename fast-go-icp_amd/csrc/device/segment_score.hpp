// The scoring kernel of the plane segmentation (fgoicp_segment_planes): K hypothesis planes against n points in one
// pass over the cloud.  Its own header so that tools/calib/segment_score.hip times the kernel the library runs.
//
//   block   256 threads hold a tile of kSegTile = 1024 points in registers, 4 per thread as doubles; a point that is not a candidate of
//           the peel (label >= 0, or past n) is held as NaN: it fails every comparison
//   loop    over the hypotheses in chunks of kSegChunk = 256.  The plane of the current hypothesis is one address for all lanes (the
//           compiler loads it through the scalar cache); a degenerate hypothesis is a NaN plane in the table.  Per point 3 multiplications,
//           3 additions and the comparison — the v_cmp's lane mask IS the ballot, so a wave's count is a scalar popcount
//   counts  every wave leaves its count of the chunk's hypotheses in its own row of LDS (4 x 256 words, no atomics); after the chunk thread t
//           adds the four rows of hypothesis t and, where the sum is not zero, adds it to the global count with one integer atomicAdd
//   grid    x: the tiles; y: a share of the chunks, so that few points with many hypotheses still fill the device
// The counts are integers: the result does not depend on the order of the additions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fgoicp {

constexpr int kSegBlock = 256, kSegPerThread = 4, kSegTile = kSegBlock * kSegPerThread, kSegChunk = 256;

struct SegPlane {  // 32 bytes
    double nx, ny, nz, d;
};

__global__ __launch_bounds__(kSegBlock) void segment_score_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ label, uint32_t n,
                                                                 const SegPlane* __restrict__ planes, uint32_t K, double T, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_count[kSegBlock / 64][kSegChunk];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double x[kSegPerThread], y[kSegPerThread], z[kSegPerThread];
#pragma unroll
    for (int p = 0; p < kSegPerThread; ++p) {
        const size_t i = (size_t)blockIdx.x * kSegTile + (size_t)p * kSegBlock + threadIdx.x;
        x[p] = y[p] = z[p] = __builtin_nan("");
        if (i < n && label[i] < 0) {
            x[p] = (double)xyz[3 * i];
            y[p] = (double)xyz[3 * i + 1];
            z[p] = (double)xyz[3 * i + 2];
        }
    }
    for (uint32_t base = blockIdx.y * kSegChunk; base < K; base += gridDim.y * kSegChunk) {
        const uint32_t here = K - base < (uint32_t)kSegChunk ? K - base : (uint32_t)kSegChunk;
        for (uint32_t c = 0; c < here; ++c) {
            const SegPlane pl = planes[base + c];
            uint32_t cnt = 0;
#pragma unroll
            for (int p = 0; p < kSegPerThread; ++p) {
                const double r = ((pl.nx * x[p] + pl.ny * y[p]) + pl.nz * z[p]) + pl.d;
                cnt += (uint32_t)__popcll(__ballot(fabs(r) <= T));
            }
            if (lane == 0) s_count[wave][c] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < here) {
            uint32_t sum = s_count[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kSegBlock / 64; ++w) sum += s_count[w][threadIdx.x];
            if (sum) atomicAdd(counts + base + threadIdx.x, sum);
        }
        __syncthreads();
    }
}

// the y extent of the grid: enough blocks to fill the device when the tiles are few, never more than the chunks
inline uint32_t segment_score_grid_y(uint32_t tiles, uint32_t K) {
    const uint32_t chunks = (K + kSegChunk - 1) / kSegChunk;
    const uint32_t want = tiles >= 2048u ? 1u : 2048u / tiles;
    return want < chunks ? want : chunks;
}

}  // namespace fgoicp
