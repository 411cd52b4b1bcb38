// The fixed-order fp64 reduction of the moment kernels and their folds (device code only).
//
//   wave    an xor butterfly: both operands of every addition are the same pair whichever lane adds them, so all 64 lanes end with the
//           same bits
//   block   the block's waves added in wave order, one MomentRow per block (block_moment_row)
//   fold    one block of 1024 threads: thread t adds rows t, t + 1024, ... from +0.0, then the butterfly and waves 0..15 in wave order
//           (moment_fold_kernel)
//
// A lane without a term adds +0.0.  No atomics: the result is a function of the terms and their thread indices alone, so the same arrays
// give the same bytes.  oracle/np_restatement.py fixed_order_sum restates the order; tests/golden/moments_bits.npz holds its bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fgoicp {

__device__ __forceinline__ double wave_xor_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int lo = __shfl_xor(__double2loint(v), off, 64), hi = __shfl_xor(__double2hiint(v), off, 64);
        v += __hiloint2double(hi, lo);
    }
    return v;
}
__device__ __forceinline__ unsigned wave_xor_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_xor_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// s[0] + s[stride] + ... + s[(W - 1) * stride], left to right: what W waves left in shared memory, in wave order
template <int W, typename T>
__device__ __forceinline__ T waves_in_order(const T* s, int stride = 1) {
    T r = s[0];
#pragma unroll
    for (int w = 1; w < W; ++w) r += s[w * stride];
    return r;
}

// a block's partial sums of K terms and its count of the lanes that had terms
template <int K>
struct MomentRow {
    uint32_t count, pad;
    double v[K];
};

// what lane 0 of each of a block's W waves leaves in shared memory
template <int K, int W, typename Count>
struct WaveSums {
    double v[W][K];
    Count count[W];
};
// the butterfly over every wave, v and the returned count; the barrier is inside, so every thread of the block calls this
template <int K, int W, typename Count>
__device__ __forceinline__ Count wave_sums(double (&v)[K], Count count, WaveSums<K, W, Count>& s) {
    count = wave_xor_sum(count);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_xor_sum(v[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s.count[wave] = count;
#pragma unroll
        for (int k = 0; k < K; ++k) s.v[wave][k] = v[k];
    }
    __syncthreads();
    return count;
}

// *row = the sums of a block of W waves over its threads' terms[K] and count (0 or 1); every thread of the block calls this.  The terms
// are copied first: the caller's array stays its own (refine_moments_kernel hands it to gicp_pair_terms by pointer, and with the butterfly
// written into that same array the compiler kept all 28 doubles in scratch memory).
template <int W, int K>
__device__ __forceinline__ void block_moment_row(const double (&terms)[K], unsigned count, MomentRow<K>* __restrict__ row) {
    __shared__ WaveSums<K, W, unsigned> s;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = terms[k];
    count = wave_sums(v, count, s);
    if (threadIdx.x < K) row->v[threadIdx.x] = waves_in_order<W>(&s.v[0][threadIdx.x], K);
    if (threadIdx.x == 0) {
        row->count = count + waves_in_order<W - 1>(s.count + 1);  // thread 0 holds wave 0's count
        row->pad = 0u;
    }
}

// One block of 1024 threads, any number of rows: out = {the count (one 64-bit integer), the bits of the K sums}.  Every thread of the
// block calls this (moment_fold_kernel; fused_moment_fold_kernel, one block per pair of a batch tick).
template <int K>
__device__ __forceinline__ void moment_fold_block(const MomentRow<K>* __restrict__ rows, int nrows, unsigned long long* __restrict__ out) {
    __shared__ WaveSums<K, 16, unsigned long long> s;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    unsigned long long count = 0ull;
    for (int b = threadIdx.x; b < nrows; b += 1024) {
        count += rows[b].count;
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += rows[b].v[k];
    }
    count = wave_sums(v, count, s);
    if (threadIdx.x < K) out[1 + threadIdx.x] = (unsigned long long)__double_as_longlong(waves_in_order<16>(&s.v[0][threadIdx.x], K));
    if (threadIdx.x == 0) out[0] = count + waves_in_order<15>(s.count + 1);
}
template <int K>
__global__ __launch_bounds__(1024) void moment_fold_kernel(const MomentRow<K>* __restrict__ rows, int nrows, unsigned long long* __restrict__ out) {
    moment_fold_block<K>(rows, nrows, out);
}

}  // namespace fgoicp
