// The bounds of many registrations in one launch (fgoicp_batch; included by kernels.hip after bounds_item.hpp, inside
// namespace fgoicp::{anonymous}).
//
// A work item is (evaluation e, chunk c) of ONE pair of the batch: e names its pair, the pair's view holds that context's source cloud
// in its device order, its packed LUT, LUT geometry and points per chunk.  The per-point code is bounds_item_kernel's (item_walk) and the
// chunk's sums are folded by the same wave tree into the same partial, so an evaluation's partials — and the row that
// fused_bounds_finalize_kernel sums from them in bounds_finalize_kernel's order — are the bits the pair's own context computes.  Full
// evaluation only: no thresholds, no twin pairs.  The layout of the packed LUT, 32/64-bit texel addressing and the weight quantisation are
// template parameters: one launch per combination present in a tick, split by the host into launches of at most 2^24 items
// (HipBatchBackend::bounds).
//
// Trimmed pairs (fused_trim_item_kernel, its own launches per class): an item writes the per-point e = max(d, 0) of its chunk and the
// row's hashed sample (trim_store) into the e-row arena at its evaluation's row_off, as bounds_item_kernel<TRIM = 1> writes a window's
// rows, and no partials; fused_trim_select_kernel (kernels.hip) then selects each row as the pair's own context does.
#pragma once

template <int LAYOUT, int TRIM, bool WIDE, bool QUANT>
__device__ __forceinline__ void fused_item(const FusedPairView* __restrict__ pairs, const FusedEval* __restrict__ evals, const uint2* __restrict__ items, unsigned nitems,
                                           double2* __restrict__ partials, float* __restrict__ arena) {
    const unsigned slot = xcd_remap(blockIdx.x, gridDim.x);
    if (slot >= nitems) return;
    const uint2 it = items[slot];  // {evaluation, chunk}
    const FusedEval e = evals[it.x];
    const FusedPairView P = pairs[e.pair];
    const int lane = (int)threadIdx.x;
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = e.R[k];
    const ItemGeom G = item_geom(P.g);
    const float trans_radius = kSqrt3 * e.span;  // registration.cu:33
    const f2v t_xy = f2v{e.tx, e.ty};
    const int chunk = (int)it.y;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float* row = TRIM ? arena + e.row_off : nullptr;
    const int samp_shift = TRIM ? e.samp_shift : 0;
    if (e.fix_rot)
        item_walk<LAYOUT, TRIM, WIDE, QUANT, 0>(P.src, P.ns, P.lutp, G, R, t_xy, e.tz, e.sin_half, trans_radius, chunk * P.chunk_pts, P.chunk_pts, lane, acc, row, nullptr, samp_shift);
    else
        item_walk<LAYOUT, TRIM, WIDE, QUANT, 1>(P.src, P.ns, P.lutp, G, R, t_xy, e.tz, e.sin_half, trans_radius, chunk * P.chunk_pts, P.chunk_pts, lane, acc, row, nullptr, samp_shift);
    if (TRIM) return;
    const double r0 = wave_sum(acc[0]), r1 = wave_sum(acc[1]);
    if (lane == 0) partials[e.partial_base + (size_t)chunk] = make_double2(r0, r1);
}

template <int LAYOUT, bool WIDE, bool QUANT>
__global__ __launch_bounds__(64) void fused_bounds_item_kernel(const FusedPairView* __restrict__ pairs, const FusedEval* __restrict__ evals,
                                                               const uint2* __restrict__ items, unsigned nitems, double2* __restrict__ partials) {
    fused_item<LAYOUT, 0, WIDE, QUANT>(pairs, evals, items, nitems, partials, nullptr);
}
template <int LAYOUT, bool WIDE, bool QUANT>
__global__ __launch_bounds__(64) void fused_trim_item_kernel(const FusedPairView* __restrict__ pairs, const FusedEval* __restrict__ evals,
                                                             const uint2* __restrict__ items, unsigned nitems, float* __restrict__ arena) {
    fused_item<LAYOUT, 1, WIDE, QUANT>(pairs, evals, items, nitems, nullptr, arena);
}

// One wave per evaluation: its nchunk partials summed as bounds_finalize_kernel sums a row (lanes stride the chunks by 64, then the wave
// tree), rounded once to fp32.
__global__ __launch_bounds__(64) void fused_bounds_finalize_kernel(const FusedEval* __restrict__ evals, int nevals, const double2* __restrict__ partials,
                                                                   float* __restrict__ out_lb, float* __restrict__ out_ub) {
    const int s = blockIdx.x;
    if (s >= nevals) return;
    const FusedEval& e = evals[s];
    const double2* row = partials + e.partial_base;
    double u = 0.0, l = 0.0;
    for (int c = threadIdx.x; c < e.nchunk; c += 64) {
        const double2 v = row[c];
        u += v.x;
        l += v.y;
    }
    u = wave_sum(u);
    l = wave_sum(l);
    if (threadIdx.x == 0) {
        out_ub[s] = (float)u;
        out_lb[s] = (float)l;
    }
}
