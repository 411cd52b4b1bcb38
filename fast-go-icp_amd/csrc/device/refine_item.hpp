// The per-thread body of the refinements' moment kernels (device code only; included by kernels.hip inside namespace fgoicp, behind
// host/gicp.hpp, host/robust.hpp and fixed_sum.hpp): refine_moments_kernel, the launch of one context, and fused_refine_moments_kernel, the
// launch of a batch tick over many contexts, run this one text per device slot — as bounds_item.hpp and trim_select_body.inc serve the solo
// and the fused bounds.  What a slot contributes depends on its own pair's arrays and scalars only.
#pragma once

__device__ __forceinline__ bool nonzero3(const float4& a) { return a.x != 0.0f || a.y != 0.0f || a.z != 0.0f; }
// the counted-set gate for the caller index o of a device slot, and the gathers behind it: true with nn = the target normal and q = the
// target point at corr[o]
__device__ __forceinline__ bool counted_pair(uint32_t o, const RefineInputs& in, float4& nn, float4& q) {
    if (!(o < (uint32_t)in.n)) return false;
    const uint32_t j = in.corr[o];
    if (!(in.inlier[o] != 0 && in.d2[o] <= in.max_d2 && j < (uint32_t)in.nt)) return false;
    nn = in.normals[j];
    if (!nonzero3(nn)) return false;
    q = in.tgt[j];
    return true;
}
// u = the 28 point-to-plane terms of one pair; returns the residual r
__device__ __forceinline__ double plane_pair_terms(const double X[3], const float4& q, const double N[3], double* u) {
    const double r = N[0] * (X[0] - (double)q.x) + N[1] * (X[1] - (double)q.y) + N[2] * (X[2] - (double)q.z);
    const double J[6] = {X[1] * N[2] - X[2] * N[1], X[2] * N[0] - X[0] * N[2], X[0] * N[1] - X[1] * N[0], N[0], N[1], N[2]};
    int m = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) u[m++] = J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) u[21 + a] = J[a] * r;
    u[27] = r * r;
    return r;
}
// Device slot i of a cloud of in.n slots: v = its K terms (all +0.0 for a slot beyond the cloud or an uncounted one), returns its count
// (0 or 1).  R9: the rotation of the pose `in.moved` was formed with (read with GICP only).  PER_POINT: residual / weight / counted at the
// slot's caller index.
template <bool GICP, bool WEIGHTED, bool PER_POINT>
__device__ __forceinline__ unsigned refine_slot_terms(int i, const RefineInputs& in, const float (&R9)[9], double eps, int loss, double scale,
                                                      double (&v)[WEIGHTED ? kRobustTerms : kPlaneTerms], double* __restrict__ residual, double* __restrict__ weight,
                                                      unsigned char* __restrict__ counted) {
    constexpr int K = WEIGHTED ? kRobustTerms : kPlaneTerms;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    unsigned cnt = 0u;
    if (i < in.n) {
        const uint32_t o = in.orig_of_slot[i];
        const float4 x = in.moved[i];
        float4 np = make_float4(0.f, 0.f, 0.f, 0.f);
        if (GICP) np = in.src_normals[i];
        float4 nn, q;
        double s = 0.0, w = 0.0;
        if ((!GICP || nonzero3(np)) && counted_pair(o, in, nn, q)) {
            const double X[3] = {(double)x.x, (double)x.y, (double)x.z}, N[3] = {(double)nn.x, (double)nn.y, (double)nn.z};
            // the pair's unweighted terms: straight into the accumulators, or (WEIGHTED) an array of their own — handed to gicp_pair_terms
            // by pointer and then scaled in place, the accumulators went to scratch memory (240 bytes per lane)
            double own[WEIGHTED ? kPlaneTerms : 1];
            double* const u = WEIGHTED ? own : v;
            if (GICP) {
                const double Q[3] = {(double)q.x, (double)q.y, (double)q.z}, NP[3] = {(double)np.x, (double)np.y, (double)np.z};
                gicp_pair_terms(X, Q, N, NP, R9, eps, nullptr, u);
                s = sqrt(u[27] > 0.0 ? u[27] : 0.0);
            } else {
                s = plane_pair_terms(X, q, N, u);
            }
            if (WEIGHTED) {
                w = robust_weight(loss, s, scale);
#pragma unroll
                for (int k = 0; k < kPlaneTerms; ++k) v[k] = u[k] * w;
                v[K - 1] = w;
            }
            cnt = 1u;
        }
        if (PER_POINT && o < (uint32_t)in.n) {
            residual[o] = s;
            weight[o] = w;
            counted[o] = (unsigned char)cnt;
        }
    }
    return cnt;
}
