// Point-to-mesh refinement (fgoicp_mesh_moments, fgoicp_mesh_refine, fgoicp_mesh_pair_terms; include/fgoicp_amd.h has the definition,
// DESIGN.md section 23 the launch chain, the slack argument and the resources).  One-shot calls: the frame is one_shot.hpp, the tree and the
// walk are mesh_tree.hpp's (one text with mesh_distance.hip), the pair's arithmetic is mesh_pair.hpp's, the sums are fixed_sum.hpp's, the
// solve and the pose update plane.hpp's, the weight robust.hpp's.
//
//   once per call    the refusals (no device); the tree (md_build) and the source points uploaded; md_key_kernel over the SOURCE-frame
//                    coordinates and rocPRIM's stable radix sort of (code, caller index) — a rigid motion keeps neighbours neighbours, so
//                    one order serves every pose, and it is the order of the sums
//   per evaluation   mr_moments_kernel, one wave per 64 sorted points (pose, threshold, loss and scale by value): the moved point, md_walk,
//                    the winner's face once more (mesh_pair_terms: direction, residual, weight, the 28 terms), block_moment_row<4, 30>;
//                    then moment_fold_kernel<30>; one copy of (1 + 30) x 8 bytes and one host synchronisation
//   host             plane_step / plane_apply_step, the stop rule of fgoicp_icp_plane / fgoicp_icp_robust
// No atomics; no loop waits on another wave.  The per-point arrays are written only by the instantiation fgoicp_mesh_moments asks for (and
// the scale estimate, once).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../host/plane.hpp"
#include "../host/robust.hpp"
#include "fixed_sum.hpp"
#include "mesh_pair.hpp"
#include "mesh_tree.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

constexpr int kMrTerms = 30;  // the 28 of plane.hpp, sum w, sum dist2
static_assert(kPlaneMoments == 28, "the layout of fgoicp_plane_moments_t::m");

struct MrPose {
    float R[9], t[3];  // glm order: R[a][b] = R[3 b + a]
};
struct MrPoint {  // caller order; all set or all nullptr
    uint32_t* face;
    float* closest;
    double* dist2;
    uint8_t* region;
    double* direction;
    double* residual;
    double* weight;
    unsigned char* counted;
};

template <bool kBrute, bool kPerPoint>
__global__ __launch_bounds__(kMdBlock) void mr_moments_kernel(MdTree t, const float* __restrict__ pts, const uint32_t* __restrict__ order, uint32_t n, MrPose pose, double slack,
                                                             double max_d2, int loss, double scale, MomentRow<kMrTerms>* __restrict__ rows, MrPoint out) {
    __shared__ uint32_t s_stack[kMdBlock / 64][kMdStack];
    const int wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * kMdBlock + threadIdx.x;
    const bool active = i < n;
    const uint32_t qi = active ? order[i] : 0u;
    double x[3] = {0.0, 0.0, 0.0};
    if (active) {
        const float* p = pts + 3 * (size_t)qi;
        const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
#pragma unroll
        for (int a = 0; a < 3; ++a)  // rounded to fp32 once: the query fgoicp_mesh_distance would be given
            x[a] = (double)(float)((((double)pose.R[a] * px + (double)pose.R[3 + a] * py) + (double)pose.R[6 + a] * pz) + (double)pose.t[a]);
    }
    const MdBest best = kBrute ? md_brute(t, x[0], x[1], x[2], active) : md_walk(t, x[0], x[1], x[2], slack, s_stack[wave], active);
    double v[kMrTerms];
#pragma unroll
    for (int k = 0; k < kMrTerms; ++k) v[k] = 0.0;
    unsigned cnt = 0u;
    if (active) {
        // the winner's face once more (the same text gives the same dist2): nothing of it lived through the walk
        const float* c = t.leaf_v + 9 * (size_t)best.slot;
        double u[kMrTerms];
        const MeshPair o = mesh_pair_terms(x[0], x[1], x[2], (double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4], (double)c[5], (double)c[6], (double)c[7],
                                           (double)c[8], loss, scale, u);
        if (o.r.d2 <= max_d2) {
            cnt = 1u;
#pragma unroll
            for (int k = 0; k < 28; ++k) v[k] = u[k];
            v[28] = o.w;
            v[29] = o.r.d2;
        }
        if (kPerPoint) {
            out.face[qi] = best.face;
            float* cl = out.closest + 3 * (size_t)qi;
            cl[0] = (float)o.r.cx; cl[1] = (float)o.r.cy; cl[2] = (float)o.r.cz;
            out.dist2[qi] = o.r.d2;
            out.region[qi] = (uint8_t)o.r.region;
            double* g = out.direction + 3 * (size_t)qi;
            g[0] = o.g[0]; g[1] = o.g[1]; g[2] = o.g[2];
            out.residual[qi] = cnt ? o.s : 0.0;
            out.weight[qi] = cnt ? o.w : 0.0;
            out.counted[qi] = (unsigned char)cnt;
        }
    }
    block_moment_row<kMdBlock / 64>(v, cnt, &rows[blockIdx.x]);
}

// ---- the host half ---------------------------------------------------------------------------------------------------------------------------
struct MrInputs {
    const float* vtx; size_t nv;
    const uint32_t* tri; size_t nf;
    const float* pts; size_t ns;
    float max_distance;
    int loss;
    double scale;
    uint32_t flags;
    int device;
};
struct MrHost {       // what the host pass over the inputs leaves
    float big_v = 0.0f;   // the largest |coordinate| of the vertices
    float big_p = 0.0f;   // ... of the source points
    float lo[3], ext = 1.0f;  // the source's box and its longest side (md_key_kernel)
    double max_d2 = 0.0;
};

bool finite_n(const float* x, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(x[k])) return false;
    return true;
}

// What fgoicp_mesh_distance refuses, in its order, then this feature's own; `scale_given`: a loss needs a scale that is finite and > 0
// (fgoicp_mesh_moments), otherwise a scale <= 0 asks for the estimate (fgoicp_mesh_refine).
int mr_refusals(const char* call, const MrInputs& in, const float* R9, const float* t3, bool scale_given, MrHost* h) {
    constexpr size_t kLimit = (size_t)1 << 31;
    if (!in.vtx || in.nv == 0) return refuse(call, "the vertices must not be null or empty");
    if (!in.tri || in.nf == 0) return refuse(call, "the triangles must not be null or empty");
    if (!in.pts || in.ns == 0) return refuse(call, "the points must not be null or empty");
    if (in.nv >= kLimit) return refuse(call, "more than 2^31 - 1 vertices");
    if (in.nf >= kLimit) return refuse(call, "more than 2^31 - 1 triangles");
    if (in.ns >= kLimit) return refuse(call, "more than 2^31 - 1 points");
    if (in.flags & ~(uint32_t)FGOICP_MESH_DISTANCE_BRUTE) return refuse(call, "unknown flag bits " + std::to_string(in.flags & ~(uint32_t)FGOICP_MESH_DISTANCE_BRUTE));
    if (!R9 || !t3) return refuse(call, "R9 and t3 must not be null");
    if (!finite_n(R9, 9) || !finite_n(t3, 3)) return refuse(call, "the pose must be finite");
    if (!std::isfinite(in.max_distance)) return refuse(call, "max_distance must be finite (<= 0: no threshold)");
    if (!robust_loss_ok(in.loss)) return refuse(call, "unknown loss " + std::to_string(in.loss));
    if (!std::isfinite(in.scale)) return refuse(call, scale_given ? "the scale must be finite and > 0" : "the scale must be finite (<= 0: estimated)");
    if (scale_given && in.loss != FGOICP_LOSS_NONE && !robust_scale_ok(in.scale)) return refuse(call, "the scale must be finite and > 0");
    for (size_t i = 0; i < in.nv; ++i)
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(in.vtx[3 * i + a])) return refuse(call, "vertex " + std::to_string(i) + " has a non-finite coordinate");
            h->big_v = std::max(h->big_v, std::fabs(in.vtx[3 * i + a]));
        }
    float lo[3] = {in.pts[0], in.pts[1], in.pts[2]}, hi[3] = {in.pts[0], in.pts[1], in.pts[2]};
    for (size_t i = 0; i < in.ns; ++i)
        for (int a = 0; a < 3; ++a) {
            const float c = in.pts[3 * i + a];
            if (!std::isfinite(c)) return refuse_non_finite(call, i);
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
            h->big_p = std::max(h->big_p, std::fabs(c));
        }
    for (size_t f = 0; f < in.nf; ++f)
        for (int c = 0; c < 3; ++c)
            if (in.tri[3 * f + c] >= in.nv)
                return refuse(call, "face " + std::to_string(f) + " has vertex index " + std::to_string(in.tri[3 * f + c]) + ": the mesh has " + std::to_string(in.nv) + " vertices");
    std::memcpy(h->lo, lo, sizeof(lo));
    float ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    if (!(ext > 0.0f) || !std::isfinite(ext)) ext = 1.0f;  // one point, or a box wider than fp32 holds: the order stays the callers'
    h->ext = ext;
    h->max_d2 = in.max_distance > 0.0f ? (double)in.max_distance * (double)in.max_distance : std::numeric_limits<double>::infinity();
    return FGOICP_OK;
}

// M of the pruning argument for the queries of this pose, without a device pass: |x[a]| <= (|R[a][0]| + |R[a][1]| + |R[a][2]|) max|p| +
// |t[a]| in exact arithmetic; the four roundings of the fp64 form and the one to fp32 are covered by the factor 1 + 2^-20.  The proof
// only needs M not too small (a larger slack prunes less and changes no winner).  false: a moved point may leave the fp32 range.
bool mr_bound(const MrHost& h, const MrPose& p, double* big) {
    double m = (double)h.big_v;
    for (int a = 0; a < 3; ++a) {
        const double row = (std::fabs((double)p.R[a]) + std::fabs((double)p.R[3 + a])) + std::fabs((double)p.R[6 + a]);
        m = std::max(m, (row * (double)h.big_p + std::fabs((double)p.t[a])) * (1.0 + 0x1p-20));
    }
    *big = m;
    return m < (double)FLT_MAX;
}

struct MrDevice {  // the call's arrays on the device, all inside its one arena
    float *box = nullptr, *leaf_v = nullptr, *pts = nullptr, *closest = nullptr;
    uint32_t *leaf_f = nullptr, *key_a = nullptr, *key_b = nullptr, *idx_a = nullptr, *idx_b = nullptr, *face = nullptr;
    double *dist2 = nullptr, *direction = nullptr, *residual = nullptr, *weight = nullptr;
    uint8_t* region = nullptr;
    unsigned char* counted = nullptr;
    char* tmp = nullptr;
    MomentRow<kMrTerms>* rows = nullptr;
    unsigned long long* out = nullptr;
    MdTree tree{};
    uint32_t n = 0;
    unsigned blocks = 0;
};

// the set-up of a call, once: the arena, the uploads, the keys and the sort.  per_point: the arrays of MrPoint too
int mr_setup(const char* call, OneShot& d, const MrInputs& in, const MrHost& h, const MdHostTree& tree, bool per_point, MrDevice* v) {
    const size_t n = in.ns, pp = per_point ? n : 0;
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    size_t sort_bytes = 0;
    ONECHK(call, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 30u, d.stream));
    v->n = (uint32_t)n;
    v->blocks = (unsigned)((n + kMdBlock - 1) / kMdBlock);
    Arena plan;
    plan.take(v->box, tree.box.size()); plan.take(v->leaf_v, tree.leaf_v.size()); plan.take(v->leaf_f, tree.leaf_f.size()); plan.take(v->pts, 3 * n);
    plan.take(v->key_a, n); plan.take(v->key_b, n); plan.take(v->idx_a, n); plan.take(v->idx_b, n); plan.take(v->tmp, sort_bytes);
    plan.take(v->rows, v->blocks); plan.take(v->out, 1 + kMrTerms);
    plan.take(v->face, pp); plan.take(v->closest, 3 * pp); plan.take(v->dist2, pp); plan.take(v->region, pp); plan.take(v->direction, 3 * pp);
    plan.take(v->residual, pp); plan.take(v->weight, pp); plan.take(v->counted, pp);
    ONECHK(call, d.arena.alloc(plan.total()));
    plan.place(d.arena);
    ONECHK(call, hipMemcpyAsync(v->box, tree.box.data(), 4 * tree.box.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(v->leaf_v, tree.leaf_v.data(), 4 * tree.leaf_v.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(v->leaf_f, tree.leaf_f.data(), 4 * tree.leaf_f.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(v->pts, in.pts, 12 * n, hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(md_key_kernel, dim3(v->blocks), dim3(kMdBlock), 0, d.stream, v->pts, v->n, h.lo[0], h.lo[1], h.lo[2], h.ext, v->key_a, v->idx_a);
    ONECHK(call, rocprim::radix_sort_pairs(v->tmp, sort_bytes, v->key_a, v->key_b, v->idx_a, v->idx_b, n, 0u, 30u, d.stream));
    v->tree = MdTree{v->box, v->leaf_v, v->leaf_f, tree.nleaves, tree.depth};
    return FGOICP_OK;
}

// One evaluation: the kernel, the fold, the copy of its 31 words and the wait.  m->n = the counted, m->m = the 28 sums and sum w;
// *sum_dist2 the 30th.  per_point: the kernel that also fills the arrays of MrPoint (they stay on the device).
int mr_evaluate(const char* call, OneShot& d, const MrDevice& v, const MrInputs& in, const MrHost& h, const MrPose& pose, int loss, double scale, bool per_point, RefineMoments* m,
                double* sum_dist2) {
    double big = 0.0;
    if (!mr_bound(h, pose, &big)) return refuse(call, "the pose moves a point beyond the fp32 range");
    const double slack = kMdSlack * big;
    const MrPoint out{v.face, v.closest, v.dist2, v.region, v.direction, v.residual, v.weight, v.counted};
    const bool brute = (in.flags & FGOICP_MESH_DISTANCE_BRUTE) != 0;
    auto* const kernel = brute ? (per_point ? mr_moments_kernel<true, true> : mr_moments_kernel<true, false>)
                               : (per_point ? mr_moments_kernel<false, true> : mr_moments_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(v.blocks), dim3(kMdBlock), 0, d.stream, v.tree, v.pts, v.idx_b, v.n, pose, slack, h.max_d2, loss, loss == FGOICP_LOSS_NONE ? 1.0 : scale, v.rows,
                       out);
    hipLaunchKernelGGL(moment_fold_kernel<kMrTerms>, dim3(1), dim3(1024), 0, d.stream, v.rows, (int)v.blocks, v.out);
    unsigned long long w[1 + kMrTerms];
    ONECHK(call, hipMemcpyAsync(w, v.out, sizeof(w), hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    m->n = w[0];
    std::memcpy(m->m, w + 1, sizeof(double) * kRobustMoments);
    std::memcpy(sum_dist2, w + 1 + kRobustMoments, sizeof(double));
    return FGOICP_OK;
}

MrPose mr_pose(const float* R9, const float* t3) {
    MrPose p;
    std::memcpy(p.R, R9, sizeof(p.R));
    std::memcpy(p.t, t3, sizeof(p.t));
    return p;
}

int mesh_moments_impl(const MrInputs& in, const float* R9, const float* t3, uint32_t* face, float* closest, double* dist2, uint8_t* region, double* direction, double* residual,
                      double* weight, unsigned char* counted, uint32_t* order, fgoicp_mesh_moments_t* out) {
    const char* const call = "fgoicp_mesh_moments";
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_mesh_moments_t, tree_depth) + 2 * sizeof(uint32_t), "fgoicp_mesh_moments_t")) return rc;
    MrHost h;
    if (const int rc = mr_refusals(call, in, R9, t3, true, &h)) return rc;
    const MrPose pose = mr_pose(R9, t3);
    double big = 0.0;
    if (!mr_bound(h, pose, &big)) return refuse(call, "the pose moves a point beyond the fp32 range");
    if (const int rc = select_device(call, in.device)) return rc;
    const MdHostTree tree = md_build(in.vtx, in.tri, in.nf);
    if (tree.faces == 0) return refuse(call, "the mesh has no area");
    const bool per_point = face || closest || dist2 || region || direction || residual || weight || counted;
    const size_t n = in.ns;
    OneShot d(call);
    MrDevice v;
    if (const int rc = mr_setup(call, d, in, h, tree, per_point, &v)) return rc;
    RefineMoments m;
    double sum_dist2 = 0.0;
    if (const int rc = mr_evaluate(call, d, v, in, h, pose, in.loss, in.scale, per_point, &m, &sum_dist2)) return rc;
    if (face) ONECHK(call, hipMemcpyAsync(face, v.face, 4 * n, hipMemcpyDeviceToHost, d.stream));
    if (closest) ONECHK(call, hipMemcpyAsync(closest, v.closest, 12 * n, hipMemcpyDeviceToHost, d.stream));
    if (dist2) ONECHK(call, hipMemcpyAsync(dist2, v.dist2, 8 * n, hipMemcpyDeviceToHost, d.stream));
    if (region) ONECHK(call, hipMemcpyAsync(region, v.region, n, hipMemcpyDeviceToHost, d.stream));
    if (direction) ONECHK(call, hipMemcpyAsync(direction, v.direction, 24 * n, hipMemcpyDeviceToHost, d.stream));
    if (residual) ONECHK(call, hipMemcpyAsync(residual, v.residual, 8 * n, hipMemcpyDeviceToHost, d.stream));
    if (weight) ONECHK(call, hipMemcpyAsync(weight, v.weight, 8 * n, hipMemcpyDeviceToHost, d.stream));
    if (counted) ONECHK(call, hipMemcpyAsync(counted, v.counted, n, hipMemcpyDeviceToHost, d.stream));
    if (order) ONECHK(call, hipMemcpyAsync(order, v.idx_b, 4 * n, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));

    fgoicp_mesh_moments_t full;
    std::memset(&full, 0, sizeof(full));  // the padding too: two results of the same inputs are the same bytes
    full.flags = in.flags;
    full.points = n;
    full.correspondences = m.n;
    std::memcpy(full.m, m.m, sizeof(full.m));
    full.weight_sum = m.m[28];
    full.sum_dist2 = sum_dist2;
    full.max_dist2 = h.max_d2;
    full.loss = in.loss;
    full.scale = in.scale;
    full.vertices = in.nv;
    full.triangles = in.nf;
    full.faces = tree.faces;
    full.zero_area = tree.zero_area;
    full.tree_depth = (uint32_t)tree.depth;
    full.leaf_faces = (uint32_t)kMdLeaf;
    write_info(out, full);
    return FGOICP_OK;
}

// fgoicp_icp_plane's / fgoicp_icp_robust's loop (ctx.hip refine_run_advance), term for term, over mr_evaluate
int mesh_refine_impl(const MrInputs& in0, const float* R0, const float* t0, size_t max_iter, float thr, fgoicp_mesh_refine_result_t* out) {
    const char* const call = "fgoicp_mesh_refine";
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_mesh_refine_result_t, zero_area) + sizeof(uint64_t), "fgoicp_mesh_refine_result_t")) return rc;
    MrInputs in = in0;
    MrHost h;
    if (const int rc = mr_refusals(call, in, R0, t0, false, &h)) return rc;
    if (!std::isfinite(thr)) return refuse(call, "conv_thr must be finite");
    MrPose pose = mr_pose(R0, t0);
    double big = 0.0;
    if (!mr_bound(h, pose, &big)) return refuse(call, "the pose moves a point beyond the fp32 range");
    if (const int rc = select_device(call, in.device)) return rc;
    const MdHostTree tree = md_build(in.vtx, in.tri, in.nf);
    if (tree.faces == 0) return refuse(call, "the mesh has no area");
    const bool estimate = in.loss != FGOICP_LOSS_NONE && !(in.scale > 0.0);
    std::vector<double> res;  // declared before the stream: they outlive every copy in flight
    std::vector<unsigned char> cnt;
    OneShot d(call);
    MrDevice v;
    if (const int rc = mr_setup(call, d, in, h, tree, estimate, &v)) return rc;
    RefineMoments m;
    double sum_dist2 = 0.0;
    int scale_estimated = 0;
    if (estimate) {  // one evaluation of its own at the start pose, unweighted, with the per-point stores; the median on the host
        if (const int rc = mr_evaluate(call, d, v, in, h, pose, FGOICP_LOSS_NONE, 1.0, true, &m, &sum_dist2)) return rc;
        res.resize(in.ns);
        cnt.resize(in.ns);
        ONECHK(call, hipMemcpyAsync(res.data(), v.residual, 8 * in.ns, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipMemcpyAsync(cnt.data(), v.counted, in.ns, hipMemcpyDeviceToHost, d.stream));
        ONECHK(call, hipStreamSynchronize(d.stream));
        double s = 0.0;
        if (!robust_mad_scale(res.data(), cnt.data(), in.ns, &s)) return refuse(call, "nothing is counted at this pose, there is no scale to estimate: pass a scale");
        if (!robust_scale_ok(s)) return refuse(call, "the median residual is 0, there is no scale to estimate: pass a scale");
        in.scale = s;
        scale_estimated = 1;
    }
    Mat3f R = Mat3f::from(R0);
    Vec3f t{t0[0], t0[1], t0[2]};
    int iterations = 0, rank = 0;
    bool stop = false;
    for (;;) {
        std::memcpy(pose.R, R.m, sizeof(pose.R));
        pose.t[0] = t.x; pose.t[1] = t.y; pose.t[2] = t.z;
        if (const int rc = mr_evaluate(call, d, v, in, h, pose, in.loss, in.scale, false, &m, &sum_dist2)) return rc;
        if (stop || (size_t)iterations >= max_iter || m.n == 0 || m.m[28] == 0.0) break;
        if (!plane_moments_finite(m.m) || !std::isfinite(m.m[28])) return refuse(call, "the normal equations are not finite");
        double xi[6];
        plane_step(m.m, xi, &rank);
        plane_apply_step(R, t, xi, R, t);
        ++iterations;
        const double step = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) + std::sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
        stop = step < (double)thr || (iterations == 1 && rank < 6);  // one more evaluation, at the pose returned, then out
    }
    fgoicp_mesh_refine_result_t full;
    std::memset(&full, 0, sizeof(full));
    std::memcpy(full.R, R.m, sizeof(full.R));
    full.t[0] = t.x; full.t[1] = t.y; full.t[2] = t.z;
    full.iterations = iterations;
    full.rank = rank;
    full.points = in.ns;
    full.correspondences = m.n;
    full.weight_sum = m.m[28];
    full.mesh_rmse = m.m[28] > 0.0 ? std::sqrt(m.m[27] / m.m[28]) : 0.0;
    full.rms_distance = m.n ? std::sqrt(sum_dist2 / (double)m.n) : 0.0;
    full.loss = in.loss;
    full.scale_estimated = scale_estimated;
    full.loss_scale = in.loss == FGOICP_LOSS_NONE ? 0.0 : in.scale;
    full.triangles = in.nf;
    full.faces = tree.faces;
    full.zero_area = tree.zero_area;
    write_info(out, full);
    return FGOICP_OK;
}

int mesh_pair_terms_impl(const float* x, const float* a, const float* b, const float* c, int loss, double scale, double* closest, double* dist2, int* region, double* g, double* s,
                         double* w, double* v28) {
    const char* const call = "fgoicp_mesh_pair_terms";
    if (!x || !a || !b || !c) return refuse(call, "x3, a3, b3 and c3 must not be null");
    for (const float* p : {x, a, b, c})
        if (!finite_n(p, 3)) return refuse(call, "a coordinate is not finite");
    if (!robust_loss_ok(loss)) return refuse(call, "unknown loss " + std::to_string(loss));
    if (loss != FGOICP_LOSS_NONE && !robust_scale_ok(scale)) return refuse(call, "the scale must be finite and > 0");
    if (md_n2(a, b, c) == 0.0) return refuse(call, "the triangle has no area");
    double v[28];
    const MeshPair o = mesh_pair_terms(x[0], x[1], x[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], loss, loss == FGOICP_LOSS_NONE ? 1.0 : scale, v);
    if (closest) { closest[0] = o.r.cx; closest[1] = o.r.cy; closest[2] = o.r.cz; }
    if (dist2) *dist2 = o.r.d2;
    if (region) *region = o.r.region;
    if (g) std::memcpy(g, o.g, sizeof(o.g));
    if (s) *s = o.s;
    if (w) *w = o.w;
    if (v28) std::memcpy(v28, v, sizeof(v));
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_mesh_pair_terms(const float* x3, const float* a3, const float* b3, const float* c3, int loss, double scale, double* closest3, double* dist2, int* region,
                                      double* g3, double* s, double* w, double* v28) {
    return fgoicp::abi_guard("fgoicp_mesh_pair_terms", [&] { return fgoicp::mesh_pair_terms_impl(x3, a3, b3, c3, loss, scale, closest3, dist2, region, g3, s, w, v28); });
}

extern "C" int fgoicp_mesh_moments(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* points_ns3, size_t ns, const float* R9,
                                   const float* t3, float max_distance, int loss, double scale, uint32_t flags, int device, uint32_t* face_ns, float* closest_ns3, double* dist2_ns,
                                   uint8_t* region_ns, double* direction_ns3, double* residual_ns, double* weight_ns, unsigned char* counted_ns, uint32_t* order_ns,
                                   fgoicp_mesh_moments_t* out) {
    return fgoicp::abi_guard("fgoicp_mesh_moments", [&] {
        const fgoicp::MrInputs in{vertices_nv3, nv, triangles_nf3, nf, points_ns3, ns, max_distance, loss, scale, flags, device};
        return fgoicp::mesh_moments_impl(in, R9, t3, face_ns, closest_ns3, dist2_ns, region_ns, direction_ns3, residual_ns, weight_ns, counted_ns, order_ns, out);
    });
}

extern "C" int fgoicp_mesh_refine(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* points_ns3, size_t ns, const float* R0_9,
                                  const float* t0_3, size_t max_iter, float conv_thr, float max_distance, int loss, double loss_scale, uint32_t flags, int device,
                                  fgoicp_mesh_refine_result_t* out) {
    return fgoicp::abi_guard("fgoicp_mesh_refine", [&] {
        const fgoicp::MrInputs in{vertices_nv3, nv, triangles_nf3, nf, points_ns3, ns, max_distance, loss, loss_scale, flags, device};
        return fgoicp::mesh_refine_impl(in, R0_9, t0_3, max_iter, conv_thr, out);
    });
}
