// icp::Registration / icp::NearestNeighborLUT for C++ callers — same constructor arguments, method
// names and return order as the reference's fgoicp/registration.hpp:18-98; every call forwards to the
// HIP context behind include/fgoicp_amd.h.  Non-copyable (the reference's versions double-free on copy).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <tuple>
#include <utility>

#include "common.hpp"

namespace icp {

class Registration;

// registration.hpp:18-42.  The LUT lives inside the Registration's device context; this view exposes
// its geometry/contents.  `search` is a device function in the reference (registration.cu:320-328);
// here it is a host call evaluating the same lookup on the device for n points.
class NearestNeighborLUT {
public:
    std::array<int, 3> dims() const {
        std::array<int, 3> d{};
        check_status(fgoicp_lut_dims(ctx_, d.data()), "fgoicp_lut_dims");
        return d;
    }
    std::vector<float> data() const {
        auto d = dims();
        std::vector<float> out((size_t)d[0] * d[1] * d[2]);
        check_status(fgoicp_lut_read(ctx_, out.data(), out.size()), "fgoicp_lut_read");
        return out;
    }
    std::vector<float> search(const PointCloud& queries) const {
        std::vector<float> out(queries.size());
        check_status(fgoicp_lut_search(ctx_, &queries.data()->x, queries.size(), out.data()), "fgoicp_lut_search");
        return out;
    }
private:
    friend class Registration;
    fgoicp_ctx* ctx_ = nullptr;
};

// EXTENSION (ours; the reference ends in (R, t) and the best error): the alignment report of fgoicp_alignment /
// fgoicp_solver_alignment.  Arrays in the caller's point order; dist2 in the frame the search ran in.
struct Alignment {
    std::vector<uint32_t> indices;     // ns: nearest target point of every source point (lowest index among sqrt-ties, icp3d.cu:20-25)
    std::vector<float> dist2;          // ns: its squared distance
    std::vector<uint8_t> inlier;       // ns: 1 = counted by the optimum (all ones unless trimmed)
    std::vector<uint8_t> target_hit;   // nt: 1 = neighbour of an inlier
    fgoicp_alignment_summary summary{};
    double fitness() const { return summary.points ? (double)summary.inliers / (double)summary.points : 0.0; }
    double inlier_rmse() const { return summary.inliers ? std::sqrt((double)summary.sse / (double)summary.inliers) / (double)summary.scaling_factor : 0.0; }
    double distance(size_t i) const { return std::sqrt((double)dist2[i]) / (double)summary.scaling_factor; }  // in the callers' units
};

// EXTENSION (ours; Open3D: get_information_matrix_from_point_clouds): the information matrix of fgoicp_information /
// fgoicp_solver_information — result.info, 6 x 6 row-major, twist order (wx, wy, wz, vx, vy, vz), over the report's inliers within the
// distance threshold.
struct Information {
    fgoicp_information_t result{};
    double operator()(int r, int c) const { return result.info[6 * r + c]; }
    double fitness() const { return result.points ? (double)result.correspondences / (double)result.points : 0.0; }
    double inlier_rmse() const { return result.correspondences ? std::sqrt(result.sum_dist2 / (double)result.correspondences) / (double)result.scaling_factor : 0.0; }  // callers' units
};

// EXTENSION (ours): point-to-plane refinement with target normals (fgoicp_ctx_set_target_normals, fgoicp_plane_moments, fgoicp_icp_plane,
// fgoicp_solver_refine_plane).  PlaneRefinement::result holds the refined pose (glm order), the iterations, the rank of the last solve,
// the counted correspondences, and plane_rmse / sse in the frame the search ran in.
struct PlaneRefinement {
    fgoicp_plane_result_t result{};
    mat3 R() const { mat3 m; for (int k = 0; k < 9; ++k) m.data()[k] = result.R[k]; return m; }
    vec3 t() const { return vec3{result.t[0], result.t[1], result.t[2]}; }
    double plane_rmse() const { return result.plane_rmse / (double)result.scaling_factor; }  // callers' units
};
// EXTENSION (ours): the robustly weighted loop of either refinement (fgoicp_icp_robust, fgoicp_solver_refine_robust): the pose as
// PlaneRefinement's, rmse() = sqrt(sum w s^2 / sum w) and loss_scale() in the callers' units.
struct RobustRefinement {
    fgoicp_robust_result_t result{};
    mat3 R() const { mat3 m; for (int k = 0; k < 9; ++k) m.data()[k] = result.R[k]; return m; }
    vec3 t() const { return vec3{result.t[0], result.t[1], result.t[2]}; }
    double rmse() const { return result.rmse / (double)result.scaling_factor; }
    double loss_scale() const { return result.scale / (double)result.scaling_factor; }
    double weight_sum() const { return result.weight_sum; }
    bool scale_estimated() const { return result.scale_estimated != 0; }
};
struct TargetKnn {
    std::vector<uint32_t> indices;  // nt rows of k: every target point's k nearest target points, itself included, sorted by (distance, index)
    std::vector<float> dist2;
    int k = 0;
};

class Registration {
public:
    // registration.hpp:68
    Registration(const PointCloud& pct, const PointCloud& pcs, const std::array<std::pair<float, float>, 3> target_bounds,
                 float lut_resolution, int device = 0, unsigned flags = 0)
        : nt(pct.size()), ns(pcs.size()) {
        const float b[6] = {target_bounds[0].first, target_bounds[0].second, target_bounds[1].first,
                            target_bounds[1].second, target_bounds[2].first, target_bounds[2].second};
        check_status(fgoicp_ctx_create(&pct.data()->x, nt, &pcs.data()->x, ns, b, lut_resolution, device, flags, &ctx_), "fgoicp_ctx_create");
        nnlut.ctx_ = ctx_;
    }
    ~Registration() { fgoicp_ctx_destroy(ctx_); }
    Registration(const Registration&) = delete;
    Registration& operator=(const Registration&) = delete;

    using BoundsResult_t = std::tuple<std::vector<float>, std::vector<float>>;

    // registration.hpp:96
    float compute_sse_error(mat3 R, vec3 t) const {
        float sse = 0.f;
        check_status(fgoicp_sse(ctx_, R.data(), &t.x, &sse), "fgoicp_sse");
        return sse;
    }
    // registration.hpp:97 — returns {lower, upper} (registration.cu:151)
    BoundsResult_t compute_sse_error(RotNode& rnode, std::vector<TransNode>& tnodes, bool fix_rot, StreamPool&) const {
        const size_t B = tnodes.size();
        std::vector<float> tn4(4 * B), lb(B), ub(B);
        for (size_t i = 0; i < B; ++i) { tn4[4 * i] = tnodes[i].t.x; tn4[4 * i + 1] = tnodes[i].t.y; tn4[4 * i + 2] = tnodes[i].t.z; tn4[4 * i + 3] = tnodes[i].span; }
        check_status(fgoicp_bounds_batch(ctx_, rnode.q.R.data(), rnode.span, tn4.data(), (int)B, fix_rot ? 1 : 0, lb.data(), ub.data()),
                     "fgoicp_bounds_batch");
        return {lb, ub};
    }

    // EXTENSION: correspondences, residuals and the inlier set of R*pcs + t (fgoicp_alignment)
    Alignment alignment(mat3 R, vec3 t) const {
        Alignment a;
        a.indices.resize(ns); a.dist2.resize(ns); a.inlier.resize(ns); a.target_hit.resize(nt);
        a.summary.struct_size = sizeof(a.summary);
        check_status(fgoicp_alignment(ctx_, R.data(), &t.x, a.indices.data(), a.dist2.data(), a.inlier.data(), a.target_hit.data(), &a.summary), "fgoicp_alignment");
        return a;
    }

    // EXTENSION: the information matrix of R*pcs + t over the report's inliers with dist2 <= max_dist2, in the frame of the clouds as passed in (fgoicp_information)
    Information information(mat3 R, vec3 t, float max_dist2 = INFINITY) const {
        Information f;
        f.result.struct_size = sizeof(f.result);
        check_status(fgoicp_information(ctx_, R.data(), &t.x, max_dist2, &f.result), "fgoicp_information");
        return f;
    }

    // EXTENSION: target normals — given (nt unit or non-unit vectors, normalised on upload), or estimated on the device from every target
    // point's k nearest target points (4 <= k <= 32); the sign of an estimated normal is arbitrary and nothing depends on it
    void set_target_normals(const PointCloud& normals) { check_status(fgoicp_ctx_set_target_normals(ctx_, &normals.data()->x, 0), "fgoicp_ctx_set_target_normals"); }
    void set_target_normals(int k = 16) { check_status(fgoicp_ctx_set_target_normals(ctx_, nullptr, k), "fgoicp_ctx_set_target_normals"); }
    PointCloud target_normals() const {
        PointCloud n(nt);
        check_status(fgoicp_target_normals(ctx_, &n.data()->x), "fgoicp_target_normals");
        return n;
    }
    TargetKnn target_knn(int k) const {
        TargetKnn r;
        r.k = k;
        r.indices.resize(nt * (size_t)(k > 0 ? k : 0)); r.dist2.resize(r.indices.size());
        check_status(fgoicp_target_knn(ctx_, k, r.indices.data(), r.dist2.data()), "fgoicp_target_knn");
        return r;
    }
    // EXTENSION: the point-to-plane normal equations of R*pcs + t (fgoicp_plane_moments) and the loop from (R, t) (fgoicp_icp_plane)
    fgoicp_plane_moments_t plane_moments(mat3 R, vec3 t, float max_dist2 = INFINITY) const {
        fgoicp_plane_moments_t m{};
        m.struct_size = sizeof(m);
        check_status(fgoicp_plane_moments(ctx_, R.data(), &t.x, max_dist2, &m), "fgoicp_plane_moments");
        return m;
    }
    PlaneRefinement icp_plane(mat3 R, vec3 t, size_t max_iter = 30, float conv_thr = 1e-6f, float max_dist2 = INFINITY) const {
        PlaneRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_icp_plane(ctx_, R.data(), &t.x, max_iter, conv_thr, max_dist2, &p.result), "fgoicp_icp_plane");
        return p;
    }
    // EXTENSION: source normals for the Generalized-ICP refinement — given, or estimated from every source point's k nearest source points
    void set_source_normals(const PointCloud& normals) { check_status(fgoicp_ctx_set_source_normals(ctx_, &normals.data()->x, 0), "fgoicp_ctx_set_source_normals"); }
    void set_source_normals(int k = 16) { check_status(fgoicp_ctx_set_source_normals(ctx_, nullptr, k), "fgoicp_ctx_set_source_normals"); }
    PointCloud source_normals() const {
        PointCloud n(ns);
        check_status(fgoicp_source_normals(ctx_, &n.data()->x), "fgoicp_source_normals");
        return n;
    }
    // EXTENSION: the Generalized-ICP normal equations of R*pcs + t (fgoicp_gicp_moments) and the loop from (R, t) (fgoicp_icp_gicp); the
    // result's plane_rmse() is the root mean squared plane-to-plane residual sqrt(sum d^T M d / N)
    fgoicp_plane_moments_t gicp_moments(mat3 R, vec3 t, float max_dist2 = INFINITY, double epsilon = 1e-3) const {
        fgoicp_plane_moments_t m{};
        m.struct_size = sizeof(m);
        check_status(fgoicp_gicp_moments(ctx_, R.data(), &t.x, max_dist2, epsilon, &m), "fgoicp_gicp_moments");
        return m;
    }
    PlaneRefinement icp_gicp(mat3 R, vec3 t, size_t max_iter = 30, float conv_thr = 1e-6f, float max_dist2 = INFINITY, double epsilon = 1e-3) const {
        PlaneRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_icp_gicp(ctx_, R.data(), &t.x, max_iter, conv_thr, max_dist2, epsilon, &p.result), "fgoicp_icp_gicp");
        return p;
    }
    // EXTENSION: robust losses over either refinement (model FGOICP_MODEL_PLANE / FGOICP_MODEL_GICP, loss FGOICP_LOSS_*): the weighted
    // normal equations at a pose (fgoicp_robust_moments), the automatic scale there (fgoicp_robust_scale) and the loop
    // (fgoicp_icp_robust; scale <= 0: estimated at (R, t))
    fgoicp_robust_moments_t robust_moments(mat3 R, vec3 t, int model, int loss, double scale, float max_dist2 = INFINITY, double epsilon = 1e-3) const {
        fgoicp_robust_moments_t m{};
        m.struct_size = sizeof(m);
        check_status(fgoicp_robust_moments(ctx_, R.data(), &t.x, max_dist2, model, epsilon, loss, scale, &m), "fgoicp_robust_moments");
        return m;
    }
    double robust_scale(mat3 R, vec3 t, int model, float max_dist2 = INFINITY, double epsilon = 1e-3) const {
        double s = 0.0;
        check_status(fgoicp_robust_scale(ctx_, R.data(), &t.x, max_dist2, model, epsilon, &s), "fgoicp_robust_scale");
        return s;
    }
    RobustRefinement icp_robust(mat3 R, vec3 t, int model, int loss, double scale = 0.0, size_t max_iter = 30, float conv_thr = 1e-6f, float max_dist2 = INFINITY,
                                double epsilon = 1e-3) const {
        RobustRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_icp_robust(ctx_, R.data(), &t.x, max_iter, conv_thr, max_dist2, model, epsilon, loss, scale, &p.result), "fgoicp_icp_robust");
        return p;
    }

    fgoicp_ctx* handle() const { return ctx_; }
    const size_t nt, ns;
    NearestNeighborLUT nnlut;
private:
    fgoicp_ctx* ctx_ = nullptr;
};

}  // namespace icp
