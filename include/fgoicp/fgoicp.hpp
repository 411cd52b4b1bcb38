// icp::FastGoICP for C++ callers — reference fgoicp/fgoicp.hpp:8-110.  The branch-and-bound runs in
// host C++ inside libfgoicp_amd.so (fast-go-icp_amd/csrc/host/driver.hpp) and calls the HIP operators.
#pragma once
#include <tuple>
#include <vector>

#include "common.hpp"
#include "registration.hpp"

namespace icp {

class FastGoICP {
public:
    // fgoicp.hpp:13 (+ optional schedule: FGOICP_SCHEDULE_SERIAL reproduces the reference's order)
    FastGoICP(std::vector<vec3> pct, std::vector<vec3> pcs, float lut_resolution, float mse_threshold,
              int schedule = FGOICP_SCHEDULE_SERIAL, int round_width = 1, int device = 0, float trim_fraction = 0.0f)
        : nt_(pct.size()), ns_(pcs.size()) {
        fgoicp_solver_opts o{schedule, round_width, 0u, device, trim_fraction};
        check_status(fgoicp_solver_create(&pct.data()->x, pct.size(), &pcs.data()->x, pcs.size(), lut_resolution, mse_threshold, &o, &s_),
                     "fgoicp_solver_create");
        check_status(fgoicp_solver_set_log(s_, &FastGoICP::log_line, nullptr), "fgoicp_solver_set_log");
    }
    ~FastGoICP() { fgoicp_solver_destroy(s_); }
    FastGoICP(const FastGoICP&) = delete;
    FastGoICP& operator=(const FastGoICP&) = delete;

    using Result_t = std::tuple<mat3, vec3>;
    Result_t run() {  // fgoicp.hpp:28
        mat3 R;
        vec3 t;
        check_status(fgoicp_solver_run(s_, R.data(), &t.x), "fgoicp_solver_run");
        Logger(LogLevel::Info) << "Searching over! Best Error: " << get_best_error() << "\n\tRotation:\n" << R << "\n\tTranslation: " << t;  // fgoicp.cpp:25-27
        return {R, t};
    }
    // interfaces for visualisation, fgoicp.hpp:31-43 (safe to poll from another thread)
    float get_best_error() const { float v = 0; check_status(fgoicp_solver_best_error(s_, &v), "fgoicp_solver_best_error"); return v; }
    Result_t get_best_transform() const { mat3 R; vec3 t; check_status(fgoicp_solver_best_transform(s_, R.data(), &t.x), "fgoicp_solver_best_transform"); return {R, t}; }
    Result_t get_last_transform() const { mat3 R; vec3 t; check_status(fgoicp_solver_last_transform(s_, R.data(), &t.x), "fgoicp_solver_last_transform"); return {R, t}; }

    // not in the reference: false = every subcube is evaluated in full, as kernComputeBounds does (default: the inner BnBs tell the bounds
    // operator what they do not need to know, fgoicp_bounds_submit_cut — same trajectory, counters and result)
    void set_early_exit(bool on) { check_status(fgoicp_solver_set_early_exit(s_, on ? 1 : 0), "fgoicp_solver_set_early_exit"); }
    // not in the reference (EXTENSION): correspondences, residuals and the inlier set at the best transform, after run()
    // (fgoicp_solver_alignment).  Indices and masks refer to the clouds as passed in; dist2 is in the solver's centred and scaled
    // frame, Alignment::distance / inlier_rmse are in the callers' units.
    Alignment alignment() const {
        Alignment a;
        a.indices.resize(ns_); a.dist2.resize(ns_); a.inlier.resize(ns_); a.target_hit.resize(nt_);
        a.summary.struct_size = sizeof(a.summary);
        check_status(fgoicp_solver_alignment(s_, a.indices.data(), a.dist2.data(), a.inlier.data(), a.target_hit.data(), &a.summary), "fgoicp_solver_alignment");
        return a;
    }
    // EXTENSION: the information matrix at the best transform, after run(), in the callers' frame (fgoicp_solver_information);
    // max_distance in the callers' units, INFINITY: no threshold
    Information information(float max_distance = INFINITY) const {
        Information f;
        f.result.struct_size = sizeof(f.result);
        check_status(fgoicp_solver_information(s_, max_distance, &f.result), "fgoicp_solver_information");
        return f;
    }
    // EXTENSION: given normals (fgoicp_solver_set_target_normals / _source_normals), one per point of the cloud as passed in — a mesh knows
    // them exactly (fgoicp_mesh_sample); the refinements below then estimate only the set that is not given
    void set_target_normals(const std::vector<vec3>& normals) {
        if (normals.size() != nt_) throw std::invalid_argument("FastGoICP::set_target_normals: one normal per target point");
        check_status(fgoicp_solver_set_target_normals(s_, &normals.data()->x), "fgoicp_solver_set_target_normals");
    }
    void set_source_normals(const std::vector<vec3>& normals) {
        if (normals.size() != ns_) throw std::invalid_argument("FastGoICP::set_source_normals: one normal per source point");
        check_status(fgoicp_solver_set_source_normals(s_, &normals.data()->x), "fgoicp_solver_set_source_normals");
    }
    // EXTENSION: point-to-plane refinement from the best transform, after run() (fgoicp_solver_refine_plane): R and t in the callers'
    // frame; normals estimated from k neighbours unless the context has some; max_distance in the callers' units, INFINITY: no threshold.
    // run() and the best transform are untouched.
    PlaneRefinement refine_plane(int k = 16, size_t max_iter = 30, float conv_thr = 1e-6f, float max_distance = INFINITY) const {
        PlaneRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_solver_refine_plane(s_, k, max_iter, conv_thr, max_distance, &p.result), "fgoicp_solver_refine_plane");
        return p;
    }
    // EXTENSION: Generalized-ICP refinement from the best transform, after run() (fgoicp_solver_refine_gicp): as refine_plane, with the
    // normals of both clouds (whichever set the context lacks is estimated from k neighbours); plane_rmse() is the plane-to-plane residual.
    PlaneRefinement refine_gicp(int k = 16, size_t max_iter = 30, float conv_thr = 1e-6f, float max_distance = INFINITY, double epsilon = 1e-3) const {
        PlaneRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_solver_refine_gicp(s_, k, max_iter, conv_thr, max_distance, epsilon, &p.result), "fgoicp_solver_refine_gicp");
        return p;
    }
    // EXTENSION: either refinement under a robust loss (fgoicp_solver_refine_robust): model FGOICP_MODEL_PLANE / FGOICP_MODEL_GICP, loss
    // FGOICP_LOSS_*, loss_scale in the callers' units (<= 0: estimated at the best transform); the rest as refine_plane / refine_gicp.
    RobustRefinement refine_robust(int model, int loss, double loss_scale = 0.0, int k = 16, size_t max_iter = 30, float conv_thr = 1e-6f, float max_distance = INFINITY,
                                   double epsilon = 1e-3) const {
        RobustRefinement p;
        p.result.struct_size = sizeof(p.result);
        check_status(fgoicp_solver_refine_robust(s_, model, k, max_iter, conv_thr, max_distance, epsilon, loss, loss_scale, &p.result), "fgoicp_solver_refine_robust");
        return p;
    }
    fgoicp_run_stats stats() const { fgoicp_run_stats st{}; check_status(fgoicp_solver_stats(s_, &st), "fgoicp_solver_stats"); return st; }
    fgoicp_solver* handle() const { return s_; }
    // the reference's own lines while the search runs (fgoicp.cpp:15-17 Info, :85-87 Debug), from the driver's log events
    static void log_line(int event, float sse, const float* R9, const float* t3, void*) {
        mat3 R;
        for (int k = 0; k < 9; ++k) R.data()[k] = R9[k];
        const vec3 t{t3[0], t3[1], t3[2]};
        if (event == FGOICP_LOG_INITIAL_ICP) Logger(LogLevel::Info) << "Initial ICP best error: " << sse << "\n\tRotation:\n" << R << "\n\tTranslation: " << t;
        else Logger(LogLevel::Debug) << "New best error: " << sse << "\n\tRotation:\n" << R << "\n\tTranslation: " << t;
    }
private:
    size_t nt_ = 0, ns_ = 0;
    fgoicp_solver* s_ = nullptr;
};

}  // namespace icp
