// Driver-level C ABI: icp::FastGoICP (reference fgoicp/fgoicp.hpp:13-43) over the HIP operator
// context.  The driver template is instantiated with the HIP backend ONLY — there is no CPU
// backend in this library.
#include <cstddef>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/fgoicp_amd.h"
#include "../device/ctx.hpp"
#include "driver.hpp"
#include "segment.hpp"

namespace fgoicp {

struct HipOps {
    fgoicp_ctx* ctx = nullptr;
    int bounds_multi(int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4, float* lb,
                     float* ub, const float* cut_above) {
        return ctx_bounds_multi(ctx, G, R9, rot_span, fix_rot, offsets, tn4, lb, ub, cut_above);
    }
    int bounds_submit(int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4,
                      const int* twin, const float* cut_above) {
        return ctx_bounds_submit(ctx, slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, cut_above);
    }
    int bounds_submit_leaf(int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4,
                           const int* twin, const float* cut_above, const float* ub_below_span) {
        return ctx_bounds_submit(ctx, slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, cut_above, ub_below_span);
    }
    int bounds_collect(int slot, float* lb, float* ub) { return ctx_bounds_collect(ctx, slot, lb, ub); }
    bool async() const { return pipeline; }
    bool twins() const { return true; }
    int icp(const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        return ctx_icp(ctx, R0, t0, max_iter, thr, sse, R9, t3, iters);
    }
    // one ICP run executed by all ranks together (cooperative refinements of the sharded ROUND schedule)
    int icp_coop(int rank, int world, int (*gather)(void*, size_t, void*), void* user, const float* R0, const float* t0, size_t max_iter, float thr, float* sse,
                 float* R9, float* t3, int* iters) {
        return ctx_icp_coop(ctx, rank, world, gather, user, R0, t0, max_iter, thr, sse, R9, t3, iters);
    }
    // a refinement that runs next to the bounds work (late-joining ICP of the ROUND schedule): ICP lane 1, its own streams
    int icp_background(const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        return ctx_icp_lane(ctx, 1, R0, t0, max_iter, thr, sse, R9, t3, iters);
    }
    bool pipeline = [] { const char* e = dev_env("FGOICP_PIPELINE"); return e ? std::atoi(e) != 0 : true; }();  // tuning knob
};

// the host half of the information matrix (information.hpp)
void information_from_moments(uint64_t n, const double* sq_s, const double* sqq_s, const float* offset3, float scale, double* info36, double* sum_q3_out,
                                     double* sum_qq6_out) {
    const double N = (double)n, s = (double)scale;
    const double c[3] = {offset3 ? (double)offset3[0] : 0.0, offset3 ? (double)offset3[1] : 0.0, offset3 ? (double)offset3[2] : 0.0};
    double q[3], qq[6];
    static const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
    if (!offset3 && scale == 1.0f) {
        for (int k = 0; k < 3; ++k) q[k] = sq_s[k];
        for (int k = 0; k < 6; ++k) qq[k] = sqq_s[k];
    } else {
        for (int k = 0; k < 3; ++k) q[k] = sq_s[k] / s + N * c[k];
        for (int k = 0; k < 6; ++k) {
            const int a = A[k], b = B[k];
            qq[k] = sqq_s[k] / (s * s) + (c[a] * sq_s[b] + sq_s[a] * c[b]) / s + N * c[a] * c[b];
        }
    }
    if (sum_q3_out) std::memcpy(sum_q3_out, q, sizeof(q));
    if (sum_qq6_out) std::memcpy(sum_qq6_out, qq, sizeof(qq));
    if (!info36) return;
    const double xx = qq[0], xy = qq[1], xz = qq[2], yy = qq[3], yz = qq[4], zz = qq[5];
    const double M[6][6] = {{yy + zz, -xy, -xz, 0.0, -q[2], q[1]},
                            {-xy, xx + zz, -yz, q[2], 0.0, -q[0]},
                            {-xz, -yz, xx + yy, -q[1], q[0], 0.0},
                            {0.0, q[2], -q[1], N, 0.0, 0.0},
                            {-q[2], 0.0, q[0], 0.0, N, 0.0},
                            {q[1], -q[0], 0.0, 0.0, 0.0, N}};
    for (int r = 0; r < 6; ++r)
        for (int k = 0; k < 6; ++k) info36[6 * r + k] = M[r][k] + 0.0;  // + 0.0: no negative zeros in the matrix
}

}  // namespace fgoicp

using namespace fgoicp;

struct fgoicp_solver {
    // FastGoICP members in declaration order (fgoicp.hpp:47-58)
    std::vector<Vec3f> pcs, pct;
    size_t ns = 0, nt = 0;
    Vec3f offset_pcs{0, 0, 0}, offset_pct{0, 0, 0};
    float scaling_factor = 1.f;
    float bounds6[6] = {0, 0, 0, 0, 0, 0};
    fgoicp_ctx* ctx = nullptr;  // "registration"
    HipOps ops;
    std::unique_ptr<GoIcpDriver<HipOps>> driver;
    fgoicp_exchange ex{};
    bool has_ex = false;
    bool ran = false;  // a run() has succeeded: the driver holds a best transform (fgoicp_solver_alignment)
    ~fgoicp_solver() {  // the context goes with the solver however the solver goes (fgoicp_solver_destroy, a failed or throwing create)
        driver.reset();
        fgoicp_ctx_destroy(ctx);
    }
};

// The refinements from the best transform, behind each entry point's own refusals.  spec.scale and max_distance are in the caller's
// units: a residual of either model and a distance scale with the frame.  Missing normals are estimated from k neighbours (they are
// invariant under the solver's centring and uniform scale).  Result: fgoicp_plane_result_t or fgoicp_robust_result_t (refine_result).
// The plain loops report a failure of the loop itself under the context entry point's name, as they always have.
template <class Result>
static int solver_refine(fgoicp_solver* s, const char* where, RefineSpec spec, float max_distance, int k, size_t max_iter, float conv_thr, const char* type, Result* out) {
    return fgoicp::abi_guard(where, [&] {
        if (!s->ctx->normals_set) {
            const int rc = ctx_set_target_normals(s->ctx, nullptr, k);
            if (rc) return rc;
        }
        if (spec.model == FGOICP_MODEL_GICP && !s->ctx->src_normals_set) {
            const int rc = ctx_set_source_normals(s->ctx, nullptr, k);
            if (rc) return rc;
        }
        Mat3f R;
        Vec3f t;
        s->driver->best_transform(R, t);  // the normalised frame the search ran in, as fgoicp_solver_information
        const float t3[3] = {t.x, t.y, t.z};
        spec.scale = spec.scale > 0.0 ? spec.scale * (double)s->scaling_factor : 0.0;
        spec.max_dist2 = information_max_dist2(max_distance, s->scaling_factor);
        RefineEnd end;
        const int rc = refine_loop(s->ctx, R.m, t3, max_iter, conv_thr, spec, spec.weighted ? where : spec.model == FGOICP_MODEL_GICP ? "fgoicp_icp_gicp" : "fgoicp_icp_plane", &end);
        if (rc) return rc;
        Result full;
        refine_result(end, &full);
        const Mat3f Rr = Mat3f::from(full.R);
        const Vec3f ts{full.t[0], full.t[1], full.t[2]};
        const Vec3f tr = ts / s->scaling_factor + Rr * s->offset_pcs - s->offset_pct;  // restore_translation, fgoicp.hpp:87-90
        full.t[0] = tr.x; full.t[1] = tr.y; full.t[2] = tr.z;
        full.scaling_factor = s->scaling_factor;
        return plane_out(full, out, where, type);
    });
}

extern "C" {

static int solver_create_impl(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, float lut_resolution, float mse_threshold, const fgoicp_solver_opts* opts,
                              fgoicp_solver** out);
int fgoicp_solver_create(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, float lut_resolution, float mse_threshold,
                         const fgoicp_solver_opts* opts, fgoicp_solver** out) {
    if (!out) return FGOICP_ERR_INVALID_ARG;
    *out = nullptr;
    // (the solver under construction is held by a unique_ptr inside: an exception unwinds it, and its destructor frees the context)
    return fgoicp::abi_guard("fgoicp_solver_create", [&] { return solver_create_impl(tgt_xyz, nt, src_xyz, ns, lut_resolution, mse_threshold, opts, out); });
}
static int solver_create_impl(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, float lut_resolution, float mse_threshold, const fgoicp_solver_opts* opts,
                              fgoicp_solver** out) {
    if (!tgt_xyz || !src_xyz || nt == 0 || ns == 0 || !(lut_resolution > 0) || !(mse_threshold >= 0)) {
        set_error("fgoicp_solver_create: invalid argument");
        return FGOICP_ERR_INVALID_ARG;
    }
    fgoicp_solver_opts o{FGOICP_SCHEDULE_SERIAL, 1, 0u, 0, 0.0f};
    if (opts) o = *opts;
    auto s = std::make_unique<fgoicp_solver>();
    s->ns = ns;
    s->nt = nt;
    s->pcs.resize(ns);
    s->pct.resize(nt);
    std::memcpy(s->pcs.data(), src_xyz, sizeof(Vec3f) * ns);
    std::memcpy(s->pct.data(), tgt_xyz, sizeof(Vec3f) * nt);
    // member-initialiser order of the reference ctor (fgoicp.hpp:13-19)
    s->offset_pcs = center_point_cloud(s->pcs);
    s->offset_pct = center_point_cloud(s->pct);
    s->scaling_factor = scale_point_clouds(s->pct, s->pcs);
    point_cloud_ranges(s->pct, s->bounds6);
    int rc = fgoicp_ctx_create(reinterpret_cast<const float*>(s->pct.data()), nt, reinterpret_cast<const float*>(s->pcs.data()), ns,
                               s->bounds6, lut_resolution, o.device, trim_ctx_flags(o.ctx_flags, o.trim_fraction), &s->ctx);
    if (rc) return rc;
    s->ops.ctx = s->ctx;
    size_t n_thr = ns;  // sse_threshold = n * mse_threshold (fgoicp.hpp:23); over the inliers when trimming
    if (const size_t k = trim_inliers(ns, o.trim_fraction)) {
        rc = ctx_set_inliers(s->ctx, k);
        if (rc) return rc;
        n_thr = k;
    }
    s->driver.reset(new GoIcpDriver<HipOps>(s->ops, n_thr, mse_threshold, o.schedule, o.round_width));
    *out = s.release();
    return FGOICP_OK;
}

void fgoicp_solver_destroy(fgoicp_solver* s) {
    if (!s) return;
    delete s;
}

int fgoicp_solver_set_exchange(fgoicp_solver* s, const fgoicp_exchange* ex_in) {
    if (!s) return FGOICP_ERR_INVALID_ARG;
    Exchange e;
    if (ex_in) {
        // only the bytes the caller's struct has are read (struct_size, ABI 2): members it does not know stay NULL
        fgoicp_exchange x{};
        const size_t n = ex_in->struct_size;
        if (n < offsetof(fgoicp_exchange, user) + sizeof(void*) || n > 4096) { set_error("fgoicp_solver_set_exchange: set struct_size = sizeof(fgoicp_exchange)"); return FGOICP_ERR_INVALID_ARG; }
        std::memcpy(&x, ex_in, n < sizeof(x) ? n : sizeof(x));
        const fgoicp_exchange* ex = &x;
        if (ex->world_size < 1 || ex->rank < 0 || ex->rank >= ex->world_size || (ex->world_size > 1 && (!ex->allreduce_min || !ex->allgather))) {
            set_error("fgoicp_solver_set_exchange: invalid exchange");
            return FGOICP_ERR_INVALID_ARG;
        }
        s->ex = *ex;
        s->has_ex = true;
        e.rank = ex->rank;
        e.world = ex->world_size;
        e.allreduce_min = ex->allreduce_min;
        e.allgather = ex->allgather;
        e.user = ex->user;
        e.allgather_device = ex->allgather_device;
    } else {
        s->has_ex = false;
    }
    s->driver->set_exchange(e);
    return FGOICP_OK;
}

int fgoicp_solver_set_log(fgoicp_solver* s, fgoicp_log_fn cb, void* user) {
    if (!s) return FGOICP_ERR_INVALID_ARG;
    if (!cb) { s->driver->set_log(nullptr); return FGOICP_OK; }
    s->driver->set_log([s, cb, user](int event, float sse, const Mat3f& R, const Vec3f& t) {
        // the initial ICP's translation is printed as returned (fgoicp.cpp:17), the incumbent's restored (:87, fgoicp.hpp:87-90)
        const Vec3f tr = event == FGOICP_LOG_NEW_BEST ? t / s->scaling_factor + R * s->offset_pcs - s->offset_pct : t;
        const float t3[3] = {tr.x, tr.y, tr.z};
        cb(event, sse, R.m, t3, user);
    });
    return FGOICP_OK;
}

int fgoicp_solver_set_early_exit(fgoicp_solver* s, int on) {
    if (!s) return FGOICP_ERR_INVALID_ARG;
    s->driver->set_use_cut(on != 0);
    return FGOICP_OK;
}

static int solver_run_impl(fgoicp_solver* s, float* R_out9, float* t_out3);
int fgoicp_solver_run(fgoicp_solver* s, float* R_out9, float* t_out3) {
    if (!s || !R_out9 || !t_out3) return FGOICP_ERR_INVALID_ARG;
    return fgoicp::abi_guard("fgoicp_solver_run", [&] { return solver_run_impl(s, R_out9, t_out3); });  // the host driver allocates (queues, tick buffers)
}
static int solver_run_impl(fgoicp_solver* s, float* R_out9, float* t_out3) {
    int rc = s->driver->run();
    if (rc == kDriverExchangeFailed) set_error("fgoicp_solver_run: exchange callback failed");
    if (rc) return rc;
    s->ran = true;
    Mat3f R;
    Vec3f t;
    s->driver->best_transform(R, t);
    // restore_translation, fgoicp.hpp:87-90
    const Vec3f tr = t / s->scaling_factor + R * s->offset_pcs - s->offset_pct;
    std::memcpy(R_out9, R.m, sizeof(R.m));
    t_out3[0] = tr.x; t_out3[1] = tr.y; t_out3[2] = tr.z;
    return FGOICP_OK;
}

int fgoicp_solver_best_error(const fgoicp_solver* s, float* sse_out) {
    if (!s || !sse_out) return FGOICP_ERR_INVALID_ARG;
    *sse_out = s->driver->best_sse();
    return FGOICP_OK;
}

int fgoicp_solver_best_transform(const fgoicp_solver* s, float* R9, float* t3) {
    if (!s || !R9 || !t3) return FGOICP_ERR_INVALID_ARG;
    Mat3f R; Vec3f t;
    s->driver->best_transform(R, t);
    std::memcpy(R9, R.m, sizeof(R.m));
    t3[0] = t.x; t3[1] = t.y; t3[2] = t.z;
    return FGOICP_OK;
}

int fgoicp_solver_last_transform(const fgoicp_solver* s, float* R9, float* t3) {
    if (!s || !R9 || !t3) return FGOICP_ERR_INVALID_ARG;
    Mat3f R; Vec3f t;
    s->driver->last_transform(R, t);
    std::memcpy(R9, R.m, sizeof(R.m));
    t3[0] = t.x; t3[1] = t.y; t3[2] = t.z;
    return FGOICP_OK;
}

int fgoicp_solver_stats(const fgoicp_solver* s, fgoicp_run_stats* out) {
    if (!s || !out) return FGOICP_ERR_INVALID_ARG;
    const DriverStats& d = s->driver->stats();
    out->trans_cubes = d.trans_cubes; out->bounds_calls = d.bounds_calls; out->rot_cubes = d.rot_cubes;
    out->icp_runs = d.icp_runs; out->icp_iters = d.icp_iters; out->inner_bnb = d.inner_bnb; out->rounds = d.rounds;
    out->seconds_total = d.seconds_total; out->seconds_bnb = d.seconds_bnb; out->seconds_icp = d.seconds_icp; out->initial_icp_sse = d.initial_icp_sse;
    return FGOICP_OK;
}

int fgoicp_solver_alignment(fgoicp_solver* s, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns, uint8_t* target_hit_nt, fgoicp_alignment_summary* out) {
    if (!s) { set_error("fgoicp_solver_alignment: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!s->ran) { set_error("fgoicp_solver_alignment: fgoicp_solver_run has not succeeded yet: there is no best transform"); return FGOICP_ERR_INVALID_ARG; }
    if (out && (out->struct_size < sizeof(uint32_t) || out->struct_size > 4096)) { set_error("fgoicp_solver_alignment: set out->struct_size = sizeof(fgoicp_alignment_summary)"); return FGOICP_ERR_INVALID_ARG; }
    Mat3f R;
    Vec3f t;
    s->driver->best_transform(R, t);  // the normalised frame the search ran in (no restore_translation)
    const float t3[3] = {t.x, t.y, t.z};
    fgoicp_alignment_summary full{};
    const int rc = ctx_alignment(s->ctx, R.m, t3, corr_idx_ns, dist2_ns, inlier_ns, target_hit_nt, &full);
    if (rc) return rc;
    full.scaling_factor = s->scaling_factor;
    return alignment_summary_out(full, out, "fgoicp_solver_alignment");
}

int fgoicp_solver_information(fgoicp_solver* s, float max_distance, fgoicp_information_t* out) {
    if (!s) { set_error("fgoicp_solver_information: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!s->ran) { set_error("fgoicp_solver_information: fgoicp_solver_run has not succeeded yet: there is no best transform"); return FGOICP_ERR_INVALID_ARG; }
    if (!information_size_ok(out)) { set_error("fgoicp_solver_information: out must not be null and out->struct_size = sizeof(fgoicp_information_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(max_distance >= 0.0f)) { set_error("fgoicp_solver_information: max_distance must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    Mat3f R;
    Vec3f t;
    s->driver->best_transform(R, t);  // the normalised frame the search ran in, as fgoicp_solver_alignment
    const float t3[3] = {t.x, t.y, t.z};
    const float max_dist2 = information_max_dist2(max_distance, s->scaling_factor);
    InfoMoments m;
    const int rc = ctx_information(s->ctx, R.m, t3, max_dist2, &m);
    if (rc) return rc;
    const float c3[3] = {-s->offset_pct.x, -s->offset_pct.y, -s->offset_pct.z};  // the centroid that was subtracted: center_point_cloud returns minus it
    fgoicp_information_t full;
    information_fill(full, s->ns, m, c3, s->scaling_factor, max_dist2);
    return information_out(full, out, "fgoicp_solver_information");
}

// Given normals: the context call with the pointer (normals do not change under the solver's centring and uniform scale); solver_refine
// then estimates only the set that is still missing.
int fgoicp_solver_set_target_normals(fgoicp_solver* s, const float* normals_nt3) {
    if (!s) { set_error("fgoicp_solver_set_target_normals: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!normals_nt3) { set_error("fgoicp_solver_set_target_normals: the normals must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_solver_set_target_normals", [&] { return ctx_set_target_normals(s->ctx, normals_nt3, 0); });
}
int fgoicp_solver_set_source_normals(fgoicp_solver* s, const float* normals_ns3) {
    if (!s) { set_error("fgoicp_solver_set_source_normals: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!normals_ns3) { set_error("fgoicp_solver_set_source_normals: the normals must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_solver_set_source_normals", [&] { return ctx_set_source_normals(s->ctx, normals_ns3, 0); });
}

int fgoicp_solver_refine_plane(fgoicp_solver* s, int k, size_t max_iter, float conv_thr, float max_distance, fgoicp_plane_result_t* out) {
    if (!s) { set_error("fgoicp_solver_refine_plane: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!s->ran) { set_error("fgoicp_solver_refine_plane: fgoicp_solver_run has not succeeded yet: there is no best transform"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error("fgoicp_solver_refine_plane: out must not be null and out->struct_size = sizeof(fgoicp_plane_result_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(max_distance >= 0.0f)) { set_error("fgoicp_solver_refine_plane: max_distance must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    return solver_refine(s, "fgoicp_solver_refine_plane", RefineSpec{}, max_distance, k, max_iter, conv_thr, "fgoicp_plane_result_t", out);
}

int fgoicp_solver_refine_gicp(fgoicp_solver* s, int k, size_t max_iter, float conv_thr, float max_distance, double epsilon, fgoicp_plane_result_t* out) {
    if (!s) { set_error("fgoicp_solver_refine_gicp: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!s->ran) { set_error("fgoicp_solver_refine_gicp: fgoicp_solver_run has not succeeded yet: there is no best transform"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error("fgoicp_solver_refine_gicp: out must not be null and out->struct_size = sizeof(fgoicp_plane_result_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(max_distance >= 0.0f)) { set_error("fgoicp_solver_refine_gicp: max_distance must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    if (!gicp_epsilon_ok(epsilon)) { set_error("fgoicp_solver_refine_gicp: epsilon must be finite and lie in (0, 1]"); return FGOICP_ERR_INVALID_ARG; }
    RefineSpec spec;
    spec.model = FGOICP_MODEL_GICP; spec.epsilon = epsilon;
    return solver_refine(s, "fgoicp_solver_refine_gicp", spec, max_distance, k, max_iter, conv_thr, "fgoicp_plane_result_t", out);
}

int fgoicp_solver_refine_robust(fgoicp_solver* s, int model, int k, size_t max_iter, float conv_thr, float max_distance, double epsilon, int loss, double loss_scale,
                                fgoicp_robust_result_t* out) {
    if (!s) { set_error("fgoicp_solver_refine_robust: the solver must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!s->ran) { set_error("fgoicp_solver_refine_robust: fgoicp_solver_run has not succeeded yet: there is no best transform"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error("fgoicp_solver_refine_robust: out must not be null and out->struct_size = sizeof(fgoicp_robust_result_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(max_distance >= 0.0f)) { set_error("fgoicp_solver_refine_robust: max_distance must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_model_ok(model)) { set_error("fgoicp_solver_refine_robust: unknown model " + std::to_string(model) + " (0: point-to-plane, 1: Generalized ICP)"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_loss_ok(loss)) { set_error("fgoicp_solver_refine_robust: unknown loss " + std::to_string(loss)); return FGOICP_ERR_INVALID_ARG; }
    if (model == FGOICP_MODEL_GICP && !gicp_epsilon_ok(epsilon)) { set_error("fgoicp_solver_refine_robust: epsilon must be finite and lie in (0, 1]"); return FGOICP_ERR_INVALID_ARG; }
    if (!std::isfinite(loss_scale)) { set_error("fgoicp_solver_refine_robust: loss_scale must be finite (<= 0: estimated)"); return FGOICP_ERR_INVALID_ARG; }
    RefineSpec spec;
    spec.model = model; spec.epsilon = epsilon; spec.weighted = true; spec.loss = loss; spec.scale = loss_scale;
    return solver_refine(s, "fgoicp_solver_refine_robust", spec, max_distance, k, max_iter, conv_thr, "fgoicp_robust_result_t", out);
}

int fgoicp_robust_weight(int loss, double s, double scale, double* w) { return robust_weight_entry(loss, s, scale, w); }

int fgoicp_gicp_terms(const float* x3, const float* q3, const float* nq3, const float* np3, const float* R9, double epsilon, double* M6_or_NULL, double* v28_or_NULL) {
    return gicp_terms_entry(x3, q3, nq3, np3, R9, epsilon, M6_or_NULL, v28_or_NULL);
}

int fgoicp_plane_step_from_moments(uint64_t n, const double* m28, double* xi6, int* rank) {
    if (!m28 || !xi6 || !rank) { set_error("fgoicp_plane_step_from_moments: m28, xi6 and rank must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (n == 0) { set_error("fgoicp_plane_step_from_moments: n = 0: nothing was counted, there is no step"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_moments_finite(m28)) { set_error("fgoicp_plane_step_from_moments: a moment is not finite"); return FGOICP_ERR_INVALID_ARG; }
    plane_step(m28, xi6, rank);
    return FGOICP_OK;
}

int fgoicp_plane_apply_step(const float* R9, const float* t3, const double* xi6, float* R_out9, float* t_out3) {
    if (!R9 || !t3 || !xi6 || !R_out9 || !t_out3) { set_error("fgoicp_plane_apply_step: no argument may be null"); return FGOICP_ERR_INVALID_ARG; }
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(xi6[k])) { set_error("fgoicp_plane_apply_step: the step is not finite"); return FGOICP_ERR_INVALID_ARG; }
    Mat3f R;
    Vec3f t;
    plane_apply_step(Mat3f::from(R9), Vec3f{t3[0], t3[1], t3[2]}, xi6, R, t);
    std::memcpy(R_out9, R.m, sizeof(R.m));
    t_out3[0] = t.x; t_out3[1] = t.y; t_out3[2] = t.z;
    return FGOICP_OK;
}

int fgoicp_information_from_moments(uint64_t n, const double* sum_q3, const double* sum_qq6, const float* offset3, float scale, double* info36, double* sum_q3_out,
                                    double* sum_qq6_out) {
    if (!sum_q3 || !sum_qq6) { set_error("fgoicp_information_from_moments: sum_q3 and sum_qq6 must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!(scale > 0.0f) || !std::isfinite(scale)) { set_error("fgoicp_information_from_moments: scale must be a positive finite number"); return FGOICP_ERR_INVALID_ARG; }
    information_from_moments(n, sum_q3, sum_qq6, offset3, scale, info36, sum_q3_out, sum_qq6_out);
    return FGOICP_OK;
}

int fgoicp_segment_hypotheses(const float* xyz, size_t n, const uint32_t* candidates_or_NULL, size_t m, int iterations, uint64_t seed, int peel, uint32_t* sample_K3,
                              double* plane_K4, uint8_t* degenerate_K) {
    return abi_guard("fgoicp_segment_hypotheses",
                     [&] { return segment_hypotheses_entry(xyz, n, candidates_or_NULL, m, iterations, seed, peel, sample_K3, plane_K4, degenerate_K); });
}

int fgoicp_segment_fit_from_moments(uint64_t count, const double* pivot3, const double* sum_u3, const double* sum_uu6, const double* toward4_or_NULL, double* plane4) {
    return segment_fit_entry(count, pivot3, sum_u3, sum_uu6, toward4_or_NULL, plane4);
}

int fgoicp_solver_preproc(const fgoicp_solver* s, float* offs6, float* scale, float* bounds6) {
    if (!s) return FGOICP_ERR_INVALID_ARG;
    if (offs6) {
        offs6[0] = s->offset_pcs.x; offs6[1] = s->offset_pcs.y; offs6[2] = s->offset_pcs.z;
        offs6[3] = s->offset_pct.x; offs6[4] = s->offset_pct.y; offs6[5] = s->offset_pct.z;
    }
    if (scale) *scale = s->scaling_factor;
    if (bounds6) std::memcpy(bounds6, s->bounds6, sizeof(s->bounds6));
    return FGOICP_OK;
}

int fgoicp_cloud_stats(const float* xyz, size_t n, fgoicp_cloud_stats_t* out) {
    if (!out || (!xyz && n)) return FGOICP_ERR_INVALID_ARG;
    *out = fgoicp_cloud_stats_t{};
    out->n = n;
    if (n == 0) return FGOICP_OK;
    double sum[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) { out->min[k] = xyz[k]; out->max[k] = xyz[k]; }
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[3 * i + k];
            sum[k] += (double)v;
            out->min[k] = v < out->min[k] ? v : out->min[k];
            out->max[k] = v > out->max[k] ? v : out->max[k];
        }
    double c[3];
    for (int k = 0; k < 3; ++k) { c[k] = sum[k] / (double)n; out->centroid[k] = (float)c[k]; }
    double r2 = 0.0, mx = 0.0;
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const double d = (double)xyz[3 * i + k] - c[k];
            r2 += d * d;
            mx = std::fabs(d) > mx ? std::fabs(d) : mx;
        }
    out->max_abs_centred = (float)mx;
    out->rms_radius = (float)std::sqrt(r2 / (double)n);
    return FGOICP_OK;
}

fgoicp_ctx* fgoicp_solver_ctx(fgoicp_solver* s) { return s ? s->ctx : nullptr; }

}  // extern "C"
