// fgoicp_batch (include/fgoicp_amd.h): many registrations on one device.  The scheduler (batch.hpp) runs every live pair's unchanged
// driver on a host thread of its own; this file is its device backend — one fgoicp_ctx per live pair, the bounds of all pending requests
// in fused launches (kernels.hip, bounds_fused.hpp), the ICP runs advanced in lock-step so that they share each host turn-around.
// Trimmed pairs evaluate their rows into one e-row arena for the whole batch and select them there; their ICP runs are not stepped.
// The launcher (the thread that calls fgoicp_batch_run) is the only thread that touches the device.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <limits>
#include <vector>

#include "../../../include/fgoicp_amd.h"
#include "../device/ctx.hpp"
#include "batch.hpp"
#include "refined_pose.hpp"

namespace fgoicp {
namespace {

#define BCHK(expr)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_error(std::string("fgoicp_batch: " #expr ": ") + hipGetErrorString(e_));    \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;             \
        }                                                                                   \
    } while (0)

// pre-processing of one pair (fgoicp_solver_create, fgoicp.cpp:176-287)
struct PairHost {
    std::vector<Vec3f> pcs, pct;
    size_t ns = 0, nt = 0;
    Vec3f offset_pcs{0, 0, 0}, offset_pct{0, 0, 0};
    float scaling_factor = 1.f;
    float bounds6[6] = {0, 0, 0, 0, 0, 0};
    float lut_resolution = 0.f, mse_threshold = 0.f;
    float trim_fraction = 0.f;
    size_t inliers = 0;  // trim_inliers(ns, trim_fraction): 0 = untrimmed
};

// a finished pair's alignment report, kept on the host (fgoicp_batch_opts.alignment): 9 bytes per source point, 1 per target point
struct PairAlign {
    std::vector<uint32_t> corr;
    std::vector<float> d2;
    std::vector<uint8_t> inlier, hit;
    fgoicp_alignment_summary sum{};
    int rc = FGOICP_OK;
    std::string err;
    bool have = false;
};

// a finished pair's information moments, kept on the host (fgoicp_batch_opts.information): context frame, as the device left them
struct PairInfo {
    InfoMoments m;
    float max_dist2 = 0.f;
    int rc = FGOICP_OK;
    std::string err;
    bool have = false;
};

// how a pair is refined after its search (fgoicp_batch_refine_t, checked by fgoicp_batch_create); model < 0: not at all
struct PairRefineSpec {
    int model = -1, k = 16;
    size_t max_iter = 0;
    float conv_thr = 0.f, max_distance = 0.f;
    double epsilon = 1e-3;
    int loss = FGOICP_LOSS_NONE;
    double loss_scale = 0.0;
    bool weighted() const { return loss != FGOICP_LOSS_NONE; }
};
// a pair's refinement, kept on the host: the result as fgoicp_solver_refine_* fills it (one of the two), or the refinement's own status
// and message; the information matrix at the refined pose (fgoicp_batch_opts.information)
struct PairRefined {
    fgoicp_plane_result_t plane{};
    fgoicp_robust_result_t robust{};
    int rc = FGOICP_OK;
    std::string err;
    bool have = false;
    fgoicp_information_t info{};
    int info_rc = FGOICP_OK;
    std::string info_err;
    bool have_info = false;
};
// the spec of one evaluation in the context's frame, as solver_refine (solver.cpp) forms it
inline RefineSpec refine_ctx_spec(const PairRefineSpec& r, float scaling_factor) {
    RefineSpec spec;
    spec.model = r.model;
    spec.epsilon = r.epsilon;
    spec.weighted = r.weighted();
    spec.loss = r.loss;
    spec.scale = r.loss_scale > 0.0 ? r.loss_scale * (double)scaling_factor : 0.0;
    spec.max_dist2 = information_max_dist2(r.max_distance, scaling_factor);
    return spec;
}
// the name a refinement's messages carry: the robust loop's caller, the plain loops' context entry points (as solver_refine)
inline const char* refine_where(const RefineSpec& spec, const char* robust_caller) {
    return spec.weighted ? robust_caller : spec.model == FGOICP_MODEL_GICP ? "fgoicp_icp_gicp" : "fgoicp_icp_plane";
}

// work items per fused launch (one 64-thread block each): a class with more is split, so that blocks x threads stay inside the 32-bit
// grid size of a dispatch, with the margin the solo path keeps (ctx.hip, launch_fit)
constexpr size_t kFusedLaunchItems = (size_t)1 << 24;

// device staging of one class of work items (same LUT layout, addressing and quantisation; trimmed or not)
struct ItemClass {
    int layout = 0;
    bool wide = false, quant = false, trim = false;
    std::vector<uint2> items;
};
// the trimmed rows of a tick that share one fill of the arena: their items per class (indexed as the tick's classes), their rows
struct TrimSubTick {
    std::vector<std::vector<uint2>> items;
    size_t first_row = 0, rows = 0, floats = 0;
};

// Grow-only buffers on the device / in pinned host memory (hipHostMallocDefault: no device alias): the handle (owned.hpp) and the elements it holds
template <class T> hipError_t alloc_elems(Dev<T>& p, size_t n) { return p.alloc(n); }
template <class T> hipError_t alloc_elems(Mapped<T>& p, size_t n) { return p.alloc(n, hipHostMallocDefault); }
template <class Handle>
struct GrowBuf {
    Handle p;
    size_t cap = 0;
    int ensure(size_t n, bool exact = false) {
        if (n <= cap) return FGOICP_OK;
        cap = 0;
        const size_t want = exact ? n : n + n / 2 + 64;
        BCHK(alloc_elems(p, want));
        cap = want;
        return FGOICP_OK;
    }
};
template <class T> using DevBuf = GrowBuf<Dev<T>>;
template <class T> using PinBuf = GrowBuf<Mapped<T>>;

struct HipBatchBackend {
    std::vector<PairHost>* pairs = nullptr;
    int device = 0;
    unsigned ctx_flags = 0;
    std::vector<fgoicp_ctx*> ctx;
    bool borrowed = false;  // the test hooks: the contexts are the caller's (not destroyed here)
    std::vector<IcpStepRun> icp_state;
    std::vector<RefineStepRun> refine_state;   // one per pair: the refinement loop cut at its host wait (ctx.hpp)
    Stream stream;  // (declared ahead of the buffers: released after them)
    uint64_t bounds_launches = 0, icp_launches = 0, selection_launches = 0;
    uint64_t refine_launches = 0, refine_evaluations = 0;   // fused moment launches (one per class per tick) / evaluations (one per active loop per tick)
    const std::vector<PairRefineSpec>* rspec = nullptr;  // fgoicp_batch_opts_refine.refine (nullptr: no pair is refined)
    std::vector<PairRefined>* refined = nullptr;          // ... and where every refined pair's result is left
    bool want_refined_info = false;                       // fgoicp_batch_opts.information: the matrix at the refined pose too
    float refined_info_distance = 0.f;                    // callers' units, <= 0: no threshold (as the command-line tool takes it)
    // refinement tick staging: the views of every class next to each other, {count, sums} per view
    PinBuf<FusedRefineView> h_rviews;
    DevBuf<FusedRefineView> d_rviews;
    PinBuf<unsigned long long> h_rout;
    DevBuf<unsigned long long> d_rout;
    size_t last_lut_bytes = 0, last_lanes = 4;
    int next_pair = 0;            // the pair the scheduler admits next (room_for_more)
    std::vector<PairAlign>* align = nullptr;   // fgoicp_batch_opts.alignment: where finished() leaves every pair's report (nullptr: off)
    std::vector<PairInfo>* info = nullptr;     // fgoicp_batch_opts.information: ... and every pair's information moments (nullptr: off)
    float info_max_distance = 0.f;             // callers' units, > 0 (+inf: no threshold)
    // trimmed pairs: one grow-only arena of e-rows for the whole run (one fill per sub-tick), the solo formula's budget (trim_rows_budget)
    size_t arena_budget = 0;      // bytes; 0 = not set yet
    size_t arena_rows_max = 0;    // test hook: at most this many rows per fill (0: the budget decides)
    DevBuf<float> d_arena;
    PinBuf<FusedTrimRow> h_trows;
    DevBuf<FusedTrimRow> d_trows;
    // tick staging
    PinBuf<FusedPairView> h_views;
    PinBuf<FusedEval> h_evals;
    PinBuf<uint2> h_items;
    PinBuf<float> h_out;
    DevBuf<FusedPairView> d_views;
    DevBuf<FusedEval> d_evals;
    DevBuf<uint2> d_items;
    DevBuf<double2> d_partials;
    DevBuf<float> d_out;

    ~HipBatchBackend() {
        if (!borrowed)
            for (fgoicp_ctx*& c : ctx) { fgoicp_ctx_destroy(c); c = nullptr; }
    }
    int init() {
        if (hipSetDevice(device) != hipSuccess) { set_error("fgoicp_batch_run: no usable HIP device (there is no CPU path)"); return FGOICP_ERR_NO_DEVICE; }
        BCHK(stream.create(hipStreamNonBlocking));
        ctx.assign(pairs->size(), nullptr);
        icp_state.assign(pairs->size(), IcpStepRun());
        refine_state.assign(pairs->size(), RefineStepRun());
        for (const PairHost& p : *pairs)
            if (p.inliers) {  // the arena's budget is set aside before any pair enters (room_for_more)
                size_t free_b = 0, total_b = 0;
                BCHK(hipMemGetInfo(&free_b, &total_b));
                arena_budget = trim_rows_budget(free_b);
                break;
            }
        return FGOICP_OK;
    }
    // the test hooks: the caller's contexts as the live pairs (checked by the caller: one device, the packed LUT)
    int init_borrowed(fgoicp_ctx* const* cs, int n) {
        borrowed = true;
        ctx.assign(cs, cs + n);
        icp_state.assign((size_t)n, IcpStepRun());
        refine_state.assign((size_t)n, RefineStepRun());
        device = n > 0 ? cs[0]->device : 0;
        BCHK(hipSetDevice(device));
        BCHK(stream.create(hipStreamNonBlocking));
        return FGOICP_OK;
    }

    int admit(int i) {
        PairHost& p = (*pairs)[(size_t)i];
        fgoicp_ctx* c = nullptr;
        next_pair = i;
        int rc = fgoicp_ctx_create(reinterpret_cast<const float*>(p.pct.data()), p.nt, reinterpret_cast<const float*>(p.pcs.data()), p.ns, p.bounds6,
                                   p.lut_resolution, device, trim_ctx_flags(ctx_flags, p.trim_fraction), &c);
        if (rc == FGOICP_ERR_OOM) return kBatchNoRoom;  // the scheduler reports OOM itself when no other pair is live
        if (rc) { next_pair = i + 1; return rc; }
        if (p.inliers && (rc = ctx_set_inliers_batch(c, p.inliers))) {  // trimmed ICP's buffers; no slot e-rows (the arena)
            fgoicp_ctx_destroy(c);
            if (rc == FGOICP_ERR_OOM) return kBatchNoRoom;
            next_pair = i + 1;
            return rc;
        }
        next_pair = i + 1;
        if (!c->d_lut_zp) {  // the fused kernel reads the packed LUT copy
            fgoicp_ctx_destroy(c);
            set_error("fgoicp_batch_run: pair " + std::to_string(i) + " has no packed LUT");
            return FGOICP_ERR_INVALID_ARG;
        }
        ctx[(size_t)i] = c;
        last_lanes = c->lanes.size();
        fgoicp_ctx_info info{};
        info.struct_size = sizeof(info);
        if (fgoicp_ctx_get_info(c, &info) == FGOICP_OK) last_lut_bytes = info.lut_bytes;
        return FGOICP_OK;
    }
    // max_live = 0: another pair enters while the device has room for one more LUT the size of the last one created (and a quarter on top),
    // the trimmed ICP buffers of the next pair if it is trimmed, and what the arena may still grow by
    bool room_for_more(int /*live*/) {
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
        size_t need = last_lut_bytes + last_lut_bytes / 4 + ((size_t)256 << 20);
        if (next_pair < (int)pairs->size() && (*pairs)[(size_t)next_pair].inliers) need += trim_icp_bytes((*pairs)[(size_t)next_pair].ns, last_lanes);
        const size_t arena_b = sizeof(float) * d_arena.cap;
        if (arena_budget > arena_b) need += arena_budget - arena_b;
        return free_b > need;
    }
    // BatchScheduler's optional hook: the pair's driver has ended, its context is still there.  The report at the pair's best transform, as
    // fgoicp_solver_alignment takes it from a solver of that pair alone (ctx_alignment on the pair's own context: nothing is shared).
    void finished(int i, const BatchPairResult& r) {
        if ((!align && !info) || r.status || !ctx[(size_t)i]) return;
        const PairHost& p = (*pairs)[(size_t)i];
        const float t3[3] = {r.t.x, r.t.y, r.t.z};
        PairInfo* f = info ? &(*info)[(size_t)i] : nullptr;
        if (f) f->max_dist2 = information_max_dist2(info_max_distance, p.scaling_factor);  // as fgoicp_solver_information
        int rc;
        if (align) {
            PairAlign& a = (*align)[(size_t)i];
            a.corr.resize(p.ns); a.d2.resize(p.ns); a.inlier.resize(p.ns); a.hit.resize(p.nt);
            // both options on: one pass of the report's device half serves both
            rc = f ? ctx_alignment_information(ctx[(size_t)i], r.R.m, t3, a.corr.data(), a.d2.data(), a.inlier.data(), a.hit.data(), &a.sum, f->max_dist2, &f->m)
                   : ctx_alignment(ctx[(size_t)i], r.R.m, t3, a.corr.data(), a.d2.data(), a.inlier.data(), a.hit.data(), &a.sum);
            a.rc = rc;
            a.sum.scaling_factor = p.scaling_factor;
            a.have = a.rc == FGOICP_OK;
            if (a.rc) a.err = fgoicp_last_error();
        } else {
            rc = ctx_information(ctx[(size_t)i], r.R.m, t3, f->max_dist2, &f->m);
        }
        if (f) {
            f->rc = rc;
            f->have = rc == FGOICP_OK;
            if (rc) f->err = fgoicp_last_error();
        }
    }
    void release(int i) {
        (void)hipSetDevice(device);
        fgoicp_ctx_destroy(ctx[(size_t)i]);
        ctx[(size_t)i] = nullptr;
    }

    // One tick: every row of every request.  Untrimmed rows: one launch per item class (more for a class above kFusedLaunchItems), one
    // finalize.  Trimmed rows: laid out in the arena in request order, in sub-ticks of what one fill holds; per sub-tick one launch per
    // class (split alike) writes the rows' e, then one selection launch reduces them.
    int bounds(std::vector<BatchBoundsReq*>& reqs) {
        BCHK(hipSetDevice(device));
        // views: one per pair that has a request
        std::vector<int> view_of(ctx.size(), -1);
        std::vector<int> view_pair;
        size_t nu = 0, nt = 0;  // untrimmed / trimmed rows
        for (BatchBoundsReq* r : reqs) {
            if (view_of[(size_t)r->pair] < 0) { view_of[(size_t)r->pair] = (int)view_pair.size(); view_pair.push_back(r->pair); }
            (ctx[(size_t)r->pair]->inliers ? nt : nu) += (size_t)r->offsets[(size_t)r->G];
        }
        const size_t nevals = nu + nt;
        if (nevals == 0) return FGOICP_OK;
        int rc;
        if ((rc = h_views.ensure(view_pair.size())) || (rc = h_evals.ensure(nevals)) || (rc = h_out.ensure(2 * nevals)) || (rc = d_views.ensure(view_pair.size())) ||
            (rc = d_evals.ensure(nevals)) || (rc = d_out.ensure(2 * nevals)) || (nt && ((rc = h_trows.ensure(nt)) || (rc = d_trows.ensure(nt)))))
            return rc;
        std::vector<ItemClass> classes;
        std::vector<int> class_of_view(view_pair.size());
        for (size_t v = 0; v < view_pair.size(); ++v) {
            const fgoicp_ctx* c = ctx[(size_t)view_pair[v]];
            FusedPairView& pv = h_views.p[v];
            pv.src = c->d_src;
            pv.lutp = reinterpret_cast<const char*>(c->d_lut_zp.get());
            pv.g = c->geom;
            pv.ns = (int)c->ns;
            pv.chunk_pts = c->chunk_pts;
            const bool wide = bounds_lut_wide(c->geom, c->lut_layout), quant = c->geom.quantize != 0, trim = c->inliers != 0;
            int k = 0;
            while (k < (int)classes.size() && !(classes[(size_t)k].layout == c->lut_layout && classes[(size_t)k].wide == wide && classes[(size_t)k].quant == quant &&
                                                 classes[(size_t)k].trim == trim))
                ++k;
            if (k == (int)classes.size()) {
                classes.emplace_back();
                classes.back().layout = c->lut_layout; classes.back().wide = wide; classes.back().quant = quant; classes.back().trim = trim;
            }
            class_of_view[v] = k;
        }
        if (nt && !arena_budget) {  // (the test hooks: set at the first trimmed tick)
            size_t free_b = 0, total_b = 0;
            BCHK(hipMemGetInfo(&free_b, &total_b));
            arena_budget = trim_rows_budget(free_b);
        }
        const size_t arena_floats = arena_budget / sizeof(float);
        // evaluations in request order, the untrimmed ones [0, nu), the trimmed ones [nu, nevals); their chunks as work items of their
        // pair's class, the trimmed ones per sub-tick
        std::vector<TrimSubTick> subs;
        size_t eu = 0, et = nu, partials = 0;
        for (BatchBoundsReq* r : reqs) {
            const int v = view_of[(size_t)r->pair];
            const fgoicp_ctx* c = ctx[(size_t)r->pair];
            const bool trim = c->inliers != 0;
            const int cls = class_of_view[(size_t)v];
            for (int g = 0; g < r->G; ++g) {
                const float half_angle = r->spans[(size_t)g] * kSqrt3 * kPi / 2.0f;  // registration.cu:42, as the context's window packing computes it
                const float sin_half = std::sin(half_angle);
                for (int i = r->offsets[(size_t)g]; i < r->offsets[(size_t)g + 1]; ++i) {
                    const size_t e = trim ? et++ : eu++;
                    FusedEval& fe = h_evals.p[e];
                    std::memcpy(fe.R, &r->R9[9 * (size_t)g], sizeof(fe.R));
                    fe.sin_half = sin_half;
                    fe.tx = r->tn4[4 * (size_t)i]; fe.ty = r->tn4[4 * (size_t)i + 1]; fe.tz = r->tn4[4 * (size_t)i + 2]; fe.span = r->tn4[4 * (size_t)i + 3];
                    fe.fix_rot = r->fix[(size_t)g] ? 1 : 0;
                    fe.pair = v;
                    fe.nchunk = c->nchunk1;
                    if (!trim) {
                        fe.samp_shift = 0;
                        fe.partial_base = partials;
                        std::vector<uint2>& items = classes[(size_t)cls].items;
                        for (int ch = 0; ch < c->nchunk1; ++ch) items.push_back(make_uint2((unsigned)e, (unsigned)ch));
                        partials += (size_t)c->nchunk1;
                        continue;
                    }
                    // a new fill of the arena when this row would not fit (a row larger than the whole budget gets a fill of its own)
                    if (subs.empty() || (subs.back().rows > 0 && ((arena_rows_max && subs.back().rows >= arena_rows_max) || subs.back().floats + c->erow > arena_floats))) {
                        subs.emplace_back();
                        subs.back().items.resize(classes.size());
                        subs.back().first_row = e - nu;
                    }
                    TrimSubTick& st = subs.back();
                    fe.samp_shift = c->trim_samp_shift;
                    fe.row_off = st.floats;
                    FusedTrimRow& tr = h_trows.p[e - nu];
                    tr.row = nullptr;  // (the arena's address is known once it has grown: below)
                    tr.n = (int)c->ns;
                    tr.k = (int)c->inliers;
                    tr.samp_shift = c->trim_samp_shift;
                    tr.margin = c->trim_margin;
                    tr.span = fe.span;
                    tr.out = (int)e;
                    for (int ch = 0; ch < c->nchunk1; ++ch) st.items[(size_t)cls].push_back(make_uint2((unsigned)e, (unsigned)ch));
                    st.floats += c->erow;
                    st.rows++;
                }
            }
        }
        size_t fill = 0, nitems = 0;
        for (const TrimSubTick& st : subs) {
            fill = std::max(fill, st.floats);
            for (const std::vector<uint2>& it : st.items) nitems += it.size();
        }
        for (const ItemClass& cl : classes) nitems += cl.items.size();
        if ((rc = h_items.ensure(nitems)) || (rc = d_items.ensure(nitems)) || (rc = d_partials.ensure(partials)) || (fill && (rc = d_arena.ensure(fill, true)))) return rc;
        for (const TrimSubTick& st : subs)
            for (size_t q = st.first_row; q < st.first_row + st.rows; ++q) h_trows.p[q].row = d_arena.p + h_evals.p[nu + q].row_off;
        size_t pos = 0;
        for (const ItemClass& cl : classes) { std::memcpy(h_items.p + pos, cl.items.data(), sizeof(uint2) * cl.items.size()); pos += cl.items.size(); }
        for (const TrimSubTick& st : subs)
            for (const std::vector<uint2>& it : st.items) { std::memcpy(h_items.p + pos, it.data(), sizeof(uint2) * it.size()); pos += it.size(); }
        BCHK(hipMemcpyAsync(d_views.p, h_views.p, sizeof(FusedPairView) * view_pair.size(), hipMemcpyHostToDevice, stream));
        BCHK(hipMemcpyAsync(d_evals.p, h_evals.p, sizeof(FusedEval) * nevals, hipMemcpyHostToDevice, stream));
        BCHK(hipMemcpyAsync(d_items.p, h_items.p, sizeof(uint2) * nitems, hipMemcpyHostToDevice, stream));
        if (nt) BCHK(hipMemcpyAsync(d_trows.p, h_trows.p, sizeof(FusedTrimRow) * nt, hipMemcpyHostToDevice, stream));
        pos = 0;
        for (const ItemClass& cl : classes) {  // one launch per class, split where it would not fit the 32-bit grid
            for (size_t first = 0; first < cl.items.size(); first += kFusedLaunchItems) {
                const size_t n = std::min(kFusedLaunchItems, cl.items.size() - first);
                launch_fused_bounds(cl.layout, cl.wide, cl.quant, d_views.p, d_evals.p, d_items.p + pos + first, (unsigned)n, d_partials.p, stream);
                ++bounds_launches;
            }
            pos += cl.items.size();
        }
        if (nu) launch_fused_finalize(d_evals.p, (int)nu, d_partials.p, d_out.p, d_out.p + nevals, stream);
        for (const TrimSubTick& st : subs) {  // one fill of the arena after the other, on the one stream
            for (size_t k = 0; k < classes.size(); ++k) {
                const ItemClass& cl = classes[k];
                const std::vector<uint2>& it = st.items[k];
                for (size_t first = 0; first < it.size(); first += kFusedLaunchItems) {
                    const size_t n = std::min(kFusedLaunchItems, it.size() - first);
                    launch_fused_trim_bounds(cl.layout, cl.wide, cl.quant, d_views.p, d_evals.p, d_items.p + pos + first, (unsigned)n, d_arena.p, stream);
                    ++bounds_launches;
                }
                pos += it.size();
            }
            launch_fused_trim_select(d_trows.p + st.first_row, (int)st.rows, d_out.p + nevals, d_out.p, stream);
            ++selection_launches;
        }
        BCHK(hipGetLastError());
        BCHK(hipMemcpyAsync(h_out.p, d_out.p, sizeof(float) * 2 * nevals, hipMemcpyDeviceToHost, stream));
        BCHK(hipStreamSynchronize(stream));
        eu = 0;
        et = nu;
        for (BatchBoundsReq* r : reqs) {
            const size_t n = (size_t)r->offsets[(size_t)r->G];
            size_t& e = ctx[(size_t)r->pair]->inliers ? et : eu;
            std::memcpy(r->lb.data(), h_out.p + e, sizeof(float) * n);
            std::memcpy(r->ub.data(), h_out.p + nevals + e, sizeof(float) * n);
            e += n;
        }
        return FGOICP_OK;
    }

    int icp_start(BatchIcpReq& r) {
        fgoicp_ctx* c = ctx[(size_t)r.pair];
        if (!ctx_icp_steppable(c)) {  // large clouds, brute-force contexts: the context's own loop, at once
            const int rc = ctx_icp(c, r.R0, r.t0, r.max_iter, r.thr, &r.sse, r.R, r.t, &r.iters);
            r.done = true;
            return rc;
        }
        return ctx_icp_step_begin(c, icp_state[(size_t)r.pair], r.R0, r.t0, r.max_iter, r.thr);
    }
    int icp_step(std::vector<BatchIcpReq*>& runs) {
        for (BatchIcpReq* r : runs) BCHK(hipStreamSynchronize(ctx[(size_t)r->pair]->stream));
        for (BatchIcpReq* r : runs) {
            IcpStepRun& s = icp_state[(size_t)r->pair];
            const int rc = ctx_icp_step(ctx[(size_t)r->pair], s);
            if (rc) return rc;
            if (s.done) {
                s.loop.result(&r->sse, r->R, r->t, &r->iters);
                r->done = true;
            }
        }
        ++icp_launches;
        return FGOICP_OK;
    }

    // One refinement tick over the runs `idx` (indices into ctx / refine_state), each advanced by ONE evaluation:
    //   1. every run's device half on its own context's stream, an event behind it;  2. the batch stream waits for the events;
    //   3. one fused moments launch (and its folds) per class present, at most kFusedRefineMax views each;  4. one copy of all outputs to
    //   pinned memory;  5. one wait;  6. every run's host step.
    // done[k]: run k's loop has ended; run_rc[k] != 0: it failed in its host step (the normal equations are not finite), with run_err[k].
    // The return value is a device failure: the tick's, not one run's.
    int refine_tick(const std::vector<int>& idx, std::vector<char>& done, std::vector<int>& run_rc, std::vector<std::string>& run_err) {
        const size_t n = idx.size();
        done.assign(n, 0);
        run_rc.assign(n, FGOICP_OK);
        run_err.assign(n, std::string());
        if (n == 0) return FGOICP_OK;
        BCHK(hipSetDevice(device));
        int rc;
        if ((rc = h_rviews.ensure(n)) || (rc = d_rviews.ensure(n)) || (rc = h_rout.ensure(kFusedRefineOut * n)) || (rc = d_rout.ensure(kFusedRefineOut * n))) return rc;
        std::vector<FusedRefineView> views(n);
        for (size_t k = 0; k < n; ++k)
            if ((rc = ctx_refine_step_enqueue(ctx[(size_t)idx[k]], refine_state[(size_t)idx[k]], &views[k]))) return rc;
        for (size_t k = 0; k < n; ++k) BCHK(hipStreamWaitEvent(stream, ctx[(size_t)idx[k]]->refine_ready, 0));
        // the table: class after class (model x weighted), the runs of a class in the order given; a launch takes up to kFusedRefineMax of them
        std::vector<size_t> slot_of(n);
        struct Launch { bool gicp, weighted; size_t first, count; int blocks; };
        std::vector<Launch> launches;
        size_t pos = 0;
        for (int cls = 0; cls < 4; ++cls) {
            const bool gicp = (cls & 1) != 0, weighted = (cls & 2) != 0;
            for (size_t k = 0; k < n; ++k) {
                const RefineSpec& sp = refine_state[(size_t)idx[k]].end.spec;
                if ((sp.model == FGOICP_MODEL_GICP) != gicp || sp.weighted != weighted) continue;
                if (launches.empty() || launches.back().gicp != gicp || launches.back().weighted != weighted || launches.back().count == (size_t)kFusedRefineMax)
                    launches.push_back(Launch{gicp, weighted, pos, 0, 0});
                Launch& l = launches.back();
                views[k].first_block = l.blocks;
                l.blocks += views[k].nblocks;
                ++l.count;
                h_rviews.p[pos] = views[k];
                slot_of[k] = pos++;
            }
        }
        BCHK(hipMemcpyAsync(d_rviews.p, h_rviews.p, sizeof(FusedRefineView) * n, hipMemcpyHostToDevice, stream));
        for (const Launch& l : launches) {
            launch_fused_refine_moments(l.gicp, l.weighted, d_rviews.p + l.first, (int)l.count, l.blocks, d_rout.p + (size_t)kFusedRefineOut * l.first, stream);
            ++refine_launches;
        }
        BCHK(hipGetLastError());
        BCHK(hipMemcpyAsync(h_rout.p, d_rout.p, sizeof(unsigned long long) * kFusedRefineOut * n, hipMemcpyDeviceToHost, stream));
        BCHK(hipStreamSynchronize(stream));  // covers every run's own stream up to its event: the report's sse is in pinned memory
        for (size_t k = 0; k < n; ++k) {
            RefineStepRun& s = refine_state[(size_t)idx[k]];
            run_rc[k] = ctx_refine_step(ctx[(size_t)idx[k]], s, h_rout.p + (size_t)kFusedRefineOut * slot_of[k]);
            if (run_rc[k]) run_err[k] = fgoicp_last_error();
            done[k] = run_rc[k] || s.done;
            ++refine_evaluations;
        }
        return FGOICP_OK;
    }

    // BatchScheduler's optional refinement hooks (BackendHasRefine)
    bool refines(int i) const { return rspec && (*rspec)[(size_t)i].model >= 0; }
    // the refinement itself was refused or failed: kept for the pair's getter; the pair's search result and status stay as they are
    void refine_failed(int i, int rc, const std::string& err) {
        PairRefined& o = (*refined)[(size_t)i];
        o.rc = rc;
        o.err = err;
        o.have = false;
    }
    int refine_start(int i, const BatchPairResult& r, bool* done) {
        const PairHost& p = (*pairs)[(size_t)i];
        const PairRefineSpec& q = (*rspec)[(size_t)i];
        const RefineSpec spec = refine_ctx_spec(q, p.scaling_factor);
        const float t3[3] = {r.t.x, r.t.y, r.t.z};  // the normalised frame the search ran in
        const int rc = ctx_refine_step_begin(ctx[(size_t)i], refine_state[(size_t)i], r.R.m, t3, q.max_iter, q.conv_thr, spec, refine_where(spec, "fgoicp_solver_refine_robust"), q.k);
        *done = rc != 0;
        if (rc == FGOICP_ERR_HIP) return rc;
        if (rc) refine_failed(i, rc, fgoicp_last_error());
        return FGOICP_OK;
    }
    // the loop has ended: the result as solver_refine (solver.cpp) hands it out, then the information matrix at that pose
    template <class Result>
    void refine_restore(const PairHost& p, const RefineEnd& end, Result* full) {
        refine_result(end, full);
        const Mat3f Rr = Mat3f::from(full->R);
        const Vec3f ts{full->t[0], full->t[1], full->t[2]};
        const Vec3f tr = ts / p.scaling_factor + Rr * p.offset_pcs - p.offset_pct;  // restore_translation, fgoicp.hpp:87-90
        full->t[0] = tr.x; full->t[1] = tr.y; full->t[2] = tr.z;
        full->scaling_factor = p.scaling_factor;
    }
    void refine_finish(int i) {
        const PairHost& p = (*pairs)[(size_t)i];
        const RefineEnd& end = refine_state[(size_t)i].end;
        PairRefined& o = (*refined)[(size_t)i];
        const float *R9, *t3;
        if (end.spec.weighted) { refine_restore(p, end, &o.robust); R9 = o.robust.R; t3 = o.robust.t; }
        else { refine_restore(p, end, &o.plane); R9 = o.plane.R; t3 = o.plane.t; }
        o.have = true;
        if (!want_refined_info) return;
        const float offs[6] = {p.offset_pcs.x, p.offset_pcs.y, p.offset_pcs.z, p.offset_pct.x, p.offset_pct.y, p.offset_pct.z};
        std::memset(&o.info, 0, sizeof(o.info));
        o.info.struct_size = (uint32_t)sizeof(o.info);
        o.info_rc = refined_information(ctx[(size_t)i], R9, t3, offs, p.scaling_factor, refined_info_distance, &o.info);
        o.have_info = o.info_rc == FGOICP_OK;
        if (o.info_rc) o.info_err = fgoicp_last_error();
    }
    int refine_step(const std::vector<int>& active, std::vector<char>& done) {
        std::vector<int> run_rc;
        std::vector<std::string> run_err;
        const int rc = refine_tick(active, done, run_rc, run_err);
        if (rc) return rc;
        for (size_t k = 0; k < active.size(); ++k) {
            if (run_rc[k]) refine_failed(active[k], run_rc[k], run_err[k]);
            else if (done[k]) refine_finish(active[k]);
        }
        return FGOICP_OK;
    }
};

}  // namespace
}  // namespace fgoicp

using namespace fgoicp;

struct fgoicp_batch {
    std::vector<PairHost> pairs;
    fgoicp_batch_opts opts{};
    std::vector<BatchPairResult> results;
    std::vector<int> status;
    uint64_t bounds_launches = 0, icp_launches = 0;
    bool ran = false;
    std::vector<PairAlign> align;  // opts.alignment: one per pair
    std::vector<PairInfo> info;    // opts.information: one per pair
    std::vector<PairRefineSpec> rspec;   // opts.refine: one per pair (empty: none)
    std::vector<PairRefined> refined;    // ... and what the last run left
    uint64_t refine_launches = 0, refine_evaluations = 0;
};

// one fgoicp_batch_refine_t entry, refused as the solo entry points refuse their arguments; `who` names the pair
static int refine_entry_check(const fgoicp_batch_refine_t& q, const std::string& who, PairRefineSpec* out) {
    if (q.struct_size < sizeof(fgoicp_batch_refine_t) || q.struct_size > 4096) { set_error(who + ": set struct_size = sizeof(fgoicp_batch_refine_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (q.model == -1) { *out = PairRefineSpec(); return FGOICP_OK; }
    if (!robust_model_ok(q.model)) { set_error(who + ": unknown model " + std::to_string(q.model) + " (-1: not refined, 0: point-to-plane, 1: Generalized ICP)"); return FGOICP_ERR_INVALID_ARG; }
    if (q.k < kKnnMin || q.k > kKnnMax) { set_error(who + ": k must lie in [4, 32]"); return FGOICP_ERR_INVALID_ARG; }
    if (!(q.max_distance >= 0.0f)) { set_error(who + ": max_distance must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_loss_ok(q.loss)) { set_error(who + ": unknown loss " + std::to_string(q.loss)); return FGOICP_ERR_INVALID_ARG; }
    if (q.model == FGOICP_MODEL_GICP && !gicp_epsilon_ok(q.epsilon)) { set_error(who + ": epsilon must be finite and lie in (0, 1]"); return FGOICP_ERR_INVALID_ARG; }
    if (!std::isfinite(q.loss_scale)) { set_error(who + ": loss_scale must be finite (<= 0: estimated)"); return FGOICP_ERR_INVALID_ARG; }
    out->model = q.model; out->k = q.k; out->max_iter = q.max_iter; out->conv_thr = q.conv_thr; out->max_distance = q.max_distance;
    out->epsilon = q.epsilon; out->loss = q.loss; out->loss_scale = q.loss_scale;
    return FGOICP_OK;
}

extern "C" {

static int batch_create_impl(const fgoicp_batch_pair* pairs, int n, const fgoicp_batch_opts* opts, fgoicp_batch** out) {
    if (!pairs || n <= 0 || !opts) { set_error("fgoicp_batch_create: invalid argument"); return FGOICP_ERR_INVALID_ARG; }
    const size_t sz = opts->struct_size;
    if (sz < offsetof(fgoicp_batch_opts, solver) + sizeof(fgoicp_solver_opts) || sz > 4096) {
        set_error("fgoicp_batch_create: set struct_size = sizeof(fgoicp_batch_opts)");
        return FGOICP_ERR_INVALID_ARG;
    }
    auto b = std::make_unique<fgoicp_batch>();
    static_assert(offsetof(fgoicp_batch_opts_refine, refine) == sizeof(fgoicp_batch_opts), "the refine table lies right behind the options as published");
    fgoicp_batch_opts_refine full{};
    std::memcpy(&full, opts, sz < sizeof(full) ? sz : sizeof(full));  // members beyond the caller's struct stay 0
    b->opts = full.opts;
    b->opts.struct_size = sizeof(b->opts);
    if (b->opts.solver.trim_fraction != 0.0f) {
        set_error("fgoicp_batch_create: solver.trim_fraction must be 0 (trimming is per pair: fgoicp_batch_opts.trim_fractions)");
        return FGOICP_ERR_INVALID_ARG;
    }
    if (b->opts.max_live < 0) { set_error("fgoicp_batch_create: max_live < 0"); return FGOICP_ERR_INVALID_ARG; }
    if (b->opts.information && b->opts.information_max_distance != b->opts.information_max_distance) {
        set_error("fgoicp_batch_create: information_max_distance is NaN");
        return FGOICP_ERR_INVALID_ARG;
    }
    const float* trim = b->opts.trim_fractions;
    b->opts.trim_fractions = nullptr;  // read here only
    const fgoicp_batch_refine_t* refine = full.refine;  // read here only
    if (refine) {
        b->rspec.resize((size_t)n);
        for (int i = 0; i < n; ++i)
            if (int rc = refine_entry_check(refine[i], "fgoicp_batch_create: refine[" + std::to_string(i) + "] (pair " + std::to_string(i) + ")", &b->rspec[(size_t)i])) return rc;
    }
    for (int i = 0; trim && i < n; ++i)
        if (!(trim[i] >= 0.0f && trim[i] < 1.0f)) { set_error("fgoicp_batch_create: trim_fractions[" + std::to_string(i) + "] is not in [0, 1)"); return FGOICP_ERR_INVALID_ARG; }
    b->pairs.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const fgoicp_batch_pair& q = pairs[i];
        if (!q.tgt_xyz || !q.src_xyz || q.nt == 0 || q.ns == 0 || !(q.lut_resolution > 0) || !(q.mse_threshold >= 0)) {
            set_error("fgoicp_batch_create: invalid pair " + std::to_string(i));
            return FGOICP_ERR_INVALID_ARG;
        }
        PairHost& p = b->pairs[(size_t)i];
        p.ns = q.ns;
        p.nt = q.nt;
        p.pcs.resize(q.ns);
        p.pct.resize(q.nt);
        std::memcpy(p.pcs.data(), q.src_xyz, sizeof(Vec3f) * q.ns);
        std::memcpy(p.pct.data(), q.tgt_xyz, sizeof(Vec3f) * q.nt);
        // member-initialiser order of the reference ctor (fgoicp.hpp:13-19), as fgoicp_solver_create
        p.offset_pcs = center_point_cloud(p.pcs);
        p.offset_pct = center_point_cloud(p.pct);
        p.scaling_factor = scale_point_clouds(p.pct, p.pcs);
        point_cloud_ranges(p.pct, p.bounds6);
        p.lut_resolution = q.lut_resolution;
        p.mse_threshold = q.mse_threshold;
        p.trim_fraction = trim ? trim[i] : 0.0f;
        p.inliers = trim_inliers(p.ns, p.trim_fraction);  // as fgoicp_solver_create
    }
    b->results.assign((size_t)n, BatchPairResult());
    b->status.assign((size_t)n, FGOICP_OK);
    *out = b.release();
    return FGOICP_OK;
}
int fgoicp_batch_create(const fgoicp_batch_pair* pairs, int n, const fgoicp_batch_opts* opts, fgoicp_batch** out) {
    if (!out) return FGOICP_ERR_INVALID_ARG;
    *out = nullptr;
    return fgoicp::abi_guard("fgoicp_batch_create", [&] { return batch_create_impl(pairs, n, opts, out); });
}

void fgoicp_batch_destroy(fgoicp_batch* b) { delete b; }

static int batch_run_impl(fgoicp_batch* b, float* R_out9n, float* t_out3n, int* status_n) {
    const int n = (int)b->pairs.size();
    HipBatchBackend be;
    be.pairs = &b->pairs;
    be.device = b->opts.solver.device;
    be.ctx_flags = b->opts.solver.ctx_flags;
    if (b->opts.alignment) {
        b->align.assign((size_t)n, PairAlign());
        be.align = &b->align;
    }
    if (b->opts.information) {
        b->info.assign((size_t)n, PairInfo());
        be.info = &b->info;
        be.info_max_distance = b->opts.information_max_distance > 0.0f ? b->opts.information_max_distance : std::numeric_limits<float>::infinity();
    }
    if (!b->rspec.empty()) {
        b->refined.assign((size_t)n, PairRefined());
        be.rspec = &b->rspec;
        be.refined = &b->refined;
        be.want_refined_info = b->opts.information != 0;
        be.refined_info_distance = b->opts.information_max_distance;
    }
    int rc = be.init();
    if (rc) return rc;
    std::vector<BatchPairSpec> specs((size_t)n);
    for (int i = 0; i < n; ++i) {  // sse_threshold over the inliers when trimming, as fgoicp_solver_create
        const PairHost& p = b->pairs[(size_t)i];
        specs[(size_t)i].n_thr = p.inliers ? p.inliers : p.ns;
        specs[(size_t)i].mse_threshold = p.mse_threshold;
    }
    {
        BatchScheduler<HipBatchBackend> sched(be, specs, b->opts.solver.schedule, b->opts.solver.round_width, b->opts.max_live);
        rc = sched.run();
        if (rc) return rc;
        for (int i = 0; i < n; ++i) {
            b->results[(size_t)i] = sched.result(i);
            b->status[(size_t)i] = sched.result(i).status;
        }
    }
    b->bounds_launches = be.bounds_launches;
    b->icp_launches = be.icp_launches;
    b->refine_launches = be.refine_launches;
    b->refine_evaluations = be.refine_evaluations;
    b->ran = true;
    for (int i = 0; i < n; ++i) {
        const BatchPairResult& r = b->results[(size_t)i];
        const PairHost& p = b->pairs[(size_t)i];
        if (status_n) status_n[i] = b->status[(size_t)i];
        if (b->status[(size_t)i]) continue;
        const Vec3f tr = r.t / p.scaling_factor + r.R * p.offset_pcs - p.offset_pct;  // restore_translation, fgoicp.hpp:87-90
        if (R_out9n) std::memcpy(R_out9n + 9 * (size_t)i, r.R.m, sizeof(r.R.m));
        if (t_out3n) { t_out3n[3 * (size_t)i] = tr.x; t_out3n[3 * (size_t)i + 1] = tr.y; t_out3n[3 * (size_t)i + 2] = tr.z; }
    }
    return FGOICP_OK;
}
int fgoicp_batch_run(fgoicp_batch* b, float* R_out9n, float* t_out3n, int* status_n) {
    if (!b) return FGOICP_ERR_INVALID_ARG;
    return fgoicp::abi_guard("fgoicp_batch_run", [&] { return batch_run_impl(b, R_out9n, t_out3n, status_n); });
}

int fgoicp_batch_best_error(const fgoicp_batch* b, int i, float* sse_out) {
    if (!b || !sse_out || i < 0 || i >= (int)b->pairs.size() || !b->ran || b->status[(size_t)i]) return FGOICP_ERR_INVALID_ARG;
    *sse_out = b->results[(size_t)i].best_sse;
    return FGOICP_OK;
}

int fgoicp_batch_stats(const fgoicp_batch* b, int i, fgoicp_run_stats* out) {
    if (!b || !out || i < 0 || i >= (int)b->pairs.size() || !b->ran || b->status[(size_t)i]) return FGOICP_ERR_INVALID_ARG;
    const DriverStats& d = b->results[(size_t)i].stats;
    out->trans_cubes = d.trans_cubes; out->bounds_calls = d.bounds_calls; out->rot_cubes = d.rot_cubes;
    out->icp_runs = d.icp_runs; out->icp_iters = d.icp_iters; out->inner_bnb = d.inner_bnb; out->rounds = d.rounds;
    out->seconds_total = d.seconds_total; out->seconds_bnb = d.seconds_bnb; out->seconds_icp = d.seconds_icp; out->initial_icp_sse = d.initial_icp_sse;
    return FGOICP_OK;
}

int fgoicp_batch_alignment(const fgoicp_batch* b, int i, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns, uint8_t* target_hit_nt,
                           fgoicp_alignment_summary* out) {
    const char* where = "fgoicp_batch_alignment";
    if (!b) { set_error(std::string(where) + ": the batch must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!b->opts.alignment) { set_error(std::string(where) + ": the batch was created with fgoicp_batch_opts.alignment = 0"); return FGOICP_ERR_INVALID_ARG; }
    if (!b->ran) { set_error(std::string(where) + ": fgoicp_batch_run has not run yet"); return FGOICP_ERR_INVALID_ARG; }
    if (i < 0 || i >= (int)b->pairs.size()) { set_error(std::string(where) + ": pair index out of range"); return FGOICP_ERR_INVALID_ARG; }
    if (b->status[(size_t)i]) { set_error(std::string(where) + ": pair " + std::to_string(i) + " failed (status " + std::to_string(b->status[(size_t)i]) + ")"); return FGOICP_ERR_INVALID_ARG; }
    if (out && (out->struct_size < sizeof(uint32_t) || out->struct_size > 4096)) { set_error(std::string(where) + ": set out->struct_size = sizeof(fgoicp_alignment_summary)"); return FGOICP_ERR_INVALID_ARG; }
    const PairAlign& a = b->align[(size_t)i];
    if (!a.have) { set_error(std::string(where) + ": pair " + std::to_string(i) + ": " + (a.err.empty() ? "no report was taken" : a.err)); return a.rc ? a.rc : FGOICP_ERR_INVALID_ARG; }
    if (corr_idx_ns) std::memcpy(corr_idx_ns, a.corr.data(), sizeof(uint32_t) * a.corr.size());
    if (dist2_ns) std::memcpy(dist2_ns, a.d2.data(), sizeof(float) * a.d2.size());
    if (inlier_ns) std::memcpy(inlier_ns, a.inlier.data(), a.inlier.size());
    if (target_hit_nt) std::memcpy(target_hit_nt, a.hit.data(), a.hit.size());
    return alignment_summary_out(a.sum, out, where);
}

int fgoicp_batch_information(const fgoicp_batch* b, int i, fgoicp_information_t* out) {
    const char* where = "fgoicp_batch_information";
    if (!b) { set_error(std::string(where) + ": the batch must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!b->opts.information) { set_error(std::string(where) + ": the batch was created with fgoicp_batch_opts.information = 0"); return FGOICP_ERR_INVALID_ARG; }
    if (!b->ran) { set_error(std::string(where) + ": fgoicp_batch_run has not run yet"); return FGOICP_ERR_INVALID_ARG; }
    if (i < 0 || i >= (int)b->pairs.size()) { set_error(std::string(where) + ": pair index out of range"); return FGOICP_ERR_INVALID_ARG; }
    if (b->status[(size_t)i]) { set_error(std::string(where) + ": pair " + std::to_string(i) + " failed (status " + std::to_string(b->status[(size_t)i]) + ")"); return FGOICP_ERR_INVALID_ARG; }
    if (!information_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(fgoicp_information_t)"); return FGOICP_ERR_INVALID_ARG; }
    const PairInfo& f = b->info[(size_t)i];
    if (!f.have) { set_error(std::string(where) + ": pair " + std::to_string(i) + ": " + (f.err.empty() ? "no moments were taken" : f.err)); return f.rc ? f.rc : FGOICP_ERR_INVALID_ARG; }
    const PairHost& p = b->pairs[(size_t)i];
    const float c3[3] = {-p.offset_pct.x, -p.offset_pct.y, -p.offset_pct.z};  // the centroid that was subtracted: center_point_cloud returns minus it
    fgoicp_information_t full;
    information_fill(full, p.ns, f.m, c3, p.scaling_factor, f.max_dist2);
    return information_out(full, out, where);
}

int fgoicp_batch_launches(const fgoicp_batch* b, uint64_t* bounds_launches, uint64_t* icp_launches) {
    if (!b) return FGOICP_ERR_INVALID_ARG;
    if (bounds_launches) *bounds_launches = b->bounds_launches;
    if (icp_launches) *icp_launches = b->icp_launches;
    return FGOICP_OK;
}

// what the refinement getters share: the refusals, then the pair's record.  weighted: the kind of result the getter serves
static int batch_refined_pair(const fgoicp_batch* b, int i, const char* where, int weighted, const PairRefined** out) {
    if (!b) { set_error(std::string(where) + ": the batch must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (i < 0 || i >= (int)b->pairs.size()) { set_error(std::string(where) + ": pair index out of range"); return FGOICP_ERR_INVALID_ARG; }
    if (b->rspec.empty() || b->rspec[(size_t)i].model < 0) { set_error(std::string(where) + ": pair " + std::to_string(i) + " has no refinement (fgoicp_batch_opts_refine.refine)"); return FGOICP_ERR_INVALID_ARG; }
    if (weighted >= 0 && (int)b->rspec[(size_t)i].weighted() != weighted) {
        set_error(std::string(where) + ": pair " + std::to_string(i) + (weighted ? " is refined without a loss: fgoicp_batch_refined_plane serves it" : " is refined under a loss: fgoicp_batch_refined_robust serves it"));
        return FGOICP_ERR_INVALID_ARG;
    }
    if (!b->ran) { set_error(std::string(where) + ": fgoicp_batch_run has not run yet"); return FGOICP_ERR_INVALID_ARG; }
    if (b->status[(size_t)i]) { set_error(std::string(where) + ": pair " + std::to_string(i) + " failed (status " + std::to_string(b->status[(size_t)i]) + ")"); return FGOICP_ERR_INVALID_ARG; }
    const PairRefined& r = b->refined[(size_t)i];
    if (!r.have) { set_error(std::string(where) + ": pair " + std::to_string(i) + ": " + (r.err.empty() ? "no refinement was run" : r.err)); return r.rc ? r.rc : FGOICP_ERR_INVALID_ARG; }
    *out = &r;
    return FGOICP_OK;
}
int fgoicp_batch_refined_plane(const fgoicp_batch* b, int i, fgoicp_plane_result_t* out) {
    const char* where = "fgoicp_batch_refined_plane";
    if (!plane_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(fgoicp_plane_result_t)"); return FGOICP_ERR_INVALID_ARG; }
    const PairRefined* r = nullptr;
    const int rc = batch_refined_pair(b, i, where, 0, &r);
    return rc ? rc : plane_out(r->plane, out, where, "fgoicp_plane_result_t");
}
int fgoicp_batch_refined_robust(const fgoicp_batch* b, int i, fgoicp_robust_result_t* out) {
    const char* where = "fgoicp_batch_refined_robust";
    if (!plane_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(fgoicp_robust_result_t)"); return FGOICP_ERR_INVALID_ARG; }
    const PairRefined* r = nullptr;
    const int rc = batch_refined_pair(b, i, where, 1, &r);
    return rc ? rc : plane_out(r->robust, out, where, "fgoicp_robust_result_t");
}
int fgoicp_batch_refined_information(const fgoicp_batch* b, int i, fgoicp_information_t* out) {
    const char* where = "fgoicp_batch_refined_information";
    if (b && !b->opts.information) { set_error(std::string(where) + ": the batch was created with fgoicp_batch_opts.information = 0"); return FGOICP_ERR_INVALID_ARG; }
    if (!information_size_ok(out)) { set_error(std::string(where) + ": out must not be null and out->struct_size = sizeof(fgoicp_information_t)"); return FGOICP_ERR_INVALID_ARG; }
    const PairRefined* r = nullptr;
    const int rc = batch_refined_pair(b, i, where, -1, &r);
    if (rc) return rc;
    if (!r->have_info) { set_error(std::string(where) + ": pair " + std::to_string(i) + ": " + (r->info_err.empty() ? "no moments were taken" : r->info_err)); return r->info_rc ? r->info_rc : FGOICP_ERR_INVALID_ARG; }
    return information_out(r->info, out, where);
}
int fgoicp_batch_refine_launches(const fgoicp_batch* b, uint64_t* fused_launches, uint64_t* evaluations) {
    if (!b) return FGOICP_ERR_INVALID_ARG;
    if (fused_launches) *fused_launches = b->refine_launches;
    if (evaluations) *evaluations = b->refine_evaluations;
    return FGOICP_OK;
}

// ---- test hooks: the backend's own bounds() / icp_start() + icp_step() over the caller's contexts ----

// what HipBatchBackend::admit asks of a context, and one device for all of them
static int borrowed_ctx_check(fgoicp_ctx* const* ctxs, int nctx, const char* where) {
    for (int i = 0; i < nctx; ++i) {
        const fgoicp_ctx* c = ctxs[i];
        if (!c) { set_error(std::string(where) + ": context " + std::to_string(i) + " is null"); return FGOICP_ERR_INVALID_ARG; }
        if (c->device != ctxs[0]->device) { set_error(std::string(where) + ": the contexts are on different devices"); return FGOICP_ERR_INVALID_ARG; }
    }
    return FGOICP_OK;
}

static int batch_test_bounds_impl(const char* where, bool allow_trim, fgoicp_ctx* const* ctxs, int nctx, int nreq, const int* req_ctx, const int* req_G,
                                  const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4, float* lb_out, float* ub_out,
                                  uint64_t* launches_out, size_t arena_rows, uint64_t* selection_launches_out) {
    if (!ctxs || nctx <= 0 || nreq < 0 || (nreq > 0 && (!req_ctx || !req_G || !offsets))) { set_error(std::string(where) + ": invalid argument"); return FGOICP_ERR_INVALID_ARG; }
    int rc = borrowed_ctx_check(ctxs, nctx, where);
    if (rc) return rc;
    size_t groups = 0, rows = 0, offs = 0;
    for (int q = 0; q < nreq; ++q) {
        const int k = req_ctx[q], G = req_G[q];
        if (k < 0 || k >= nctx || G < 0) { set_error(std::string(where) + ": request " + std::to_string(q) + ": context index or group count out of range"); return FGOICP_ERR_INVALID_ARG; }
        const fgoicp_ctx* c = ctxs[k];
        if (c->inliers && !allow_trim) { set_error(std::string(where) + ": context " + std::to_string(k) + " is trimmed (fgoicp_batch_test_trim_bounds takes trimmed contexts)"); return FGOICP_ERR_INVALID_ARG; }
        if (!c->d_lut_zp) { set_error(std::string(where) + ": context " + std::to_string(k) + " has no packed LUT"); return FGOICP_ERR_INVALID_ARG; }
        const int* o = offsets + offs;
        for (int g = 0; g < G; ++g)
            if (o[0] != 0 || o[g + 1] < o[g]) { set_error(std::string(where) + ": request " + std::to_string(q) + ": offsets must start at 0 and be non-decreasing"); return FGOICP_ERR_INVALID_ARG; }
        groups += (size_t)G;
        rows += (size_t)o[G];
        offs += (size_t)G + 1;
    }
    if ((groups > 0 && (!R9 || !rot_span || !fix_rot)) || (rows > 0 && (!tn4 || !lb_out || !ub_out))) { set_error(std::string(where) + ": invalid argument"); return FGOICP_ERR_INVALID_ARG; }
    // the requests as the scheduler hands them over (BatchScheduler::submit)
    std::vector<BatchBoundsReq> reqs((size_t)nreq);
    std::vector<BatchBoundsReq*> tick;
    groups = rows = offs = 0;
    for (int q = 0; q < nreq; ++q) {
        BatchBoundsReq& r = reqs[(size_t)q];
        const int G = req_G[q], n = offsets[offs + (size_t)G];
        r.pair = req_ctx[q];
        r.G = G;
        r.R9.assign(R9 + 9 * groups, R9 + 9 * (groups + G));
        r.spans.assign(rot_span + groups, rot_span + groups + G);
        r.fix.assign(fix_rot + groups, fix_rot + groups + G);
        r.offsets.assign(offsets + offs, offsets + offs + G + 1);
        r.tn4.assign(tn4 + 4 * rows, tn4 + 4 * (rows + n));
        r.lb.assign((size_t)n, 0.f);
        r.ub.assign((size_t)n, 0.f);
        tick.push_back(&r);
        groups += (size_t)G;
        rows += (size_t)n;
        offs += (size_t)G + 1;
    }
    HipBatchBackend be;
    be.arena_rows_max = arena_rows;
    if ((rc = be.init_borrowed(ctxs, nctx))) return rc;
    if (!tick.empty() && (rc = be.bounds(tick))) return rc;
    rows = 0;
    for (const BatchBoundsReq& r : reqs) {
        std::memcpy(lb_out + rows, r.lb.data(), sizeof(float) * r.lb.size());
        std::memcpy(ub_out + rows, r.ub.data(), sizeof(float) * r.ub.size());
        rows += r.lb.size();
    }
    if (launches_out) *launches_out = be.bounds_launches;
    if (selection_launches_out) *selection_launches_out = be.selection_launches;
    return FGOICP_OK;
}
int fgoicp_batch_test_bounds(fgoicp_ctx* const* ctxs, int nctx, int nreq, const int* req_ctx, const int* req_G, const float* R9, const float* rot_span,
                             const int* fix_rot, const int* offsets, const float* tn4, float* lb_out, float* ub_out, uint64_t* launches_out) {
    return fgoicp::abi_guard("fgoicp_batch_test_bounds", [&] {
        return batch_test_bounds_impl("fgoicp_batch_test_bounds", false, ctxs, nctx, nreq, req_ctx, req_G, R9, rot_span, fix_rot, offsets, tn4, lb_out, ub_out,
                                      launches_out, 0, nullptr);
    });
}
int fgoicp_batch_test_trim_bounds(fgoicp_ctx* const* ctxs, int nctx, int nreq, const int* req_ctx, const int* req_G, const float* R9, const float* rot_span,
                                  const int* fix_rot, const int* offsets, const float* tn4, float* lb_out, float* ub_out, uint64_t* launches_out,
                                  size_t arena_rows, uint64_t* selection_launches_out) {
    return fgoicp::abi_guard("fgoicp_batch_test_trim_bounds", [&] {
        return batch_test_bounds_impl("fgoicp_batch_test_trim_bounds", true, ctxs, nctx, nreq, req_ctx, req_G, R9, rot_span, fix_rot, offsets, tn4, lb_out,
                                      ub_out, launches_out, arena_rows, selection_launches_out);
    });
}

static int batch_test_icp_impl(fgoicp_ctx* const* ctxs, int n, const int* start_pass, const float* R0s_9, const float* t0s_3, const size_t* max_iter,
                               const float* thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out) {
    const char* where = "fgoicp_batch_test_icp";
    if (n < 0 || (n > 0 && (!ctxs || !start_pass || !R0s_9 || !t0s_3 || !max_iter || !thr || !sse_out || !R_out9 || !t_out3 || !iters_out))) {
        set_error(std::string(where) + ": invalid argument");
        return FGOICP_ERR_INVALID_ARG;
    }
    if (n == 0) return FGOICP_OK;
    int rc = borrowed_ctx_check(ctxs, n, where);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        if (start_pass[i] < 0) { set_error(std::string(where) + ": start_pass < 0"); return FGOICP_ERR_INVALID_ARG; }
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) { set_error(std::string(where) + ": a context may run one ICP at a time"); return FGOICP_ERR_INVALID_ARG; }
    }
    std::vector<BatchIcpReq> reqs((size_t)n);
    for (int i = 0; i < n; ++i) {
        BatchIcpReq& r = reqs[(size_t)i];
        r.pair = i;
        std::memcpy(r.R0, R0s_9 + 9 * (size_t)i, sizeof(r.R0));
        std::memcpy(r.t0, t0s_3 + 3 * (size_t)i, sizeof(r.t0));
        r.max_iter = max_iter[i];
        r.thr = thr[i];
    }
    HipBatchBackend be;
    if ((rc = be.init_borrowed(ctxs, n))) return rc;
    // the launcher's passes (BatchScheduler::run): the runs that start now, then one step of every active run
    std::vector<BatchIcpReq*> active;
    int left = n;
    for (int pass = 0; left > 0; ++pass) {
        if (active.empty()) {  // nothing to step: on to the next pass that starts a run
            int next = -1;
            for (int i = 0; i < n; ++i)
                if (!reqs[(size_t)i].started && (next < 0 || start_pass[i] < next)) next = start_pass[i];
            if (next > pass) pass = next;
        }
        for (int i = 0; i < n; ++i) {
            BatchIcpReq& r = reqs[(size_t)i];
            if (r.started || start_pass[i] != pass) continue;
            r.started = true;
            if ((rc = be.icp_start(r))) return rc;
            if (!r.done) active.push_back(&r);
        }
        if (!active.empty()) {
            std::vector<BatchIcpReq*> step = active;
            if ((rc = be.icp_step(step))) return rc;
        }
        std::vector<BatchIcpReq*> still;
        for (BatchIcpReq* r : active) if (!r->done) still.push_back(r);
        active.swap(still);
        left = 0;
        for (const BatchIcpReq& r : reqs) left += r.done ? 0 : 1;
    }
    for (int i = 0; i < n; ++i) {
        const BatchIcpReq& r = reqs[(size_t)i];
        sse_out[i] = r.sse;
        std::memcpy(R_out9 + 9 * (size_t)i, r.R, sizeof(r.R));
        std::memcpy(t_out3 + 3 * (size_t)i, r.t, sizeof(r.t));
        iters_out[i] = r.iters;
    }
    return FGOICP_OK;
}
int fgoicp_batch_test_icp(fgoicp_ctx* const* ctxs, int n, const int* start_pass, const float* R0s_9, const float* t0s_3, const size_t* max_iter,
                          const float* thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out) {
    return fgoicp::abi_guard("fgoicp_batch_test_icp", [&] {
        return batch_test_icp_impl(ctxs, n, start_pass, R0s_9, t0s_3, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
    });
}

static int batch_test_refine_impl(fgoicp_ctx* const* ctxs, int n, const fgoicp_batch_refine_t* specs, const int* start_pass, const float* R0s_9, const float* t0s_3,
                                  fgoicp_robust_result_t* out_n, int* status_n, char* messages, uint64_t* fused_launches_out) {
    const char* where = "fgoicp_batch_test_refine";
    if (n < 0 || (n > 0 && (!ctxs || !specs || !start_pass || !R0s_9 || !t0s_3 || !out_n || !status_n))) { set_error(std::string(where) + ": invalid argument"); return FGOICP_ERR_INVALID_ARG; }
    if (fused_launches_out) *fused_launches_out = 0;
    if (n == 0) return FGOICP_OK;
    int rc = borrowed_ctx_check(ctxs, n, where);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        if (start_pass[i] < 0) { set_error(std::string(where) + ": start_pass < 0"); return FGOICP_ERR_INVALID_ARG; }
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) { set_error(std::string(where) + ": a context may run one refinement at a time"); return FGOICP_ERR_INVALID_ARG; }
        if (specs[i].struct_size < sizeof(fgoicp_batch_refine_t)) { set_error(std::string(where) + ": set specs[i].struct_size"); return FGOICP_ERR_INVALID_ARG; }
    }
    HipBatchBackend be;
    if ((rc = be.init_borrowed(ctxs, n))) return rc;
    std::memset(out_n, 0, sizeof(fgoicp_robust_result_t) * (size_t)n);
    auto fail = [&](int i, int status) {
        status_n[i] = status;
        if (messages) { std::strncpy(messages + 256 * (size_t)i, fgoicp_last_error(), 255); messages[256 * (size_t)i + 255] = 0; }
    };
    auto finish = [&](int i) {
        const RefineEnd& end = be.refine_state[(size_t)i].end;
        if (end.spec.weighted) {
            refine_result(end, &out_n[i]);
        } else {
            fgoicp_plane_result_t full;
            refine_result(end, &full);
            static_assert(sizeof(fgoicp_plane_result_t) <= sizeof(fgoicp_robust_result_t), "a plain result fits the run's slot");
            std::memcpy(&out_n[i], &full, sizeof(full));
        }
    };
    std::vector<char> started((size_t)n, 0), ended((size_t)n, 0);
    std::vector<int> active;
    for (int i = 0; i < n; ++i) { status_n[i] = FGOICP_OK; if (messages) messages[256 * (size_t)i] = 0; }
    int left = n;
    for (int pass = 0; left > 0; ++pass) {
        if (active.empty()) {  // nothing to step: on to the next pass that starts a run
            int next = -1;
            for (int i = 0; i < n; ++i)
                if (!started[(size_t)i] && (next < 0 || start_pass[i] < next)) next = start_pass[i];
            if (next > pass) pass = next;
        }
        for (int i = 0; i < n; ++i) {
            if (started[(size_t)i] || start_pass[i] != pass) continue;
            started[(size_t)i] = 1;
            RefineSpec spec;  // the context frame: max_dist2 and the scale as given
            spec.model = specs[i].model; spec.epsilon = specs[i].epsilon; spec.weighted = specs[i].loss != FGOICP_LOSS_NONE; spec.loss = specs[i].loss;
            spec.scale = specs[i].loss_scale; spec.max_dist2 = specs[i].max_distance;
            const int r1 = ctx_refine_step_begin(ctxs[i], be.refine_state[(size_t)i], R0s_9 + 9 * (size_t)i, t0s_3 + 3 * (size_t)i, specs[i].max_iter, specs[i].conv_thr, spec,
                                                 refine_where(spec, "fgoicp_icp_robust"), 0);
            if (r1 == FGOICP_ERR_HIP) return r1;
            if (r1) { fail(i, r1); ended[(size_t)i] = 1; continue; }
            active.push_back(i);
        }
        if (!active.empty()) {
            std::vector<char> done;
            std::vector<int> run_rc;
            std::vector<std::string> run_err;
            if ((rc = be.refine_tick(active, done, run_rc, run_err))) return rc;
            std::vector<int> still;
            for (size_t k = 0; k < active.size(); ++k) {
                const int i = active[k];
                if (run_rc[k]) { set_error(run_err[k]); fail(i, run_rc[k]); ended[(size_t)i] = 1; }
                else if (done[k]) { finish(i); ended[(size_t)i] = 1; }
                else still.push_back(i);
            }
            active.swap(still);
        }
        left = 0;
        for (int i = 0; i < n; ++i) left += ended[(size_t)i] ? 0 : 1;
    }
    if (fused_launches_out) *fused_launches_out = be.refine_launches;
    return FGOICP_OK;
}
int fgoicp_batch_test_refine(fgoicp_ctx* const* ctxs, int n, const fgoicp_batch_refine_t* specs, const int* start_pass, const float* R0s_9, const float* t0s_3,
                             fgoicp_robust_result_t* out_n, int* status_n, char* messages_n256, uint64_t* fused_launches_out) {
    return fgoicp::abi_guard("fgoicp_batch_test_refine", [&] {
        return batch_test_refine_impl(ctxs, n, specs, start_pass, R0s_9, t0s_3, out_n, status_n, messages_n256, fused_launches_out);
    });
}

}  // extern "C"
