// Internal layout of the opaque fgoicp_ctx (include/fgoicp_amd.h).  Shared by the operator ABI
// (ctx.hip) and the driver ABI (solver.cpp); not installed.
#pragma once
#include <exception>
#include <new>
#include <string>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../host/math3.hpp"
#include "../host/icp_loop.hpp"
#include "../host/abi_guard.hpp"
#include "../host/information.hpp"
#include "../host/plane.hpp"
#include "../host/gicp.hpp"
#include "../host/robust.hpp"
#include "bvh.hpp"
#include "kernels.hpp"
#include "owned.hpp"

// Every buffer, stream and event below is a handle (owned.hpp) and goes with its owner: the context, a tick slot or an ICP lane.
struct fgoicp_ctx {
    ~fgoicp_ctx();  // sets the device, drains every stream the context owns, then lets the members go (ctx.hip)
    int device = 0;
    fgoicp::Stream stream;  // declared first, destroyed last: lane 0, both slots and (FGOICP_SORT_STREAM=0) the sort streams borrow it
    size_t ns = 0, nt = 0;
    bool profile = false;

    // HBM-resident state
    fgoicp::Dev<float4> d_src;           // ns  x {x,y,z,|p|^2}, Morton order (pristine source, registration.hpp:63)
    fgoicp::Dev<float4> d_tgt;           // nt  x {x,y,z,0}, caller order (registration.hpp:61)
    fgoicp::Dev<float> d_lut;            // (dx+2)(dy+2)(dz+2) floats, x fastest, replicated border
    int lut_layout = 1;          // 1: d_lut_zp is the z-paired copy (float2), 2: the yz-quad copy (float4), 4: the apron-bricked yz-quads (float4), 6: the z-pair apron bricks (float2)
    int source_order = 0, tree_order = 0;  // what ctx_create chose (fgoicp_ctx_get_info)
    fgoicp::Dev<uint32_t> d_lut_idx;        // index LUT (geom.idx): per padded node the caller index of a nearest target point; seeds of the exact scans (FGOICP_LUT_INDEX=0: none)
    fgoicp::Dev<float2> d_lut_zp;        // z-paired copy {T[o], T[o + z-slice]} for the bounds kernel (2x the bytes, half the gathers)
    fgoicp::LutGeom geom{};
    fgoicp::BvhOwned bvh_tgt;    // exact-NN tree over the target (caller indices in pts[].w)
    bool brute_force_nn = false; // FGOICP_FLAG_BRUTE_FORCE_NN: O(ns*nt) kernels instead of the tree
    std::vector<uint32_t> perm;  // device slot i holds caller point perm[i]

    // bounds-operator scratch (persistent: the reference mallocs/frees per call, registration.cu:95-149)
    int max_subcubes = 0;

    // locality-sorted whole-tick path (kernels.hip, bounds_item.hpp): chunk_pts-point chunks.
    // Two tick slots: the host prepares / consumes one half of a round's inner BnBs while the device
    // evaluates the other (fgoicp_bounds_submit / _collect).
    struct TickSlot {
        fgoicp::Stream stream;                           // both slots queue on the context stream (borrowed): their kernels run back to back, never
                                                 // concurrently (two sorted kernels at once would thrash each other's L2 neighbourhoods)
        fgoicp::Event done;                              // recorded behind the slot's last kernel; collect waits on it, not on the stream
        fgoicp::Stream sort_stream;                      // descriptors upload + locality sort of THIS slot run here, next to the other
        fgoicp::Event bounds_ev;                         // bounds kernel of this slot finished (the finalize on the side stream waits for it)
        fgoicp::Event sorted_ev;                         //   slot's bounds kernel on the main stream, which then waits for sorted_ev
        fgoicp::Dev<fgoicp::TickGroup> d_groups; fgoicp::Mapped<fgoicp::TickGroup> h_groups;   // device / pinned staging (dev(): its device alias)
        fgoicp::Dev<fgoicp::TickSub> d_subs; fgoicp::Mapped<fgoicp::TickSub> h_subs;
        fgoicp::Dev<unsigned short> d_keys;
        fgoicp::Dev<unsigned> d_ranks;                   // place of every item inside its key's bin (returned by the histogram atomic)
        fgoicp::Dev<unsigned> d_hist, d_block_sums, d_cursor, d_sorted;
        fgoicp::Dev<unsigned> d_hist_xcd, d_xoff;        // per-XCD histograms of the tick sort and their offsets inside a bin
        fgoicp::Dev<double2> d_partials;                 // [max_subcubes][nchunk1] {sum_ub, sum_lb}
        fgoicp::Dev<double> d_cut_acc;                   // early exit (fgoicp_bounds_submit_cut): 2 running sums per evaluation, zero between windows
        fgoicp::Dev<float> d_row_cut;                    // ... and the threshold of every output row
        unsigned* d_row_term = nullptr;          // ... and whether the row is terminal (fgoicp_bounds_submit_leaf): a view of the tail of d_row_cut's allocation
        fgoicp::Dev<fgoicp::TickGate> d_cut_gate;        // ... and what an item waits for first: "finished" and "cutting" per evaluation
        bool win_cut = false;                    // the window in flight carries thresholds
        fgoicp::Mapped<float> h_lb, h_ub;                // pinned results of the window in flight
        fgoicp::Dev<float> d_evals;                      // trimmed mode: per-point e = max(d, 0) of every output row, [vals_rows][erow]
        fgoicp::Mapped<float> h_row_span;                // translation span of every output row of the window (pinned)
        fgoicp::Mapped<unsigned> h_sort_err;             // pinned: set by the bounds kernel when `sorted` is no permutation
        int win_groups = 0, win_evals = 0;       // the window in flight: groups and evaluations in the staging buffers
        std::vector<float> lb, ub;
        std::vector<int> row_group;              // window-local group of every output row (packing scratch)               // results of the whole submission
        int total = 0, win_pos = 0, win_rows = 0;
        bool inflight = false;
    };
    fgoicp::Dev<unsigned long long> d_cut_stat;          // items the early exit did not evaluate, since creation (device counter)
    uint64_t cut_items_offered = 0;              // items of the windows submitted with thresholds
    uint64_t cut_verify_windows = 0, cut_verify_rows = 0, cut_verify_above = 0, cut_verify_bad = 0;  // development build, FGOICP_CUT_VERIFY
    uint64_t cut_stat_base = 0;                  // value of *d_cut_stat at the last reset
    bool sort_xcd = true;                    // XCD-private histograms for the tick sort (cleared for good if a permutation check fails)
    bool sort_check = true;                  // verify on the device that every tick's `sorted` is a permutation
    int sort_fault_tick = 0;                 // test hook
    uint64_t sorted_ticks = 0, sort_fallbacks = 0;
    int nchunk1 = 0, max_groups = 0, cell_shift = 4;
    int chunk_pts = 256;                     // points per (subcube, chunk) work item of the sorted path
    bool finalize_on_side = true;
    int small_tick_items = 4096;             // ticks of at most this many items skip the descriptor copies and the locality sort
    size_t coop_split_min = (size_t)-1;      // cooperative ICP: source clouds of at least this many points split the two scans of an iteration over the ranks (FGOICP_COOP_SPLIT_MIN); default: never —
                                             // the loop runs replicated on every rank (same bits).  Measured at 437k points on 8 ranks: a 55k-query share is a latency chain like the whole scan, 2 gathers and 4 syncs per
                                             // iteration on top: 25-44 ms of ICP per rank split against 41 ms replicated, 6.2x against 6.4x with the gathers charged
    size_t coop_split_trim_min = 262144;     // ... trimmed contexts split from this size on: a trimmed iteration is long (1.5 ms at 1M points, 85 % of it the walk) and splitting pays — 8-rank replay of the 1M trimmed run 1.84x -> 2.69x (2.45x with the 632 gathers charged)
    bool icp_seeding = true;                 // ICP passes seed their exact NN search with the previous pass's correspondences
    fgoicp::Dev<float4> d_chunk_cen;                 // centroid of every chunk (source frame)
    float cut_tier_level = 0.5f;             // windows with thresholds: items whose per-point term at the patch centre reaches this multiple of T / ns go first (0: one tier)
    int cut_span = 1;                        // chunks per work item in windows with thresholds (2 on sparse clouds: see bounds_item_kernel)
    fgoicp::Dev<float4> d_span_cen;                  // centroid of every run of cut_span chunks
    TickSlot slots[2];

    // EXTENSION: trimmed Go-ICP (sum of the `inliers` smallest per-point terms; 0 = off)
    size_t inliers = 0;
    int vals_rows = 0;                       // subcubes per window in trimmed mode (memory budget)
    size_t erow = 0;                         // floats per row of d_evals (ns rounded up to a multiple of 4, plus the row's sample)
    int trim_samp_shift = 5;                 // trimmed mode: every 2^shift-th point goes into the row's sample (0: none, two-pass selection)
    float trim_margin_sd = 1.0f;             // bracket half-width in standard deviations of a binomial sample rank
    int trim_margin = 0;                     // ... in sample ranks (set with the inlier count)
    fgoicp::Dev<uint32_t> d_coop;                    // cooperative ICP: {correspondence indices | bits of the minima}, coop_cap entries each (all ranks' shares)
    size_t coop_cap = 0;
    fgoicp::Dev<unsigned long long> d_trim_stat;              // {rows selected, rows that fell back to two passes, bracket members}
    uint64_t trim_stat_acc[3] = {0, 0, 0};
    bool trim_ready = false;                 // trimmed-mode buffers allocated
    bool trim_skip = true;                   // exact NN only for queries that can be among the k smallest (nn_prep_kernel)
    float bounds6[6] = {0, 0, 0, 0, 0, 0};   // target_bounds as passed to fgoicp_ctx_create (they place the LUT)
    float tgt_box6[6] = {0, 0, 0, 0, 0, 0};  // the target's bounding box computed from the points (trimmed search: nn_prep_kernel)
    fgoicp::Dev<uint32_t> d_orig_of_slot;            // caller index of every device slot (ties at the inlier cut; the alignment report)

    // the alignment report (ctx_alignment) and the information moments (ctx_information): one allocation on the first call, 13 bytes per source
    // point, one per target point and 88 per block of kBlock source points
    struct AlignScratch {
        fgoicp::Dev<char> base;                          // the one allocation; every pointer below is a view into it (Arena)
        uint32_t* d_idx = nullptr;               // correspondences, device order
        uint32_t* d_corr = nullptr;              // ... and the report in caller order: correspondences, squared distances, inlier flags
        float* d_d2 = nullptr;
        unsigned char *d_inl = nullptr, *d_hit = nullptr;   // d_hit: nt16 bytes
        uint2* d_partials = nullptr;
        uint32_t* d_sum = nullptr;               // {inliers, targets hit, bits of the largest inlier squared distance}
        size_t nt16 = 0;
        fgoicp::MomentRow<fgoicp::kAlignInfoTerms>* d_info_rows = nullptr;   // the moments: one row of partial sums per block of the report
        unsigned long long* d_info = nullptr;    // {count, the bits of ten sums} (launch_align_info)
    } align;

    // target normals (ctx_set_target_normals): allocated by the first call, 16 bytes per target point
    fgoicp::Dev<float4> d_normals;                   // nt x {n.x, n.y, n.z, 0}, caller order; the zero vector: no normal
    bool normals_set = false;
    // source normals of the Generalized-ICP refinement (ctx_set_source_normals): allocated by the first call, 16 bytes per source point
    fgoicp::Dev<float4> d_src_normals;               // ns x {n.x, n.y, n.z, 0}, DEVICE SLOT order (perm); the zero vector: no normal
    bool src_normals_set = false;
    // the refinements' normal equations (refine_evaluate), each allocated by the first call that needs it.  One output; two sets of rows,
    // 232 and 240 bytes per block of kBlock source points: the unweighted and the weighted kernel reduce rows of 28 and of 29 terms, and
    // one allocation behind both types would take a cast.  The per-point outputs (fgoicp_robust_residuals, the scale): 17 bytes per source point
    fgoicp::Dev<fgoicp::MomentRow<fgoicp::kPlaneTerms>> d_plane_rows;
    fgoicp::Dev<fgoicp::MomentRow<fgoicp::kRobustTerms>> d_robust_rows;
    fgoicp::Dev<unsigned long long> d_refine_out;        // {count, the bits of 28 or 29 sums} (launch_refine_moments)
    fgoicp::Dev<double> d_robust_point;                  // ns residuals, then ns weights, caller order
    fgoicp::Dev<unsigned char> d_robust_counted;         // ns flags, caller order
    fgoicp::Event refine_ready;                          // stepped refinement (ctx_refine_step_begin creates it): recorded on lane 0's stream behind an evaluation's device half

    // exact-NN / ICP scratch, one set per lane: ICP runs on different lanes may be in flight together (ctx_icp_batch).  Lane 0 is
    // the lane of fgoicp_sse / fgoicp_icp / fgoicp_procrustes and queues on the context's main stream.
    struct IcpLane {
        fgoicp::Stream stream;                           // main stream of the lane (SSE pass, working-cloud transforms); lane 0 borrows the context's
        fgoicp::Stream icp_stream;                       // side stream (correspondence + covariance pass of the NEXT iteration)
        fgoicp::Event icp_ev_w, icp_ev_b;                // working cloud transformed / side-stream pass finished
        fgoicp::Dev<float4> d_work;                      // ns x {x,y,z,-}: ICP working copy (icp3d.hpp:24)
        fgoicp::Dev<uint32_t> d_min_bits, d_thr_bits, d_first_idx, d_first_idx2;
        fgoicp::Dev<double> d_bp, d_bp2, d_bp3;          // per-block partial sums (sums / covariance / SSE)
        fgoicp::Mapped<double> h_sums;                   // pinned result of the last reduction (<= 16 doubles)
        fgoicp::Dev<float> d_cen;                        // centroids {src, corr} on the device
        fgoicp::Mapped<float> h_cen;                     // ... and their pinned host copy
        // trimmed mode
        fgoicp::Dev<float> d_d2;                         // squared correspondence distances
        fgoicp::Dev<float> d_nn_lb, d_nn_ub, d_nn_lb2, d_nn_ub2;  // LUT brackets of the nearest distance (SSE pass / correspondence pass)
        fgoicp::Dev<uint32_t> d_sel, d_eq, d_sel_wide, d_sel_wide2;
        fgoicp::Dev<unsigned char> d_use;                // inlier mask of the current Procrustes step
        fgoicp::Mapped<float> h_trim;                    // pinned trimmed SSE
        // fused reductions of small clouds (ns <= 262144; ctx.hip icp_fused): wave sums from the scans' epilogues, final folds on the host
        fgoicp::Dev<double> d_wsum;                      // [groups][6] wave-level sums {query xyz, correspondence xyz} of the last correspondence scan
        fgoicp::Mapped<double> h_wsse;                   // pinned: [groups] wave-level sums of the last SSE scan
        fgoicp::Mapped<double> h_covbp;                  // pinned: [blocks][9] block partials of the covariance
        bool cov_on_host = false, sse_on_host = false;    // where the result of the last enqueued pass lands
        int cov_blocks = 0;
    };
    std::vector<IcpLane> lanes;
    bool icp_overlap = true;
    bool icp_fuse = true;                    // small clouds: reductions started in the scans' epilogues, folded on the host (FGOICP_ICP_FUSE=0: separate kernels)
    int icp_dual_env = -1;                   // FGOICP_ICP_DUAL: one walk serves the two scans of an ICP iteration (nn_scan_dual_kernel); -1 = by cloud size

    // HIP-event profile of the bounds kernel
    std::vector<fgoicp::Event> ev_start, ev_stop, ev_sel_start, ev_sel_stop;   // bounds kernel / trimmed selection kernel of the same window
    std::vector<char> ev_has_sel;
    std::vector<int> ev_evals;          // evaluations of the launch an event pair brackets (FGOICP_TICK_LOG)
    double prof_sel_ms = 0.0, prof_sel_ms_last = 0.0;
    int ev_used = 0;
    double prof_ms = 0.0;
    uint64_t prof_launches = 0, prof_subcubes = 0, prof_evals = 0;
};

namespace fgoicp {
void set_error(const std::string& s);

int ctx_bounds_multi(fgoicp_ctx* c, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                     const float* tn4, float* lb_out, float* ub_out, const float* cut_above = nullptr);
int ctx_cut_stats(fgoicp_ctx* c, uint64_t* items_offered, uint64_t* items_cut, int reset);
int ctx_bounds_submit(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4,
                      const int* twin = nullptr, const float* cut_above = nullptr, const float* ub_below_span = nullptr);
int ctx_bounds_collect(fgoicp_ctx* c, int slot, float* lb_out, float* ub_out);
int ctx_set_inliers(fgoicp_ctx* c, size_t k);
// Trimmed Go-ICP as fgoicp_solver_create and fgoicp_batch set a context up for trim fraction f: the context flags (curve order) and the
// inlier count — inlierNum = (int)(Nd * (1 - trimFraction)), as in Go-ICP, at least 1; 0 = untrimmed (f <= 0, or no point trimmed).
inline unsigned trim_ctx_flags(unsigned flags, float f) { return flags | (f > 0.0f ? (unsigned)FGOICP_FLAG_CURVE_ORDER : 0u); }
inline size_t trim_inliers(size_t ns, float f) {
    if (!(f > 0.0f)) return 0;
    size_t k = (size_t)((double)ns * (1.0 - (double)f));
    if (k < 1) k = 1;
    return k < ns ? k : 0;
}
// fgoicp_batch: ctx_set_inliers without the slots' e-rows (the batch evaluates trimmed bounds into an arena of its own)
int ctx_set_inliers_batch(fgoicp_ctx* c, size_t k);
size_t trim_rows_budget(size_t free_bytes);        // bytes of e-rows per slot (solo) / per batch arena
size_t trim_icp_bytes(size_t ns, size_t lanes);    // device bytes trimmed ICP adds to a context
int ctx_sse(fgoicp_ctx* c, const float* R9, const float* t3, float* sse_out, const uint32_t* seed_idx = nullptr);
// fgoicp_alignment on lane 0; every output may be null.  `out` is filled whole (scaling_factor = 1), whatever its struct_size says.
int ctx_alignment(fgoicp_ctx* c, const float* R9, const float* t3, uint32_t* corr_idx, float* dist2, uint8_t* inlier, uint8_t* target_hit,
                  fgoicp_alignment_summary* out);
// fgoicp_information on lane 0: the report's device half (shared with ctx_alignment), then the moments of the counted correspondences
// (launch_align_info).  max_dist2 must have been checked (not NaN, >= 0).  Context frame.
int ctx_information(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, InfoMoments* m);
// both from one pass of the report's device half (fgoicp_batch with both options on): ctx_alignment's outputs and ctx_information's
int ctx_alignment_information(fgoicp_ctx* c, const float* R9, const float* t3, uint32_t* corr_idx, float* dist2, uint8_t* inlier, uint8_t* target_hit,
                              fgoicp_alignment_summary* out, float max_dist2, InfoMoments* m);
// EXTENSION: target normals and the point-to-plane refinement (include/fgoicp_amd.h).  normals = nullptr: estimated from k neighbours.
int ctx_set_target_normals(fgoicp_ctx* c, const float* normals, int k);
int ctx_target_normals(fgoicp_ctx* c, float* out_nt3);
int ctx_target_knn(fgoicp_ctx* c, int k, uint32_t* idx, float* d2);
// EXTENSION: source normals and the Generalized-ICP refinement (include/fgoicp_amd.h).  normals = nullptr: estimated from the k nearest
// SOURCE points through a throw-away tree over the source.
int ctx_set_source_normals(fgoicp_ctx* c, const float* normals, int k);
int ctx_source_normals(fgoicp_ctx* c, float* out_ns3);
// EXTENSION: the point-to-plane and Generalized-ICP refinements and their robust losses (include/fgoicp_amd.h).  What one evaluation
// takes; checked by refine_refusals first.
struct RefineSpec {
    int model = FGOICP_MODEL_PLANE;
    double epsilon = 1e-3;  // FGOICP_MODEL_GICP only
    bool weighted = false;  // false, the plain calls: the unweighted kernel and its 28 sums; loss and scale are not read
    int loss = FGOICP_LOSS_NONE;
    double scale = 0.0;
    float max_dist2 = 0.f;
};
// how a call takes its scale: not at all, as given (finite and > 0 unless the loss is none), or given or estimated (finite)
enum class ScaleCheck { none, given, or_estimated };
// what every refinement call on the context refuses before any device work (the list and its order: ctx.hip)
int refine_refusals(const fgoicp_ctx* c, const RefineSpec& r, ScaleCheck scale, const char* where);
// one evaluation on lane 0: the report's device half (its index scan keeps the moved queries), then launch_refine_moments.  Unweighted,
// m->m[28] is the count.  sse_out (optional): the report's sse, the bits of fgoicp_sse.  residual / weight / counted (each optional, ns
// entries, caller order; weighted specs only): the per-point outputs, read back behind the evaluation.
int refine_evaluate(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, RefineMoments* m, float* sse_out = nullptr, double* residual = nullptr,
                    double* weight = nullptr, unsigned char* counted = nullptr);
// fgoicp_robust_scale: one evaluation with the per-point outputs, the median on the host
int ctx_robust_scale(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, double* scale, const char* where);
// where a loop ended: the pose, the last evaluation there, and the spec it ran with (its scale: given or estimated)
struct RefineEnd {
    Mat3f R;
    Vec3f t;
    RefineMoments m;
    float sse = 0.f;
    int iterations = 0, rank = 0;
    RefineSpec spec;
    int scale_estimated = 0;
};
// fgoicp_icp_plane, fgoicp_icp_gicp, fgoicp_icp_robust (weighted; spec.scale <= 0: estimated at (R0, t0))
int refine_loop(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float thr, const RefineSpec& spec, const char* where, RefineEnd* end);
// One refine_loop run cut at its host wait (fgoicp_batch): refine_loop itself runs on this state, so there is one
// loop logic.  After ctx_refine_step_begin, per tick and until `done`:
//   ctx_refine_step_enqueue   the evaluation's device half at the run's pose on lane 0's stream, c->refine_ready recorded behind it;
//                             *view = what the batch's fused launch reduces (first_block is the batch's to set)
//   (the batch: its stream waits for refine_ready, launch_fused_refine_moments, one copy of the outputs, one wait)
//   ctx_refine_step           out = the pair's {count, sums}; the sse is read here, behind that wait; then the loop's host arithmetic
// end holds refine_loop's result, bit for bit.
struct RefineStepRun {
    RefineEnd end;
    size_t max_iter = 0;
    float thr = 0.f;
    std::string where;
    bool stop = false, done = false;
    int evaluations = 0;
};
// begin: estimate_k > 0 estimates the normals the spec needs and the context lacks from estimate_k neighbours (as fgoicp_solver_refine_*);
// then refine_refusals, then the scale estimate where the spec asks for one (ctx_robust_scale, whole).  Enqueues no evaluation.
int ctx_refine_step_begin(fgoicp_ctx* c, RefineStepRun& s, const float* R0, const float* t0, size_t max_iter, float thr, const RefineSpec& spec, const char* where,
                          int estimate_k);
int ctx_refine_step_enqueue(fgoicp_ctx* c, const RefineStepRun& s, FusedRefineView* view);
int ctx_refine_step(fgoicp_ctx* c, RefineStepRun& s, const unsigned long long* out);
// `full` is filled whole (scaling_factor = 1): plane_rmse = sqrt(m[27] / N), rmse = sqrt(m[27] / sum w)
void refine_result(const RefineEnd& e, fgoicp_plane_result_t* full);
void refine_result(const RefineEnd& e, fgoicp_robust_result_t* full);
// a summary handed to a caller: no byte beyond the struct_size the caller set is written (0, or less than the size field itself: refused)
inline int alignment_summary_out(const fgoicp_alignment_summary& full, fgoicp_alignment_summary* out, const char* where) {
    if (!out) return FGOICP_OK;
    const uint32_t n = out->struct_size;
    if (n < sizeof(uint32_t) || n > 4096) { set_error(std::string(where) + ": set out->struct_size = sizeof(fgoicp_alignment_summary)"); return FGOICP_ERR_INVALID_ARG; }
    std::memcpy(out, &full, n < sizeof(full) ? n : sizeof(full));
    out->struct_size = n;
    return FGOICP_OK;
}
int ctx_icp(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3,
            int* iters_out);
int ctx_icp_coop(fgoicp_ctx* c, int rank, int world, int (*gather)(void* dev_buf, size_t bytes_per_rank, void* user), void* user, const float* R0,
                 const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out);
int ctx_icp_lane(fgoicp_ctx* c, int lane, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3,
                 int* iters_out);
int ctx_icp_batch(fgoicp_ctx* c, int n, const float* R0s, const float* t0s, size_t max_iter, float thr, float* sse_out, float* R_out9s, float* t_out3s,
                  int* iters_out);

// One ctx_icp run cut at its host turn-arounds (fgoicp_batch): begin enqueues, then ctx_icp_step after every drain of the context's
// stream until `done`.  Only where ctx_icp_steppable (the small-cloud loop); the result is ctx_icp's, bit for bit.
struct IcpStepRun {
    IcpLoop loop;
    bool have_sse = false, done = false;  // an SSE is in flight / the loop has ended: loop.result() has the outputs
};
bool ctx_icp_steppable(const fgoicp_ctx* c);
int ctx_icp_step_begin(fgoicp_ctx* c, IcpStepRun& s, const float* R0, const float* t0, size_t max_iter, float thr);
int ctx_icp_step(fgoicp_ctx* c, IcpStepRun& s);
}  // namespace fgoicp
