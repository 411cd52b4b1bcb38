// Launch-side declarations of the gfx950 kernels (kernels.hip).  Host-callable wrappers only;
// everything takes an explicit hipStream_t and never allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fixed_sum.hpp"

namespace fgoicp {

struct BvhView;

constexpr int kMaxBatch = 32;          // the fewest subcubes a bounds window holds (FGOICP_MAX_SUBCUBES)
constexpr int kBlock = 256;            // 4 wave64 per workgroup everywhere
constexpr float kSqrt3 = 1.732050807568877f;   // fgoicp/common.hpp:19
constexpr float kPi = 3.141592653589793f;      // fgoicp/common.hpp:17
constexpr float kInf = 1E+10f;                 // fgoicp/common.hpp:18

// Geometry of the nearest-squared-distance LUT (fgoicp/registration.cu:180-207).  The device
// copy is stored with a one-voxel replicated border on every side, so that CUDA's clamp
// addressing (registration.cu:226-228) needs no per-texel branch: padded[k] = T[clamp(k-1)].
struct LutGeom {
    float off_x, off_y, off_z;   // offset = -min_bound (registration.cu:202-204)
    float scale;                 // 1/resolution (registration.cu:201)
    float resolution;
    int dx, dy, dz;              // reference dims (registration.cu:186-188)
    int px, py, pz;              // padded dims = d + 2
    int quantize;                // 1: interpolation weights in 1.8 fixed point (CUDA linear filtering)
    const uint32_t* idx;         // optional (nullptr: none): per padded node the caller index of A nearest target point — the exact scans seed their
                                 // pruning bound with the distance to it (round 3, kernels.hip lut_upper_bound_d2); not read by the bounds kernels
};

// The bounds of a whole tick: all subcubes of all rotation nodes in ONE launch, work items ordered by LUT locality
// (kernels.hip).  groups/subs are device arrays of TickGroup (48 B) / TickSub (48 B); partials is indexed
// [s * nchunk + chunk]; events (optional) bracket the bounds kernel only.
struct TickGroup {   // one rotation node
    float R[9];
    float sin_half;
    int fix_rot;
    int pad_;
};
struct TickSub {     // one EVALUATION: a translation node + its rotation node, and where its sums go
    float tx, ty, tz, span;
    int group;
    int out0;        // output row of the result (dual: of the fix_rot = 1 variant)
    int out1;        // dual only: output row of the fix_rot = 0 variant
    int dual;        // 1 = the UB task and the LB task of one rotation cube both hold this translation node in the same
                     // submission: one lookup per point, both variants of the bound formulae (registration.cu:39-58)
    float cut0;      // cut_above of out0's group (fgoicp_bounds_submit_cut; +inf = none): once the lower-bound sums of the evaluation's
    float cut1;      // finished items reach it, the remaining items are not evaluated (dual: both variants must have reached theirs)
    unsigned term;   // kSubTerm0 / kSubTerm1: the row out0 / out1 is TERMINAL (fgoicp_bounds_submit_leaf): the sums that are run against its
                     // threshold, and the bound that decides {T, T}, are the UPPER bound's
    int pad_;
};
constexpr unsigned kSubTerm0 = 1u, kSubTerm1 = 2u;
static_assert(sizeof(TickSub) == 48, "TickSub is copied in 16-byte units");
// Early exit (fgoicp_bounds_submit_cut): acc = 2 doubles per evaluation (sum of the lower-bound partials of its finished items — of a
// terminal row: the upper-bound partials — per variant; zero on entry, re-zeroed by bounds_finalize_kernel), row_cut = the threshold of every output row (written ahead of the
// bounds kernel, applied by bounds_finalize_kernel), stat = {items not evaluated} (optional).  acc == nullptr: off.
constexpr int kCutStatSlots = 64;  // the counter is spread over this many words (one atomic per output row with skipped items)
constexpr float kCutNone = 3.0e38f;  // thresholds at or above this (fgoicp_bounds_submit_cut: +inf) switch the early exit off
// What a work item of a window with thresholds waits for before anything else: an item whose evaluation is over ends after two
// dependent loads (its slot of `sorted`, then this) and no store.  Written per window, before its bounds kernel, by the kernel that
// also leaves the "not evaluated" partials of every chunk (tick_keys_kernel / tick_prefill_kernel).
struct TickGate {
    unsigned done;      // 1 = the running sums have been seen at their thresholds (set by the bounds kernel; a stale 0 only costs time)
    unsigned flags;     // kGateCutting, kGateTerm0, kGateTerm1
};
static_assert(sizeof(TickGate) == 8, "TickGate is read and written as one 8-byte word");
constexpr unsigned kGateCutting = 1u;  // every variant of the evaluation has a threshold below kCutNone
constexpr unsigned kGateTerm0 = 2u, kGateTerm1 = 4u;  // TickSub::term of the evaluation (kSubTerm0, kSubTerm1), one bit up
struct TickCut {
    double* acc = nullptr;
    TickGate* gate = nullptr;             // per evaluation (see TickGate)
    float* row_cut = nullptr;
    unsigned* row_term = nullptr;         // per output row: 1 = terminal, the row's rule is "upper bound >= T" (fgoicp_bounds_submit_leaf)
    unsigned long long* stat = nullptr;   // [kCutStatSlots]
    const unsigned* tier_split = nullptr; // items of the first tier of `sorted` (launch_tick_sort with tier_lut): the grid walks them before the others
    int probe = 0;                        // development build, FGOICP_CUT_PROBE: 1 = the running sums are not read (nothing is ever cut), 2 = not added to, 4 = the gate's `done` is not honoured
};
constexpr int kTickNumKeys = 1 << 15;
void launch_tick_sort(const LutGeom& g, const float4* chunk_cen, int nchunk, const TickGroup* groups, const TickSub* subs, int nsub, int cell_shift,
                      unsigned short* keys, unsigned* ranks /* per item, like keys */, unsigned* hist /* kTickNumKeys, zero on entry and on exit */,
                      unsigned* hist_xcd /* 16 x kTickNumKeys, zero on entry and on exit (optional) */, unsigned* xoff /* 16 x kTickNumKeys (optional) */,
                      unsigned* block_sums /* 64 */, unsigned* cursor, unsigned* sorted,
                      int allow_xcd /* 0: device-scope histogram atomics */, int prefill /* 1: `sorted` is filled with 0xFFFFFFFF first, for the permutation check in launch_bounds_sorted */,
                      int inject_fault /* test hook */, hipStream_t s,
                      const float* tier_lut = nullptr /* windows with thresholds: the plain LUT — items likely to carry much of their evaluation's lower bound are sorted
                                                         in front of the others (two tiers; cursor[kTickTierSplit] = items of the first) */,
                      float tier_level = 0.0f /* ... those whose per-point term at the patch centre reaches tier_level * T */,
                      const TickCut* prefill_cut = nullptr /* windows with thresholds: the key kernel also writes gate, row_cut and the "not evaluated" partials */,
                      double2* partials = nullptr, int row_chunks = 0 /* chunks per row of `partials` */, int span = 1 /* chunks per item: nchunk = ceil(row_chunks / span) */);
constexpr int kTickTierSplit = 1 << 14;
// The same for a window that skips the sort (small ticks): gate, row_cut and the "not evaluated" partials of its evaluations, one launch on `s`.
void launch_tick_prefill(const TickSub* subs, int nsub, int nchunk, const TickCut& cut, double2* partials, hipStream_t s);
// descriptors of a tick: pinned staging (device-visible addresses) -> device arrays, one launch
void launch_tick_upload(const TickGroup* hd_groups, TickGroup* d_groups, int ngroups, const TickSub* hd_subs, TickSub* d_subs, int nsubs, hipStream_t s);
// Returns true if the early exit was in force: the window carried thresholds and is untrimmed (trimmed windows carry none, so trimmed
// contexts are the only case where fgoicp_bounds_submit_cut returns exact rows above the threshold).
bool launch_bounds_sorted(const float4* src, int ns, const float2* packed, int layout /* 1 z-pair, 2 yz-quad, 4 apron-bricked yz-quad, 6 z-pair apron */, const LutGeom& g,
                          int nchunk, int chunk_pts /* 256 .. 2048 points per item */, const TickGroup* groups, const TickSub* subs, int nsub, const unsigned* sorted,
                          double2* partials, float* evals_or_null /* trimmed mode: row r = the per-point e = max(d, 0) of output row r */, size_t erow /* floats per row, multiple of 4 */,
                          int samp_shift /* trimmed mode: > 0 = every 2^samp_shift-th point once more in the sample behind the row (offset: ns rounded up to 64 floats) */,
                          unsigned* sort_err /* optional, host-visible: set to 1 unless `sorted` (prefilled, see launch_tick_sort) is a permutation of the items */,
                          const TickCut& cut /* early exit of evaluations whose lower bound has reached its group's cut_above */,
                          int span /* chunks per work item: `sorted` then orders nsub * ceil(nchunk / span) items */,
                          hipEvent_t ev_start, hipEvent_t ev_stop, hipStream_t s);
// EXTENSION (trimmed Go-ICP): per output row the sums of ub = e*e and lb = max(e - sqrt3*span, 0)^2 over the row's k smallest e
// (one exact selection per row, kernels.hip trim_rows_kernel); row_span[r] = translation span of row r (device-readable)
// samp_shift > 0: one pass per row (trim_rows_sampled_kernel) — the bracket of the cut comes from the row's sample, `margin` sample ranks
// either side of the expected rank, verified exactly, two-pass fallback inside the kernel; stat (optional): {rows, fallbacks, members}
void launch_trim_rows(const float* evals, size_t erow, int n, int k, int rows, const float* row_span, float* out_ub, float* out_lb, hipStream_t s,
                      int samp_shift = 0, int margin = 0, unsigned long long* stat = nullptr);
// one row: out[0] (optional) = sum of the k smallest of vals[0..n), sel_info (optional) = {bits of the k-th smallest, copies of it needed}
void launch_trim_select(const float* vals, int n, int k, float* out, uint32_t* sel_info,
                        uint32_t* wide_scratch /* 64 KiB, optional: rows of n >= 32768 are then selected by the whole device */, hipStream_t s);
void launch_icp_inliers(const float4* work, const float4* tgt, const uint32_t* idx, int n, int nt, int k, float* d2, uint32_t* sel_info,
                        uint32_t* equal_count, const uint32_t* orig_of_slot, unsigned char* use, uint32_t* wide_scratch, hipStream_t s);
// launch_icp_inliers on given squared distances (fgoicp_alignment: the exact minima of a scan): use[i] = 1 for the k smallest of d2[0..n), ties at
// the cut to the lowest caller indices (orig_of_slot)
void launch_inlier_mask(const float* d2, int n, int k, uint32_t* sel_info, uint32_t* equal_count, const uint32_t* orig_of_slot, unsigned char* use,
                        uint32_t* wide_scratch, hipStream_t s);
// The alignment report (fgoicp_alignment; kernels.hip align_scatter_kernel, align_fold_kernel): idx / min_bits / use (nullptr: every point is an
// inlier) per device slot -> corr_out / d2_out / inlier_out per caller index (n entries each); target_hit[j] = 1 for every neighbour of an inlier
// (nt16 = nt rounded up to 16 bytes, zero on entry); partials: ceil(n / kBlock) entries; summary3 = {inliers, distinct targets hit, bits of the
// largest inlier squared distance}
void launch_align_scatter(const uint32_t* idx, const uint32_t* min_bits, const unsigned char* use, const uint32_t* orig_of_slot, int n, int nt, uint32_t* corr_out,
                          float* d2_out, unsigned char* inlier_out, unsigned char* target_hit, size_t nt16, uint2* partials, uint32_t* summary3, hipStream_t s);
// The information matrix's moments (fgoicp_information; kernels.hip align_info_kernel, fixed_sum.hpp moment_fold_kernel) over the report's arrays in caller
// order: the counted correspondences are the i with inlier[i] != 0, d2[i] <= max_d2 and corr[i] < nt.  rows: ceil(n / kBlock) entries;
// out11 = {count, sum q (3), sum q q^T (xx xy xz yy yz zz), sum d2} — the count a 64-bit integer, the rest the bits of doubles.  Fixed
// order of every addition: the same arrays give the same bits.
constexpr int kAlignInfoTerms = 10;
void launch_align_info(const unsigned char* inlier, const float* d2, const uint32_t* corr, const float4* tgt, int n, int nt, float max_d2, MomentRow<kAlignInfoTerms>* rows,
                       unsigned long long* out11, hipStream_t s);
// Target normals (fgoicp_ctx_set_target_normals, fgoicp_target_knn; kernels.hip target_knn_kernel): per target point its k nearest target points
// (itself included) by the total order (bits of the fp32 squared distance, caller index), and the unit direction of least variance of
// those k points.  4 <= k <= 32, k <= nt.  knn_idx / knn_d2 (optional): nt rows of k entries, rows and indices in caller order;
// normals (optional): nt x {n.x, n.y, n.z, 0} in caller order, the zero vector for a degenerate neighbourhood.
constexpr int kKnnMin = 4, kKnnMax = 32;
void launch_target_knn(const BvhView& t, const float4* tgt, int nt, int k, uint32_t* knn_idx, float* knn_d2, float4* normals, hipStream_t s);
// Outlier removal (fgoicp_remove_outliers; kernels.hip outlier_knn_kernel, the walk and the list of target_knn_kernel): per point of the tree,
// at its caller index, the mean of the fp64 square roots of its k smallest squared distances (itself included) and the k-th of them.
// 2 <= k <= 32, k <= nt.
constexpr int kOutlierKnnMin = 2;
void launch_outlier_knn(const BvhView& t, int nt, int k, double* mean_dist, float* kth_dist2, hipStream_t s);
// Density clustering (fgoicp_cluster_dbscan; kernels.hip radius_walk and its consumers): every array is indexed by CALLER index, nt entries.
// count: neighbours[i] = the points within eps2 of point i (itself included, d2 <= eps2 on the scans' fp32 dist_sq), core[i] = 0 / 1 =
// neighbours[i] >= min_points, *core_count += the number of core points.
void launch_cluster_count(const BvhView& t, int nt, float eps2, uint32_t min_points, uint32_t* neighbours, uint32_t* core, unsigned long long* core_count, hipStream_t s);
// One round of the union-find over the core points: hook (every core point, for each core neighbour of a lower index, atomicMin of the larger
// root's parent with the smaller root; *changed = 1 if any hook was made), then compress (parent[i] = root(i) for every core i).  parent[i] = i
// before the first round; the caller repeats the round until one leaves *changed at 0: then parent[i] is the lowest index of i's component.
void launch_cluster_round(const BvhView& t, int nt, float eps2, const uint32_t* core, uint32_t* parent, uint32_t* changed, hipStream_t s);
// label[i] = rank[parent[i]] for a core point; for another point the same of its core neighbour with the smallest key (bits(d2) << 32) | index,
// -1 if it has none.  rank: the dense number of every root (the exclusive scan of the root flags over caller index).
void launch_cluster_border(const BvhView& t, int nt, float eps2, const uint32_t* core, const uint32_t* parent, const uint32_t* rank, int32_t* label, hipStream_t s);
// The normal equations of the refinements (kernels.hip refine_moments_kernel, then fixed_sum.hpp moment_fold_kernel) over the report's arrays
// (caller order) and the moved queries of its index scan (device order, `moved`): counted are the caller indices with inlier != 0,
// d2 <= max_d2, corr < nt and a non-zero normal at corr; gicp: whose own source normal is non-zero too.  src_normals: the source normals in
// DEVICE SLOT order (n x {n.x, n.y, n.z, 0}), read only with gicp.
struct RefineInputs {
    const float4* moved;
    const uint32_t* orig_of_slot;
    const unsigned char* inlier;
    const float* d2;
    const uint32_t* corr;
    const float4 *tgt, *normals, *src_normals;
    int n, nt;
    float max_d2;
};
// K = kPlaneTerms, the unweighted sums: out = {count, the bits of 28 doubles} — gicp = false (fgoicp_plane_moments): the upper triangle of
// sum J^T J row by row (21), sum J^T r (6), sum r^2; gicp = true (fgoicp_gicp_moments; host/gicp.hpp): the same of J^T M J, J^T M d,
// d^T M d, with R9 the rotation of the pose `moved` was formed with (glm order) and eps in (0, 1].  loss, scale and the per-point outputs
// are not read.
// K = kRobustTerms, the weighted sums (fgoicp_robust_moments): each of those terms times w(s) (host/robust.hpp robust_weight; loss and scale
// c as fgoicp_robust_weight takes them), and w as the 29th: out = {count, the bits of 29 doubles}.  residual / weight / counted (all three
// or none): per-point outputs at the CALLER index, n entries each, 0 / 0 / 0 for an uncounted point; with nullptr the launch is the kernel
// without those stores.
// rows: ceil(n / kBlock) entries.  Fixed order of every addition.
constexpr int kPlaneTerms = 28, kRobustTerms = 29;
template <int K>
void launch_refine_moments(const RefineInputs& in, bool gicp, const float* R9, double eps, int loss, double scale, MomentRow<K>* rows, unsigned long long* out,
                           double* residual, double* weight, unsigned char* counted, hipStream_t s);
// The same reduction for the refining pairs of a batch tick in one launch per class (fgoicp_batch; kernels.hip fused_refine_moments_kernel,
// fused_moment_fold_kernel).  A class is gicp x weighted; its views lie next to each other in the table.  View p owns the blocks
// [first_block, first_block + ceil(in.n / kBlock)) of the launch — block b of them is the solo launch's block b - first_block: the same slots,
// the same per-thread text (refine_item.hpp), the same row of the pair's OWN rows — and one fold block, which leaves {count, the bits of the
// K sums} at out + kFusedRefineOut * p.  No block, wave or addition is shared between two pairs: every pair's bytes are its solo launch's.
constexpr int kFusedRefineMax = 16;  // views per launch: the batch's limit on live pairs (kBatchAutoLive)
constexpr int kFusedRefineOut = 1 + kRobustTerms;
struct FusedRefineView {
    RefineInputs in;
    float R[9];        // the rotation of the pose in.moved was formed with
    int loss;
    double eps, scale;
    void* rows;        // MomentRow<kPlaneTerms>* (unweighted) or MomentRow<kRobustTerms>* (weighted): the context's own
    int first_block;   // of this view inside its class's launch
    int nblocks;
};
// views: the n (1 .. kFusedRefineMax) views of one class, device memory; total_blocks = the sum of their nblocks
void launch_fused_refine_moments(bool gicp, bool weighted, const FusedRefineView* views, int n, int total_blocks, unsigned long long* out, hipStream_t s);
// out[i] = in[orig_of_slot[i]], i < n: caller order -> device slot order
void launch_slot_order(const float4* in, const uint32_t* orig_of_slot, int n, float4* out, hipStream_t s);
// The bounds of many registrations in one launch (fgoicp_batch, bounds_fused.hpp): a view per pair of the batch, an evaluation per output
// row, work items {evaluation, chunk}.  Every row is the bits its pair's own context computes with thresholds off.
struct FusedPairView {
    const float4* src;           // the context's d_src (its device order)
    const char* lutp;            // its packed LUT (d_lut_zp)
    LutGeom g;
    int ns;
    int chunk_pts;               // its points per work item
};
struct FusedEval {
    float R[9];
    float sin_half;              // sin(rot_span * sqrt3 * pi / 2), computed as the context's window packing does (registration.cu:42)
    float tx, ty, tz, span;
    int fix_rot;
    int pair;                    // index into the views
    int nchunk;                  // the pair's chunks per evaluation
    int samp_shift;              // trimmed rows: the pair's sample shift (trim_store; 0 = no sample); 0 otherwise
    union {
        unsigned long long partial_base;  // untrimmed rows: its nchunk partials start here
        unsigned long long row_off;       // trimmed rows: its e-row starts here in the arena (floats; 16-byte aligned)
    };
};
static_assert(sizeof(FusedEval) == 80, "FusedEval: one layout for both kinds of row");
// one trimmed row of a batch tick for fused_trim_select_kernel: the row's n values of e (its sample behind them), its pair's k, sample
// shift and margin (fgoicp_ctx::inliers, trim_samp_shift, trim_margin), its translation span and where its {ub, lb} go
struct FusedTrimRow {
    const float* row;
    int n, k, samp_shift, margin;
    float span;
    int out;
};
bool bounds_lut_wide(const LutGeom& g, int layout);
size_t packed_lut_bytes(const LutGeom& g, int layout);  // of the packed copy alone
// layout: fgoicp_ctx::lut_layout (1, 2, 4, 6) of EVERY pair the items belong to; wide = bounds_lut_wide, quant = g.quantize, alike for all of them
void launch_fused_bounds(int layout, bool wide, bool quant, const FusedPairView* pairs, const FusedEval* evals, const uint2* items, unsigned nitems, double2* partials,
                         hipStream_t s);
void launch_fused_finalize(const FusedEval* evals, int nevals, const double2* partials, float* out_lb, float* out_ub, hipStream_t s);
// trimmed pairs: the items' per-point e (and samples) into their rows of the arena; then one selection workgroup per row
void launch_fused_trim_bounds(int layout, bool wide, bool quant, const FusedPairView* pairs, const FusedEval* evals, const uint2* items, unsigned nitems, float* arena,
                              hipStream_t s);
void launch_fused_trim_select(const FusedTrimRow* rows, int nrows, float* out_ub, float* out_lb, hipStream_t s);

// out_lb[i], out_ub[i] = float(sum over chunks), fixed order → bit-reproducible
void launch_bounds_finalize(const double2* partials, int nchunk, int total, float* out_lb, float* out_ub, const TickCut& cut, hipStream_t s);

void launch_lut_build(const float4* tgt_shifted, int nt, const LutGeom& g, float* lut_padded, hipStream_t s);
// zp[o] = {lut[o], lut[o + one z-slice]}: the z-paired copy the bounds kernel gathers from (kernels.hip)
void launch_lut_zpair(const float* lut_padded, const LutGeom& g, float2* zp, hipStream_t s);
void launch_lut_quad(const float* lut_padded, const LutGeom& g, float4* qd, hipStream_t s);
void launch_lut_quad_apron(const float* lut_padded, const LutGeom& g, float4* qd /* ceil(px/3)*ceil(py/2)*pz*8 quads */, hipStream_t s);
void launch_lut_zpair_apron(const float* lut_padded, const LutGeom& g, float2* zp /* ceil(px/3)*ceil(py/3)*pz*16 z-pairs */, hipStream_t s);
void launch_lut_unpad(const float* lut_padded, const LutGeom& g, float* out, hipStream_t s);
void launch_lut_search(const float* lut, const LutGeom& g, const float* q_xyz, size_t n, float* out, hipStream_t s);
void launch_lut_nodes(const float* lut_padded, const LutGeom& g, const int* xyz /* device, n node indices (clamped into the grid) */, size_t n, float* out, hipStream_t s);

// Exact nearest neighbour (brute force, tiled through LDS).
//   queries: if `apply` q_i = R*pts_i + t (fma convention) else q_i = pts_i.
//   min_bits[i] = bit pattern of min_j |q_i - tgt_j|^2 (must be pre-filled with bits(1e10f)).
void launch_fill_u32(uint32_t* p, uint32_t v, size_t n, hipStream_t s);
void launch_nn_min(const float4* pts, int n, const float4* tgt, int nt, const float* R9, const float* t3, int apply,
                   uint32_t* min_bits, hipStream_t s);
// thr_bits[i] = largest float x with sqrtf(x) == sqrtf(min_i): every target within it ties under
// glm::distance (icp3d.cu:20-25); first_idx must be pre-filled with 0x7fffffff.
void launch_nn_tie_threshold(const uint32_t* min_bits, int n, uint32_t* thr_bits, hipStream_t s);
void launch_nn_first_index(const float4* pts, int n, const float4* tgt, int nt, const uint32_t* thr_bits, uint32_t* first_idx,
                           hipStream_t s);

// Exact NN through the two-level box scan (bvh.hpp) — bit-identical to the brute-force kernels above.
//   want_index = 0: out[i] = bits(min squared distance);  1: out[i] = lowest index in the sqrt-tie set
// seed_idx (optional, may alias out): per query the caller-order index of some target point, e.g. the correspondence of the
// previous ICP pass; its distance tightens the pruning bound, the result is the same exact minimum.
void launch_nn_scan(const float4* pts, int n, const BvhView& t, const float* lut, const LutGeom& g, const float* R9, const float* t3, int apply,
                    int want_index, const float4* tgt, int nt, const uint32_t* seed_idx,
                    const float* skip_lb /* optional (trimmed): queries with skip_lb[i] > float(skip_u[0]) are left out */, const uint32_t* skip_u, uint32_t* out, hipStream_t s,
                    float4* writeback = nullptr /* optional, with apply: the moved queries are stored here (may be `pts`: kernRotateTranslateInplace folded in) */,
                    const float* rt_dev = nullptr /* optional: the motion (R[9], t[3]) is read from device memory instead of R9 / t3 */,
                    const int* done = nullptr /* optional: the kernel returns at once when *done != 0 */,
                    double* wsum = nullptr /* optional, n <= 262144: per group of 64 queries the wave-level sums of the reduction that follows the scan —
                                              index mode {sum query xyz, sum correspondence xyz} (6), distance mode the sum of the minima (1) */);
// The two scans of an ICP iteration in ONE walk (kernels.hip nn_scan_dual_kernel): set A = ptsA (moved by (RA, tA) when applyA; written back to
// `writeback`) -> lowest index of the sqrt-tie set in out_idx; set B = ptsB under (RB, tB) -> bits of the minimum in out_min.  Same results as
// launch_nn_scan with want_index = 1 / 0.  skip_*: trimmed mode, per set.  wsumA / wsumB: as launch_nn_scan's wsum.
void launch_nn_scan_dual(const float4* ptsA, const float* RA9, const float* tA3, int applyA, const float4* ptsB, const float* RB9, const float* tB3, int n, const BvhView& t,
                         const float* lut, const LutGeom& g, const float4* tgt, int nt, const uint32_t* seed_idx, const float* skip_lbA, const uint32_t* skip_uA,
                         const float* skip_lbB, const uint32_t* skip_uB, uint32_t* out_idx, uint32_t* out_min, float4* writeback, double* wsumA, double* wsumB, hipStream_t s);
// EXTENSION (trimmed Go-ICP): per query a rigorous bracket [lb, ub] of its nearest squared distance from the LUT (kernels.hip, nn_prep_kernel);
// box6 = the target's bounding box {minx,maxx,miny,maxy,minz,maxz}
void launch_nn_prep(const float4* pts, int n, const float* lut, const LutGeom& g, const float* R9, const float* t3, int apply, const float4* tgt, int nt,
                    const uint32_t* seed_idx, const float* box6, float* ub_out, float* lb_out, hipStream_t s);
void launch_lut_build_scan(const BvhView& shifted_targets, const LutGeom& g, float* scratch_padded, float* lut_padded, hipStream_t s, uint32_t* lut_idx_padded = nullptr);  // lut_idx: optional, per node the caller index of a nearest target

// deterministic double sums: out[k] = sum_i vals[i*stride + k]  (k < width <= 16)
void launch_sum_f32_as_f64(const uint32_t* bits, int n, double* block_partials, int nblocks, hipStream_t s, const int* done = nullptr);
void launch_sum_partials(const double* block_partials, int nblocks, int width, double* out, hipStream_t s);

// ICP pieces (fgoicp/icp3d.cu:30-52)
void launch_transform_inplace(float4* pts, int n, const float* R9, const float* t3, hipStream_t s);
void launch_icp_sums(const float4* work, const float4* tgt, const uint32_t* idx, int n, int nt, const unsigned char* use_or_null,
                     double* block_partials, int nblocks, hipStream_t s, const int* done = nullptr);  // width 6: sum src xyz, sum corr xyz
void launch_icp_centroids(const double* block_partials, int nblocks, int ns, float* cen_dev, float* cen_host, hipStream_t s);
void launch_icp_cov(const float4* work, const float4* tgt, const uint32_t* idx, int n, int nt, const float* cen_dev, const unsigned char* use_or_null,
                    double* block_partials, int nblocks, hipStream_t s);  // width 9: glm mat3 order


// icp_cov with the centroid kernel folded in (same bits); cen_out receives the six centroid components
// sums_bp: block partials of icp_sums_kernel (from_waves = 0) or the per-wave sums of the scan's epilogue (from_waves = their count)
void launch_icp_cov_cen(const float4* work, const float4* tgt, const uint32_t* idx, int n, int nt, const double* sums_bp, int sums_nblocks, int from_waves,
                        float* cen_out, double* block_partials, int nblocks, hipStream_t s, const int* done = nullptr);

int reduce_blocks_for(int n);

}  // namespace fgoicp
