// Operator-level C ABI (include/fgoicp_amd.h): one context = one HIP device + one stream + all
// device memory of icp::Registration / icp::NearestNeighborLUT / icp::IterativeClosestPoint3D.
// No CPU fallback: without a HIP device fgoicp_ctx_create fails with FGOICP_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <limits>
#include <memory>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/fgoicp_amd.h"
#include "../host/math3.hpp"
#include "../host/knobs.hpp"
#include "ctx.hpp"
#include "kernels.hpp"
#include "arena.hpp"
#include "morton.hpp"

namespace fgoicp {

thread_local std::string g_last_error;
void set_error(const std::string& s) { g_last_error = s; }

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_error(std::string(#expr) + " failed: " + hipGetErrorString(e_));                        \
            return e_ == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP;                         \
        }                                                                                              \
    } while (0)

// Waiting for the device with the host's latency in mind.  hipEventSynchronize / hipStreamSynchronize park the thread in the runtime (the wake-up
// costs 5-8 us on this image); the ICP loop pays that twice per iteration and an iteration is 45-55 us at 40k points.  These poll the event /
// stream for a bounded time first (an iteration's kernels are tens of microseconds) and fall back to the blocking call for long waits.
// MEASURED (profiles/r04_ab_spin_sync.txt): nothing — 54.7-55.9 us per ICP iteration blocking against 54.7-60.3 polling, every bench leg within noise: the
// runtime's own wait is not what an iteration's 18-us host turn-around consists of.  OFF (0) by default; FGOICP_SPIN_SYNC_US=<us> is the development knob.
static const int g_spin_sync_us = [] { const char* e = dev_env("FGOICP_SPIN_SYNC_US"); return e ? std::atoi(e) : 0; }();
template <class Query, class Block>
static hipError_t spin_then_block(Query query, Block block) {
    if (g_spin_sync_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; ++spins) {
            const hipError_t q = query();
            if (q != hipErrorNotReady) return q;
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if ((spins & 15u) == 15u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(g_spin_sync_us)) break;
        }
    }
    return block();
}
static hipError_t wait_event(hipEvent_t ev) { return spin_then_block([&] { return hipEventQuery(ev); }, [&] { return hipEventSynchronize(ev); }); }
static hipError_t wait_stream(hipStream_t st) { return spin_then_block([&] { return hipStreamQuery(st); }, [&] { return hipStreamSynchronize(st); }); }

int ctx_flush_profile(fgoicp_ctx* c) {
    for (int i = 0; i < c->ev_used; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_start[i], c->ev_stop[i]));
        c->prof_ms += ms;
        static const bool tick_log = dev_env("FGOICP_TICK_LOG") != nullptr;  // debugging aid: one line per bounds launch on stderr
        if (tick_log && i < (int)c->ev_evals.size()) std::fprintf(stderr, "[tick] evals %d us %.1f\n", c->ev_evals[i], ms * 1e3);
        if (c->ev_has_sel[i]) {  // trimmed mode: the selection kernel of the same window (side stream)
            HIPCHK(hipEventSynchronize(c->ev_sel_stop[i]));
            HIPCHK(hipEventElapsedTime(&ms, c->ev_sel_start[i], c->ev_sel_stop[i]));
            c->prof_sel_ms += ms;
            c->ev_has_sel[i] = 0;
        }
    }
    c->ev_used = 0;
    return FGOICP_OK;
}

// -------------------------------------------------------------------------------------------
// Registration::compute_sse_error(RotNode&, vector<TransNode>&, bool, StreamPool&) for G groups,
// locality-sorted whole-tick path: descriptors -> device, sort the (subcube, chunk) items by LUT
// cell, one bounds launch, one finalize, one host sync per window of <= max_subcubes subcubes.
// -------------------------------------------------------------------------------------------
namespace {
struct TickTiming {  // FGOICP_TIMING=1: where a tick's wall time goes (host side), printed at context destruction
    bool on = dev_env("FGOICP_TIMING") != nullptr;
    double pack = 0, enqueue = 0, wait = 0, copyout = 0;
    uint64_t ticks = 0;
};
TickTiming g_tt;
constexpr float kNoCut = std::numeric_limits<float>::infinity();  // TickSub::cut0 / cut1 of a group without a threshold
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

// Device half of a window whose descriptors sit in the slot's staging buffers (sl.win_groups groups, sl.win_evals evaluations,
// sl.win_rows output rows): descriptors -> device, locality sort of the (evaluation, chunk) items, one bounds launch, one
// finalize (or, trimmed, one selection).  Called again by tick_wait_window if the sort check failed.
static int tick_launch_window(fgoicp_ctx* c, fgoicp_ctx::TickSlot& sl) {
    const int ng = sl.win_groups, neval = sl.win_evals, rows = sl.win_rows;
    // A small tick (the tail of a round: a few long-running tasks left, or one of many ranks) is pure latency: its bounds
    // kernel reads the descriptors straight from the pinned staging buffers and takes the items in submission order —
    // two copies and four sort launches fewer on the critical path.  Results do not depend on the item order.
    // windows with thresholds: an item may span several chunks (fewer workgroups to dispatch for the items that end early)
    const int span = sl.win_cut ? c->cut_span : 1;
    const int per_eval = (c->nchunk1 + span - 1) / span;  // work items per evaluation
    const bool tiers = sl.win_cut && c->cut_tier_level > 0.0f;   // ... and its items in two tiers, the heavy ones first (launch_tick_sort)
    const size_t nitems = (size_t)neval * (size_t)per_eval;
    const bool small = nitems <= (size_t)c->small_tick_items;
    const TickGroup* dev_groups = small ? sl.h_groups.dev() : sl.d_groups;
    const TickSub* dev_subs = small ? sl.h_subs.dev() : sl.d_subs;
    TickCut cut;  // early exit of evaluations that have reached their group's threshold (fgoicp_bounds_submit_cut)
    if (sl.win_cut) { cut.acc = sl.d_cut_acc; cut.gate = sl.d_cut_gate; cut.row_cut = sl.d_row_cut; cut.row_term = sl.d_row_term; cut.stat = c->d_cut_stat; }
    if (tiers && !small) cut.tier_split = sl.d_cursor + kTickTierSplit;
    static const int cut_probe = [] { const char* e = dev_env("FGOICP_CUT_PROBE"); return e ? std::atoi(e) : 0; }();  // measurement of the early exit's own cost (tools/op_bench.py)
    cut.probe = cut_probe;
    *sl.h_sort_err = 0u;
    unsigned* fused_err = !small && c->sort_check ? sl.h_sort_err.dev() : nullptr;  // the bounds kernel checks the permutation it walks
    if (!small) {
        // descriptors + locality sort on the slot's side stream (overlaps the other slot's bounds kernel); the main stream joins behind it
        static const int upload_kernel = [] { const char* e = dev_env("FGOICP_UPLOAD_KERNEL"); return e ? std::atoi(e) : 1; }();  // tuning knob: 0 = two hipMemcpyAsync
        if (upload_kernel) {
            launch_tick_upload(sl.h_groups.dev(), sl.d_groups, ng, sl.h_subs.dev(), sl.d_subs, neval, sl.sort_stream);
        } else {
            HIPCHK(hipMemcpyAsync(sl.d_groups, sl.h_groups, sizeof(TickGroup) * ng, hipMemcpyHostToDevice, sl.sort_stream));
            HIPCHK(hipMemcpyAsync(sl.d_subs, sl.h_subs, sizeof(TickSub) * neval, hipMemcpyHostToDevice, sl.sort_stream));
        }
        ++c->sorted_ticks;
        const int fault = c->sort_fault_tick && c->sorted_ticks == (uint64_t)c->sort_fault_tick;
        launch_tick_sort(c->geom, span > 1 ? c->d_span_cen : c->d_chunk_cen, per_eval, sl.d_groups, sl.d_subs, neval, c->cell_shift, sl.d_keys, sl.d_ranks, sl.d_hist, sl.d_hist_xcd, sl.d_xoff, sl.d_block_sums, sl.d_cursor, sl.d_sorted,
                         c->sort_xcd ? 1 : 0, c->sort_check ? 1 : 0, fault, sl.sort_stream, tiers ? c->d_lut : nullptr, c->cut_tier_level / (float)c->ns,
                         sl.win_cut ? &cut : nullptr, sl.d_partials, c->nchunk1, span);
        HIPCHK(hipEventRecord(sl.sorted_ev, sl.sort_stream));
        HIPCHK(hipStreamWaitEvent(sl.stream, sl.sorted_ev, 0));
    } else if (sl.win_cut) {
        // (the sorted path's key kernel does this on its way: the gates of the window's evaluations and the partials of the chunks nobody evaluates)
        launch_tick_prefill(dev_subs, neval, c->nchunk1, cut, sl.d_partials, sl.stream);
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->profile) {
        if (c->ev_used == (int)c->ev_start.size()) {  // drain both slots before recycling events
            HIPCHK(hipStreamSynchronize(c->stream));
            int rc = ctx_flush_profile(c);
            if (rc) return rc;
        }
        e0 = c->ev_start[c->ev_used];
        e1 = c->ev_stop[c->ev_used];
        if ((int)c->ev_evals.size() <= c->ev_used) c->ev_evals.resize(c->ev_start.size(), 0);
        c->ev_evals[c->ev_used] = neval;
        c->ev_used++;
        c->prof_launches++;
        c->prof_subcubes += rows;
        c->prof_evals += neval;  // a twin pair is two subcubes and one evaluation
    }
    const bool cut_on = launch_bounds_sorted(c->d_src, (int)c->ns, c->d_lut_zp, c->lut_layout, c->geom, c->nchunk1, c->chunk_pts, dev_groups, dev_subs, neval, small ? nullptr : sl.d_sorted,
                                             sl.d_partials, c->inliers ? sl.d_evals : nullptr, c->erow, c->trim_samp_shift, fused_err, cut, span, e0, e1, sl.stream);
    if (cut_on) c->cut_items_offered += (size_t)neval * c->nchunk1;  // (counted in chunks, like the skipped ones: bounds_finalize_kernel)
    // the per-subcube sums run on the slot's side stream, so the main stream holds nothing but bounds kernels back to back
    hipStream_t fin = c->finalize_on_side ? sl.sort_stream : sl.stream;
    if (fin != sl.stream) {
        HIPCHK(hipEventRecord(sl.bounds_ev, sl.stream));
        HIPCHK(hipStreamWaitEvent(fin, sl.bounds_ev, 0));
    }
    if (c->inliers) {  // trimmed: per row one selection of the k smallest e, both sums from it
        const int pi = e0 ? c->ev_used - 1 : -1;
        if (pi >= 0) { HIPCHK(hipEventRecord(c->ev_sel_start[pi], fin)); c->ev_has_sel[pi] = 1; }
        launch_trim_rows(sl.d_evals, c->erow, (int)c->ns, (int)c->inliers, rows, sl.h_row_span.dev(), sl.h_ub.dev(), sl.h_lb.dev(), fin, c->trim_samp_shift, c->trim_margin, c->d_trim_stat);
        if (pi >= 0) HIPCHK(hipEventRecord(c->ev_sel_stop[pi], fin));
    } else
        launch_bounds_finalize(sl.d_partials, c->nchunk1, rows, sl.h_lb.dev(), sl.h_ub.dev(), cut_on ? cut : TickCut(), fin);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sl.done, fin));
    return FGOICP_OK;
}

// Enqueues the window [pos, pos+rows) of a submission on its slot: packs the descriptors (host), then tick_launch_window.
// Returns the window end.
static int tick_enqueue_window(fgoicp_ctx* c, fgoicp_ctx::TickSlot& sl, int G, const float* R9, const float* rot_span, const int* fix_rot,
                               const int* offsets, const float* tn4, const int* twin, const float* cut_above, const float* ub_below_span, int pos, int* end_out) {
    const double t0 = g_tt.on ? now_s() : 0;
    int g = 0;
    while (g < G && offsets[g + 1] <= pos) ++g;
    const int cap = c->inliers ? std::min(c->max_subcubes, c->vals_rows) : c->max_subcubes;  // subcubes per window
    int end = pos, ng = 0;
    sl.row_group.resize((size_t)cap);
    for (int gg = g; gg < G && ng < c->max_groups && end - pos < cap; ++gg) {
        TickGroup& tg = sl.h_groups[ng];
        std::memcpy(tg.R, R9 + 9 * gg, sizeof(tg.R));
        const float half_angle = rot_span[gg] * kSqrt3 * kPi / 2.0f;  // registration.cu:42
        tg.sin_half = std::sin(half_angle);
        tg.fix_rot = fix_rot[gg] ? 1 : 0;
        tg.pad_ = gg;  // the submission's group index (twin validation below)
        const int first = std::max(offsets[gg], pos);
        const int last = std::min(offsets[gg + 1], pos + cap);
        for (int i = first; i < last; ++i) sl.row_group[(size_t)(i - pos)] = ng;
        end = std::max(end, last);
        ++ng;
        if (last < offsets[gg + 1]) break;  // window full in the middle of a group
    }
    const int rows = end - pos;  // output rows of this window
    *end_out = end;
    if (rows <= 0) return FGOICP_OK;
    // terminal rows (fgoicp_bounds_submit_leaf): span below the group's ub_below_span, in a group with a threshold
    static const bool leaf_rule = [] { const char* e = dev_env("FGOICP_CUT_LEAF"); return !e || std::atoi(e) != 0; }();  // development build, A/B: 0 = every row by the lower-bound rule
    const auto terminal = [&](int sub_group, float span) { return leaf_rule && cut_above && ub_below_span && span < ub_below_span[sub_group]; };
    // evaluations: one per output row, or one per twin pair (both inside this window, same rotation, same translation node,
    // one in a fix_rot group and one not — checked here, the caller's hint is not trusted)
    int neval = 0;
    for (int r = 0; r < rows; ++r) {
        const int i = pos + r;
        const int gi = sl.row_group[(size_t)r];
        sl.h_row_span[r] = tn4[4 * (size_t)i + 3];
        int j = twin ? twin[i] : -1;
        if (j >= pos && j < end && j != i && twin[j] == i) {
            const int gj = sl.row_group[(size_t)(j - pos)];
            const TickGroup &a = sl.h_groups[gi], &b = sl.h_groups[gj];
            const bool ok = a.fix_rot != b.fix_rot && a.sin_half == b.sin_half && std::memcmp(a.R, b.R, sizeof(a.R)) == 0 &&
                            std::memcmp(tn4 + 4 * (size_t)i, tn4 + 4 * (size_t)j, 4 * sizeof(float)) == 0;
            if (ok) {
                if (j < i) continue;  // evaluated with its twin
                TickSub& ts = sl.h_subs[neval++];
                ts.tx = tn4[4 * (size_t)i]; ts.ty = tn4[4 * (size_t)i + 1]; ts.tz = tn4[4 * (size_t)i + 2]; ts.span = tn4[4 * (size_t)i + 3];
                ts.group = gi;
                ts.out0 = a.fix_rot ? r : j - pos;  // the fix_rot = 1 variant belongs to the fix_rot group's row
                ts.out1 = a.fix_rot ? j - pos : r;
                ts.dual = 1;
                const float ca = cut_above ? cut_above[a.pad_] : kNoCut, cb = cut_above ? cut_above[b.pad_] : kNoCut;  // (pad_: the submission's group index)
                ts.cut0 = a.fix_rot ? ca : cb;
                ts.cut1 = a.fix_rot ? cb : ca;
                const unsigned ta = terminal(a.pad_, ts.span) ? 1u : 0u, tb = terminal(b.pad_, ts.span) ? 1u : 0u;
                ts.term = a.fix_rot ? (ta * kSubTerm0 | tb * kSubTerm1) : (tb * kSubTerm0 | ta * kSubTerm1);
                ts.pad_ = 0;
                continue;
            }
        }
        TickSub& ts = sl.h_subs[neval++];
        ts.tx = tn4[4 * (size_t)i]; ts.ty = tn4[4 * (size_t)i + 1]; ts.tz = tn4[4 * (size_t)i + 2]; ts.span = tn4[4 * (size_t)i + 3];
        ts.group = gi;
        ts.out0 = r;
        ts.out1 = r;
        ts.dual = 0;
        ts.cut0 = ts.cut1 = cut_above ? cut_above[sl.h_groups[gi].pad_] : kNoCut;
        ts.term = terminal(sl.h_groups[gi].pad_, ts.span) ? kSubTerm0 : 0u;
        ts.pad_ = 0;
    }
    sl.win_cut = cut_above != nullptr && !c->inliers;
    for (int k = 0; k < ng; ++k) sl.h_groups[k].pad_ = 0;
    const double t1 = g_tt.on ? now_s() : 0;
    sl.win_pos = pos;
    sl.win_rows = rows;
    sl.win_groups = ng;
    sl.win_evals = neval;
    const int rc = tick_launch_window(c, sl);
    if (g_tt.on) { g_tt.pack += t1 - t0; g_tt.enqueue += now_s() - t1; g_tt.ticks++; }
    return rc;
}

static int tick_wait_window(fgoicp_ctx* c, fgoicp_ctx::TickSlot& sl) {
    const double t2 = g_tt.on ? now_s() : 0;
    HIPCHK(wait_event(sl.done));
    if (*sl.h_sort_err) {
        // The tick's `sorted` was not a permutation: the XCD-private histogram (workgroup-scope atomics, see kernels.hip) is
        // not a single point of coherence on this device.  Switch this context to device-scope atomics for good and repeat
        // the window (its descriptors are still in the staging buffers); a second failure is an error.
        c->sort_xcd = false;
        c->sort_fallbacks++;
        HIPCHK(hipStreamSynchronize(sl.sort_stream));
        HIPCHK(hipMemsetAsync(sl.d_hist, 0, sizeof(unsigned) * kTickNumKeys, sl.sort_stream));   // state a failed sort may have left
        HIPCHK(hipMemsetAsync(sl.d_hist_xcd, 0, sizeof(unsigned) * 16 * kTickNumKeys, sl.sort_stream));
        int rc = tick_launch_window(c, sl);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(sl.done));
        if (*sl.h_sort_err) { set_error("tick sort did not produce a permutation of the work items (device-scope atomics)"); return FGOICP_ERR_HIP; }
    }
#ifdef FGOICP_DEV_KNOBS
    // FGOICP_CUT_VERIFY=1 (development build): every window that carried thresholds is evaluated once more WITHOUT them and each row is checked against
    // the contract of fgoicp_bounds_submit_cut — at or above its threshold T in the exact evaluation: {T, T} was reported; below: the exact bits —
    // a terminal row (fgoicp_bounds_submit_leaf) by its own rule: "at or above" is said of its UPPER bound.
    // The answers handed on are the first run's, so the search goes on as it would; the tally is printed when the context is destroyed.
    const bool cut_verify = [] { const char* e = dev_env("FGOICP_CUT_VERIFY"); return e && std::atoi(e) != 0; }();  // (read per window: a test toggles it)
    if (cut_verify && sl.win_cut) {
        const int rows = sl.win_rows;
        std::vector<float> lb(sl.h_lb.get(), sl.h_lb + rows), ub(sl.h_ub.get(), sl.h_ub + rows);
        sl.win_cut = false;
        int rc = tick_launch_window(c, sl);
        sl.win_cut = true;
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(sl.done));
        if (*sl.h_sort_err) { set_error("FGOICP_CUT_VERIFY: the repeated window's sort failed"); return FGOICP_ERR_HIP; }
        for (int e = 0; e < sl.win_evals; ++e) {
            const TickSub& ts = sl.h_subs[e];
            for (int v = 0; v < (ts.dual ? 2 : 1); ++v) {
                const int r = v ? ts.out1 : ts.out0;
                const float T = v ? ts.cut1 : ts.cut0;
                const bool term = (ts.term & (v ? kSubTerm1 : kSubTerm0)) != 0u;
                const bool above = (term ? sl.h_ub[r] : sl.h_lb[r]) >= T;
                const bool ok = above ? (lb[(size_t)r] == T && ub[(size_t)r] == T)
                                      : (std::memcmp(&lb[(size_t)r], &sl.h_lb[r], 4) == 0 && std::memcmp(&ub[(size_t)r], &sl.h_ub[r], 4) == 0);
                c->cut_verify_rows++;
                c->cut_verify_above += above ? 1 : 0;
                if (!ok) {
                    if (c->cut_verify_bad++ < 5)
                        std::fprintf(stderr, "[fgoicp cut verify] row %d: threshold %.9g, exact {%.9g, %.9g}, reported {%.9g, %.9g}\n", r, (double)T, (double)sl.h_lb[r], (double)sl.h_ub[r],
                                     (double)lb[(size_t)r], (double)ub[(size_t)r]);
                }
            }
        }
        c->cut_verify_windows++;
        std::memcpy(sl.h_lb, lb.data(), sizeof(float) * rows);
        std::memcpy(sl.h_ub, ub.data(), sizeof(float) * rows);
    }
#endif
    const double t3 = g_tt.on ? now_s() : 0;
    std::memcpy(sl.lb.data() + sl.win_pos, sl.h_lb, sizeof(float) * sl.win_rows);
    std::memcpy(sl.ub.data() + sl.win_pos, sl.h_ub, sizeof(float) * sl.win_rows);
    if (g_tt.on) { g_tt.wait += t3 - t2; g_tt.copyout += now_s() - t3; }
    return FGOICP_OK;
}

// fgoicp_bounds_submit: all windows but the last are completed here, the last one stays in flight.
int ctx_bounds_submit(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                      const float* tn4, const int* twin, const float* cut_above, const float* ub_below_span) {
    HIPCHK(hipSetDevice(c->device));
    fgoicp_ctx::TickSlot& sl = c->slots[slot];
    if (sl.inflight) { set_error("fgoicp_bounds_submit: slot still in flight (collect it first)"); return FGOICP_ERR_INVALID_ARG; }
    sl.total = offsets[G];
    sl.lb.resize(sl.total);
    sl.ub.resize(sl.total);
    sl.win_rows = 0;
    int pos = 0;
    while (pos < sl.total) {
        int end = pos;
        int rc = tick_enqueue_window(c, sl, G, R9, rot_span, fix_rot, offsets, tn4, twin, cut_above, ub_below_span, pos, &end);
        if (rc) return rc;
        if (end <= pos) break;
        pos = end;
        if (pos < sl.total) {  // more windows follow: this one has to be drained first (its buffers are reused)
            rc = tick_wait_window(c, sl);
            if (rc) return rc;
            sl.win_rows = 0;
        }
    }
    sl.inflight = true;
    return FGOICP_OK;
}

// Items (evaluation x chunk of source points) of the windows submitted with thresholds since the last reset, and how many of
// them the early exit did not evaluate.  Call between submissions (it synchronises the context's streams).
int ctx_cut_stats(fgoicp_ctx* c, uint64_t* items_offered, uint64_t* items_cut, int reset) {
    HIPCHK(hipSetDevice(c->device));
    unsigned long long now = 0;
    if (c->d_cut_stat) {
        unsigned long long part[kCutStatSlots];
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(part, c->d_cut_stat, sizeof(part), hipMemcpyDeviceToHost));
        for (unsigned long long v : part) now += v;
    }
    if (items_offered) *items_offered = c->cut_items_offered;
    if (items_cut) *items_cut = (uint64_t)now - c->cut_stat_base;
    if (reset) { c->cut_items_offered = 0; c->cut_stat_base = (uint64_t)now; }
    return FGOICP_OK;
}

int ctx_bounds_collect(fgoicp_ctx* c, int slot, float* lb_out, float* ub_out) {
    HIPCHK(hipSetDevice(c->device));
    fgoicp_ctx::TickSlot& sl = c->slots[slot];
    if (!sl.inflight) { set_error("fgoicp_bounds_collect: nothing submitted on this slot"); return FGOICP_ERR_INVALID_ARG; }
    if (sl.win_rows > 0) {
        int rc = tick_wait_window(c, sl);
        if (rc) return rc;
    }
    sl.inflight = false;
    std::memcpy(lb_out, sl.lb.data(), sizeof(float) * sl.total);
    std::memcpy(ub_out, sl.ub.data(), sizeof(float) * sl.total);
    if (c->profile && !c->slots[0].inflight && !c->slots[1].inflight) {
        int rc = ctx_flush_profile(c);
        if (rc) return rc;
    }
    return FGOICP_OK;
}

// -------------------------------------------------------------------------------------------
// Registration::compute_sse_error(RotNode&, vector<TransNode>&, bool, StreamPool&) for G groups: one submission on slot 0, collected at once.
// -------------------------------------------------------------------------------------------
int ctx_bounds_multi(fgoicp_ctx* c, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                     const float* tn4, float* lb_out, float* ub_out, const float* cut_above) {
    HIPCHK(hipSetDevice(c->device));
    int rc = ctx_bounds_submit(c, 0, G, R9, rot_span, fix_rot, offsets, tn4, nullptr, cut_above);
    if (rc) return rc;
    return ctx_bounds_collect(c, 0, lb_out, ub_out);
}

// ---- host-side final folds of the fused reductions (small clouds) -----------------------------------------------------------------
// The device reduces in three levels: the shuffle tree of a wave (kernels.hip wave_sum: v[i] += v[i + off], off = 32 .. 1), the four
// waves of a block in order, then sum_partials_kernel / icp_centroids_kernel over the blocks (lane-strided partial sums + the same
// tree).  With the first level done in the scan's epilogue, the rest are a few hundred additions: done here, in the device's
// order, on values the kernels wrote straight into pinned memory — the same bits, two launches less per pass.
static double tree64(double (&v)[64]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    return v[0];
}
static double fold_blocks(const double* bp, int nblocks, int width, int k) {  // sum_partials_kernel
    double lane[64] = {0};
    for (int b = 0; b < nblocks; ++b) lane[b & 63] += bp[(size_t)b * width + k];
    return tree64(lane);
}
static double fold_wave_sums(const double* w, int nwaves) {  // block_sum<1> of sum_f32_kernel over the waves, then sum_partials_kernel
    double lane[64] = {0};
    const int nblocks = (nwaves + 3) / 4;
    for (int b = 0; b < nblocks; ++b) {
        double blk = w[4 * b];
        for (int k = 1; k < 4; ++k) blk += 4 * b + k < nwaves ? w[4 * b + k] : 0.0;
        lane[b & 63] += blk;
    }
    return tree64(lane);
}
static bool icp_fused(const fgoicp_ctx* c) { return c->icp_fuse && !c->brute_force_nn && !c->inliers && c->ns <= 262144; }

static bool trim_skips(const fgoicp_ctx* c) { return c->inliers && c->trim_skip; }

// the caller index of every device slot, on the device: allocated by the first call that needs it (trimmed ICP, the alignment report, source normals)
static int ensure_orig_of_slot(fgoicp_ctx* c) {
    if (c->d_orig_of_slot) return FGOICP_OK;
    HIPCHK(c->d_orig_of_slot.alloc(c->ns));
    HIPCHK(hipMemcpy(c->d_orig_of_slot, c->perm.data(), sizeof(uint32_t) * c->ns, hipMemcpyHostToDevice));
    return FGOICP_OK;
}
// the working cloud: a copy of the source moved by (R0, t0) — icp3d.cu:85
static int work_begin_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R0, const float* t0, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(L.d_work, c->d_src, sizeof(float4) * c->ns, hipMemcpyDeviceToDevice, st));
    launch_transform_inplace(L.d_work, (int)c->ns, R0, t0, st);
    return FGOICP_OK;
}

// Trimmed search: the LUT brackets of one query set's nearest distances (launch_nn_prep) and the cut among their upper ends
// (launch_trim_select).  The exact scan that follows leaves out the queries whose lower end `lb` lies above the cut `sel`.
struct TrimQueries {
    const float4* pts;
    const float *R9, *t3;  // the motion the scan applies to pts (null: none)
    float *ub, *lb;
    uint32_t *sel, *wide;
};
static TrimQueries trim_working(const fgoicp_ctx::IcpLane& L, uint32_t* wide) { return {L.d_work, nullptr, nullptr, L.d_nn_ub2, L.d_nn_lb2, L.d_sel + 4, wide}; }
static TrimQueries trim_pristine(const fgoicp_ctx* c, const fgoicp_ctx::IcpLane& L, const float* R9, const float* t3) {  // the source under (R, t)
    return {c->d_src, R9, t3, L.d_nn_ub, L.d_nn_lb, L.d_sel + 8, L.d_sel_wide};
}
static void trim_prep(const fgoicp_ctx* c, const TrimQueries& q, const uint32_t* seed_idx, hipStream_t st) {
    launch_nn_prep(q.pts, (int)c->ns, c->d_lut, c->geom, q.R9, q.t3, q.R9 ? 1 : 0, c->d_tgt, (int)c->nt, seed_idx, c->tgt_box6, q.ub, q.lb, st);
}
static void trim_cut(const fgoicp_ctx* c, const TrimQueries& q, hipStream_t st) { launch_trim_select(q.ub, (int)c->ns, (int)c->inliers, nullptr, q.sel, q.wide, st); }
static void trim_brackets(const fgoicp_ctx* c, const TrimQueries& q, const uint32_t* seed_idx, hipStream_t st) {
    trim_prep(c, q, seed_idx, st);
    trim_cut(c, q, st);
}

// float Registration::compute_sse_error(glm::mat3, glm::vec3) — registration.cu:62-86.  Enqueue only: the result lands in
// pinned memory (sse_result) once `st` has drained.  Two halves, the search and the sum (the ICP loop interleaves the launches of its
// two streams: both long scans first — a launch costs the submitting thread ~5 us, and whatever is enqueued last starts that much later).
static int sse_search_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R9, const float* t3, const uint32_t* seed_idx, bool fused, bool skip, hipStream_t st) {
    const int ns = (int)c->ns;
    if (fused) {  // one launch: the scan leaves the wave-level sums of its minima in pinned memory, sse_result() folds them
        launch_nn_scan(c->d_src, ns, c->bvh_tgt.view(), c->d_lut, c->geom, R9, t3, 1, 0, c->d_tgt, (int)c->nt, seed_idx, nullptr, nullptr, L.d_min_bits, st, nullptr, nullptr, nullptr,
                       L.h_wsse.dev());
    } else if (c->brute_force_nn) {
        launch_fill_u32(L.d_min_bits, 0x501502F9u /* bits(1e10f) */, c->ns, st);
        launch_nn_min(c->d_src, ns, c->d_tgt, (int)c->nt, R9, t3, 1, L.d_min_bits, st);
    } else {
        const TrimQueries q = trim_pristine(c, L, R9, t3);
        if (skip) trim_brackets(c, q, seed_idx, st);  // trimmed: queries provably beyond the k-th smallest distance are left out of the exact search
        launch_nn_scan(c->d_src, ns, c->bvh_tgt.view(), c->d_lut, c->geom, R9, t3, 1, 0, c->d_tgt, (int)c->nt, seed_idx, skip ? q.lb : nullptr, skip ? q.sel : nullptr, L.d_min_bits, st);
    }
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
// ... and the sum over the minima in `mins` (trimmed: the k smallest nearest-neighbour terms); fused: the search has left it in pinned memory
static int sse_sum_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const uint32_t* mins, bool fused, hipStream_t st) {
    const int ns = (int)c->ns;
    L.sse_on_host = fused;
    if (fused) {
    } else if (c->inliers) {
        launch_trim_select(reinterpret_cast<const float*>(mins), ns, (int)c->inliers, L.h_trim.dev(), nullptr, L.d_sel_wide, st);
    } else {
        const int nb = reduce_blocks_for(ns);
        launch_sum_f32_as_f64(mins, ns, L.d_bp3, nb, st);
        launch_sum_partials(L.d_bp3, nb, 1, L.h_sums.dev() + 12, st);
    }
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
static int sse_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R9, const float* t3, const uint32_t* seed_idx, hipStream_t st, bool may_skip = true) {
    const bool fused = icp_fused(c);
    const int rc = sse_search_enqueue(c, L, R9, t3, seed_idx, fused, may_skip && trim_skips(c), st);
    return rc ? rc : sse_sum_enqueue(c, L, L.d_min_bits, fused, st);
}
static float sse_result(const fgoicp_ctx* c, const fgoicp_ctx::IcpLane& L) {
    if (L.sse_on_host) return (float)fold_wave_sums(L.h_wsse, (int)((c->ns + 63) / 64));
    return c->inliers ? L.h_trim[0] : (float)L.h_sums[12];
}

static int lane_sse(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R9, const float* t3, float* sse_out, const uint32_t* seed_idx) {
    int rc = sse_enqueue(c, L, R9, t3, seed_idx, L.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(L.stream));
    *sse_out = sse_result(c, L);
    return FGOICP_OK;
}
int ctx_sse(fgoicp_ctx* c, const float* R9, const float* t3, float* sse_out, const uint32_t* seed_idx) {
    HIPCHK(hipSetDevice(c->device));
    return lane_sse(c, c->lanes[0], R9, t3, sse_out, seed_idx);
}

// EXTENSION: the alignment report (fgoicp_alignment) for the pristine source under (R, t), on lane 0.
//   1. the minima by the path fgoicp_sse takes for this context (sse_enqueue: fused scan, tree scan or brute force; its sum is the
//      summary's sse, so the bits are fgoicp_sse's by construction) — with the trimmed skip off, so that every query is searched; the k
//      smallest minima and the fixed order of their sum do not change, the skipped queries' stand-ins lay above the cut like the true
//      minima they replace;
//   2. the correspondences by a second walk in index mode (nn_scan_kernel<1> returns the index, not the minimum), or the brute-force
//      tie-set kernels on the moved cloud;
//   3. trimmed: the inlier mask from those exact minima (selection + mask + ties, launch_inlier_mask);
//   4. device order -> caller order, target marks and the integer summary (launch_align_scatter).
// Everything written is scratch that every other path fills before it reads (d_min_bits, d_work, d_thr_bits, d_sel, d_eq, d_use, the
// pinned sums) or the report's own allocation; d_first_idx / d_first_idx2, the seeds of a later ICP pass, are not touched.
// The device half: everything above is enqueued on lane 0's stream, nothing is waited for.
// keep_moved: the index scan also stores its moved queries R p + t in L.d_work, device order (ctx_plane_moments reads them; the brute-force
// path has them there anyway).
static int alignment_enqueue(fgoicp_ctx* c, const float* R9, const float* t3, bool keep_moved = false) {
    HIPCHK(hipSetDevice(c->device));
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    fgoicp_ctx::AlignScratch& A = c->align;
    const int ns = (int)c->ns, nt = (int)c->nt;
    int rc = ensure_orig_of_slot(c);  // untrimmed contexts have had no use for it so far
    if (rc) return rc;
    if (!A.base) {
        A.nt16 = (c->nt + 15) & ~(size_t)15;
        const size_t nblk = (c->ns + kBlock - 1) / kBlock;
        Arena plan;
        plan.take(A.d_idx, c->ns);
        plan.take(A.d_corr, c->ns);
        plan.take(A.d_d2, c->ns);
        plan.take(A.d_inl, c->ns);
        plan.take(A.d_hit, A.nt16);
        plan.take(A.d_partials, nblk);
        plan.take(A.d_sum, 3);
        static_assert(sizeof(MomentRow<kAlignInfoTerms>) == 88 && kAlignInfoTerms == 10 && kBlock == 256, "tests/host_harness/arena_check.cpp restates these");
        plan.take(A.d_info_rows, nblk);
        plan.take(A.d_info, 1 + kAlignInfoTerms);
        HIPCHK(A.base.alloc(plan.total()));
        plan.place(A.base);
    }
    hipStream_t st = L.stream;
    rc = sse_enqueue(c, L, R9, t3, nullptr, st, false);
    if (rc) return rc;
    if (c->brute_force_nn) {  // kernFindNearestNeighbor (icp3d.cu:11-28) as procrustes_enqueue runs it, on the source moved as the scan's queries are
        rc = work_begin_enqueue(c, L, R9, t3, st);
        if (rc) return rc;
        launch_fill_u32(A.d_idx, 0x7fffffffu, c->ns, st);
        launch_nn_tie_threshold(L.d_min_bits, ns, L.d_thr_bits, st);
        launch_nn_first_index(L.d_work, ns, c->d_tgt, nt, L.d_thr_bits, A.d_idx, st);
    } else {
        launch_nn_scan(c->d_src, ns, c->bvh_tgt.view(), c->d_lut, c->geom, R9, t3, 1, 1, c->d_tgt, nt, nullptr, nullptr, nullptr, A.d_idx, st, keep_moved ? L.d_work : nullptr);
    }
    const unsigned char* use = nullptr;
    if (c->inliers) {
        launch_inlier_mask(reinterpret_cast<const float*>(L.d_min_bits.get()), ns, (int)c->inliers, L.d_sel, L.d_eq, c->d_orig_of_slot, L.d_use, L.d_sel_wide, st);
        use = L.d_use;
    }
    HIPCHK(hipMemsetAsync(A.d_hit, 0, A.nt16, st));
    launch_align_scatter(A.d_idx, L.d_min_bits, use, c->d_orig_of_slot, ns, nt, A.d_corr, A.d_d2, A.d_inl, A.d_hit, A.nt16, A.d_partials, A.d_sum, st);
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
// The copy-out half: waits for lane 0's stream and hands the report over; every output may be null.
static int alignment_copy_out(fgoicp_ctx* c, uint32_t* corr_idx, float* dist2, uint8_t* inlier, uint8_t* target_hit, fgoicp_alignment_summary* out) {
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    fgoicp_ctx::AlignScratch& A = c->align;
    HIPCHK(hipStreamSynchronize(L.stream));
    uint32_t sum3[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(sum3, A.d_sum, sizeof(sum3), hipMemcpyDeviceToHost));
    if (corr_idx) HIPCHK(hipMemcpy(corr_idx, A.d_corr, sizeof(uint32_t) * c->ns, hipMemcpyDeviceToHost));
    if (dist2) HIPCHK(hipMemcpy(dist2, A.d_d2, sizeof(float) * c->ns, hipMemcpyDeviceToHost));
    if (inlier) HIPCHK(hipMemcpy(inlier, A.d_inl, c->ns, hipMemcpyDeviceToHost));
    if (target_hit) HIPCHK(hipMemcpy(target_hit, A.d_hit, c->nt, hipMemcpyDeviceToHost));
    if (out) {
        out->points = c->ns;
        out->inliers = sum3[0];
        out->targets_hit = sum3[1];
        out->sse = sse_result(c, L);
        std::memcpy(&out->max_inlier_dist2, &sum3[2], sizeof(float));
        out->scaling_factor = 1.0f;
    }
    return FGOICP_OK;
}
int ctx_alignment(fgoicp_ctx* c, const float* R9, const float* t3, uint32_t* corr_idx, float* dist2, uint8_t* inlier, uint8_t* target_hit,
                  fgoicp_alignment_summary* out) {
    const int rc = alignment_enqueue(c, R9, t3);
    return rc ? rc : alignment_copy_out(c, corr_idx, dist2, inlier, target_hit, out);
}

// EXTENSION: the moments behind the information matrix (fgoicp_information), enqueued behind the report's device half on the same stream:
// one scan of the report's caller-order arrays (the report has just written them), one gather of the target per counted point.  Writes
// the report's own allocation only.
static int information_enqueue(fgoicp_ctx* c, float max_dist2) {
    fgoicp_ctx::AlignScratch& A = c->align;
    launch_align_info(A.d_inl, A.d_d2, A.d_corr, c->d_tgt, (int)c->ns, (int)c->nt, max_dist2, A.d_info_rows, A.d_info, c->lanes[0].stream);
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
static int information_copy_out(fgoicp_ctx* c, InfoMoments* m) {
    HIPCHK(hipStreamSynchronize(c->lanes[0].stream));
    unsigned long long h[1 + kAlignInfoTerms];
    HIPCHK(hipMemcpy(h, c->align.d_info, sizeof(h), hipMemcpyDeviceToHost));
    double v[kAlignInfoTerms];
    std::memcpy(v, h + 1, sizeof(v));
    m->n = h[0];
    for (int k = 0; k < 3; ++k) m->sum_q[k] = v[k];
    for (int k = 0; k < 6; ++k) m->sum_qq[k] = v[3 + k];
    m->sum_d2 = v[9];
    return FGOICP_OK;
}
int ctx_information(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, InfoMoments* m) {
    int rc = alignment_enqueue(c, R9, t3);
    if (!rc) rc = information_enqueue(c, max_dist2);
    return rc ? rc : information_copy_out(c, m);
}
int ctx_alignment_information(fgoicp_ctx* c, const float* R9, const float* t3, uint32_t* corr_idx, float* dist2, uint8_t* inlier, uint8_t* target_hit,
                              fgoicp_alignment_summary* out, float max_dist2, InfoMoments* m) {
    int rc = alignment_enqueue(c, R9, t3);
    if (!rc) rc = information_enqueue(c, max_dist2);
    if (!rc) rc = alignment_copy_out(c, corr_idx, dist2, inlier, target_hit, out);
    return rc ? rc : information_copy_out(c, m);
}

// What the entry points of the target's and the source's normals share.
// given normals: each checked (finite, not zero) and normalised in fp64 -> {x, y, z, 0}; `where` names the entry point in the message
static int unit_normals(const char* where, const float* normals, size_t n, std::vector<float4>& out) {
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const double x = normals[3 * i], y = normals[3 * i + 1], z = normals[3 * i + 2];
        const double len = std::sqrt(x * x + y * y + z * z);
        if (!std::isfinite(len) || !(len > 0.0)) {
            set_error(std::string(where) + ": normal " + std::to_string(i) + " is zero or not finite");
            return FGOICP_ERR_INVALID_ARG;
        }
        out[i] = make_float4((float)(x / len), (float)(y / len), (float)(z / len), 0.f);
    }
    return FGOICP_OK;
}
// the neighbour count of target_knn_kernel over a cloud ("target" / "source") of n points
static int knn_k_ok(const char* where, int k, size_t n, const char* cloud) {
    if (k >= kKnnMin && k <= kKnnMax && (size_t)k <= n) return FGOICP_OK;
    set_error(std::string(where) + ": k must lie in [4, 32] and be at most the number of " + cloud + " points");
    return FGOICP_ERR_INVALID_ARG;
}
// out[3 * (perm ? perm[i] : i) ..] = the three floats of the device's d[i], i < n, behind the work queued on lane 0
static int read_back_xyz(fgoicp_ctx* c, const float4* d, size_t n, const uint32_t* perm, float* out) {
    HIPCHK(hipSetDevice(c->device));
    std::vector<float4> h(n);
    HIPCHK(hipStreamSynchronize(c->lanes[0].stream));
    HIPCHK(hipMemcpy(h.data(), d, sizeof(float4) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        float* o = out + 3 * (perm ? (size_t)perm[i] : i);
        o[0] = h[i].x; o[1] = h[i].y; o[2] = h[i].z;
    }
    return FGOICP_OK;
}

// EXTENSION: target normals (fgoicp_ctx_set_target_normals).  Given: checked and normalised on the host (fp64), uploaded.  Estimated:
// target_knn_kernel over the target's own tree, one launch.
int ctx_set_target_normals(fgoicp_ctx* c, const float* normals, int k) {
    const size_t nt = c->nt;
    std::vector<float4> h;
    if (normals) {
        if (int rc = unit_normals("fgoicp_ctx_set_target_normals", normals, nt, h)) return rc;
    } else {
        if (int rc = knn_k_ok("fgoicp_ctx_set_target_normals", k, nt, "target")) return rc;
        if (c->brute_force_nn) { set_error("fgoicp_ctx_set_target_normals: estimating normals needs the search tree, which a brute-force context does not build: pass normals"); return FGOICP_ERR_INVALID_ARG; }
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->d_normals.ensure(nt));
    hipStream_t st = c->lanes[0].stream;
    c->normals_set = false;
    if (normals) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(c->d_normals, h.data(), sizeof(float4) * nt, hipMemcpyHostToDevice));
    } else {
        launch_target_knn(c->bvh_tgt.view(), c->d_tgt, (int)nt, k, nullptr, nullptr, c->d_normals, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    c->normals_set = true;
    return FGOICP_OK;
}
int ctx_target_normals(fgoicp_ctx* c, float* out) {
    if (!c->normals_set) { set_error("fgoicp_target_normals: the target normals are not set (fgoicp_ctx_set_target_normals)"); return FGOICP_ERR_INVALID_ARG; }
    return read_back_xyz(c, c->d_normals, c->nt, nullptr, out);
}
int ctx_target_knn(fgoicp_ctx* c, int k, uint32_t* idx, float* d2) {
    if (int rc = knn_k_ok("fgoicp_target_knn", k, c->nt, "target")) return rc;
    if (c->brute_force_nn) { set_error("fgoicp_target_knn: needs the search tree, which a brute-force context does not build"); return FGOICP_ERR_INVALID_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const size_t n = c->nt * (size_t)k;
    Dev<uint32_t> d_idx;
    Dev<float> d_d2;
    hipError_t e = hipSuccess;
    if (idx) e = d_idx.alloc(n);
    if (e == hipSuccess && d2) e = d_d2.alloc(n);
    hipStream_t st = c->lanes[0].stream;
    if (e == hipSuccess) {
        launch_target_knn(c->bvh_tgt.view(), c->d_tgt, (int)c->nt, k, d_idx, d_d2, nullptr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && idx) e = hipMemcpy(idx, d_idx, sizeof(uint32_t) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && d2) e = hipMemcpy(d2, d_d2, sizeof(float) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error(std::string("fgoicp_target_knn: ") + hipGetErrorString(e)); return e == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP; }
    return FGOICP_OK;
}

// EXTENSION: the refinements (fgoicp_plane_moments, fgoicp_gicp_moments, fgoicp_robust_*, the three loops; DESIGN.md sections 12, 15, 19).
// What every one of their context entry points refuses before any device work, in this order (each only where it applies):
//   the scale is not finite (ScaleCheck::or_estimated); max_dist2; the model; the loss; epsilon (Generalized ICP); the scale is not finite
//   and > 0 (ScaleCheck::given, a loss other than none); the target normals; the source normals (Generalized ICP)
int refine_refusals(const fgoicp_ctx* c, const RefineSpec& r, ScaleCheck scale, const char* where) {
    const std::string w(where);
    if (scale == ScaleCheck::or_estimated && !std::isfinite(r.scale)) { set_error(w + ": the scale must be finite (<= 0: estimated)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(r.max_dist2 >= 0.0f)) { set_error(w + ": max_dist2 must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_model_ok(r.model)) { set_error(w + ": unknown model " + std::to_string(r.model) + " (0: point-to-plane, 1: Generalized ICP)"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_loss_ok(r.loss)) { set_error(w + ": unknown loss " + std::to_string(r.loss)); return FGOICP_ERR_INVALID_ARG; }
    if (r.model == FGOICP_MODEL_GICP && !gicp_epsilon_ok(r.epsilon)) { set_error(w + ": epsilon must be finite and lie in (0, 1]"); return FGOICP_ERR_INVALID_ARG; }
    if (scale == ScaleCheck::given && r.loss != FGOICP_LOSS_NONE && !robust_scale_ok(r.scale)) { set_error(w + ": the scale must be finite and > 0"); return FGOICP_ERR_INVALID_ARG; }
    if (!c->normals_set) { set_error(w + ": the target normals are not set: call fgoicp_ctx_set_target_normals first"); return FGOICP_ERR_INVALID_ARG; }
    if (r.model == FGOICP_MODEL_GICP && !c->src_normals_set) { set_error(w + ": the source normals are not set: call fgoicp_ctx_set_source_normals first"); return FGOICP_ERR_INVALID_ARG; }
    return FGOICP_OK;
}
// One evaluation at (R, t) in two halves.  The enqueue half: the pair's rows, then the report's device half on lane 0's stream (its index
// scan keeps the moved queries) — nothing is waited for, on trimmed and brute-force contexts too.  What reduces the moments behind it is the
// caller's: the context's own launch (refine_evaluate) or a batch's fused one over refine_inputs (ctx_refine_step_enqueue).
static int refine_enqueue(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r) {
    const size_t nb = (c->ns + kBlock - 1) / kBlock;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(r.weighted ? c->d_robust_rows.ensure(nb) : c->d_plane_rows.ensure(nb));
    return alignment_enqueue(c, R9, t3, true);
}
// what the moments kernel reads: the report's arrays, the moved queries the index scan left in d_work, the target and the normals
static RefineInputs refine_inputs(const fgoicp_ctx* c, const RefineSpec& r) {
    const fgoicp_ctx::IcpLane& L = c->lanes[0];
    const fgoicp_ctx::AlignScratch& A = c->align;
    return RefineInputs{L.d_work, c->d_orig_of_slot, A.d_inl, A.d_d2, A.d_corr, c->d_tgt, c->d_normals, c->d_src_normals, (int)c->ns, (int)c->nt, r.max_dist2};
}
// The collect half, behind a wait that covers lane 0's stream: h = {n, the bits of the 28 or 29 sums} as the fold left them; unweighted,
// m->m[28] is the count.  sse_out (optional): the report's sse.
static void refine_collect(const fgoicp_ctx* c, const RefineSpec& r, const unsigned long long* h, RefineMoments* m, float* sse_out) {
    static_assert(kRobustTerms == kRobustMoments && kPlaneTerms == kPlaneMoments && kRobustTerms == kPlaneTerms + 1, "the device's rows and the host's moments are the same terms");
    const size_t K = r.weighted ? kRobustTerms : kPlaneTerms;
    m->n = h[0];
    std::memcpy(m->m, h + 1, sizeof(double) * K);
    if (!r.weighted) m->m[kPlaneMoments] = (double)m->n;  // every counted pair weighs 1
    if (sse_out) *sse_out = sse_result(c, c->lanes[0]);
}
// One evaluation on the context alone: the two halves around its own launch, one wait.  The per-point outputs are stored by the kernel
// only when a caller asks.
int refine_evaluate(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, RefineMoments* m, float* sse_out, double* residual, double* weight,
                    unsigned char* counted) {
    const bool per_point = residual || weight || counted;
    const size_t ns = c->ns;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->d_refine_out.ensure(1 + kRobustTerms));
    if (per_point) {
        HIPCHK(c->d_robust_point.ensure(2 * ns));
        HIPCHK(c->d_robust_counted.ensure(ns));
    }
    const int rc = refine_enqueue(c, R9, t3, r);
    if (rc) return rc;
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    const RefineInputs in = refine_inputs(c, r);
    const bool gicp = r.model == FGOICP_MODEL_GICP;
    double* const d_res = per_point ? (double*)c->d_robust_point : nullptr;
    if (r.weighted)
        launch_refine_moments<kRobustTerms>(in, gicp, R9, r.epsilon, r.loss, r.loss == FGOICP_LOSS_NONE ? 1.0 : r.scale, c->d_robust_rows, c->d_refine_out, d_res,
                                            per_point ? d_res + ns : nullptr, per_point ? (unsigned char*)c->d_robust_counted : nullptr, L.stream);
    else
        launch_refine_moments<kPlaneTerms>(in, gicp, R9, r.epsilon, FGOICP_LOSS_NONE, 1.0, c->d_plane_rows, c->d_refine_out, nullptr, nullptr, nullptr, L.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(L.stream));
    const size_t K = r.weighted ? kRobustTerms : kPlaneTerms;
    unsigned long long h[1 + kRobustTerms];
    HIPCHK(hipMemcpy(h, c->d_refine_out, sizeof(h[0]) * (1 + K), hipMemcpyDeviceToHost));
    refine_collect(c, r, h, m, sse_out);
    if (residual) HIPCHK(hipMemcpy(residual, d_res, sizeof(double) * ns, hipMemcpyDeviceToHost));
    if (weight) HIPCHK(hipMemcpy(weight, d_res + ns, sizeof(double) * ns, hipMemcpyDeviceToHost));
    if (counted) HIPCHK(hipMemcpy(counted, c->d_robust_counted, ns, hipMemcpyDeviceToHost));
    return FGOICP_OK;
}
int ctx_robust_scale(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, double* scale, const char* where) {
    RefineSpec plain = r;
    plain.weighted = true;  // the kernel with the per-point stores
    plain.loss = FGOICP_LOSS_NONE;
    std::vector<double> res(c->ns);
    std::vector<unsigned char> cnt(c->ns);
    RefineMoments m;
    const int rc = refine_evaluate(c, R9, t3, plain, &m, nullptr, res.data(), nullptr, cnt.data());
    if (rc) return rc;
    double s = 0.0;
    if (!robust_mad_scale(res.data(), cnt.data(), c->ns, &s)) { set_error(std::string(where) + ": nothing is counted at this pose, there is no scale to estimate: pass a scale"); return FGOICP_ERR_INVALID_ARG; }
    if (!robust_scale_ok(s)) { set_error(std::string(where) + ": the median residual is 0, there is no scale to estimate: pass a scale"); return FGOICP_ERR_INVALID_ARG; }
    *scale = s;
    return FGOICP_OK;
}

// fgoicp_icp_plane, fgoicp_icp_gicp, fgoicp_icp_robust: evaluate, solve, update (plane.hpp), until the step is short, the first solve is
// rank-deficient, nothing is counted, the weights sum to 0 or max_iter steps are done; the end's moments and sse are those of one more
// evaluation at the pose returned.  A weighted loss without a scale > 0: estimated at (R0, t0) first.
// The loop's state before its first evaluation (the scale estimate is one evaluation of its own, ctx_robust_scale, whole).
static int refine_run_begin(fgoicp_ctx* c, RefineStepRun& s, const float* R0, const float* t0, size_t max_iter, float thr, const RefineSpec& spec, const char* where) {
    s = RefineStepRun();
    s.max_iter = max_iter;
    s.thr = thr;
    s.where = where;
    RefineEnd& e = s.end;
    e.spec = spec;
    if (spec.weighted && spec.loss != FGOICP_LOSS_NONE && !(spec.scale > 0.0)) {
        const int rc = ctx_robust_scale(c, R0, t0, spec, &e.spec.scale, where);
        if (rc) return rc;
        e.scale_estimated = 1;
    }
    e.R = Mat3f::from(R0);
    e.t = Vec3f{t0[0], t0[1], t0[2]};
    return FGOICP_OK;
}
// The host arithmetic between two evaluations, for the context's own loop and for the stepped one: s.end.m / s.end.sse hold the evaluation
// at (s.end.R, s.end.t).  Leaves s.done set, or the next pose to evaluate.
static int refine_run_advance(RefineStepRun& s) {
    RefineEnd& e = s.end;
    ++s.evaluations;
    if (s.stop || (size_t)e.iterations >= s.max_iter || e.m.n == 0 || e.m.m[28] == 0.0) { s.done = true; return FGOICP_OK; }
    if (!plane_moments_finite(e.m.m) || !std::isfinite(e.m.m[28])) { set_error(s.where + ": the normal equations are not finite"); return FGOICP_ERR_INVALID_ARG; }
    double xi[6];
    plane_step(e.m.m, xi, &e.rank);
    plane_apply_step(e.R, e.t, xi, e.R, e.t);
    ++e.iterations;
    const double step = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) + std::sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
    s.stop = step < (double)s.thr || (e.iterations == 1 && e.rank < 6);  // one more evaluation, at the pose returned, then out
    return FGOICP_OK;
}
int refine_loop(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float thr, const RefineSpec& spec, const char* where, RefineEnd* end) {
    RefineStepRun s;
    int rc = refine_run_begin(c, s, R0, t0, max_iter, thr, spec, where);
    while (!rc && !s.done) {
        RefineEnd& e = s.end;
        const float t3[3] = {e.t.x, e.t.y, e.t.z};
        rc = refine_evaluate(c, e.R.m, t3, e.spec, &e.m, &e.sse);
        if (!rc) rc = refine_run_advance(s);
    }
    if (rc) return rc;
    *end = s.end;
    return FGOICP_OK;
}
// The same loop cut at its host wait (fgoicp_batch): begin, then per tick ctx_refine_step_enqueue, the batch's fused reduction of
// *view, a wait that covers s.ready, and ctx_refine_step with the fold's output — until s.done.
int ctx_refine_step_begin(fgoicp_ctx* c, RefineStepRun& s, const float* R0, const float* t0, size_t max_iter, float thr, const RefineSpec& spec, const char* where,
                          int estimate_k) {
    s = RefineStepRun();
    if (estimate_k > 0 && !c->normals_set) {
        const int rc = ctx_set_target_normals(c, nullptr, estimate_k);
        if (rc) return rc;
    }
    if (estimate_k > 0 && spec.model == FGOICP_MODEL_GICP && !c->src_normals_set) {
        const int rc = ctx_set_source_normals(c, nullptr, estimate_k);
        if (rc) return rc;
    }
    int rc = refine_refusals(c, spec, spec.weighted ? ScaleCheck::or_estimated : ScaleCheck::none, where);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (!c->refine_ready) HIPCHK(c->refine_ready.create(hipEventDisableTiming));
    return refine_run_begin(c, s, R0, t0, max_iter, thr, spec, where);
}
int ctx_refine_step_enqueue(fgoicp_ctx* c, const RefineStepRun& s, FusedRefineView* view) {
    const RefineEnd& e = s.end;
    const float t3[3] = {e.t.x, e.t.y, e.t.z};
    const int rc = refine_enqueue(c, e.R.m, t3, e.spec);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->refine_ready, c->lanes[0].stream));
    view->in = refine_inputs(c, e.spec);
    std::memcpy(view->R, e.R.m, sizeof(view->R));
    view->eps = e.spec.epsilon;
    view->loss = e.spec.weighted ? e.spec.loss : FGOICP_LOSS_NONE;  // as refine_evaluate hands them to its own launch
    view->scale = e.spec.weighted && e.spec.loss != FGOICP_LOSS_NONE ? e.spec.scale : 1.0;
    view->rows = e.spec.weighted ? (void*)c->d_robust_rows.get() : (void*)c->d_plane_rows.get();
    view->first_block = 0;
    view->nblocks = (int)((c->ns + kBlock - 1) / kBlock);
    return FGOICP_OK;
}
int ctx_refine_step(fgoicp_ctx* c, RefineStepRun& s, const unsigned long long* out) {
    refine_collect(c, s.end.spec, out, &s.end.m, &s.end.sse);
    return refine_run_advance(s);
}
// what fgoicp_plane_result_t and fgoicp_robust_result_t share
template <class Result>
static void refine_result_head(const RefineEnd& e, Result* full) {
    std::memset(full, 0, sizeof(*full));  // the padding too: two results of the same inputs are the same bytes
    full->struct_size = (uint32_t)sizeof(*full);
    std::memcpy(full->R, e.R.m, sizeof(e.R.m));
    full->t[0] = e.t.x; full->t[1] = e.t.y; full->t[2] = e.t.z;
    full->iterations = e.iterations;
    full->rank = e.rank;
    full->correspondences = e.m.n;
    full->sse = e.sse;
    full->scaling_factor = 1.0f;
}
void refine_result(const RefineEnd& e, fgoicp_plane_result_t* full) {
    refine_result_head(e, full);
    full->plane_rmse = e.m.n ? std::sqrt(e.m.m[27] / (double)e.m.n) : 0.0;
}
void refine_result(const RefineEnd& e, fgoicp_robust_result_t* full) {
    refine_result_head(e, full);
    full->weight_sum = e.m.m[28];
    full->rmse = e.m.m[28] > 0.0 ? std::sqrt(e.m.m[27] / e.m.m[28]) : 0.0;
    full->loss = e.spec.loss;
    full->scale_estimated = e.scale_estimated;
    full->scale = e.spec.loss == FGOICP_LOSS_NONE ? 0.0 : e.spec.scale;
}

// EXTENSION: source normals (fgoicp_ctx_set_source_normals), kept in device slot order for refine_moments_kernel.  Given: checked and
// normalised on the host (fp64) as the target's, permuted, uploaded.  Estimated: the rule of the target's normals over the source itself —
// a caller-order float4 copy of the source as the context holds it, a throw-away tree over it (bvh_build_host), one launch of
// target_knn_kernel, the result moved from caller order into slot order; tree, copy and caller-order normals are freed before the call returns.
int ctx_set_source_normals(fgoicp_ctx* c, const float* normals, int k) {
    const size_t ns = c->ns;
    std::vector<float4> h;
    if (normals) {
        std::vector<float4> caller;
        if (int rc = unit_normals("fgoicp_ctx_set_source_normals", normals, ns, caller)) return rc;
        h.resize(ns);
        for (size_t i = 0; i < ns; ++i) h[i] = caller[c->perm[i]];
    } else {
        if (int rc = knn_k_ok("fgoicp_ctx_set_source_normals", k, ns, "source")) return rc;
        if (c->brute_force_nn) { set_error("fgoicp_ctx_set_source_normals: estimating normals needs the search tree, which a brute-force context does not build: pass normals"); return FGOICP_ERR_INVALID_ARG; }
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->d_src_normals.ensure(ns));
    hipStream_t st = c->lanes[0].stream;
    HIPCHK(hipStreamSynchronize(st));
    if (normals) {
        c->src_normals_set = false;
        HIPCHK(hipMemcpy(c->d_src_normals, h.data(), sizeof(float4) * ns, hipMemcpyHostToDevice));
        c->src_normals_set = true;
        return FGOICP_OK;
    }
    if (int rc = ensure_orig_of_slot(c)) return rc;
    h.resize(ns);
    HIPCHK(hipMemcpy(h.data(), c->d_src, sizeof(float4) * ns, hipMemcpyDeviceToHost));
    std::vector<float4> caller(ns);
    for (size_t i = 0; i < ns; ++i) caller[c->perm[i]] = make_float4(h[i].x, h[i].y, h[i].z, 0.f);
    BvhOwned tree;
    Dev<float4> d_caller;  // the source in caller order, then its normals in caller order behind it
    hipError_t e = bvh_upload(bvh_build_host(caller.data(), ns), &tree);
    if (e == hipSuccess) e = d_caller.alloc(2 * ns);
    if (e == hipSuccess) e = hipMemcpy(d_caller, caller.data(), sizeof(float4) * ns, hipMemcpyHostToDevice);
    c->src_normals_set = false;
    if (e == hipSuccess) {
        launch_target_knn(tree.view(), d_caller, (int)ns, k, nullptr, nullptr, d_caller + ns, st);
        launch_slot_order(d_caller + ns, c->d_orig_of_slot, (int)ns, c->d_src_normals, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_error(std::string("fgoicp_ctx_set_source_normals: ") + hipGetErrorString(e)); return e == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP; }
    c->src_normals_set = true;
    return FGOICP_OK;
}
int ctx_source_normals(fgoicp_ctx* c, float* out) {
    if (!c->src_normals_set) { set_error("fgoicp_source_normals: the source normals are not set (fgoicp_ctx_set_source_normals)"); return FGOICP_ERR_INVALID_ARG; }
    return read_back_xyz(c, c->d_src_normals, c->ns, c->perm.data(), out);
}

// IterativeClosestPoint3D::procrustes() on L.d_work — icp3d.cu:140-172.  The device half (enqueue only), itself in two halves: the correspondences
// into `idx`; then the inlier cut (trimmed), centroids and covariance into pinned memory.  `wide` is the selection scratch of the trimmed variant.
// move9 / move3 (optional): the working cloud is first moved by this (R_, t_) — icp3d.cu:100 of the iteration before — inside the
// correspondence scan where that is possible (one launch less on the iteration's critical chain), by its own kernel otherwise.
static int procrustes_corr_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const uint32_t* seed_idx, uint32_t* idx, uint32_t* wide, bool fused, hipStream_t st,
                                   const float* move9 = nullptr, const float* move3 = nullptr) {
    const int ns = (int)c->ns, nt = (int)c->nt;
    if (fused) {  // two launches: scan (+ move, + wave-level sums of points and correspondences), covariance (+ centroids) into pinned memory
        launch_nn_scan(L.d_work, ns, c->bvh_tgt.view(), c->d_lut, c->geom, move9, move3, move9 ? 1 : 0, 1, c->d_tgt, nt, seed_idx, nullptr, nullptr, idx, st,
                       move9 ? L.d_work : nullptr, nullptr, nullptr, L.d_wsum);
        HIPCHK(hipGetLastError());
        return FGOICP_OK;
    }
    static const bool fold_move = [] { const char* e = dev_env("FGOICP_ICP_FOLD_MOVE"); return !e || std::atoi(e) != 0; }();  // tuning knob / A-B
    const bool skip = trim_skips(c), fold = move9 && fold_move && !c->brute_force_nn && !skip;
    if (move9 && !fold) launch_transform_inplace(L.d_work, ns, move9, move3, st);
    // kernFindNearestNeighbor (icp3d.cu:11-28): min distance, tie set, lowest index
    if (c->brute_force_nn) {
        launch_fill_u32(L.d_min_bits, 0x501502F9u, c->ns, st);
        launch_fill_u32(idx, 0x7fffffffu, c->ns, st);
        launch_nn_min(L.d_work, ns, c->d_tgt, nt, nullptr, nullptr, 0, L.d_min_bits, st);
        launch_nn_tie_threshold(L.d_min_bits, ns, L.d_thr_bits, st);
        launch_nn_first_index(L.d_work, ns, c->d_tgt, nt, L.d_thr_bits, idx, st);
    } else {
        const TrimQueries q = trim_working(L, wide);
        if (skip) trim_brackets(c, q, seed_idx, st);  // trimmed: points provably outside the inlier set get no correspondence
        launch_nn_scan(L.d_work, ns, c->bvh_tgt.view(), c->d_lut, c->geom, fold ? move9 : nullptr, fold ? move3 : nullptr, fold ? 1 : 0, 1, c->d_tgt, nt, seed_idx,
                       skip ? q.lb : nullptr, skip ? q.sel : nullptr, idx, st, fold ? L.d_work : nullptr);
    }
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
static int procrustes_sums_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const uint32_t* idx, uint32_t* wide, bool fused, hipStream_t st) {
    const int ns = (int)c->ns, nt = (int)c->nt, nb = reduce_blocks_for(ns);
    L.cov_on_host = fused;
    if (fused) {
        launch_icp_cov_cen(L.d_work, c->d_tgt, idx, ns, nt, L.d_wsum, nb, (ns + 63) / 64, L.h_cen.dev(), L.h_covbp.dev(), nb, st);
        L.cov_blocks = nb;
        HIPCHK(hipGetLastError());
        return FGOICP_OK;
    }
    const unsigned char* use = nullptr;
    int ncount = ns;
    if (c->inliers) {  // trimmed ICP: only the k closest correspondences enter the Procrustes sums
        launch_icp_inliers(L.d_work, c->d_tgt, idx, ns, nt, (int)c->inliers, L.d_d2, L.d_sel, L.d_eq, c->d_orig_of_slot, L.d_use, wide, st);
        use = L.d_use;
        ncount = (int)c->inliers;
    }
    // (Folding the block partials in the grid's last block instead of a follow-up one-block kernel — the threadfence reduction —
    // was measured and lost, 62 -> 91 us per iteration: an agent-scope fence per block writes back the XCD's L2 on this 8-XCD part.)
    launch_icp_sums(L.d_work, c->d_tgt, idx, ns, nt, use, L.d_bp, nb, st);
    launch_icp_centroids(L.d_bp, nb, ncount, L.d_cen, L.h_cen.dev(), st);  // icp3d.cu:152-156, no host round trip
    launch_icp_cov(L.d_work, c->d_tgt, idx, ns, nt, L.d_cen, use, L.d_bp2, nb, st);
    launch_sum_partials(L.d_bp2, nb, 9, L.h_sums.dev(), st);
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
static int procrustes_enqueue(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const uint32_t* seed_idx, uint32_t* idx, uint32_t* wide, hipStream_t st,
                              const float* move9 = nullptr, const float* move3 = nullptr) {
    const bool fused = icp_fused(c);
    const int rc = procrustes_corr_enqueue(c, L, seed_idx, idx, wide, fused, st, move9, move3);
    return rc ? rc : procrustes_sums_enqueue(c, L, idx, wide, fused, st);
}
// ... and the host half, once the stream has drained: 3x3 SVD, icp3d.cu:168-169
static void procrustes_finish(const fgoicp_ctx::IcpLane& L, Mat3f* R_out, Vec3f* t_out, float* centroids6_out, Mat3f* ABt_out) {
    float cen[6];
    std::memcpy(cen, L.h_cen, sizeof(cen));
    Mat3f ABt;
    for (int k = 0; k < 9; ++k) ABt.m[k] = L.cov_on_host ? (float)fold_blocks(L.h_covbp, L.cov_blocks, 9, k) : (float)L.h_sums[k];
    const Mat3f Rn = closest_orthogonal_approximation(ABt);  // icp3d.cu:168
    const Vec3f sc{cen[0], cen[1], cen[2]}, cc{cen[3], cen[4], cen[5]};
    *R_out = Rn;
    *t_out = cc - Rn * sc;  // icp3d.cu:169
    if (centroids6_out) std::memcpy(centroids6_out, cen, sizeof(cen));
    if (ABt_out) *ABt_out = ABt;
}

int ctx_procrustes_device(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, Mat3f* R_out, Vec3f* t_out, float* centroids6_out, Mat3f* ABt_out, bool seeded) {
    int rc = procrustes_enqueue(c, L, seeded ? L.d_first_idx : nullptr, L.d_first_idx, L.d_sel_wide, L.stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(L.stream));
    procrustes_finish(L, R_out, t_out, centroids6_out, ABt_out);
    return FGOICP_OK;
}

// IterativeClosestPoint3D ctor + run() — icp3d.cu:55-108.
// Two streams: the exact SSE of iteration k (pristine source under the composed transform, main stream) and the
// correspondence + covariance pass of iteration k+1 (working cloud, side stream) depend on nothing but the transform of
// iteration k, so they run next to each other — both are latency chains that fill half the device at 40k points.  The pass of
// iteration k+1 is speculative (the loop may end on the SSE of iteration k); it is drained before returning.  Same kernels,
// same arithmetic, same order of every sum as the one-stream loop (FGOICP_ICP_OVERLAP=0).
static int lane_icp_dual(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9,
                         float* t_out3, int* iters_out);
static int lane_icp(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3,
                    int* iters_out) {
    // one walk for both scans where the device is full anyway (clouds beyond 262 144 points, trimmed runs: -3 ... -5 % of the ICP time); below
    // that the two scans of an iteration overlap on two streams and a wave carrying both query sets only lengthens the chain (40k points:
    // 51-53 -> 55-56 us per iteration) — FGOICP_ICP_DUAL = 1 / 0 forces either
    const bool dual = c->icp_dual_env >= 0 ? c->icp_dual_env != 0 : !icp_fused(c);
    if (dual && c->icp_overlap && !c->brute_force_nn) return lane_icp_dual(c, L, R0, t0, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
    HIPCHK(hipSetDevice(c->device));  // per host thread
    const int ns = (int)c->ns;
    const bool overlap = c->icp_overlap && !c->brute_force_nn;
    const bool seeding = c->icp_seeding && !c->brute_force_nn;
    const bool fused = icp_fused(c);
    hipStream_t A = L.stream, B = overlap ? L.icp_stream : L.stream;
    uint32_t* idx[2] = {L.d_first_idx, overlap ? L.d_first_idx2 : L.d_first_idx};
    int rc = work_begin_enqueue(c, L, R0, t0, A);
    if (rc) return rc;
    IcpLoop s;
    s.begin(R0, t0, max_iter, thr);
    bool chain_pending = false;  // a correspondence pass is in flight on B
    if (overlap && max_iter > 0) {
        HIPCHK(hipEventRecord(L.icp_ev_w, A));
        HIPCHK(hipStreamWaitEvent(B, L.icp_ev_w, 0));
        rc = procrustes_enqueue(c, L, nullptr, idx[0], L.d_sel_wide2, B);
        if (rc) return rc;
        HIPCHK(hipEventRecord(L.icp_ev_b, B));
        chain_pending = true;
    }
    while (s.next()) {
        Mat3f Rn;
        Vec3f tn;
        if (overlap) {
            HIPCHK(wait_event(L.icp_ev_b));
            chain_pending = false;
            procrustes_finish(L, &Rn, &tn, nullptr, nullptr);
        } else {
            // every pass after the first seeds its exact search with the correspondences of the pass before it
            rc = ctx_procrustes_device(c, L, &Rn, &tn, nullptr, nullptr, s.iters > 0 && seeding);
            if (rc) return rc;
        }
        const float tn3[3] = {tn.x, tn.y, tn.z};
        s.compose(Rn, tn);
        const float t3[3] = {s.t.x, s.t.y, s.t.z};
        float sse = 0.f;
        if (overlap) {
            // The working cloud and the next iteration's pass are the critical path (transform -> correspondences -> sums -> host):
            // they go to the side stream FIRST; this iteration's SSE, which needs nothing but (R, t), is enqueued behind them on the
            // main stream.  (Enqueued after the SSE chain, the correspondence scan started 25 us late: five launches of host time.)
            const uint32_t* seed = seeding ? idx[s.cur] : nullptr;  // the pass the host has just consumed
            const bool next = s.rides();  // the next iteration's pass (it moves the cloud first, :100), next to this iteration's SSE
            uint32_t* idx_out = idx[s.cur ^ 1];
            if (next) rc = procrustes_corr_enqueue(c, L, seed, idx_out, L.d_sel_wide2, fused, B, Rn.m, tn3);
            else launch_transform_inplace(L.d_work, ns, Rn.m, tn3, B);  // :100 (B is in order behind the pass that read d_work)
            if (rc) return rc;
            rc = sse_search_enqueue(c, L, s.R.m, t3, seed, fused, trim_skips(c), A);  // :103
            if (rc) return rc;
            if (next) {
                rc = procrustes_sums_enqueue(c, L, idx_out, L.d_sel_wide2, fused, B);
                if (rc) return rc;
                s.flip();
            }
            HIPCHK(hipEventRecord(L.icp_ev_b, B));
            chain_pending = true;
            rc = sse_sum_enqueue(c, L, L.d_min_bits, fused, A);
            if (rc) return rc;
            HIPCHK(wait_stream(A));
            sse = sse_result(c, L);
        } else {
            launch_transform_inplace(L.d_work, ns, Rn.m, tn3, A);  // :100
            rc = lane_sse(c, L, s.R.m, t3, &sse, seeding ? L.d_first_idx : nullptr);  // :103
            if (rc) return rc;
        }
        s.took(sse);
    }
    if (chain_pending) HIPCHK(hipEventSynchronize(L.icp_ev_b));  // the speculative pass: drained, not used
    s.result(sse_out, R_out9, t_out3, iters_out);
    return FGOICP_OK;
}

int ctx_icp(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out) {
    return lane_icp(c, c->lanes[0], R0, t0, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
}

// lane_icp's overlapped loop on ONE stream, cut at its host turn-arounds (fgoicp_batch: many contexts share every turn-around).  Each
// step enqueues what the loop enqueues between two waits — the correspondence pass of the next iteration (which moves the working cloud
// first) and this iteration's SSE — so the kernels, their inputs and the order of every sum are lane_icp's: the same (sse, R, t, iterations).
bool ctx_icp_steppable(const fgoicp_ctx* c) { return icp_fused(c) && c->icp_overlap && c->icp_dual_env <= 0; }
int ctx_icp_step_begin(fgoicp_ctx* c, IcpStepRun& s, const float* R0, const float* t0, size_t max_iter, float thr) {
    HIPCHK(hipSetDevice(c->device));
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    s = IcpStepRun();
    s.loop.begin(R0, t0, max_iter, thr);
    int rc = work_begin_enqueue(c, L, R0, t0, L.stream);
    if (rc) return rc;
    if (max_iter > 0) {
        rc = procrustes_enqueue(c, L, nullptr, L.d_first_idx, L.d_sel_wide2, L.stream);
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}
// Call once the context's stream has drained.  Sets s.done when the loop has ended (s.loop.result() then hands the outputs over).
int ctx_icp_step(fgoicp_ctx* c, IcpStepRun& s) {
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    IcpLoop& lp = s.loop;
    if (s.have_sse) lp.took(sse_result(c, L));
    if (!lp.next()) {
        s.done = true;
        return FGOICP_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    Mat3f Rn;
    Vec3f tn;
    procrustes_finish(L, &Rn, &tn, nullptr, nullptr);
    const float tn3[3] = {tn.x, tn.y, tn.z};
    lp.compose(Rn, tn);
    const float t3[3] = {lp.t.x, lp.t.y, lp.t.z};
    uint32_t* idx[2] = {L.d_first_idx, L.d_first_idx2};
    const uint32_t* seed = c->icp_seeding ? idx[lp.cur] : nullptr;
    const bool next = lp.rides();
    if (next) {
        int rc = procrustes_enqueue(c, L, seed, idx[lp.cur ^ 1], L.d_sel_wide2, L.stream, Rn.m, tn3);
        if (rc) return rc;
    }
    int rc = sse_enqueue(c, L, lp.R.m, t3, seed, L.stream);  // :103
    if (rc) return rc;
    if (next) lp.flip();
    s.have_sse = true;
    HIPCHK(hipGetLastError());
    return FGOICP_OK;
}

// COOPERATIVE ICP (round 3): `world` ranks that hold the same clouds run ONE IterativeClosestPoint3D::run() (icp3d.cu:80-108)
// together.  The two exact scans of an iteration — what an ICP run consists of (600-1900 us per iteration at 437k points) — are
// split by query range: rank r scans the Hilbert-consecutive queries [r * per, (r + 1) * per), `gather` all-gathers the results
// (correspondence indices / bits of the minima: 4 B per query) IN PLACE on device memory, and every rank then runs the cheap
// reductions (sums, centroids, covariance, SSE) over the WHOLE cloud with the single-GPU kernels and the 3x3 SVD on its host.  A
// query's nearest neighbour does not depend on which queries are scanned next to it and the reductions see the same arrays in the
// same order on every rank, so (sse, R, t, iterations) are the single-GPU loop's bits on every rank — no result needs to be
// exchanged, and an N-rank run refines exactly like a one-rank run.  Brute-force contexts, and every context below
// coop_split_min source points (the default: never split), run the whole loop on every rank instead (replicated: same bits).  `gather(buf, bytes_per_rank, user)`: the caller's stream is idle when it is
// called; on return chunk r of buf holds rank r's results, for every r.
int ctx_icp_coop(fgoicp_ctx* c, int rank, int world, int (*gather)(void* dev_buf, size_t bytes_per_rank, void* user), void* user, const float* R0,
                 const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out) {
    const size_t split_min = c->inliers ? std::min(c->coop_split_min, c->coop_split_trim_min) : c->coop_split_min;
    if (world <= 1 || !gather || c->brute_force_nn || c->ns < split_min || !c->icp_overlap) return ctx_icp(c, R0, t0, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
    if (rank < 0 || rank >= world) { set_error("ctx_icp_coop: rank out of range"); return FGOICP_ERR_INVALID_ARG; }
    HIPCHK(hipSetDevice(c->device));
    fgoicp_ctx::IcpLane& L = c->lanes[0];
    const int ns = (int)c->ns, nt = (int)c->nt;
    const size_t per = ((((size_t)ns + world - 1) / world) + 255) & ~(size_t)255;  // whole 256-query blocks per rank
    if (c->coop_cap < per * world) {
        c->coop_cap = 0;
        HIPCHK(c->d_coop.alloc(3 * per * world));
        HIPCHK(hipMemset(c->d_coop, 0, sizeof(uint32_t) * 3 * per * world));
        c->coop_cap = per * world;
    }
    // the gathered correspondences are double-buffered, like idx[cur] / idx[cur ^ 1] of the one-GPU loop: a pass reads its seeds from the
    // buffer the pass before it wrote and writes the other one (round 3 used ONE buffer as seed and output of the same kernel: with skip
    // lists the kernel wrote 0x7fffffff to a slot before every wave of the block had read its seed — results stayed exact, a seed only
    // tightens a bound, but the work done varied from run to run)
    uint32_t* idx_buf[2] = {c->d_coop, c->d_coop + c->coop_cap};
    uint32_t* mins = c->d_coop + 2 * c->coop_cap;
    const int qb = (int)std::min<size_t>((size_t)ns, per * rank), nq = (int)std::min<size_t>((size_t)ns, per * (rank + 1)) - qb;
    const bool seeding = c->icp_seeding;
    hipStream_t S = L.stream;
    int rc = work_begin_enqueue(c, L, R0, t0, S);
    if (rc) return rc;
    IcpLoop s;
    s.begin(R0, t0, max_iter, thr);
    // The loop is lane_icp_dual's (one walk per iteration serves the exact SSE of iteration k and the correspondences of iteration k + 1),
    // with the walk cut down to this rank's queries and two in-place all-gathers behind it: ONE scan, two gathers and two host syncs
    // per iteration (a first version ran the two scans one after the other: two scans, two gathers, four syncs).  Trimmed contexts
    // (c->inliers): the LUT brackets, the cuts and the inlier selection run over the whole cloud on every rank (cheap, replicated), the
    // walk — 85 % of a trimmed iteration at 1M points — on the share; the reductions are the single-GPU loop's own sum halves, unfused
    // (the share's scan leaves no wave sums) and over the gathered arrays.
    const bool skip = trim_skips(c);
    const TrimQueries qA = trim_working(L, L.d_sel_wide2);
    bool pending = false;
    if (max_iter > 0) {  // pass 1 (icp3d.cu:140-172): correspondences of my share, gathered; sums over everything
        uint32_t* idx = idx_buf[0];
        if (skip) trim_brackets(c, qA, nullptr, S);
        if (nq > 0)
            launch_nn_scan(L.d_work + qb, nq, c->bvh_tgt.view(), c->d_lut, c->geom, nullptr, nullptr, 0, 1, c->d_tgt, nt, nullptr, skip ? qA.lb + qb : nullptr,
                           skip ? qA.sel : nullptr, idx + qb, S);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(S));
        if (gather(idx, sizeof(uint32_t) * per, user)) return FGOICP_ERR_EXCHANGE;
        rc = procrustes_sums_enqueue(c, L, idx, L.d_sel_wide2, false, S);
        if (rc) return rc;
        pending = true;
    }
    while (s.next()) {
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(S));  // first iteration: pass 1; later: a no-op (the SSE's sync below drained the stream)
        pending = false;
        Mat3f Rn;
        Vec3f tn;
        procrustes_finish(L, &Rn, &tn, nullptr, nullptr);
        const float tn3[3] = {tn.x, tn.y, tn.z};
        s.compose(Rn, tn);
        const float t3[3] = {s.t.x, s.t.y, s.t.z};
        launch_transform_inplace(L.d_work, ns, Rn.m, tn3, S);    // :100 (the whole cloud: the reductions read all of it)
        const bool next = s.rides();
        const uint32_t* seed = seeding ? idx_buf[s.cur] : nullptr;  // the gathered correspondences of the pass the host has just consumed
        uint32_t* idx_out = idx_buf[s.cur ^ 1];                     // where the pass riding along writes (never the buffer the seeds come from)
        const TrimQueries qB = trim_pristine(c, L, s.R.m, t3);
        if (skip) {  // trimmed: brackets and cuts of both query sets, whole cloud, as lane_icp_dual
            if (next) trim_brackets(c, qA, seed, S);
            trim_brackets(c, qB, seed, S);
        }
        const float* lbB = skip ? qB.lb + qb : nullptr;
        const uint32_t* uB = skip ? qB.sel : nullptr;
        if (nq > 0) {
            if (next)  // compute_sse_error(R, t) (:103) of this iteration and the correspondences of the next: one walk, my share
                launch_nn_scan_dual(L.d_work + qb, nullptr, nullptr, 0, c->d_src + qb, s.R.m, t3, nq, c->bvh_tgt.view(), c->d_lut, c->geom, c->d_tgt, nt, seed ? seed + qb : nullptr,
                                    skip ? qA.lb + qb : nullptr, skip ? qA.sel : nullptr, lbB, uB, idx_out + qb, mins + qb, nullptr, nullptr, nullptr, S);
            else       // the last iteration the loop can make: no pass rides along
                launch_nn_scan(c->d_src + qb, nq, c->bvh_tgt.view(), c->d_lut, c->geom, s.R.m, t3, 1, 0, c->d_tgt, nt, seed ? seed + qb : nullptr, lbB, uB, mins + qb, S);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(S));
        if (next && gather(idx_out, sizeof(uint32_t) * per, user)) return FGOICP_ERR_EXCHANGE;
        if (gather(mins, sizeof(uint32_t) * per, user)) return FGOICP_ERR_EXCHANGE;
        if (next) {  // speculative, as on one GPU (the loop may end on this iteration's SSE)
            rc = procrustes_sums_enqueue(c, L, idx_out, L.d_sel_wide2, false, S);
            if (rc) return rc;
            s.flip();
            pending = true;
        }
        rc = sse_sum_enqueue(c, L, mins, false, S);  // compute_sse_error's sum over the gathered minima
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(S));
        s.took(sse_result(c, L));
    }
    if (pending) HIPCHK(hipStreamSynchronize(S));  // the speculative pass: drained, not used
    s.result(sse_out, R_out9, t_out3, iters_out);
    return FGOICP_OK;
}

// The loop with ONE walk per iteration (kernels.hip nn_scan_dual_kernel; default).  Once the host has (R_, t_) of iteration k, the exact
// SSE of iteration k and the correspondences of iteration k+1 are two query sets of the same walk, so the lane needs one stream and the
// host one sync per iteration: [trimmed: move, LUT brackets and cuts of both sets] -> dual scan -> inlier cut / sums / covariance of pass
// k+1 -> sum (or trimmed selection) of the SSE -> sync.  Pass k+1 is speculative as before (the loop may end on the SSE of iteration
// k).  Same per-query results, same sums in the same order: the bits of the two-stream loop (FGOICP_ICP_DUAL=0; tests).
static int lane_icp_dual(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9,
                         float* t_out3, int* iters_out) {
    HIPCHK(hipSetDevice(c->device));
    const int ns = (int)c->ns, nt = (int)c->nt;
    const bool seeding = c->icp_seeding, fused = icp_fused(c), skip = trim_skips(c);
    hipStream_t S = L.stream;
    uint32_t* idx[2] = {L.d_first_idx, L.d_first_idx2};
    int rc = work_begin_enqueue(c, L, R0, t0, S);
    if (rc) return rc;
    IcpLoop s;
    s.begin(R0, t0, max_iter, thr);
    bool pending = false;
    if (max_iter > 0) {
        rc = procrustes_enqueue(c, L, nullptr, idx[0], L.d_sel_wide2, S);
        if (rc) return rc;
        pending = true;
    }
    while (s.next()) {
        HIPCHK(wait_stream(S));  // first iteration: pass 1; later: a no-op (the SSE's sync below drained the stream)
        pending = false;
        Mat3f Rn;
        Vec3f tn;
        procrustes_finish(L, &Rn, &tn, nullptr, nullptr);
        const float tn3[3] = {tn.x, tn.y, tn.z};
        s.compose(Rn, tn);
        const float t3[3] = {s.t.x, s.t.y, s.t.z};
        const uint32_t* seed = seeding ? idx[s.cur] : nullptr;
        if (s.rides()) {
            uint32_t* idx_out = idx[s.cur ^ 1];
            const TrimQueries qA = trim_working(L, L.d_sel_wide2), qB = trim_pristine(c, L, s.R.m, t3);
            if (skip) {  // trimmed: the brackets need the moved cloud, so the move is its own kernel here (as in the two-stream loop)
                launch_transform_inplace(L.d_work, ns, Rn.m, tn3, S);  // :100
                trim_prep(c, qA, seed, S);
                trim_prep(c, qB, seed, S);
                trim_cut(c, qA, S);
                trim_cut(c, qB, S);
            }
            launch_nn_scan_dual(L.d_work, skip ? nullptr : Rn.m, skip ? nullptr : tn3, skip ? 0 : 1, c->d_src, s.R.m, t3, ns, c->bvh_tgt.view(), c->d_lut, c->geom, c->d_tgt, nt, seed,
                                skip ? qA.lb : nullptr, skip ? qA.sel : nullptr, skip ? qB.lb : nullptr, skip ? qB.sel : nullptr, idx_out, L.d_min_bits, skip ? nullptr : L.d_work,
                                fused ? L.d_wsum : nullptr, fused ? L.h_wsse.dev() : nullptr, S);
            rc = procrustes_sums_enqueue(c, L, idx_out, L.d_sel_wide2, fused, S);  // inlier cut, sums, covariance of pass k+1
            if (rc) return rc;
            rc = sse_sum_enqueue(c, L, L.d_min_bits, fused, S);                    // sum / trimmed selection of the SSE
            if (rc) return rc;
            s.flip();
            pending = true;
        } else {  // the last iteration the loop can make: no pass rides along
            launch_transform_inplace(L.d_work, ns, Rn.m, tn3, S);  // :100
            rc = sse_enqueue(c, L, s.R.m, t3, seed, S);            // :103
            if (rc) return rc;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(wait_stream(S));
        s.took(sse_result(c, L));
    }
    if (pending) HIPCHK(hipStreamSynchronize(S));  // the speculative pass: drained, not used
    s.result(sse_out, R_out9, t_out3, iters_out);
    return FGOICP_OK;
}

// One ICP run on a lane of its own (lane >= 1: own scratch, own two streams — nothing of it queues on the context's main stream,
// where the bounds kernels run): the late-joining refinement of the ROUND schedule (driver.hpp) calls this from a background
// host thread while the main thread keeps submitting bounds ticks.  Same kernels and sums as ctx_icp.
int ctx_icp_lane(fgoicp_ctx* c, int lane, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out) {
    if (lane < 0 || lane >= (int)c->lanes.size() || c->brute_force_nn) lane = 0;  // the brute-force kernels keep their scratch on lane 0
    return lane_icp(c, c->lanes[(size_t)lane], R0, t0, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
}

// Several ICP runs at once (the triggers of one expansion round, driver.hpp): run i goes to lane i % lanes, every lane has its
// own scratch and streams and a host thread of its own (an ICP iteration is a chain of small kernels with two host syncs — at
// 40k points one run fills a fraction of the device).  Each run is exactly the run ctx_icp would do: same kernels, same sums.
int ctx_icp_batch(fgoicp_ctx* c, int n, const float* R0s, const float* t0s, size_t max_iter, float thr, float* sse_out, float* R_out9s, float* t_out3s, int* iters_out) {
    const int nl = std::min<int>(n, (int)c->lanes.size());
    if (n <= 0) return FGOICP_OK;
    if (nl <= 1 || c->brute_force_nn) {
        for (int i = 0; i < n; ++i) {
            int rc = lane_icp(c, c->lanes[0], R0s + 9 * i, t0s + 3 * i, max_iter, thr, sse_out + i, R_out9s + 9 * i, t_out3s + 3 * i, iters_out ? iters_out + i : nullptr);
            if (rc) return rc;
        }
        return FGOICP_OK;
    }
    std::vector<int> rcs(nl, FGOICP_OK);
    std::vector<std::string> errs(nl);
    std::vector<std::thread> th;
    for (int l = 0; l < nl; ++l)
        th.emplace_back([&, l] {
            for (int i = l; i < n && rcs[l] == FGOICP_OK; i += nl)
                rcs[l] = lane_icp(c, c->lanes[l], R0s + 9 * i, t0s + 3 * i, max_iter, thr, sse_out + i, R_out9s + 9 * i, t_out3s + 3 * i, iters_out ? iters_out + i : nullptr);
            if (rcs[l]) errs[l] = g_last_error;
        });
    for (auto& t : th) t.join();
    for (int l = 0; l < nl; ++l)
        if (rcs[l]) { set_error(errs[l]); return rcs[l]; }
    return FGOICP_OK;
}

// per-point e of one window, per slot: up to 12 GiB (a sixth of what is free): 3000 subcubes of a 1M-point cloud per window — the
// selection launches one workgroup per row and wants several hundred of them.  A batch's e-row arena has the same budget.
size_t trim_rows_budget(size_t free_b) { return std::max<size_t>((size_t)3 << 29, std::min<size_t>((size_t)12 << 30, free_b / 6)); }

// device bytes of what trimmed ICP adds to a context of ns points and `lanes` ICP lanes (trim_setup below)
size_t trim_icp_bytes(size_t ns, size_t lanes) { return lanes * (5 * sizeof(float) * ns + ns + 2 * (size_t)65536 + 17 * sizeof(uint32_t)) + sizeof(uint32_t) * ns; }

// EXTENSION: trimmed Go-ICP.  k = 0 (or k >= ns) switches trimming off.  slot_rows = false (fgoicp_batch): everything trimmed ICP and a
// batch's fused bounds need, but not the windows' e-rows in the two slots (nor the selection statistics) — the batch keeps one arena.
static int trim_setup(fgoicp_ctx* c, size_t k, bool slot_rows) {
    HIPCHK(hipSetDevice(c->device));
    if (k >= c->ns) k = 0;
    if (c->slots[0].inflight || c->slots[1].inflight) { set_error("fgoicp_ctx_set_inliers: a bounds submission is in flight"); return FGOICP_ERR_INVALID_ARG; }
    if (k && !c->trim_ready) {
        if (const char* e = dev_env("FGOICP_TRIM_SAMPLE")) c->trim_samp_shift = std::max(0, std::min(10, std::atoi(e)));  // tuning knob: 0 = two-pass selection, no sample
        if (const char* e = dev_env("FGOICP_TRIM_MARGIN")) c->trim_margin_sd = (float)std::atof(e);                          // tuning knob: bracket half-width (standard deviations)
        c->erow = (c->ns + 3) & ~(size_t)3;  // rows start 16-byte aligned
        if (c->trim_samp_shift > 0)  // + the row's sample (trim_store); rows and samples then start on 256-byte boundaries
            c->erow = ((c->ns + 63) & ~(size_t)63) + (((((c->ns + ((size_t)1 << c->trim_samp_shift) - 1) >> c->trim_samp_shift)) + 63) & ~(size_t)63);
        // every handle allocates only if it is empty (ensure): a call that failed half-way (out of memory) can be repeated without leaking
        if (slot_rows) {
            size_t free_b = 0, total_b = 0;
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
            const size_t budget = trim_rows_budget(free_b);
            if (!c->d_trim_stat) { HIPCHK(c->d_trim_stat.alloc(4)); HIPCHK(hipMemset(c->d_trim_stat, 0, sizeof(unsigned long long) * 4)); }
            size_t rows = budget / (sizeof(float) * c->erow);
            rows = std::max<size_t>(1, std::min<size_t>(rows, (size_t)c->max_subcubes));
            c->vals_rows = (int)rows;
            for (auto& sl : c->slots) HIPCHK(sl.d_evals.ensure(c->erow * rows));
        }
        for (auto& L : c->lanes) {
            for (Dev<float>* d : {&L.d_d2, &L.d_nn_lb, &L.d_nn_ub, &L.d_nn_lb2, &L.d_nn_ub2}) HIPCHK(d->ensure(c->ns));
            HIPCHK(L.d_sel.ensure(16));
            HIPCHK(L.d_eq.ensure(1));
            const char* e = dev_env("FGOICP_SELECT_WIDE");  // tuning knob: 0 = always the one-block selection for single rows
            if (!(e && std::atoi(e) == 0)) {
                for (Dev<uint32_t>* d : {&L.d_sel_wide, &L.d_sel_wide2}) HIPCHK(d->ensure(65536 / sizeof(uint32_t)));
            }
            HIPCHK(L.d_use.ensure(c->ns));
            HIPCHK(L.h_trim.ensure(4));
        }
        if (int rc = ensure_orig_of_slot(c)) return rc;
        c->trim_ready = slot_rows;  // (a batch context never gets its slot rows: a later call with them allocates only what is missing)
    }
    c->inliers = k;
    if (k && c->trim_samp_shift > 0) {
        // the cut's rank in a sample of m points: binomial standard deviation sqrt(m p (1 - p)) if the sample were random (a systematic
        // sample of a Hilbert-ordered surface is tighter); the bracket spans trim_margin_sd of them either side, at least 2 ranks
        const double m = (double)((c->ns + ((size_t)1 << c->trim_samp_shift) - 1) >> c->trim_samp_shift), p = (double)k / (double)c->ns;
        c->trim_margin = 2 + (int)std::ceil((double)c->trim_margin_sd * std::sqrt(m * p * (1.0 - p)));
    }
    return FGOICP_OK;
}
int ctx_set_inliers(fgoicp_ctx* c, size_t k) { return trim_setup(c, k, true); }
int ctx_set_inliers_batch(fgoicp_ctx* c, size_t k) { return trim_setup(c, k, false); }

// ---- fgoicp_ctx_create in stages: each returns FGOICP_OK or the status to return, with the message set.  The context under construction
// is held by ctx_create_impl; a stage that fails just returns, and whatever exists by then goes with the context.
namespace {
struct CreateArgs {  // fgoicp_ctx_create's
    const float* tgt_xyz; size_t nt; const float* src_xyz; size_t ns; const float* bounds6; float lut_resolution; int device; unsigned flags;
};

int create_refuse_args(const CreateArgs& a) {  // no device needed
    if (!a.tgt_xyz || !a.src_xyz || !a.bounds6 || a.nt == 0 || a.ns == 0 || !(a.lut_resolution > 0) || a.nt > 0x7ffffffeull || a.ns > 0x7ffffffeull) {
        set_error("fgoicp_ctx_create: invalid argument");
        return FGOICP_ERR_INVALID_ARG;
    }
    // non-finite coordinates: the reference would carry them into every sum (NaN bounds, a search that never prunes); refused here
    auto finite_cloud = [](const float* p, size_t n) {
        float acc = 0.0f;
        for (size_t i = 0; i < 3 * n; ++i) acc += p[i] * 0.0f;  // stays 0 unless some coordinate is NaN or infinite
        return acc == 0.0f;
    };
    if (!finite_cloud(a.tgt_xyz, a.nt) || !finite_cloud(a.src_xyz, a.ns) || !finite_cloud(a.bounds6, 2)) {
        set_error("fgoicp_ctx_create: a cloud (or the target bounds) holds a non-finite coordinate");
        return FGOICP_ERR_INVALID_ARG;
    }
    return FGOICP_OK;
}
int create_select_device(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error(std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
                  "); fgoicp_amd has no CPU path");
        return FGOICP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_error("fgoicp_ctx_create: device ordinal out of range");
        return FGOICP_ERR_INVALID_ARG;
    }
    HIPCHK(hipSetDevice(device));
    return FGOICP_OK;
}
// what the arguments say about the context, the target's box, the main stream
int create_head(fgoicp_ctx* c, const CreateArgs& a) {
    c->device = a.device; c->ns = a.ns; c->nt = a.nt;
    c->profile = (a.flags & FGOICP_FLAG_PROFILE) != 0;
    c->brute_force_nn = (a.flags & FGOICP_FLAG_BRUTE_FORCE_NN) != 0;
    std::memcpy(c->bounds6, a.bounds6, sizeof(c->bounds6));
    // The trimmed search drops queries whose distance to the target's box already exceeds the cut (nn_prep_kernel): that box is taken
    // from the DATA, not from the caller's `bounds6` — the reference's Registration accepts any target_bounds (they only place the
    // LUT, registration.hpp:68), and with cropped bounds "every target point lies inside the box" would be false.
    for (int k = 0; k < 3; ++k) { c->tgt_box6[2 * k] = a.tgt_xyz[k]; c->tgt_box6[2 * k + 1] = a.tgt_xyz[k]; }
    for (size_t i = 1; i < a.nt; ++i)
        for (int k = 0; k < 3; ++k) {
            const float v = a.tgt_xyz[3 * i + k];
            c->tgt_box6[2 * k] = std::min(c->tgt_box6[2 * k], v);
            c->tgt_box6[2 * k + 1] = std::max(c->tgt_box6[2 * k + 1], v);
        }
    if (const char* e = dev_env("FGOICP_TRIM_SKIP")) c->trim_skip = std::atoi(e) != 0;        // tuning knob
    if (const char* e = dev_env("FGOICP_SORT_XCD")) c->sort_xcd = std::atoi(e) != 0;          // tuning knob
    if (const char* e = dev_env("FGOICP_SORT_CHECK")) c->sort_check = std::atoi(e) != 0;      // tuning knob: 0 = no permutation check of the tick sort
    HIPCHK(c->stream.create(hipStreamNonBlocking));
    return FGOICP_OK;
}
// LUT geometry — NearestNeighborLUT ctor, registration.cu:186-204
int create_lut_geometry(fgoicp_ctx* c, const CreateArgs& a) {
    LutGeom& g = c->geom;
    const float* bounds6 = a.bounds6;
    g.resolution = a.lut_resolution;
    g.dx = (int)std::ceil((bounds6[1] - bounds6[0]) / a.lut_resolution);
    g.dy = (int)std::ceil((bounds6[3] - bounds6[2]) / a.lut_resolution);
    g.dz = (int)std::ceil((bounds6[5] - bounds6[4]) / a.lut_resolution);
    if (g.dx < 1 || g.dy < 1 || g.dz < 1 || g.dx > 4094 || g.dy > 4094 || g.dz > 4094) {
        set_error("fgoicp_ctx_create: LUT dims out of range (" + std::to_string(g.dx) + "," + std::to_string(g.dy) + "," + std::to_string(g.dz) + ")");
        return FGOICP_ERR_INVALID_ARG;
    }
    g.px = g.dx + 2; g.py = g.dy + 2; g.pz = g.dz + 2;
    g.scale = 1.0f / a.lut_resolution;
    g.off_x = -bounds6[0]; g.off_y = -bounds6[2]; g.off_z = -bounds6[4];
    g.quantize = (a.flags & FGOICP_FLAG_NO_WEIGHT_QUANT) ? 0 : 1;
    g.idx = nullptr;  // set once the index LUT has been built (create_target_lut)
    return FGOICP_OK;
}
// The source as float4 on the device, in the chosen order, w = x*x+y*y+z*z in the device contraction order (registration.cu:39-41).
int create_source(fgoicp_ctx* c, const CreateArgs& a) {
    const size_t ns = a.ns;
    c->perm.resize(ns);
    if (a.flags & FGOICP_FLAG_NO_MORTON) std::iota(c->perm.begin(), c->perm.end(), 0u);
    else {
        // k-d order with runs of 64 points (a wave of the exact scan; any chunk of 64 << k consecutive points is one k-d cell,
        // morton.hpp) unless the caller asks for the Hilbert curve (FGOICP_FLAG_CURVE_ORDER).  Measured against the curve (round 3,
        // profiles/r03_ab_kd_order.txt): bounds kernel 1625 -> 1478 us per launch on the bunny shape (a chunk's LUT footprint is one
        // compact cell instead of a run that straddles curve cells), 5540 -> 5324 us on the dragon shape, ICP iteration 222 -> 169 us
        // at 437k points; with 20 % volume outliers (1M trimmed) the cells grow tails along the surface normal and the trimmed ICP is
        // 13 % SLOWER — hence the flag.  FGOICP_POINT_CURVE overrides: 2 = k-d, 1 = Hilbert, 0 = Z-order.
        static const int forced = [] { const char* e = dev_env("FGOICP_POINT_CURVE"); return e ? std::atoi(e) : -1; }();  // tuning knob
        const int mode = forced >= 0 ? forced : ((a.flags & FGOICP_FLAG_CURVE_ORDER) ? 1 : 2);
        c->perm = point_order(a.src_xyz, ns, 3, 64, mode);
        c->source_order = mode;
    }
    std::vector<float4> h(ns);
    for (size_t i = 0; i < ns; ++i) {
        const float* p = a.src_xyz + 3 * (size_t)c->perm[i];
        h[i] = make_float4(p[0], p[1], p[2], std::fmaf(p[2], p[2], std::fmaf(p[1], p[1], p[0] * p[0])));
    }
    HIPCHK(c->d_src.alloc(ns));
    HIPCHK(hipMemcpy(c->d_src, h.data(), sizeof(float4) * ns, hipMemcpyHostToDevice));
    return FGOICP_OK;
}
// The target on the device (caller order: the index tie rule; w = 0), its exact-NN tree, and the LUT — buildLUTKernel, registration.cu:258-318
int create_target_lut(fgoicp_ctx* c, const CreateArgs& a) {
    const size_t nt = a.nt;
    LutGeom& g = c->geom;
    std::vector<float4> h(nt), hs(nt);
    for (size_t i = 0; i < nt; ++i) {
        const float* p = a.tgt_xyz + 3 * i;
        h[i] = make_float4(p[0], p[1], p[2], 0.f);
        hs[i] = make_float4(p[0] + g.off_x, p[1] + g.off_y, p[2] + g.off_z, 0.f);  // registration.cu:289-296
    }
    HIPCHK(c->d_tgt.alloc(nt));
    HIPCHK(hipMemcpy(c->d_tgt, h.data(), sizeof(float4) * nt, hipMemcpyHostToDevice));
    const size_t total = (size_t)g.px * g.py * g.pz;
    HIPCHK(c->d_lut.alloc(total));
    hipError_t e3 = hipSuccess;
    if (c->brute_force_nn) {
        Dev<float4> d_tgt_shift;
        e3 = d_tgt_shift.alloc(nt);
        if (e3 == hipSuccess) e3 = hipMemcpy(d_tgt_shift, hs.data(), sizeof(float4) * nt, hipMemcpyHostToDevice);
        if (e3 == hipSuccess) {
            launch_lut_build(d_tgt_shift, (int)nt, g, c->d_lut, c->stream);
            e3 = hipGetLastError();
            if (e3 == hipSuccess) e3 = hipStreamSynchronize(c->stream);
        }
    } else {
        std::vector<uint32_t> order;  // one sort for both trees
        c->tree_order = bvh_kd_order() ? 1 : 0;
        HIPCHK(bvh_upload(bvh_build_host(h.data(), nt, &order), &c->bvh_tgt));
        BvhOwned shifted;  // the LUT is built from the SHIFTED targets (pc + offset in fp32), its own tree
        e3 = bvh_upload(bvh_build_host(hs.data(), nt, &order), &shifted);
        Dev<float> scratch;
        if (e3 == hipSuccess) e3 = scratch.alloc(total);
        // the index LUT (4 B per node; an allocation that fails just leaves the feature off).  Built in round 3, bit-identical (146 GPU
        // tests with it on), measured — and it buys NOTHING (profiles/r03_ab_lut_index.txt: ICP iteration 44.7 -> 46.4 us at 40k points,
        // 169 -> 170 us at 437k, trimmed 1M ICP 463 -> 465 ms): the triangle bound's slack is not what makes the scans of a far state
        // expensive — the leaf BOXES a large ball cuts are (tools/kd_sim.py-style count: 5.4 -> 16 leaves per query group 20 degrees
        // off the optimum even with exact bounds).  OFF by default; FGOICP_LUT_INDEX=1 builds and uses it.
        static const bool want_idx = [] { const char* e = dev_env("FGOICP_LUT_INDEX"); return e && std::atoi(e) != 0; }();  // tuning knob / A-B
        if (e3 == hipSuccess && want_idx && c->d_lut_idx.alloc(total) != hipSuccess) (void)hipGetLastError();
        if (e3 == hipSuccess) {
            launch_lut_build_scan(shifted.view(), g, scratch, c->d_lut, c->stream, c->d_lut_idx);
            e3 = hipGetLastError();
            if (e3 == hipSuccess) e3 = hipStreamSynchronize(c->stream);
        }
    }
    if (e3 != hipSuccess) { set_error(std::string("LUT build failed: ") + hipGetErrorString(e3)); return e3 == hipErrorOutOfMemory ? FGOICP_ERR_OOM : FGOICP_ERR_HIP; }
    g.idx = c->d_lut_idx;  // from here on the exact scans seed their bounds with it (kernels.hip lut_upper_bound_d2)
    return FGOICP_OK;
}
// Packed copy for the bounds kernel: 1 z-pair (2x bytes, two rows per lookup), 2 yz-quad (4x bytes, one
// line per lookup).  Measured: the quad wins on sparse clouds (every lane-gather its own line; +8 % at 40k
// points), loses on dense ones (lanes share lines and the 4x footprint falls out of cache; -5 % at 437k), so it
// is chosen by the number of source points per voxel of the LUT's projected faces.
int create_packed_lut(fgoicp_ctx* c) {
    const LutGeom& g = c->geom;
    const size_t total = (size_t)g.px * g.py * g.pz;
    const double face_voxels = (double)g.dx * g.dy + (double)g.dy * g.dz + (double)g.dx * g.dz;
    int layout = ((double)c->ns / face_voxels < 0.5 && total * sizeof(float4) <= ((size_t)16 << 30)) ? 2 : 1;
    // sparse clouds, round 3: the apron-bricked quads (kernels.hip apron_index: every lookup inside one line, a line serves a 3 x 2
    // patch of base voxels; 21.3 instead of 16 B per node) — bounds kernel -1.1 % on the bunny shape, three A/B pairs
    const size_t apron_bytes = packed_lut_bytes(g, 4);
    if (layout == 2 && apron_bytes <= ((size_t)16 << 30)) layout = 4;
    // ... and once that copy no longer fits the 256 MiB Infinity Cache, where every byte of a gathered line comes from memory: the z-pair
    // apron bricks (kernels.hip zpair_apron_index: still one line per lookup, a line serves a 3 x 3 patch; 14.2 B per node) —
    // profiles/ab_zpair_apron.txt.  Below it the copy is served on die and the quads' single 32-byte piece per lookup stays.
    if (layout == 4 && apron_bytes > ((size_t)256 << 20)) layout = 6;
    if (const char* e = dev_env("FGOICP_LUT_ZPAIR")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4 || v == 6) layout = v; }  // tuning knob
    if ((layout == 4 || layout == 6) && (g.px > 1023 || g.py > 1023 || g.pz > 1023)) layout = 2;  // the apron copies pack indices in 10 bits
    c->lut_layout = layout;
    // (d_lut_zp counts float2: a float4 is two of them)
    if (layout == 6) {
        HIPCHK(c->d_lut_zp.alloc(packed_lut_bytes(g, 6) / sizeof(float2)));
        launch_lut_zpair_apron(c->d_lut, g, c->d_lut_zp, c->stream);
    } else if (layout == 4) {
        HIPCHK(c->d_lut_zp.alloc(apron_bytes / sizeof(float2)));
        launch_lut_quad_apron(c->d_lut, g, reinterpret_cast<float4*>(c->d_lut_zp.get()), c->stream);
    } else if (layout == 2) {
        HIPCHK(c->d_lut_zp.alloc(total * 2));
        launch_lut_quad(c->d_lut, g, reinterpret_cast<float4*>(c->d_lut_zp.get()), c->stream);
    } else {
        HIPCHK(c->d_lut_zp.alloc(total));
        launch_lut_zpair(c->d_lut, g, c->d_lut_zp, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return FGOICP_OK;
}
// Window sizing: pure arithmetic on ns, the geometry and the knobs.
int create_window_sizes(fgoicp_ctx* c) {
    const LutGeom& g = c->geom;
    const size_t ns = c->ns;
    // points per work item of the sorted path: the patch of 256 Morton-consecutive points of a sparse cloud spans
    // ~28 voxels; in a dense cloud (>= 1 point per voxel of the LUT's faces) it shrinks to ~6, so the items grow to
    // 2048 points — 8x fewer items to sort, 8x fewer partials, same locality.  Measured (437k points, density 1.8,
    // one certify run): 256 / 512 / 1024 / 2048 / 4096 points per item -> 4.68 / 3.34 / 2.70 / 2.48 / 2.60 s;
    // 40k points, density 0.1: 256 -> 512 points 8 % slower.
    const double face_voxels = (double)g.dx * g.dy + (double)g.dy * g.dz + (double)g.dx * g.dz;
    const double density = (double)ns / face_voxels;
    c->chunk_pts = density >= 1.0 ? 2048 : density >= 0.5 ? 1024 : density >= 0.25 ? 512 : 256;
    if (const char* e = dev_env("FGOICP_CHUNK_PTS")) {  // tuning knob
        const int v = std::atoi(e);
        if (v == 256 || v == 512 || v == 1024 || v == 2048 || v == 4096) c->chunk_pts = v;
    }
    // subcubes per window: as many as 4 GiB of per-(subcube, chunk) scratch per slot hold, 4096..131072 (wide rounds submit
    // tens of thousands per tick; bigger launches sort into longer runs of items per LUT cell and re-use the L2 better)
    const size_t nchunk1 = (ns + c->chunk_pts - 1) / c->chunk_pts;
    const size_t fit = ((size_t)4 << 30) / (nchunk1 * (sizeof(double2) + 2 * sizeof(unsigned) + sizeof(unsigned short)));
    c->max_subcubes = (int)std::max<size_t>(4096, std::min<size_t>(131072, fit));
    if (const char* e = dev_env("FGOICP_MAX_SUBCUBES")) c->max_subcubes = std::max(kMaxBatch, std::min(1 << 18, std::atoi(e)));  // tuning knob: subcubes per window
    // one launch = one workgroup per (subcube, chunk) item: keep items x 256 threads inside the 32-bit grid
    const size_t launch_fit = (((size_t)1 << 24) - 1) / nchunk1;
    if (launch_fit < (size_t)kMaxBatch) {
        set_error("fgoicp_ctx_create: source cloud too large for one bounds launch per batch (ns > ~134M)");
        return FGOICP_ERR_TOO_LARGE;
    }
    c->max_subcubes = (int)std::min<size_t>((size_t)c->max_subcubes, launch_fit);
    c->nchunk1 = (int)nchunk1;
    c->max_groups = std::max(512, c->max_subcubes / 8);
    if (const char* e = dev_env("FGOICP_FINALIZE_SIDE")) c->finalize_on_side = std::atoi(e) != 0;  // tuning knob
    if (const char* e = dev_env("FGOICP_ICP_SEED")) c->icp_seeding = std::atoi(e) != 0;             // tuning knob
    if (const char* e = dev_env("FGOICP_COOP_SPLIT_MIN")) c->coop_split_min = c->coop_split_trim_min = (size_t)std::max(0L, std::atol(e));  // tuning knob (both thresholds)
    if (const char* e = dev_env("FGOICP_SMALL_TICK")) c->small_tick_items = std::max(0, std::atoi(e));  // tuning knob: items
    const int maxd = std::max(g.dx, std::max(g.dy, g.dz));
    c->cell_shift = 0;
    while ((maxd >> c->cell_shift) > 32) ++c->cell_shift;  // 5 bits per axis
    // Windows with thresholds (fgoicp_bounds_submit_cut) on sparse clouds: two chunks per work item.  Half of such a window's items end
    // after three loads, and what they cost is their workgroup's dispatch (profiles/r04_dispatch_rate.txt); measured on the bunny
    // shape with the early exit, 256 / 512 / 1024 points per item: 243 / 220 / 245 ms per certify run — while without thresholds
    // 512 points are 8 % slower than 256 (above).  The sums stay per chunk, so both kinds of window return the same bits.
    c->cut_span = c->chunk_pts == 256 ? 2 : 1;
    if (const char* e = dev_env("FGOICP_CUT_TIERS")) c->cut_tier_level = (float)std::atof(e);  // tuning knob: 0 = one tier
    if (const char* e = dev_env("FGOICP_CUT_SPAN")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4) c->cut_span = v; }  // tuning knob
    return FGOICP_OK;
}
// centres of the runs of `pts` consecutive points (the tick sort's keys), on the device
int create_run_centres(fgoicp_ctx* c, const float* src_xyz, size_t pts, Dev<float4>& d_cen) {
    const size_t ns = c->ns, n = (ns + pts - 1) / pts;
    std::vector<float4> cen(n);
    for (size_t k = 0; k < n; ++k) {
        double sx = 0, sy = 0, sz = 0;
        const size_t a = k * pts, b = std::min(ns, a + pts);
        for (size_t i = a; i < b; ++i) {
            const float* p = src_xyz + 3 * (size_t)c->perm[i];
            sx += p[0]; sy += p[1]; sz += p[2];
        }
        const double inv = 1.0 / (double)(b - a);
        cen[k] = make_float4((float)(sx * inv), (float)(sy * inv), (float)(sz * inv), 0.f);
    }
    HIPCHK(d_cen.alloc(n));
    HIPCHK(hipMemcpy(d_cen, cen.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    return FGOICP_OK;
}
// one slot of the locality-sorted whole-tick path
int create_tick_slot(fgoicp_ctx* c, fgoicp_ctx::TickSlot& sl) {
    const size_t subcubes = (size_t)c->max_subcubes, max_items = subcubes * c->nchunk1;
    sl.stream.borrow(c->stream);
    HIPCHK(sl.done.create(hipEventDisableTiming));
    const char* e = dev_env("FGOICP_SORT_STREAM");  // tuning knob: 0 = sort on the main stream
    if (e && std::atoi(e) == 0) sl.sort_stream.borrow(c->stream);
    else {
        const char* pe = dev_env("FGOICP_SIDE_PRIORITY");  // tuning knob: -1 = the side streams (sort, finalize / selection) above the bounds kernels' stream, 1 = below
        const int pri = pe ? std::atoi(pe) : 0;
        int least = 0, greatest = 0;
        if (pri) HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        if (pri) HIPCHK(sl.sort_stream.create(hipStreamNonBlocking, pri < 0 ? greatest : least));
        else HIPCHK(sl.sort_stream.create(hipStreamNonBlocking));
    }
    for (Event* ev : {&sl.sorted_ev, &sl.bounds_ev}) HIPCHK(ev->create(hipEventDisableTiming));
    HIPCHK(sl.d_groups.alloc(c->max_groups));
    HIPCHK(sl.d_subs.alloc(subcubes));
    HIPCHK(sl.h_groups.alloc(c->max_groups));
    HIPCHK(sl.h_subs.alloc(subcubes));
    HIPCHK(sl.h_row_span.alloc(subcubes));
    HIPCHK(sl.h_sort_err.alloc(4));
    *sl.h_sort_err = 0u;
    HIPCHK(sl.d_keys.alloc(max_items));
    HIPCHK(sl.d_ranks.alloc(max_items));
    HIPCHK(sl.d_hist.alloc(kTickNumKeys));
    HIPCHK(hipMemset(sl.d_hist, 0, sizeof(unsigned) * kTickNumKeys));  // the scan kernel re-zeroes it after every tick
    HIPCHK(sl.d_block_sums.alloc(64));
    HIPCHK(sl.d_hist_xcd.alloc(16 * kTickNumKeys));
    HIPCHK(hipMemset(sl.d_hist_xcd, 0, sizeof(unsigned) * 16 * kTickNumKeys));
    HIPCHK(sl.d_xoff.alloc(16 * kTickNumKeys));
    HIPCHK(sl.d_cursor.alloc(kTickNumKeys));
    HIPCHK(sl.d_sorted.alloc(max_items));
    HIPCHK(sl.d_partials.alloc(max_items));
    HIPCHK(sl.d_cut_acc.alloc(2 * subcubes));
    HIPCHK(hipMemset(sl.d_cut_acc, 0, sizeof(double) * 2 * subcubes));  // bounds_finalize_kernel re-zeroes what a window used
    static_assert(sizeof(float) == sizeof(unsigned), "d_row_term is the second half of d_row_cut's allocation");
    HIPCHK(sl.d_row_cut.alloc(2 * subcubes));
    sl.d_row_term = reinterpret_cast<unsigned*>(sl.d_row_cut + subcubes);
    HIPCHK(sl.d_cut_gate.alloc(subcubes));  // written per window, ahead of its bounds kernel
    if (!c->d_cut_stat) { HIPCHK(c->d_cut_stat.alloc(kCutStatSlots)); HIPCHK(hipMemset(c->d_cut_stat, 0, sizeof(unsigned long long) * kCutStatSlots)); }  // (with the first slot)
    for (Mapped<float>* h : {&sl.h_lb, &sl.h_ub}) HIPCHK(h->alloc(subcubes));
    return FGOICP_OK;
}
// exact-NN / ICP scratch of one lane; the first lane shares the context's main stream
int create_icp_lane(fgoicp_ctx* c, fgoicp_ctx::IcpLane& L, bool first) {
    const size_t ns = c->ns;
    if (first) L.stream.borrow(c->stream);
    else HIPCHK(L.stream.create(hipStreamNonBlocking));
    HIPCHK(L.d_work.alloc(ns));
    HIPCHK(L.d_min_bits.alloc(ns));
    if (first) HIPCHK(L.d_thr_bits.alloc(ns));  // brute-force kernels only, which run on lane 0
    for (Dev<uint32_t>* d : {&L.d_first_idx, &L.d_first_idx2}) HIPCHK(d->alloc(ns));
    for (Dev<double>* d : {&L.d_bp, &L.d_bp2, &L.d_bp3}) HIPCHK(d->alloc(1024 * 16));
    HIPCHK(L.icp_stream.create(hipStreamNonBlocking));
    for (Event* e : {&L.icp_ev_w, &L.icp_ev_b}) HIPCHK(e->create(hipEventDisableTiming));
    HIPCHK(L.d_cen.alloc(8));
    HIPCHK(L.h_cen.alloc(8));
    HIPCHK(L.h_sums.alloc(16));
    HIPCHK(L.d_wsum.alloc(4096 * 6));
    HIPCHK(L.h_wsse.alloc(4096));
    HIPCHK(L.h_covbp.alloc(1024 * 9));
    return FGOICP_OK;
}
}  // namespace

// fgoicp_lut_nodes, fgoicp_lut_search: n queries of three T each through `launch`, one float back per query, on the context's stream
template <class T, class Launch>
static int lut_query(fgoicp_ctx* c, const T* q, size_t n, float* out, Launch launch) {
    if (!c || !q || !out) return FGOICP_ERR_INVALID_ARG;
    if (n == 0) return FGOICP_OK;
    HIPCHK(hipSetDevice(c->device));
    Dev<T> dq;
    Dev<float> dout;
    HIPCHK(dq.alloc(3 * n));
    hipError_t e = dout.alloc(n);
    if (e == hipSuccess) e = hipMemcpyAsync(dq, q, 3 * n * sizeof(T), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch(dq.get(), dout.get()); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIPCHK(e);
    return FGOICP_OK;
}

}  // namespace fgoicp

using namespace fgoicp;

// The refinements' entry points on the context.  Each refuses, before any device work: a null context, R or t (fgoicp_robust_scale: or
// scale), a bad out->struct_size, then refine_refusals' list, of which
//   fgoicp_plane_moments, fgoicp_icp_plane          max_dist2, the target normals
//   fgoicp_gicp_moments, fgoicp_icp_gicp            max_dist2, epsilon, the target normals, the source normals
//   fgoicp_robust_moments, fgoicp_robust_residuals  max_dist2, the model, the loss, epsilon (Generalized ICP), the scale (finite and > 0,
//                                                   a loss other than none), the target normals, the source normals (Generalized ICP)
//   fgoicp_robust_scale                             the same without the loss and the scale
//   fgoicp_icp_robust                               the scale (finite) first, then fgoicp_robust_moments' list without its scale
// apply (the plain calls' model and loss are always good ones).  fgoicp_robust_residuals has no out struct.
static RefineSpec refine_spec(bool weighted, float max_dist2, int model, double epsilon, int loss, double scale) {
    RefineSpec r;
    r.weighted = weighted; r.model = model; r.epsilon = epsilon; r.loss = loss; r.scale = scale; r.max_dist2 = max_dist2;  // a scale that does not matter is carried as given
    return r;
}
// fgoicp_plane_moments_t, or the fields fgoicp_robust_moments_t shares with it
template <class Moments>
static int refine_moments_call(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, const char* where, RefineMoments* m, Moments* full) {
    int rc = refine_refusals(c, r, ScaleCheck::given, where);
    if (rc) return rc;
    rc = refine_evaluate(c, R9, t3, r, m);
    if (rc) return rc;
    std::memset(full, 0, sizeof(*full));  // the padding too: two results of the same inputs are the same bytes
    full->struct_size = (uint32_t)sizeof(*full);
    full->points = c->ns;
    full->correspondences = m->n;
    std::memcpy(full->m, m->m, sizeof(full->m));
    full->max_dist2 = r.max_dist2;
    return FGOICP_OK;
}
static int plain_moments_call(fgoicp_ctx* c, const float* R9, const float* t3, const RefineSpec& r, const char* where, fgoicp_plane_moments_t* out) {
    const std::string w(where);
    if (!c || !R9 || !t3) { set_error(w + ": the context, R and t must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error(w + ": out must not be null and out->struct_size = sizeof(fgoicp_plane_moments_t)"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard(where, [&] {
        RefineMoments m;
        fgoicp_plane_moments_t full;
        const int rc = refine_moments_call(c, R9, t3, r, where, &m, &full);
        return rc ? rc : plane_out(full, out, where, "fgoicp_plane_moments_t");
    });
}
template <class Result>
static int refine_loop_call(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float conv_thr, const RefineSpec& r, const char* where, const char* type,
                            Result* out) {
    const std::string w(where);
    if (!c || !R0 || !t0) { set_error(w + ": the context, R0 and t0 must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error(w + ": out must not be null and out->struct_size = sizeof(" + type + ")"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard(where, [&] {
        int rc = refine_refusals(c, r, r.weighted ? ScaleCheck::or_estimated : ScaleCheck::none, where);
        if (rc) return rc;
        RefineEnd end;
        rc = refine_loop(c, R0, t0, max_iter, conv_thr, r, where, &end);
        if (rc) return rc;
        Result full;
        refine_result(end, &full);
        return plane_out(full, out, where, type);
    });
}

extern "C" {

const char* fgoicp_last_error(void) { return g_last_error.c_str(); }
const char* fgoicp_version(void) { return kDevKnobs ? "fgoicp_amd 0.4 (gfx950, development build)" : "fgoicp_amd 0.4 (gfx950)"; }
int fgoicp_dev_knobs(void) { return kDevKnobs ? 1 : 0; }
int fgoicp_abi_version(void) { return FGOICP_ABI_VERSION; }

static int ctx_create_impl(const CreateArgs& a, fgoicp_ctx** out) {
    int rc = create_refuse_args(a);
    if (!rc) rc = create_select_device(a.device);
    if (rc) return rc;
    // what a failed stage or an exception (std::bad_alloc in a host-side table, a thread that cannot start) leaves half-built goes with `c`
    std::unique_ptr<fgoicp_ctx, void (*)(fgoicp_ctx*)> c(new fgoicp_ctx(), fgoicp_ctx_destroy);
    if ((rc = create_head(c.get(), a)) || (rc = create_lut_geometry(c.get(), a)) || (rc = create_source(c.get(), a)) || (rc = create_target_lut(c.get(), a)) ||
        (rc = create_packed_lut(c.get())) || (rc = create_window_sizes(c.get())))
        return rc;
    if ((rc = create_run_centres(c.get(), a.src_xyz, (size_t)c->chunk_pts, c->d_chunk_cen)) ||
        (c->cut_span > 1 && (rc = create_run_centres(c.get(), a.src_xyz, (size_t)c->chunk_pts * c->cut_span, c->d_span_cen))))
        return rc;
    for (auto& sl : c->slots)
        if ((rc = create_tick_slot(c.get(), sl))) return rc;
    int nl = 4;  // concurrent ICP runs (ctx_icp_batch)
    if (const char* e = dev_env("FGOICP_ICP_LANES")) nl = std::max(1, std::min(16, std::atoi(e)));  // tuning knob
    if (const char* e = dev_env("FGOICP_ICP_OVERLAP")) c->icp_overlap = std::atoi(e) != 0;       // tuning knob
    if (const char* e = dev_env("FGOICP_ICP_DUAL")) c->icp_dual_env = std::atoi(e) != 0 ? 1 : 0; // tuning knob / A-B: 1 = one walk for both scans of an iteration, 0 = two scans on two streams
    if (const char* e = dev_env("FGOICP_ICP_FUSE")) c->icp_fuse = std::atoi(e) != 0;             // tuning knob / A-B: 0 = separate reduction kernels
    c->lanes.resize((size_t)nl);
    for (int l = 0; l < nl; ++l)
        if ((rc = create_icp_lane(c.get(), c->lanes[(size_t)l], l == 0))) return rc;
    if (c->profile) {
        c->profile = false;
        if ((rc = fgoicp_ctx_set_profile(c.get(), 1))) return rc;
    }
    *out = c.release();
    return FGOICP_OK;
}
int fgoicp_ctx_create(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, const float* bounds6, float lut_resolution,
                      int device, unsigned flags, fgoicp_ctx** out) {
    if (!out) return FGOICP_ERR_INVALID_ARG;
    *out = nullptr;
    const CreateArgs a{tgt_xyz, nt, src_xyz, ns, bounds6, lut_resolution, device, flags};
    return fgoicp::abi_guard("fgoicp_ctx_create", [&] { return ctx_create_impl(a, out); });
}

fgoicp_ctx::~fgoicp_ctx() {
    (void)hipSetDevice(device);
    stream.sync();
    for (auto& L : lanes) { L.stream.sync(); L.icp_stream.sync(); }
    for (auto& sl : slots) sl.sort_stream.sync();
}

void fgoicp_ctx_destroy(fgoicp_ctx* c) {
    if (!c) return;
    if (c->cut_verify_windows)
        std::fprintf(stderr, "[fgoicp cut verify] %llu windows with thresholds evaluated again without them: %llu rows, %llu of them at or above their threshold, %llu violations of the contract\n",
                     (unsigned long long)c->cut_verify_windows, (unsigned long long)c->cut_verify_rows, (unsigned long long)c->cut_verify_above, (unsigned long long)c->cut_verify_bad);
    if (g_tt.on && g_tt.ticks) {
        std::fprintf(stderr, "[fgoicp timing] ticks %llu: pack %.1f us, enqueue %.1f us, wait %.1f us, copyout %.1f us per tick\n", (unsigned long long)g_tt.ticks,
                     1e6 * g_tt.pack / g_tt.ticks, 1e6 * g_tt.enqueue / g_tt.ticks, 1e6 * g_tt.wait / g_tt.ticks, 1e6 * g_tt.copyout / g_tt.ticks);
        g_tt = TickTiming{};
    }
    delete c;
}

int fgoicp_lut_dims(const fgoicp_ctx* c, int* dims3) {
    if (!c || !dims3) return FGOICP_ERR_INVALID_ARG;
    dims3[0] = c->geom.dx; dims3[1] = c->geom.dy; dims3[2] = c->geom.dz;
    return FGOICP_OK;
}

int fgoicp_ctx_get_info(const fgoicp_ctx* c, fgoicp_ctx_info* out) {
    if (!c || !out) return FGOICP_ERR_INVALID_ARG;
    // the caller says how large ITS struct is; everything is assembled in a full-size local and only that many bytes are copied out
    const size_t caller = out->struct_size;
    if (caller < offsetof(fgoicp_ctx_info, lut_layout)) { set_error("fgoicp_ctx_get_info: set struct_size = sizeof(fgoicp_ctx_info) before the call"); return FGOICP_ERR_INVALID_ARG; }
    fgoicp_ctx_info full{};
    fgoicp_ctx_info* const user_out = out;
    out = &full;
    const LutGeom& g = c->geom;
    *out = fgoicp_ctx_info{};
    out->lut_dims[0] = g.dx; out->lut_dims[1] = g.dy; out->lut_dims[2] = g.dz;
    out->lut_layout = c->d_lut_zp ? c->lut_layout : 0;
    out->lut_nodes = (uint64_t)g.dx * g.dy * g.dz;
    const uint64_t padded = (uint64_t)g.px * g.py * g.pz;
    const size_t packed = c->d_lut_zp ? packed_lut_bytes(g, c->lut_layout) : 0;
    out->lut_bytes = padded * sizeof(float) + packed + (c->d_lut_idx ? padded * sizeof(uint32_t) : 0);  // + the index LUT of the exact scans
    out->source_points_per_face_voxel = (double)c->ns / ((double)g.dx * g.dy + (double)g.dy * g.dz + (double)g.dx * g.dz);
    out->points_per_item = c->chunk_pts;
    out->items_per_evaluation = c->nchunk1;
    out->max_subcubes_per_window = c->max_subcubes;
    out->source_order = c->source_order;
    out->tree_order = c->tree_order;
    out->chunks_per_item_with_thresholds = c->cut_span;
    full.struct_size = caller < sizeof(full) ? caller : sizeof(full);
    std::memcpy(user_out, &full, full.struct_size);
    return FGOICP_OK;
}

int fgoicp_lut_read(fgoicp_ctx* c, float* out, size_t capacity) {
    if (!c || !out) return FGOICP_ERR_INVALID_ARG;
    const size_t total = (size_t)c->geom.dx * c->geom.dy * c->geom.dz;
    if (capacity < total) { set_error("fgoicp_lut_read: buffer too small"); return FGOICP_ERR_INVALID_ARG; }
    HIPCHK(hipSetDevice(c->device));
    Dev<float> d;
    HIPCHK(d.alloc(total));
    launch_lut_unpad(c->d_lut, c->geom, d, c->stream);
    HIPCHK(hipMemcpyAsync(out, d, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FGOICP_OK;
}

int fgoicp_lut_nodes(fgoicp_ctx* c, const int* xyz, size_t n, float* out) {
    return lut_query(c, xyz, n, out, [&](const int* dq, float* dout) { launch_lut_nodes(c->d_lut, c->geom, dq, n, dout, c->stream); });
}
int fgoicp_lut_search(fgoicp_ctx* c, const float* q, size_t n, float* out) {
    return lut_query(c, q, n, out, [&](const float* dq, float* dout) { launch_lut_search(c->d_lut, c->geom, dq, n, dout, c->stream); });
}

int fgoicp_bounds_multi(fgoicp_ctx* c, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                        const float* tn4, float* lb_out, float* ub_out) {
    if (!c || G < 0 || (G > 0 && (!R9 || !rot_span || !fix_rot || !offsets || !tn4 || !lb_out || !ub_out))) return FGOICP_ERR_INVALID_ARG;
    if (G == 0) return FGOICP_OK;
    for (int g = 0; g < G; ++g)
        if (offsets[g + 1] < offsets[g] || offsets[0] != 0) { set_error("fgoicp_bounds_multi: offsets must start at 0 and be non-decreasing"); return FGOICP_ERR_INVALID_ARG; }
    if (offsets[G] == 0) return FGOICP_OK;
    return ctx_bounds_multi(c, G, R9, rot_span, fix_rot, offsets, tn4, lb_out, ub_out);
}

int fgoicp_bounds_submit_twins(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                               const float* tn4, const int* twin) {
    return fgoicp_bounds_submit_cut(c, slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, nullptr);
}

int fgoicp_bounds_submit_cut(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                             const float* tn4, const int* twin, const float* cut_above) {
    return fgoicp_bounds_submit_leaf(c, slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, cut_above, nullptr);
}

int fgoicp_bounds_submit_leaf(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                              const float* tn4, const int* twin, const float* cut_above, const float* ub_below_span) {
    if (!c || slot < 0 || slot > 1 || G < 0 || (G > 0 && (!R9 || !rot_span || !fix_rot || !offsets || !tn4))) return FGOICP_ERR_INVALID_ARG;
    static const int zero[1] = {0};
    if (G == 0) offsets = zero;
    for (int g = 0; g < G; ++g)
        if (offsets[g + 1] < offsets[g] || offsets[0] != 0) { set_error("fgoicp_bounds_submit: offsets must start at 0 and be non-decreasing"); return FGOICP_ERR_INVALID_ARG; }
    return ctx_bounds_submit(c, slot, G, R9, rot_span, fix_rot, offsets, tn4, twin, cut_above, ub_below_span);
}

int fgoicp_ctx_cut_stats(fgoicp_ctx* c, uint64_t* items_offered, uint64_t* items_cut, int reset) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    return ctx_cut_stats(c, items_offered, items_cut, reset);
}

int fgoicp_bounds_submit(fgoicp_ctx* c, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets,
                         const float* tn4) {
    return fgoicp_bounds_submit_twins(c, slot, G, R9, rot_span, fix_rot, offsets, tn4, nullptr);
}

int fgoicp_bounds_collect(fgoicp_ctx* c, int slot, float* lb_out, float* ub_out) {
    if (!c || slot < 0 || slot > 1 || !lb_out || !ub_out) return FGOICP_ERR_INVALID_ARG;
    return ctx_bounds_collect(c, slot, lb_out, ub_out);
}

int fgoicp_bounds_batch(fgoicp_ctx* c, const float* R9, float rot_span, const float* tn4, int B, int fix_rot, float* lb_out, float* ub_out) {
    if (B < 0) return FGOICP_ERR_INVALID_ARG;
    const int offsets[2] = {0, B};
    return fgoicp_bounds_multi(c, 1, R9, &rot_span, &fix_rot, offsets, tn4, lb_out, ub_out);
}

int fgoicp_bounds_point_distances(fgoicp_ctx* c, const float* R9, float rot_span, const float* tnode4, int fix_rot, float* e_out) {
    if (!c || !R9 || !tnode4 || !e_out) return FGOICP_ERR_INVALID_ARG;
    if (!c->inliers) { set_error("fgoicp_bounds_point_distances: trimming is off (fgoicp_ctx_set_inliers)"); return FGOICP_ERR_INVALID_ARG; }
    const int offsets[2] = {0, 1};
    float lb = 0.f, ub = 0.f;
    int rc = ctx_bounds_submit(c, 0, 1, R9, &rot_span, &fix_rot, offsets, tnode4, nullptr);
    if (rc) return rc;
    rc = ctx_bounds_collect(c, 0, &lb, &ub);
    if (rc) return rc;
    std::vector<float> row(c->ns);
    HIPCHK(hipMemcpy(row.data(), c->slots[0].d_evals, sizeof(float) * c->ns, hipMemcpyDeviceToHost));  // row 0 of the window just collected
    for (size_t i = 0; i < c->ns; ++i) e_out[c->perm[i]] = row[i];
    return FGOICP_OK;
}

// TEST HOOK (tests/test_gpu_fullsize.py): the n-th sorted tick from now on gets a slot of `sorted` spoiled, so that the on-device
// permutation check has something to find.  Nothing in the product calls it.
int fgoicp_ctx_test_sort_fault(fgoicp_ctx* c, int nth_tick) {
    if (!c || nth_tick < 0) return FGOICP_ERR_INVALID_ARG;
    c->sort_fault_tick = nth_tick ? (int)c->sorted_ticks + nth_tick : 0;
    return FGOICP_OK;
}

// TEST HOOK (tests/test_gpu_ctx_lifetime.py): the live counts of owned.hpp
int fgoicp_test_live_resources(uint64_t out4[4]) {
    if (!out4) return FGOICP_ERR_INVALID_ARG;
    out4[0] = live::dev; out4[1] = live::pinned; out4[2] = live::streams; out4[3] = live::events;
    return FGOICP_OK;
}

int fgoicp_ctx_sort_fallbacks(const fgoicp_ctx* c, uint64_t* sorted_ticks, uint64_t* fallbacks) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    if (sorted_ticks) *sorted_ticks = c->sorted_ticks;
    if (fallbacks) *fallbacks = c->sort_fallbacks;
    return FGOICP_OK;
}

int fgoicp_sse(fgoicp_ctx* c, const float* R9, const float* t3, float* sse_out) {
    if (!c || !R9 || !t3 || !sse_out) return FGOICP_ERR_INVALID_ARG;
    return ctx_sse(c, R9, t3, sse_out, nullptr);
}

int fgoicp_alignment(fgoicp_ctx* c, const float* R9, const float* t3, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns, uint8_t* target_hit_nt,
                     fgoicp_alignment_summary* out) {
    if (!c || !R9 || !t3) { set_error("fgoicp_alignment: the context, R and t must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (out && (out->struct_size < sizeof(uint32_t) || out->struct_size > 4096)) { set_error("fgoicp_alignment: set out->struct_size = sizeof(fgoicp_alignment_summary)"); return FGOICP_ERR_INVALID_ARG; }
    fgoicp_alignment_summary full{};
    const int rc = ctx_alignment(c, R9, t3, corr_idx_ns, dist2_ns, inlier_ns, target_hit_nt, &full);
    return rc ? rc : alignment_summary_out(full, out, "fgoicp_alignment");
}

int fgoicp_information(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, fgoicp_information_t* out) {
    if (!c || !R9 || !t3) { set_error("fgoicp_information: the context, R and t must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!information_size_ok(out)) { set_error("fgoicp_information: out must not be null and out->struct_size = sizeof(fgoicp_information_t)"); return FGOICP_ERR_INVALID_ARG; }
    if (!(max_dist2 >= 0.0f)) { set_error("fgoicp_information: max_dist2 must be >= 0 (+inf: no threshold)"); return FGOICP_ERR_INVALID_ARG; }
    InfoMoments m;
    const int rc = ctx_information(c, R9, t3, max_dist2, &m);
    if (rc) return rc;
    fgoicp_information_t full;
    information_fill(full, c->ns, m, nullptr, 1.0f, max_dist2);
    return information_out(full, out, "fgoicp_information");
}

int fgoicp_icp(fgoicp_ctx* c, const float* R0, const float* t0, size_t max_iter, float thr, float* sse_out, float* R_out9, float* t_out3,
               int* iters_out) {
    if (!c || !R0 || !t0 || !sse_out || !R_out9 || !t_out3) return FGOICP_ERR_INVALID_ARG;
    return ctx_icp(c, R0, t0, max_iter, thr, sse_out, R_out9, t_out3, iters_out);
}

int fgoicp_icp_batch(fgoicp_ctx* c, int n, const float* R0s_9, const float* t0s_3, size_t max_iter, float thr, float* sse_out, float* R_out9s, float* t_out3s,
                     int* iters_out) {
    if (!c || n < 0 || (n > 0 && (!R0s_9 || !t0s_3 || !sse_out || !R_out9s || !t_out3s))) return FGOICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    return ctx_icp_batch(c, n, R0s_9, t0s_3, max_iter, thr, sse_out, R_out9s, t_out3s, iters_out);
}

int fgoicp_procrustes(fgoicp_ctx* c, const float* working_xyz, float* R_out9, float* t_out3, float* centroids6, float* ABt9, int* corr_idx) {
    if (!c || !working_xyz || !R_out9 || !t_out3) return FGOICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    std::vector<float4> h(c->ns);
    for (size_t i = 0; i < c->ns; ++i) {
        const float* p = working_xyz + 3 * (size_t)c->perm[i];
        h[i] = make_float4(p[0], p[1], p[2], 0.f);
    }
    HIPCHK(hipMemcpy(c->lanes[0].d_work, h.data(), sizeof(float4) * c->ns, hipMemcpyHostToDevice));
    Mat3f R, ABt;
    Vec3f t;
    int rc = ctx_procrustes_device(c, c->lanes[0], &R, &t, centroids6, &ABt, false);
    if (rc) return rc;
    std::memcpy(R_out9, R.m, sizeof(R.m));
    t_out3[0] = t.x; t_out3[1] = t.y; t_out3[2] = t.z;
    if (ABt9) std::memcpy(ABt9, ABt.m, sizeof(ABt.m));
    if (corr_idx) {
        std::vector<uint32_t> idx(c->ns);
        HIPCHK(hipMemcpy(idx.data(), c->lanes[0].d_first_idx, sizeof(uint32_t) * c->ns, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < c->ns; ++i) corr_idx[c->perm[i]] = (int)idx[i];
    }
    return FGOICP_OK;
}

int fgoicp_ctx_set_target_normals(fgoicp_ctx* c, const float* normals_nt3_or_NULL, int k) {
    if (!c) { set_error("fgoicp_ctx_set_target_normals: the context must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_ctx_set_target_normals", [&] { return ctx_set_target_normals(c, normals_nt3_or_NULL, k); });
}
int fgoicp_target_normals(fgoicp_ctx* c, float* out_nt3) {
    if (!c || !out_nt3) { set_error("fgoicp_target_normals: the context and the output must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_target_normals", [&] { return ctx_target_normals(c, out_nt3); });
}
int fgoicp_target_knn(fgoicp_ctx* c, int k, uint32_t* idx_ntk, float* d2_ntk) {
    if (!c) { set_error("fgoicp_target_knn: the context must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return ctx_target_knn(c, k, idx_ntk, d2_ntk);
}
int fgoicp_ctx_set_source_normals(fgoicp_ctx* c, const float* normals_ns3_or_NULL, int k) {
    if (!c) { set_error("fgoicp_ctx_set_source_normals: the context must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_ctx_set_source_normals", [&] { return ctx_set_source_normals(c, normals_ns3_or_NULL, k); });
}
int fgoicp_source_normals(fgoicp_ctx* c, float* out_ns3) {
    if (!c || !out_ns3) { set_error("fgoicp_source_normals: the context and the output must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_source_normals", [&] { return ctx_source_normals(c, out_ns3); });
}
int fgoicp_plane_moments(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, fgoicp_plane_moments_t* out) {
    return plain_moments_call(c, R9, t3, refine_spec(false, max_dist2, FGOICP_MODEL_PLANE, 0.0, FGOICP_LOSS_NONE, 0.0), "fgoicp_plane_moments", out);
}
int fgoicp_icp_plane(fgoicp_ctx* c, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, fgoicp_plane_result_t* out) {
    return refine_loop_call(c, R0_9, t0_3, max_iter, conv_thr, refine_spec(false, max_dist2, FGOICP_MODEL_PLANE, 0.0, FGOICP_LOSS_NONE, 0.0), "fgoicp_icp_plane",
                            "fgoicp_plane_result_t", out);
}
int fgoicp_gicp_moments(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, double epsilon, fgoicp_plane_moments_t* out) {
    return plain_moments_call(c, R9, t3, refine_spec(false, max_dist2, FGOICP_MODEL_GICP, epsilon, FGOICP_LOSS_NONE, 0.0), "fgoicp_gicp_moments", out);
}
int fgoicp_icp_gicp(fgoicp_ctx* c, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, double epsilon, fgoicp_plane_result_t* out) {
    return refine_loop_call(c, R0_9, t0_3, max_iter, conv_thr, refine_spec(false, max_dist2, FGOICP_MODEL_GICP, epsilon, FGOICP_LOSS_NONE, 0.0), "fgoicp_icp_gicp",
                            "fgoicp_plane_result_t", out);
}
int fgoicp_robust_moments(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, int model, double epsilon, int loss, double scale,
                          fgoicp_robust_moments_t* out) {
    if (!c || !R9 || !t3) { set_error("fgoicp_robust_moments: the context, R and t must not be null"); return FGOICP_ERR_INVALID_ARG; }
    if (!plane_size_ok(out)) { set_error("fgoicp_robust_moments: out must not be null and out->struct_size = sizeof(fgoicp_robust_moments_t)"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_robust_moments", [&] {
        RefineMoments m;
        fgoicp_robust_moments_t full;
        const int rc = refine_moments_call(c, R9, t3, refine_spec(true, max_dist2, model, epsilon, loss, scale), "fgoicp_robust_moments", &m, &full);
        if (rc) return rc;
        full.weight_sum = m.m[28];
        full.loss = loss;
        full.scale = scale;
        return plane_out(full, out, "fgoicp_robust_moments", "fgoicp_robust_moments_t");
    });
}
int fgoicp_robust_residuals(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, int model, double epsilon, int loss, double scale,
                            double* residual_ns, double* weight_ns, unsigned char* counted_ns) {
    if (!c || !R9 || !t3) { set_error("fgoicp_robust_residuals: the context, R and t must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_robust_residuals", [&] {
        const RefineSpec r = refine_spec(true, max_dist2, model, epsilon, loss, scale);
        const int rc = refine_refusals(c, r, ScaleCheck::given, "fgoicp_robust_residuals");
        if (rc) return rc;
        RefineMoments m;
        std::vector<unsigned char> cnt;  // the kernel stores all three or none
        if (!residual_ns && !weight_ns && !counted_ns) cnt.resize(c->ns);
        return refine_evaluate(c, R9, t3, r, &m, nullptr, residual_ns, weight_ns, cnt.empty() ? counted_ns : cnt.data());
    });
}
int fgoicp_robust_scale(fgoicp_ctx* c, const float* R9, const float* t3, float max_dist2, int model, double epsilon, double* scale) {
    if (!c || !R9 || !t3 || !scale) { set_error("fgoicp_robust_scale: the context, R, t and scale must not be null"); return FGOICP_ERR_INVALID_ARG; }
    return fgoicp::abi_guard("fgoicp_robust_scale", [&] {
        const RefineSpec r = refine_spec(true, max_dist2, model, epsilon, FGOICP_LOSS_NONE, 0.0);
        const int rc = refine_refusals(c, r, ScaleCheck::none, "fgoicp_robust_scale");
        return rc ? rc : ctx_robust_scale(c, R9, t3, r, scale, "fgoicp_robust_scale");
    });
}
int fgoicp_icp_robust(fgoicp_ctx* c, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, int model, double epsilon, int loss,
                      double scale, fgoicp_robust_result_t* out) {
    return refine_loop_call(c, R0_9, t0_3, max_iter, conv_thr, refine_spec(true, max_dist2, model, epsilon, loss, scale), "fgoicp_icp_robust", "fgoicp_robust_result_t", out);
}

int fgoicp_ctx_set_inliers(fgoicp_ctx* c, size_t k) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    return ctx_set_inliers(c, k);
}

static int flush_pending_profile(fgoicp_ctx* c) {  // drains the main stream if events are waiting to be read
    if (!c->ev_used) return FGOICP_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ctx_flush_profile(c);
}
int fgoicp_ctx_profile(fgoicp_ctx* c, double* kernel_ms, uint64_t* launches, uint64_t* subcubes, int reset) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    if (int rc = flush_pending_profile(c)) return rc;
    if (kernel_ms) *kernel_ms = c->prof_ms;
    if (launches) *launches = c->prof_launches;
    if (subcubes) *subcubes = c->prof_subcubes;
    if (reset) { c->prof_ms = 0; c->prof_launches = 0; c->prof_subcubes = 0; c->prof_evals = 0; c->prof_sel_ms_last = c->prof_sel_ms; c->prof_sel_ms = 0; }
    return FGOICP_OK;
}

int fgoicp_ctx_profile_select_ms(fgoicp_ctx* c, double* select_ms) {
    if (!c || !select_ms) return FGOICP_ERR_INVALID_ARG;
    if (int rc = flush_pending_profile(c)) return rc;
    *select_ms = c->prof_sel_ms;
    return FGOICP_OK;
}

int fgoicp_ctx_trim_stats(fgoicp_ctx* c, uint64_t* out3, int reset) {
    if (!c || !out3) return FGOICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (c->d_trim_stat) {
        unsigned long long h[4] = {0, 0, 0, 0};
        for (auto& sl : c->slots) if (sl.inflight) { set_error("fgoicp_ctx_trim_stats: a bounds submission is in flight"); return FGOICP_ERR_INVALID_ARG; }
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h, c->d_trim_stat, sizeof(h), hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(c->d_trim_stat, 0, sizeof(h)));
        for (int i = 0; i < 3; ++i) c->trim_stat_acc[i] += h[i];
    }
    for (int i = 0; i < 3; ++i) out3[i] = c->trim_stat_acc[i];
    if (reset) for (auto& v : c->trim_stat_acc) v = 0;
    return FGOICP_OK;
}

int fgoicp_ctx_profile_evaluations(fgoicp_ctx* c, uint64_t* evaluations) {
    if (!c || !evaluations) return FGOICP_ERR_INVALID_ARG;
    *evaluations = c->prof_evals;
    return FGOICP_OK;
}

int fgoicp_ctx_set_coop_split(fgoicp_ctx* c, size_t min_points_untrimmed, size_t min_points_trimmed) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    c->coop_split_min = min_points_untrimmed;
    c->coop_split_trim_min = min_points_trimmed;
    return FGOICP_OK;
}

int fgoicp_ctx_set_profile(fgoicp_ctx* c, int enabled) {
    if (!c) return FGOICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (enabled && c->ev_start.empty()) {
        c->ev_has_sel.assign(1024, 0);
        std::vector<Event>* const evs[4] = {&c->ev_start, &c->ev_stop, &c->ev_sel_start, &c->ev_sel_stop};
        for (auto* v : evs) *v = std::vector<Event>(1024);
        for (size_t i = 0; i < 1024; ++i)
            for (auto* v : evs) HIPCHK((*v)[i].create());  // start, stop, sel_start, sel_stop per index; default flags: they time
    }
    if (!enabled)
        if (int rc = flush_pending_profile(c)) return rc;
    c->profile = enabled != 0;
    return FGOICP_OK;
}

size_t fgoicp_ctx_ns(const fgoicp_ctx* c) { return c ? c->ns : 0; }
size_t fgoicp_ctx_nt(const fgoicp_ctx* c) { return c ? c->nt : 0; }

}  // extern "C"
