// Host side of fgoicp_batch: many registrations on one device, every link of their latency chains paid once for all of them.
//
// Each live pair runs its own, unchanged GoIcpDriver (driver.hpp) on a host thread of its own, over BatchOps: bounds_submit queues
// the request, bounds_collect and icp block.  ONE launcher thread (the caller of run()) loops:
//   1. wait until every live driver is blocked or has finished;
//   2. hand every pending bounds request to the backend at once (one fused evaluation per tick);
//   3. start the ICP runs that were asked for and advance every active one by one iteration (one shared host turn-around);
//   4. wake the drivers whose requests are complete.
// Pairs enter a window of at most max_live live pairs in index order; the backend creates a pair's device state when it enters and
// frees it when it finishes.  Written against an abstract backend, without HIP (like multi_link.hpp), so that the CPU tests run it over
// the oracle's operators and under ThreadSanitizer:
//
//     int  Backend::admit(int pair)                     device state of the pair (0, or a status; kBatchNoRoom = retry when a slot frees)
//     bool Backend::room_for_more(int live)             max_live = 0: may another pair enter next to `live` live ones?
//     void Backend::release(int pair)
//     int  Backend::bounds(std::vector<BatchBoundsReq*>&)   every request's lb / ub
//     int  Backend::icp_start(BatchIcpReq&)             a run of fgoicp_icp; may complete it at once (req.done)
//     int  Backend::icp_step(std::vector<BatchIcpReq*>&)    one iteration of every active run; completes those whose loop ended
//     void Backend::finished(int pair, const BatchPairResult&)   optional (BackendHasFinished): before release, the driver has ended
//     bool Backend::refines(int pair)                   optional, with the two below (BackendHasRefine): the pair is refined after its search
//     int  Backend::refine_start(int pair, const BatchPairResult&, bool* done)   a refinement loop from the search's pose; may end it at once
//     int  Backend::refine_step(const std::vector<int>& pairs, std::vector<char>& done)   one evaluation of every active loop
//
// A request's results depend on its pair and its inputs only, never on which other requests share the launch, so every pair gets the
// bits of its own solo run whatever the grouping (tests/test_batch_host.py varies it at random).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/fgoicp_amd.h"
#include "driver.hpp"

namespace fgoicp {

void set_error(const std::string& s);  // the thread's fgoicp_last_error

// max_live = 0: at most this many live pairs (each holds a host thread and a context with its streams), fewer if device memory says so
constexpr int kBatchAutoLive = 16;
constexpr int kBatchNoRoom = -1;  // Backend::admit: out of device memory while other pairs are live — wait for one of them to finish

struct BatchBoundsReq {
    int pair = 0;
    int G = 0;
    std::vector<float> R9, spans, tn4, lb, ub;
    std::vector<int> fix, offsets;
    bool pending = false, done = false;
    int rc = 0;
};
struct BatchIcpReq {
    int pair = 0;
    float R0[9], t0[3];
    size_t max_iter = 0;
    float thr = 0.f;
    float sse = 0.f, R[9], t[3];
    int iters = 0;
    bool pending = false, started = false, done = false;
    int rc = 0;
};

// what one pair of the batch is run with
struct BatchPairSpec {
    size_t n_thr = 0;        // points behind sse_threshold (ns)
    float mse_threshold = 0.f;
};
struct BatchPairResult {
    int status = 0;
    Mat3f R = Mat3f::identity();
    Vec3f t{0.f, 0.f, 0.f};  // in the solver's scaled frame (the caller restores it)
    float best_sse = 0.f;
    DriverStats stats;
};

template <class Backend> class BatchScheduler;

// Optional backend hook: void Backend::finished(int pair, const BatchPairResult&), called on the launcher thread once the pair's driver has
// ended, before release(pair) — the pair's device state still exists (the HIP backend takes the alignment report there).
template <class Backend, class = void>
struct BackendHasFinished : std::false_type {};
template <class Backend>
struct BackendHasFinished<Backend, std::void_t<decltype(std::declval<Backend&>().finished(0, std::declval<const BatchPairResult&>()))>> : std::true_type {};

// Optional backend hooks (all three or none): a pair whose driver has ended with status 0 and for which refines(pair) holds is not released
// but REFINING — still live for the window, its device state kept.  Every launcher pass starts the new refinements and advances every
// active one by one evaluation, next to the bounds tick and the ICP step; finished(pair) and release(pair) follow the pass in which the
// pair's loop ended.  A refinement that is refused or fails is the backend's to record (done, status 0): only a device failure returns
// non-zero, and that ends the batch like a failed bounds tick.
template <class Backend, class = void>
struct BackendHasRefine : std::false_type {};
template <class Backend>
struct BackendHasRefine<Backend, std::void_t<decltype(std::declval<Backend&>().refines(0)),
                                             decltype(std::declval<Backend&>().refine_start(0, std::declval<const BatchPairResult&>(), (bool*)nullptr)),
                                             decltype(std::declval<Backend&>().refine_step(std::declval<const std::vector<int>&>(), std::declval<std::vector<char>&>()))>>
    : std::true_type {};

// The operator interface of driver.hpp as seen by one driver of a batch.
template <class Backend>
struct BatchOps {
    BatchScheduler<Backend>* s = nullptr;
    int pair = 0;
    int bounds_submit(int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4, const int* /*twin: rows apart*/,
                      const float* /*cut_above: full evaluation*/) {
        return s->submit(pair, slot, G, R9, rot_span, fix_rot, offsets, tn4);
    }
    int bounds_collect(int slot, float* lb, float* ub) { return s->collect(pair, slot, lb, ub); }
    int bounds_multi(int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4, float* lb, float* ub, const float* cut_above) {
        const int rc = bounds_submit(0, G, R9, rot_span, fix_rot, offsets, tn4, nullptr, cut_above);
        return rc ? rc : bounds_collect(0, lb, ub);
    }
    bool async() const { return true; }
    // as the solo context answers: its LB tasks then keep the memo of their twins' rows, and under ROUND the memo decides how many
    // batches a task consumes per tick — hence which tasks share a half, hence the tail batch sizes and the counters.  The fused kernel
    // evaluates a twin pair as two rows: same bits (fgoicp_bounds_submit_twins).
    bool twins() const { return true; }
    int icp(const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        return s->icp(pair, R0, t0, max_iter, thr, sse, R9, t3, iters);
    }
    int icp_background(const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        return icp(R0, t0, max_iter, thr, sse, R9, t3, iters);
    }
    int icp_coop(int, int, int (*)(void*, size_t, void*), void*, const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        return icp(R0, t0, max_iter, thr, sse, R9, t3, iters);  // a batch has one rank
    }
};

template <class Backend>
class BatchScheduler {
public:
    BatchScheduler(Backend& be, std::vector<BatchPairSpec> specs, int schedule, int round_width, int max_live)
        : be_(be), specs_(std::move(specs)), schedule_(schedule), round_width_(round_width), max_live_(max_live < 0 ? 0 : max_live), pairs_(specs_.size()) {}
    ~BatchScheduler() { join_all(); }

    // Test hook: with seed != 0 every launcher pass serves a random non-empty subset of the pending requests, after a random pause of up to
    // max_pause_us, so that the grouping of requests into launches varies from run to run.
    void set_jitter(uint64_t seed, int max_pause_us) { jitter_seed_ = seed; jitter_pause_us_ = max_pause_us; }

    // Runs every pair; returns 0 when the batch ran (per-pair outcomes in result(i)), or the status of a launcher failure.
    int run() {
        std::mt19937_64 rng(jitter_seed_);
        const int n = (int)pairs_.size();
        for (auto& p : pairs_) p = std::make_unique<PairState>();
        int next = 0, live = 0, rc_all = 0;
        bool no_room = false;  // the last admission ran out of device memory: retried once a live pair has finished
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            // admission, in index order
            while (next < n && !no_room && (max_live_ == 0 ? (live == 0 || (live < kBatchAutoLive && be_.room_for_more(live))) : live < max_live_)) {
                lk.unlock();
                const int rc = be_.admit(next);
                lk.lock();
                if (rc == kBatchNoRoom && live > 0) { no_room = true; break; }  // wait for a live pair to finish before the next attempt
                if (rc) { pairs_[(size_t)next]->result.status = rc == kBatchNoRoom ? FGOICP_ERR_OOM : rc; ++next; continue; }
                start_pair(next);
                ++live;
                ++next;
            }
            if (live == 0 && next >= n) break;
            cv_launcher_.wait(lk, [&] { return running_ == 0; });
            // finished drivers: join, free their device state
            bool reaped = false;
            for (int i = 0; i < n; ++i) {
                PairState& p = *pairs_[(size_t)i];
                if (p.thread.joinable() && p.finished) {
                    lk.unlock();
                    p.thread.join();
                    bool refine = false;
                    if constexpr (BackendHasRefine<Backend>::value) refine = p.result.status == 0 && be_.refines(i);
                    if (refine) {  // the search is over, the refinement is not: the pair stays live, its device state stays
                        refine_new_.push_back(i);
                        lk.lock();
                        continue;
                    }
                    retire(i);
                    lk.lock();
                    p.released = true;
                    --live;
                    no_room = false;
                    reaped = true;
                }
            }
            std::vector<int> rstarts = refine_new_;
            std::vector<BatchBoundsReq*> breqs;
            std::vector<BatchIcpReq*> starts;
            for (auto& pp : pairs_) {
                PairState& p = *pp;
                for (auto& r : p.slot) if (r.pending) breqs.push_back(&r);
                if (p.icp.pending && !p.icp.started) starts.push_back(&p.icp);
            }
            if (jitter_seed_) {
                auto thin = [&](auto& v) {
                    if (v.size() < 2) return;
                    std::vector<typename std::decay_t<decltype(v)>::value_type> keep;
                    for (auto* r : v) if (rng() & 1) keep.push_back(r);
                    if (keep.empty()) keep.push_back(v[rng() % v.size()]);
                    v.swap(keep);
                };
                thin(breqs);
                thin(starts);
                if (rstarts.size() >= 2) {
                    std::vector<int> keep;
                    for (int i : rstarts) if (rng() & 1) keep.push_back(i);
                    if (keep.empty()) keep.push_back(rstarts[rng() % rstarts.size()]);
                    rstarts.swap(keep);
                }
            }
            if (breqs.empty() && starts.empty() && active_icp_.empty() && rstarts.empty() && refine_active_.empty()) {
                if (reaped) continue;
                // nothing to serve and nobody running: every live driver would wait for ever (cannot happen: a blocked driver has a request)
                fgoicp::set_error("fgoicp_batch_run: the launcher found no request while drivers waited");
                return abort_all(lk, FGOICP_ERR_HIP);
            }
            lk.unlock();
            if (jitter_pause_us_ > 0) std::this_thread::sleep_for(std::chrono::microseconds((int)(rng() % (uint64_t)jitter_pause_us_)));
            int rc = breqs.empty() ? 0 : be_.bounds(breqs);
            for (BatchIcpReq* r : starts) {
                if (rc) break;
                r->started = true;
                rc = be_.icp_start(*r);
                if (!rc && !r->done) active_icp_.push_back(r);
            }
            if (!rc && !active_icp_.empty()) {
                std::vector<BatchIcpReq*> step = active_icp_;
                rc = be_.icp_step(step);
            }
            std::vector<int> refined;  // pairs whose refinement ended in this pass
            if constexpr (BackendHasRefine<Backend>::value) {
                for (int i : rstarts) {
                    if (rc) break;
                    bool done = false;
                    rc = be_.refine_start(i, pairs_[(size_t)i]->result, &done);
                    for (size_t k = 0; k < refine_new_.size(); ++k)
                        if (refine_new_[k] == i) { refine_new_.erase(refine_new_.begin() + (std::ptrdiff_t)k); break; }
                    if (!rc) (done ? refined : refine_active_).push_back(i);
                }
                if (!rc && !refine_active_.empty()) {
                    std::vector<char> done(refine_active_.size(), 0);
                    rc = be_.refine_step(refine_active_, done);
                    if (!rc) {
                        std::vector<int> still;
                        for (size_t k = 0; k < refine_active_.size(); ++k) (done[k] ? refined : still).push_back(refine_active_[k]);
                        refine_active_.swap(still);
                    }
                }
                for (int i : refined) retire(i);
            }
            lk.lock();
            for (int i : refined) {
                pairs_[(size_t)i]->released = true;
                --live;
                no_room = false;
            }
            if (rc) {
                rc_all = rc;
                for (BatchBoundsReq* r : breqs) { r->rc = rc; r->done = true; }
                for (BatchIcpReq* r : active_icp_) { r->rc = rc; r->done = true; }
                for (BatchIcpReq* r : starts) { r->rc = rc; r->done = true; }
            }
            for (BatchBoundsReq* r : breqs) { r->pending = false; r->done = true; }
            std::vector<BatchIcpReq*> still;
            for (BatchIcpReq* r : active_icp_) if (!r->done) still.push_back(r);
            active_icp_.swap(still);
            for (BatchIcpReq* r : starts) if (r->done) r->pending = false;
            for (auto& pp : pairs_) {
                PairState& p = *pp;
                if (p.icp.done) p.icp.pending = false;
                if (p.waiting && (p.wait_slot == 2 ? p.icp.done : p.slot[p.wait_slot].done)) wake(p);
            }
            cv_drivers_.notify_all();
            if (rc) return abort_all(lk, rc_all);  // the device failed: every driver gets the status, the launcher drains them and stops
        }
        lk.unlock();
        join_all();
        return rc_all;
    }
    const BatchPairResult& result(int i) const { return pairs_[(size_t)i]->result; }
    int size() const { return (int)pairs_.size(); }

    // ---- driver side (BatchOps) ----
    int submit(int pair, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot, const int* offsets, const float* tn4) {
        PairState& p = *pairs_[(size_t)pair];
        std::lock_guard<std::mutex> g(mu_);
        BatchBoundsReq& r = p.slot[slot];
        if (r.pending) return FGOICP_ERR_INVALID_ARG;
        r.pair = pair;
        r.G = G;
        const int total = offsets[G];
        r.R9.assign(R9, R9 + 9 * G);
        r.spans.assign(rot_span, rot_span + G);
        r.fix.assign(fix_rot, fix_rot + G);
        r.offsets.assign(offsets, offsets + G + 1);
        r.tn4.assign(tn4, tn4 + 4 * (size_t)total);
        r.lb.assign((size_t)total, 0.f);
        r.ub.assign((size_t)total, 0.f);
        r.rc = 0;
        r.done = false;
        r.pending = true;
        return 0;
    }
    int collect(int pair, int slot, float* lb, float* ub) {
        PairState& p = *pairs_[(size_t)pair];
        std::unique_lock<std::mutex> lk(mu_);
        BatchBoundsReq& r = p.slot[slot];
        block(lk, p, slot, [&] { return r.done || abort_; });
        if (!r.done) return FGOICP_ERR_HIP;  // the launcher stopped (its status is the run's)
        r.done = false;
        if (r.rc) return r.rc;
        std::memcpy(lb, r.lb.data(), sizeof(float) * r.lb.size());
        std::memcpy(ub, r.ub.data(), sizeof(float) * r.ub.size());
        return 0;
    }
    int icp(int pair, const float* R0, const float* t0, size_t max_iter, float thr, float* sse, float* R9, float* t3, int* iters) {
        PairState& p = *pairs_[(size_t)pair];
        std::unique_lock<std::mutex> lk(mu_);
        BatchIcpReq& r = p.icp;
        r.pair = pair;
        std::memcpy(r.R0, R0, sizeof(r.R0));
        std::memcpy(r.t0, t0, sizeof(r.t0));
        r.max_iter = max_iter;
        r.thr = thr;
        r.rc = 0;
        r.done = r.started = false;
        r.pending = true;
        block(lk, p, 2, [&] { return r.done || abort_; });
        if (!r.done) return FGOICP_ERR_HIP;  // the launcher stopped (its status is the run's)
        r.done = false;
        if (r.rc) return r.rc;
        *sse = r.sse;
        std::memcpy(R9, r.R, sizeof(r.R));
        std::memcpy(t3, r.t, sizeof(r.t));
        *iters = r.iters;
        return 0;
    }

private:
    // mu_ held: every driver is released with an error status, joined, and every live pair's device state freed
    int abort_all(std::unique_lock<std::mutex>& lk, int rc) {
        abort_ = true;
        for (auto& pp : pairs_) if (pp->waiting) wake(*pp);
        cv_drivers_.notify_all();
        lk.unlock();
        join_all();
        for (size_t i = 0; i < pairs_.size(); ++i)
            if (pairs_[i]->admitted && !pairs_[i]->released) { be_.release((int)i); pairs_[i]->released = true; }
        return rc;
    }
    struct PairState {
        std::thread thread;
        BatchBoundsReq slot[2];
        BatchIcpReq icp;
        bool waiting = false, finished = false, admitted = false, released = false;
        int wait_slot = 0;          // 0, 1: a bounds slot, 2: the ICP run
        BatchPairResult result;
    };
    // called with mu_ held: the driver waits until `ready`; while it waits it does not count as running
    template <class Pred>
    void block(std::unique_lock<std::mutex>& lk, PairState& p, int what, Pred ready) {
        if (ready()) return;
        p.waiting = true;
        p.wait_slot = what;
        if (--running_ == 0) cv_launcher_.notify_one();
        cv_drivers_.wait(lk, [&] { return !p.waiting; });
    }
    void wake(PairState& p) {  // mu_ held
        p.waiting = false;
        ++running_;
    }
    void start_pair(int i) {  // mu_ held
        PairState& p = *pairs_[(size_t)i];
        p.admitted = true;
        ++running_;
        p.thread = std::thread([this, i] { drive(i); });
    }
    void drive(int i) {
        PairState& p = *pairs_[(size_t)i];
        BatchOps<Backend> ops;
        ops.s = this;
        ops.pair = i;
        BatchPairResult res;
        {
            GoIcpDriver<BatchOps<Backend>> drv(ops, specs_[(size_t)i].n_thr, specs_[(size_t)i].mse_threshold, schedule_, round_width_, 1);
            res.status = drv.run();
            drv.best_transform(res.R, res.t);
            res.best_sse = drv.best_sse();
            res.stats = drv.stats();
        }
        std::lock_guard<std::mutex> g(mu_);
        p.result = res;
        p.finished = true;
        if (--running_ == 0) cv_launcher_.notify_one();
    }
    // launcher, mu_ not held: the pair's driver thread has been joined (and its refinement, if any, has ended): its result is final
    void retire(int i) {
        if constexpr (BackendHasFinished<Backend>::value) be_.finished(i, pairs_[(size_t)i]->result);
        be_.release(i);
    }
    void join_all() {
        for (auto& p : pairs_)
            if (p && p->thread.joinable()) p->thread.join();
    }

    Backend& be_;
    std::vector<BatchPairSpec> specs_;
    int schedule_, round_width_, max_live_;
    std::vector<std::unique_ptr<PairState>> pairs_;
    std::vector<BatchIcpReq*> active_icp_;   // launcher only
    std::vector<int> refine_new_, refine_active_;  // launcher only: refining pairs that have not started yet / whose loops are running
    std::mutex mu_;
    std::condition_variable cv_launcher_, cv_drivers_;
    int running_ = 0;                        // live drivers that are neither blocked nor finished
    bool abort_ = false;
    uint64_t jitter_seed_ = 0;
    int jitter_pause_us_ = 0;
};

}  // namespace fgoicp
