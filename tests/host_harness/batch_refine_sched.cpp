// TEST-ONLY: the REFINING state of the batch scheduler (fast-go-icp_amd/csrc/host/batch.hpp, BackendHasRefine) over the CPU oracle's
// operators and a fake refinement: the refinement of pair i takes ticks[i] launcher passes (0: it ends when it starts, -1: the pair is not
// refined, -2: its start is refused).  Built as a program by tests/test_batch_refine_host.py.  Checked, with the launcher's random grouping on:
//   release(i) comes only after pair i's last step, and after finished(i); finished(i) is called exactly once; every refining pair is
//   stepped exactly ticks[i] times, one step per pass; the pairs that hold state never exceed max_live (1, 3), refining pairs counted; a pair
//   whose refinement is refused does not disturb the others; every pair's search result is its solo driver run's.
//
//   batch_refine_sched [pairs] [runs] [seed]      exit status 0 = every check of every run held
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../fast-go-icp_amd/csrc/host/batch.hpp"
#include "oracle_ops.hpp"

namespace fgoicp {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
}  // namespace fgoicp

namespace {
using host_harness::Harness;

struct RefiningBackend {
    std::vector<Harness*> h;
    std::vector<int> ticks;  // per pair, see above
    std::vector<int> steps, started, finished_calls, released, refused, holds;
    int live = 0, max_seen_live = 0, errors = 0;
    void init(size_t n) { steps.assign(n, 0); started.assign(n, 0); finished_calls.assign(n, 0); released.assign(n, 0); refused.assign(n, 0); holds.assign(n, 0); }
    void bad(const char* what, int i) { std::fprintf(stderr, "batch_refine_sched: %s (pair %d)\n", what, i); ++errors; }

    int admit(int i) { holds[(size_t)i] = 1; ++live; max_seen_live = std::max(max_seen_live, live); return 0; }
    bool room_for_more(int live_now) { return live_now < 4; }
    void release(int i) {
        if (!holds[(size_t)i] || released[(size_t)i]) bad("released twice or without state", i);
        if (ticks[(size_t)i] >= 0 && (!started[(size_t)i] || steps[(size_t)i] != ticks[(size_t)i])) bad("released before its last refinement step", i);
        if (ticks[(size_t)i] == -2 && !refused[(size_t)i]) bad("released before its refinement was started", i);
        if (finished_calls[(size_t)i] != 1) bad("released without finished()", i);
        released[(size_t)i] = 1;
        holds[(size_t)i] = 0;
        --live;
    }
    void finished(int i, const BatchPairResult&) {
        if (released[(size_t)i]) bad("finished() after release", i);
        if (ticks[(size_t)i] >= 0 && steps[(size_t)i] != ticks[(size_t)i]) bad("finished() before the refinement ended", i);
        ++finished_calls[(size_t)i];
    }
    int bounds(std::vector<BatchBoundsReq*>& reqs) {
        for (BatchBoundsReq* r : reqs) {
            const int rc = h[(size_t)r->pair]->ops.bounds_multi(r->G, r->R9.data(), r->spans.data(), r->fix.data(), r->offsets.data(), r->tn4.data(), r->lb.data(), r->ub.data());
            if (rc) return rc;
        }
        return 0;
    }
    int icp_start(BatchIcpReq& r) {
        r.done = true;
        return h[(size_t)r.pair]->ops.icp(r.R0, r.t0, r.max_iter, r.thr, &r.sse, r.R, r.t, &r.iters);
    }
    int icp_step(std::vector<BatchIcpReq*>&) { return 0; }

    bool refines(int i) const { return ticks[(size_t)i] != -1; }
    int refine_start(int i, const BatchPairResult& r, bool* done) {
        if (r.status != 0 || started[(size_t)i] || refused[(size_t)i] || released[(size_t)i]) bad("refine_start out of turn", i);
        if (ticks[(size_t)i] == -2) { refused[(size_t)i] = 1; *done = true; return 0; }  // the refinement's own refusal: kept by the backend, status 0
        started[(size_t)i] = 1;
        *done = ticks[(size_t)i] == 0;
        return 0;
    }
    int refine_step(const std::vector<int>& active, std::vector<char>& done) {
        for (size_t k = 0; k < active.size(); ++k) {
            const int i = active[k];
            if (!started[(size_t)i] || released[(size_t)i] || steps[(size_t)i] >= ticks[(size_t)i]) bad("refine_step of a pair that is not refining", i);
            for (size_t j = 0; j < k; ++j)
                if (active[j] == i) bad("stepped twice in one pass", i);
            done[k] = ++steps[(size_t)i] == ticks[(size_t)i];
        }
        return 0;
    }
};
static_assert(fgoicp::BackendHasRefine<RefiningBackend>::value && fgoicp::BackendHasFinished<RefiningBackend>::value, "the hooks are detected");

// a backend without the hooks: compiles, and is not detected
struct PlainBackend {
    int admit(int) { return 0; }
    bool room_for_more(int) { return true; }
    void release(int) {}
    int bounds(std::vector<fgoicp::BatchBoundsReq*>&) { return 0; }
    int icp_start(fgoicp::BatchIcpReq&) { return 0; }
    int icp_step(std::vector<fgoicp::BatchIcpReq*>&) { return 0; }
};
static_assert(!fgoicp::BackendHasRefine<PlainBackend>::value, "no hooks, no refining state");

// a bumpy closed surface and a rotated, shifted part of it (as batch_sched.cpp)
void make_pair(std::mt19937& rng, size_t nt, size_t ns, std::vector<float>& tgt, std::vector<float>& src) {
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    const float a = 0.3f + 0.2f * u(rng), b = 0.2f * u(rng);
    auto surf = [&](float& x, float& y, float& z) {
        float r2;
        do { x = u(rng); y = u(rng); z = u(rng); r2 = x * x + y * y + z * z; } while (r2 < 1e-4f);
        const float r = 1.0f + a * std::sin(3.f * x) * std::cos(2.f * y) + b * z, inv = r / std::sqrt(r2);
        x *= inv; y *= inv; z *= inv;
    };
    tgt.resize(3 * nt);
    for (size_t i = 0; i < nt; ++i) surf(tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2]);
    const float ang = 0.4f + 0.3f * u(rng), c = std::cos(ang), s = std::sin(ang);
    src.resize(3 * ns);
    for (size_t i = 0; i < ns; ++i) {
        float x, y, z;
        do surf(x, y, z); while (x < -0.3f);
        src[3 * i] = c * x - s * y + 0.05f;
        src[3 * i + 1] = s * x + c * y - 0.03f;
        src[3 * i + 2] = z + 0.02f;
    }
}
}  // namespace

int main(int argc, char** argv) {
    using namespace fgoicp;
    const int npairs = argc > 1 ? std::atoi(argv[1]) : 6;
    const int runs = argc > 2 ? std::atoi(argv[2]) : 4;
    const unsigned seed = argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u;
    std::mt19937 rng(seed);
    std::vector<std::vector<float>> tgts((size_t)npairs), srcs((size_t)npairs);
    std::vector<std::unique_ptr<Harness>> solo, pairs;
    const float mse = 5e-2f;  // short searches: the scheduler is under test, not the search
    for (int i = 0; i < npairs; ++i) {
        make_pair(rng, 150 + 40 * (size_t)(i % 4), 60 + 20 * (size_t)(i % 3), tgts[(size_t)i], srcs[(size_t)i]);
        const size_t nt = tgts[(size_t)i].size() / 3, ns = srcs[(size_t)i].size() / 3;
        solo.emplace_back(host_harness::make_harness(tgts[(size_t)i].data(), nt, srcs[(size_t)i].data(), ns, 0.08f, mse, 5, 1, 0.f, 1, 0));
        if (solo.back()->drv->run()) { std::fprintf(stderr, "batch_refine_sched: solo run failed\n"); return 2; }
        pairs.emplace_back(host_harness::make_harness(tgts[(size_t)i].data(), nt, srcs[(size_t)i].data(), ns, 0.08f, mse, 0, 0, 0.f, 1, 0));
    }
    int failures = 0;
    const int pattern[8] = {3, 0, -1, 7, -2, 1, 12, 2};  // ticks per pair: refined for 3 passes, at once, not at all, ..., refused, ...
    for (int run = 0; run < runs; ++run) {
        RefiningBackend be;
        be.init((size_t)npairs);
        std::vector<BatchPairSpec> specs((size_t)npairs);
        for (int i = 0; i < npairs; ++i) {
            be.h.push_back(pairs[(size_t)i].get());
            be.ticks.push_back(pattern[(i + run) % 8]);
            specs[(size_t)i].n_thr = srcs[(size_t)i].size() / 3;
            specs[(size_t)i].mse_threshold = mse;
        }
        const int max_live = run % 2 ? 3 : 1;
        BatchScheduler<RefiningBackend> sched(be, specs, 0, 1, max_live);
        sched.set_jitter(seed * 1000003ull + (uint64_t)run * 7919ull + 1, 100);
        const int rc = sched.run();
        if (rc) { std::fprintf(stderr, "batch_refine_sched: run failed with %d\n", rc); return 2; }
        failures += be.errors;
        if (be.live != 0 || be.max_seen_live > max_live) {
            std::fprintf(stderr, "batch_refine_sched: window broken (live %d at the end, max live %d of %d)\n", be.live, be.max_seen_live, max_live);
            ++failures;
        }
        for (int i = 0; i < npairs; ++i) {
            const int t = be.ticks[(size_t)i];
            if (!be.released[(size_t)i] || be.finished_calls[(size_t)i] != 1 || (t >= 0 && be.steps[(size_t)i] != t) || (t < 0 && be.steps[(size_t)i] != 0) ||
                (t == -2 && !be.refused[(size_t)i]) || (t == -1 && be.started[(size_t)i])) {
                std::fprintf(stderr, "batch_refine_sched: pair %d: released %d, finished %d times, %d steps of %d\n", i, be.released[(size_t)i], be.finished_calls[(size_t)i],
                             be.steps[(size_t)i], t);
                ++failures;
            }
            Mat3f R; Vec3f tt;
            solo[(size_t)i]->drv->best_transform(R, tt);
            const float e = solo[(size_t)i]->drv->best_sse();
            const BatchPairResult& a = sched.result(i);
            if (a.status != 0 || std::memcmp(a.R.m, R.m, sizeof(R.m)) || std::memcmp(&a.t, &tt, sizeof(tt)) || std::memcmp(&a.best_sse, &e, 4)) {
                std::fprintf(stderr, "batch_refine_sched: pair %d: the search result differs from its solo run\n", i);
                ++failures;
            }
        }
    }
    std::fprintf(stderr, "batch_refine_sched: %d pairs x %d runs checked\n", npairs, runs);
    if (failures) { std::fprintf(stderr, "batch_refine_sched: %d failures\n", failures); return 1; }
    std::fprintf(stderr, "batch_refine_sched: all runs matched\n");
    return 0;
}
