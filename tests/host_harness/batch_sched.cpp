// TEST-ONLY: the batch scheduler of the product (fast-go-icp_amd/csrc/host/batch.hpp: window, rendezvous, one launcher, one driver thread
// per live pair) over the CPU oracle's operators, built as a program (tests/test_batch_host.py; with -fsanitize=thread: test_batch_tsan.py).  Every
// pair of a batch must end with the incumbent bits and the counters of its own solo driver run (the same driver over the same operators),
// while the launcher groups the requests at random (BatchScheduler::set_jitter).
//
//   batch_sched [pairs] [jitter_runs] [seed] [mse_threshold]      exit status 0 = every pair of every run matched its solo run
//   (mse_threshold: of every pair, default 1e-2 / 2e-2 alternating; larger = shorter searches)
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

struct OracleBatchBackend {
    std::vector<Harness*> h;
    int admitted = 0, live = 0, max_seen_live = 0;
    int admit(int) { ++admitted; ++live; max_seen_live = std::max(max_seen_live, live); return 0; }
    bool room_for_more(int live_now) { return live_now < 4; }
    void release(int) { --live; }
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
};

// a bumpy closed surface and a rotated, shifted part of it
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
        do surf(x, y, z); while (x < -0.3f);  // a part of the surface
        src[3 * i] = c * x - s * y + 0.05f;
        src[3 * i + 1] = s * x + c * y - 0.03f;
        src[3 * i + 2] = z + 0.02f;
    }
}

bool same(const BatchPairResult& a, Harness& solo, const char* what, int i) {
    Mat3f R; Vec3f t;
    solo.drv->best_transform(R, t);
    const float e = solo.drv->best_sse();
    const DriverStats& s = solo.drv->stats();
    const bool ok = std::memcmp(a.R.m, R.m, sizeof(R.m)) == 0 && std::memcmp(&a.t, &t, sizeof(t)) == 0 && std::memcmp(&a.best_sse, &e, 4) == 0 &&
                    a.stats.trans_cubes == s.trans_cubes && a.stats.rot_cubes == s.rot_cubes && a.stats.inner_bnb == s.inner_bnb && a.stats.icp_runs == s.icp_runs &&
                    a.stats.icp_iters == s.icp_iters && a.stats.rounds == s.rounds && a.stats.initial_icp_sse == s.initial_icp_sse && a.status == 0;
    if (!ok)
        std::fprintf(stderr, "batch_sched: %s pair %d differs: sse %.9g / %.9g, trans_cubes %llu / %llu, icp_iters %llu / %llu, status %d\n", what, i, (double)a.best_sse,
                     (double)e, (unsigned long long)a.stats.trans_cubes, (unsigned long long)s.trans_cubes, (unsigned long long)a.stats.icp_iters,
                     (unsigned long long)s.icp_iters, a.status);
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    const int npairs = argc > 1 ? std::atoi(argv[1]) : 6;
    const int runs = argc > 2 ? std::atoi(argv[2]) : 3;
    const unsigned seed = argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u;
    const float mse_all = argc > 4 ? (float)std::atof(argv[4]) : 0.0f;
    std::mt19937 rng(seed);
    std::vector<std::vector<float>> tgts((size_t)npairs), srcs((size_t)npairs);
    std::vector<float> luts, mses;
    for (int i = 0; i < npairs; ++i) {
        make_pair(rng, 150 + 40 * (size_t)(i % 4), 60 + 20 * (size_t)(i % 3), tgts[(size_t)i], srcs[(size_t)i]);
        luts.push_back(i % 2 ? 0.05f : 0.08f);
        mses.push_back(mse_all > 0.0f ? mse_all : i % 3 ? 1e-2f : 2e-2f);
    }
    int failures = 0;
    for (int schedule = 0; schedule < 2; ++schedule) {
        // solo: the driver over the oracle's operators with the two-slot loop and the twin memo, as a batch's drivers run (harness schedules 5 / 4)
        std::vector<std::unique_ptr<Harness>> solo, pairs;
        for (int i = 0; i < npairs; ++i) {
            const size_t nt = tgts[(size_t)i].size() / 3, ns = srcs[(size_t)i].size() / 3;
            solo.emplace_back(host_harness::make_harness(tgts[(size_t)i].data(), nt, srcs[(size_t)i].data(), ns, luts[(size_t)i], mses[(size_t)i], schedule ? 4 : 5, schedule ? 4 : 1, 0.f, 1, 0));
            if (solo.back()->drv->run()) { std::fprintf(stderr, "batch_sched: solo run failed\n"); return 2; }
            pairs.emplace_back(host_harness::make_harness(tgts[(size_t)i].data(), nt, srcs[(size_t)i].data(), ns, luts[(size_t)i], mses[(size_t)i], 0, 0, 0.f, 1, 0));
        }
        for (int run = 0; run < runs; ++run) {
            OracleBatchBackend be;
            std::vector<BatchPairSpec> specs((size_t)npairs);
            for (int i = 0; i < npairs; ++i) {
                be.h.push_back(pairs[(size_t)i].get());
                specs[(size_t)i].n_thr = srcs[(size_t)i].size() / 3;
                specs[(size_t)i].mse_threshold = mses[(size_t)i];
            }
            const int max_live = run % 3;  // 0 (room_for_more), 1, 2
            BatchScheduler<OracleBatchBackend> sched(be, specs, schedule, schedule ? 4 : 1, max_live);
            sched.set_jitter(seed * 1000003ull + (uint64_t)run * 7919ull + (uint64_t)schedule + 1, run == 0 ? 0 : 200);
            const int rc = sched.run();
            if (rc) { std::fprintf(stderr, "batch_sched: run failed with %d\n", rc); return 2; }
            if (be.live != 0 || be.admitted != npairs || (max_live > 0 && be.max_seen_live > max_live)) {
                std::fprintf(stderr, "batch_sched: window broken (live %d, admitted %d, max live %d of %d)\n", be.live, be.admitted, be.max_seen_live, max_live);
                ++failures;
            }
            for (int i = 0; i < npairs; ++i)
                if (!same(sched.result(i), *solo[(size_t)i], schedule ? "ROUND" : "SERIAL", i)) ++failures;
        }
        std::fprintf(stderr, "batch_sched: %s: %d pairs x %d runs checked\n", schedule ? "ROUND" : "SERIAL", npairs, runs);
    }
    if (failures) { std::fprintf(stderr, "batch_sched: %d mismatches\n", failures); return 1; }
    std::fprintf(stderr, "batch_sched: all runs matched\n");
    return 0;
}
