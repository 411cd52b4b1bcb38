// TEST-ONLY: the four owning handles (fast-go-icp_amd/csrc/device/owned.hpp) on a machine WITHOUT a device, where every create fails with
// hipErrorNoDevice: a failed create leaves the handle empty and the live counts at zero, a moved-from handle is empty, a second reset() is
// harmless, a borrowed stream releases nothing.  Built with hipcc by tests/test_owned_host.py; exit 0 and "OK", or the first failed check.
#include <cstdio>
#include <utility>

#include "../../fast-go-icp_amd/csrc/device/owned.hpp"

using namespace fgoicp;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

static bool counts_zero() { return live::dev == 0 && live::pinned == 0 && live::streams == 0 && live::events == 0; }

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) { std::printf("SKIP a device is visible\n"); return 0; }
    {
        Dev<float> d;
        CHECK(d.alloc(16) != hipSuccess);
        CHECK(!d && d.get() == nullptr && counts_zero());
        CHECK(d.ensure(16) != hipSuccess && !d && counts_zero());  // empty, so ensure tries again
        d.reset();
        d.reset();
        CHECK(!d && counts_zero());
        Dev<float> e(std::move(d));
        Dev<float> f;
        f = std::move(e);
        CHECK(!d && !e && !f && static_cast<float*>(f) == nullptr);
    }
    {
        Mapped<double> m;
        CHECK(m.alloc(4, hipHostMallocMapped) != hipSuccess);
        CHECK(!m && m.get() == nullptr && m.dev() == nullptr && counts_zero());
        CHECK(m.alloc(4, hipHostMallocDefault) != hipSuccess && !m && counts_zero());
        m.reset();
        m.reset();
        Mapped<double> n(std::move(m));
        m = std::move(n);
        CHECK(!m && !n && m.dev() == nullptr && n.dev() == nullptr);
    }
    {
        Stream s;
        CHECK(s.create(hipStreamNonBlocking) != hipSuccess);
        CHECK(s.get() == nullptr && !s.owned() && counts_zero());
        CHECK(s.create(hipStreamNonBlocking, 0) != hipSuccess && s.get() == nullptr && !s.owned() && counts_zero());
        s.reset();
        s.reset();
        // a borrowed stream: the handle hands it on and never synchronises or destroys it (this one is no stream at all)
        int not_a_stream = 0;
        const hipStream_t fake = reinterpret_cast<hipStream_t>(&not_a_stream);
        s.borrow(fake);
        CHECK(static_cast<hipStream_t>(s) == fake && !s.owned() && counts_zero());
        s.sync();
        Stream t(std::move(s));
        CHECK(s.get() == nullptr && t.get() == fake && !t.owned());
        s = std::move(t);
        CHECK(t.get() == nullptr && s.get() == fake);
        s.reset();
        s.reset();
        CHECK(s.get() == nullptr && counts_zero());
        s.borrow(fake);  // ... and one that goes out of scope still borrowed
    }
    {
        Event e;
        CHECK(e.create(hipEventDisableTiming) != hipSuccess);
        CHECK(e.get() == nullptr && counts_zero());
        CHECK(e.create() != hipSuccess && e.get() == nullptr && counts_zero());
        e.reset();
        e.reset();
        Event f(std::move(e));
        e = std::move(f);
        CHECK(e.get() == nullptr && f.get() == nullptr);
    }
    CHECK(counts_zero());
    if (!g_failed) std::printf("OK\n");
    return g_failed ? 1 : 0;
}
