// TEST-ONLY: the alignment scratch as ctx.hip's alignment_enqueue plans it with Arena (csrc/device/arena.hpp, included alone: no HIP),
// printed as the nine offsets and the total for tests/test_arena_host.py to compare with the formula the planner replaced.
//   arena_check NS NT   ->   "o_idx o_corr o_d2 o_inl o_hit o_partials o_sum o_info_rows o_info total"
//   arena_check         ->   "EMPTY <1 if an array of no elements got nullptr and took no room> <total>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fast-go-icp_amd/csrc/device/arena.hpp"

namespace {
constexpr size_t kBlock = 256;        // kernels.hpp: source points per block of the report
struct Uint2 { uint32_t x, y; };      // uint2
struct InfoRow { uint32_t count, pad; double v[10]; };   // MomentRow<kAlignInfoTerms> (fixed_sum.hpp): a count and ten fp64 partial sums
static_assert(sizeof(Uint2) == 8 && sizeof(InfoRow) == 88, "the element sizes of the device's types");
}  // namespace

int main(int argc, char** argv) {
    fgoicp::Arena plan;
    alignas(256) static char small[512];
    char* base = small;
    if (argc == 1) {
        float *a = nullptr, *none = reinterpret_cast<float*>(base), *b = nullptr;  // `none` starts non-null: place() has to clear it
        plan.take(a, 3);
        plan.take(none, 0);
        plan.take(b, 1);
        plan.place(base);
        const bool ok = none == nullptr && reinterpret_cast<char*>(a) == base && reinterpret_cast<char*>(b) == base + 256;
        std::printf("EMPTY %d %zu\n", ok ? 1 : 0, plan.total());
        return 0;
    }
    if (argc != 3) return 3;
    const size_t ns = std::strtoull(argv[1], nullptr, 10), nt = std::strtoull(argv[2], nullptr, 10);
    const size_t nt16 = (nt + 15) & ~(size_t)15, nblk = (ns + kBlock - 1) / kBlock;
    uint32_t *d_idx = nullptr, *d_corr = nullptr, *d_sum = nullptr;
    float* d_d2 = nullptr;
    unsigned char *d_inl = nullptr, *d_hit = nullptr;
    Uint2* d_partials = nullptr;
    InfoRow* d_info_rows = nullptr;
    unsigned long long* d_info = nullptr;
    plan.take(d_idx, ns);
    plan.take(d_corr, ns);
    plan.take(d_d2, ns);
    plan.take(d_inl, ns);
    plan.take(d_hit, nt16);
    plan.take(d_partials, nblk);
    plan.take(d_sum, 3);
    plan.take(d_info_rows, nblk);
    plan.take(d_info, 1 + 10);
    std::vector<char> room(plan.total() + 256);  // every pointer place() forms lies inside it
    base = room.data() + (256 - reinterpret_cast<uintptr_t>(room.data()) % 256) % 256;
    plan.place(base);
    const void* p[9] = {d_idx, d_corr, d_d2, d_inl, d_hit, d_partials, d_sum, d_info_rows, d_info};
    for (const void* q : p) std::printf("%zu ", (size_t)(static_cast<const char*>(q) - base));
    std::printf("%zu\n", plan.total());
    return 0;
}
