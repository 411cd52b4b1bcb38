// The scoring kernel of fgoicp_segment_planes alone, timed with HIP events: the kernel is the library's own text
// (csrc/device/segment_score.hpp), the points uniform in a cube, the planes through three of them each, every point a candidate.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o segment_score segment_score.hip && ./segment_score [points] [hypotheses] [runs]
// One line: points, hypotheses, grid, the median and the fastest of `runs` launches in ms, K * n * 7 fp64 operations over the median in
// Tops/s, and the sum of the counts (a check that the work was done).  tools/segment_bench.py runs it for the table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../fast-go-icp_amd/csrc/device/segment_score.hpp"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

int main(int argc, char** argv) {
    using namespace fgoicp;
    const long long n = argc > 1 ? std::atoll(argv[1]) : 1000000, K = argc > 2 ? std::atoll(argv[2]) : 1000;
    const int runs = argc > 3 ? std::atoi(argv[3]) : 20;
    if (n < 3 || n >= (1ll << 31) || K < 1 || K > 65536 || runs < 1 || runs > 1000) { std::fprintf(stderr, "points in [3, 2^31), hypotheses in [1, 65536], runs in [1, 1000]\n"); return 2; }
    std::vector<float> xyz(3 * (size_t)n);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    auto next = [&] { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)((s >> 40) * (2.0 / 16777216.0) - 1.0); };
    for (float& v : xyz) v = next();
    std::vector<SegPlane> planes((size_t)K);
    for (long long h = 0; h < K; ++h) {  // through the points 3h, 3h + 1, 3h + 2 (mod n)
        const float *a = &xyz[3 * (size_t)((3 * h) % n)], *b = &xyz[3 * (size_t)((3 * h + 1) % n)], *c = &xyz[3 * (size_t)((3 * h + 2) % n)];
        const double e1[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]}, e2[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
        const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
        planes[(size_t)h] = SegPlane{N[0] / len, N[1] / len, N[2] / len, -(N[0] * a[0] + N[1] * a[1] + N[2] * a[2]) / len};
    }
    float* d_xyz;
    int32_t* d_label;
    SegPlane* d_planes;
    uint32_t* d_counts;
    CHK(hipMalloc(&d_xyz, 12 * (size_t)n));
    CHK(hipMalloc(&d_label, 4 * (size_t)n));
    CHK(hipMalloc(&d_planes, sizeof(SegPlane) * (size_t)K));
    CHK(hipMalloc(&d_counts, 4 * (size_t)K));
    CHK(hipMemcpy(d_xyz, xyz.data(), 12 * (size_t)n, hipMemcpyHostToDevice));
    CHK(hipMemset(d_label, 0xFF, 4 * (size_t)n));  // -1: every point is a candidate
    CHK(hipMemcpy(d_planes, planes.data(), sizeof(SegPlane) * (size_t)K, hipMemcpyHostToDevice));
    const uint32_t tiles = (uint32_t)((n + kSegTile - 1) / kSegTile), gy = segment_score_grid_y(tiles, (uint32_t)K);
    hipEvent_t t0, t1;
    CHK(hipEventCreate(&t0));
    CHK(hipEventCreate(&t1));
    std::vector<float> ms;
    for (int r = 0; r < runs + 2; ++r) {  // two warm-up launches
        CHK(hipMemset(d_counts, 0, 4 * (size_t)K));
        CHK(hipEventRecord(t0));
        hipLaunchKernelGGL(segment_score_kernel, dim3(tiles, gy), dim3(kSegBlock), 0, 0, d_xyz, d_label, (uint32_t)n, d_planes, (uint32_t)K, 0.02, d_counts);
        CHK(hipEventRecord(t1));
        CHK(hipEventSynchronize(t1));
        CHK(hipGetLastError());
        float t;
        CHK(hipEventElapsedTime(&t, t0, t1));
        if (r >= 2) ms.push_back(t);
    }
    std::vector<uint32_t> counts((size_t)K);
    CHK(hipMemcpy(counts.data(), d_counts, 4 * (size_t)K, hipMemcpyDeviceToHost));
    unsigned long long total = 0;
    for (uint32_t c : counts) total += c;
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    std::printf("{\"points\": %lld, \"hypotheses\": %lld, \"grid\": [%u, %u], \"kernel_ms_median\": %.4f, \"kernel_ms_min\": %.4f, \"fp64_tops_per_s\": %.3f, \"count_sum\": %llu}\n", n, K,
                tiles, gy, med, (double)ms[0], 7.0 * (double)n * (double)K / (med * 1e-3) / 1e12, total);
    CHK(hipFree(d_xyz)); CHK(hipFree(d_label)); CHK(hipFree(d_planes)); CHK(hipFree(d_counts));
    return 0;
}
