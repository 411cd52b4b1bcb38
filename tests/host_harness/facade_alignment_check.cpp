// Test-only: the alignment extension of the header-only C++ façades (include/fgoicp/registration.hpp icp::Registration::alignment,
// include/fgoicp/fgoicp.hpp icp::FastGoICP::alignment) built with a plain C++17 compiler against the C ABI alone.  Reads two raw clouds
// (count, then x y z per line), runs the solver, prints the report's summary and arrays as one JSON object on the last line.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../include/fgoicp/fgoicp.hpp"
#include "../../include/fgoicp/registration.hpp"

static icp::PointCloud read_txt(const std::string& path) {
    std::ifstream f(path);
    size_t n = 0;
    f >> n;
    icp::PointCloud pc(n);
    for (size_t i = 0; i < n; ++i) f >> pc[i].x >> pc[i].y >> pc[i].z;
    return pc;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    icp::FastGoICP solver(read_txt(argv[1]), read_txt(argv[2]), std::stof(argv[3]), 1e-3f, FGOICP_SCHEDULE_SERIAL, 1, 0, std::stof(argv[4]));
    solver.run();
    const icp::Alignment a = solver.alignment();
    std::cout.flush();
    std::printf("{\"points\": %llu, \"inliers\": %llu, \"targets_hit\": %llu, \"sse\": %.9g, \"best_error\": %.9g, \"fitness\": %.9g, \"inlier_rmse\": %.9g, \"distance0\": %.9g, \"indices\": [",
                (unsigned long long)a.summary.points, (unsigned long long)a.summary.inliers, (unsigned long long)a.summary.targets_hit, a.summary.sse, solver.get_best_error(),
                a.fitness(), a.inlier_rmse(), a.distance(0));
    for (size_t i = 0; i < a.indices.size(); ++i) std::printf("%s%u", i ? ", " : "", a.indices[i]);
    std::printf("], \"inlier\": [");
    for (size_t i = 0; i < a.inlier.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)a.inlier[i]);
    std::printf("]}\n");
    return 0;
}
