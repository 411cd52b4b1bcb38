// Test-only: the information extension of the header-only C++ façades (include/fgoicp/registration.hpp icp::Registration::information,
// include/fgoicp/fgoicp.hpp icp::FastGoICP::information) built with a plain C++17 compiler against the C ABI alone.  Reads two raw clouds
// (count, then x y z per line), runs the solver, prints the matrix at the given distance (0: none) as one JSON object on the last line.
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
    // the host half needs no device
    const double sq[3] = {1.0, 2.0, 3.0}, sqq[6] = {1.0, 2.0, 3.0, 4.0, 6.0, 9.0};
    double info[36];
    icp::check_status(fgoicp_information_from_moments(1, sq, sqq, nullptr, 1.0f, info, nullptr, nullptr), "fgoicp_information_from_moments");
    if (info[0] != 13.0 || info[35] != 1.0) return 3;
    icp::FastGoICP solver(read_txt(argv[1]), read_txt(argv[2]), std::stof(argv[3]), 1e-3f, FGOICP_SCHEDULE_SERIAL, 1, 0, 0.0f);
    solver.run();
    const float d = std::stof(argv[4]);
    const icp::Information f = d > 0.0f ? solver.information(d) : solver.information();
    std::cout.flush();
    std::printf("{\"points\": %llu, \"correspondences\": %llu, \"fitness\": %.17g, \"inlier_rmse\": %.17g, \"m00\": %.17g, \"matrix\": [", (unsigned long long)f.result.points,
                (unsigned long long)f.result.correspondences, f.fitness(), f.inlier_rmse(), f(0, 0));
    for (int k = 0; k < 36; ++k) std::printf("%s%.17g", k ? ", " : "", f.result.info[k]);
    std::printf("]}\n");
    return 0;
}
