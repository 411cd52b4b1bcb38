// Test-only: the point-to-plane extension of the header-only C++ façades (include/fgoicp/registration.hpp icp::Registration::
// set_target_normals / target_normals / target_knn / plane_moments / icp_plane, include/fgoicp/fgoicp.hpp icp::FastGoICP::refine_plane)
// built with a plain C++17 compiler against the C ABI alone.  Reads two raw clouds (count, then x y z per line), runs the solver,
// refines, prints one JSON object on the last line.
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

// instantiated, not run: the operator-level members
[[maybe_unused]] static double operator_level(const icp::Registration& reg, icp::mat3 R, icp::vec3 t) {
    const_cast<icp::Registration&>(reg).set_target_normals(12);
    const_cast<icp::Registration&>(reg).set_target_normals(reg.target_normals());
    return (double)reg.target_knn(8).dist2[1] + reg.plane_moments(R, t).m[27] + reg.icp_plane(R, t).plane_rmse();
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    // the host half needs no device: one correspondence, x = (1, 0, 0), n = (0, 0, 1), r = 0.5 — J = (0, -1, 0, 0, 0, 1)
    double m[28] = {}, xi[6];
    int rank = -1;
    m[6] = 1.0; m[10] = -1.0; m[20] = 1.0; m[22] = -0.5; m[26] = 0.5; m[27] = 0.25;
    icp::check_status(fgoicp_plane_step_from_moments(1, m, xi, &rank), "fgoicp_plane_step_from_moments");
    if (rank != 1 || !(xi[1] > 0.24 && xi[1] < 0.26) || !(xi[5] < -0.24 && xi[5] > -0.26)) return 3;
    icp::FastGoICP solver(read_txt(argv[1]), read_txt(argv[2]), std::stof(argv[3]), 1e-3f, FGOICP_SCHEDULE_SERIAL, 1, 0, 0.0f);
    solver.run();
    const icp::PlaneRefinement p = solver.refine_plane();
    std::cout.flush();
    std::printf("{\"iterations\": %d, \"rank\": %d, \"correspondences\": %llu, \"plane_rmse\": %.17g, \"t\": [%.9g, %.9g, %.9g]}\n", p.result.iterations, p.result.rank,
                (unsigned long long)p.result.correspondences, p.plane_rmse(), p.t().x, p.t().y, p.t().z);
    return 0;
}
