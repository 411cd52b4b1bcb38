// TEST-ONLY: the mesh side of the CLI's parsers (fast-go-icp_amd/csrc/cli/config.hpp).
//   mesh_config_check config FILE.toml   prints the two mesh keys as the configuration parser reads them; exit code 2 and the message when
//                                        the parser refuses the file
//   mesh_config_check mesh FILE.ply      prints what load_mesh_ply reads: the counts, then one line per vertex and per triangle
//   mesh_config_check cloud FILE.ply     prints what load_cloud reads of the same file (no subsampling): the vertices
#include <cstdio>
#include <cstring>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    try {
        if (!std::strcmp(argv[1], "config")) {
            cli::Config c(argv[2]);
            std::printf("MESH_POINTS %d %d\n", c.params.target.mesh_points, c.params.source.mesh_points);
            return 0;
        }
        std::vector<icp::vec3> v;
        std::vector<uint32_t> t;
        size_t dropped = 0;
        if (!std::strcmp(argv[1], "mesh")) cli::load_mesh_ply(argv[2], v, t, &dropped);
        else if (!std::strcmp(argv[1], "cloud")) cli::load_cloud(argv[2], 1.0f, v, 1);
        else return 3;
        std::printf("MESH %zu %zu %zu\n", v.size(), t.size() / 3, dropped);
        for (const icp::vec3& p : v) std::printf("V %.9g %.9g %.9g\n", p.x, p.y, p.z);
        for (size_t f = 0; f < t.size() / 3; ++f) std::printf("T %u %u %u\n", t[3 * f], t[3 * f + 1], t[3 * f + 2]);
        return 0;
    } catch (const std::exception& e) {
        std::printf("REFUSED %s\n", e.what());
        return 2;
    }
}
