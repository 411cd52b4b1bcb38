// TEST-ONLY: prints the cluster-filter keys of a configuration as the CLI's parser (fast-go-icp_amd/csrc/cli/config.hpp) reads them; exit code 2
// and the message when the parser refuses the file.
#include <cstdio>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

int main(int argc, char** argv) {
    if (argc != 2) return 3;
    try {
        cli::Config c(argv[1]);
        std::printf("CLUSTER %.9g %.9g %d %d %d %d\n", c.params.target.cluster_eps, c.params.source.cluster_eps, c.params.target.cluster_min_points,
                    c.params.source.cluster_min_points, c.params.target.cluster_min_size, c.params.source.cluster_min_size);
        return 0;
    } catch (const std::exception& e) {
        std::printf("REFUSED %s\n", e.what());
        return 2;
    }
}
