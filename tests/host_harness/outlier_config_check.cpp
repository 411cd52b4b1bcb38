// TEST-ONLY: prints the outlier keys of a configuration as the CLI's parser (fast-go-icp_amd/csrc/cli/config.hpp) reads them; exit code 2 and
// the message when the parser refuses the file.
#include <cstdio>

#include "../../fast-go-icp_amd/csrc/cli/config.hpp"

extern "C" const char* fgoicp_last_error(void) { return ""; }  // icp::check_status is never reached here

int main(int argc, char** argv) {
    if (argc != 2) return 3;
    try {
        cli::Config c(argv[1]);
        std::printf("OUTLIER %d %d %.9g %.9g %.9g %.9g\n", c.params.target.outlier_knn, c.params.source.outlier_knn, c.params.target.outlier_std, c.params.source.outlier_std,
                    c.params.target.outlier_radius, c.params.source.outlier_radius);
        return 0;
    } catch (const std::exception& e) {
        std::printf("REFUSED %s\n", e.what());
        return 2;
    }
}
