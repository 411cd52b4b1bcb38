// fast-go-icp — the reference's CLI (src/main.cpp:8-58) over libfgoicp_amd.so:
//     fast-go-icp -c config.toml [-v]
//     fast-go-icp --batch LIST [-v]      (EXTENSION: every config of LIST as one batch on one GPU, fgoicp_batch_*)
// Same flags, same TOML keys / defaults / clamps, same log lines; the search runs on the MI355X.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/fgoicp/fgoicp.hpp"
#include "config.hpp"
#include "../host/refined_pose.hpp"

static std::string usage(const std::string& exe) {
    return "Fast Go-ICP: an MI355X (HIP) implementation of Go-ICP\nUsage: " + exe + " [OPTIONS]\n\nOptions:\n"
           "  -h,--help                   Print this help message and exit\n"
           "  -c,--config TEXT REQUIRED   Path to the TOML configuration file\n"
           "  -v,--verbose                Enable verbose logging\n"
           "  -g,--gpus N                 Shard the search over N GPUs of this node (default: params.gpus, 1)\n"
           "  -b,--batch LIST             Run every config listed in LIST (one path per line, relative to LIST) as one batch on one GPU\n\nExample Usage:\n  " + exe + " -c config.toml --verbose\n  " + exe + " --config=config.toml\n";
}

// One cloud of a run.  params.*_mesh_points off: cli::load_cloud, as ever.  On: the file is read as a triangle mesh (cli::load_mesh_ply) and
// the cloud is that many samples of its surface (fgoicp_mesh_sample on device 0; the seed is params.seed if >= 0, else 0), then thinned by
// *_subsample as a loaded cloud is: everything downstream sees the samples.  A TXT file, a PLY without faces and a mesh without area are
// errors of the configuration: exit code 1.  The face normals are not carried through the filters: params.refine = "plane" / "gicp" keep estimating
// their own ("mesh" refines against the file's triangles themselves, refine_to_mesh below).
static void load_input(const std::string& path, float subsample, int mesh_points, long long load_seed, long long params_seed, std::vector<icp::vec3>& pc, const char* which) {
    if (mesh_points <= 0) {
        cli::load_cloud(path, subsample, pc, load_seed);
        return;
    }
    auto fail = [&](const std::string& why) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_mesh_points = " << mesh_points << ": " << why;
        std::exit(1);
    };
    if (!cli::is_ply(path)) fail(path + " is not a PLY file: only a PLY holds a mesh");
    std::vector<icp::vec3> vertices;
    std::vector<uint32_t> triangles;
    size_t short_faces = 0;
    cli::load_mesh_ply(path, vertices, triangles, &short_faces);
    if (triangles.empty()) fail(path + " has no faces (element face with a vertex_indices list)");
    pc.assign((size_t)mesh_points, icp::vec3{});
    fgoicp_mesh_info_t mi{};
    mi.struct_size = sizeof(mi);
    const int rc = fgoicp_mesh_sample(&vertices.data()->x, vertices.size(), triangles.data(), triangles.size() / 3, pc.size(), (uint64_t)(params_seed < 0 ? 0 : params_seed), 0,
                                      &pc.data()->x, nullptr, nullptr, nullptr, nullptr, &mi);
    if (rc != FGOICP_OK) fail("status " + std::to_string(rc) + ": " + fgoicp_last_error());
    icp::Logger log(icp::LogLevel::Info);
    log << "Mesh sampling (" << which << "): " << mi.vertices << " vertices, " << mi.triangles << " triangles (" << mi.zero_area << " zero-area, " << mi.unweighted
        << " unweighted), area " << mi.area << " -> " << pc.size() << " points";
    if (short_faces) log << "; " << short_faces << " faces of fewer than 3 vertices dropped";
    cli::subsample_cloud(pc, subsample, load_seed);
}

// io.deviation: the target FILE's mesh — every vertex and face (cli::load_mesh_ply), whether or not params.target_mesh_points sampled it for the
// registration — read before anything runs, so that a TXT target and a PLY without faces end the run at once: exit code 1, the key named.
struct DeviationMesh {
    std::vector<icp::vec3> vertices;
    std::vector<uint32_t> triangles;
};
// params.refine = "mesh" needs the same mesh, read by the same loader at the same moment: without io.deviation the errors name that key.
static std::string mesh_key(const cli::Config& c) { return c.io.deviation.empty() ? "params.refine = \"mesh\"" : "io.deviation = \"" + c.io.deviation + "\""; }
static void load_deviation_mesh(const cli::Config& c, DeviationMesh& m) {
    if (c.io.deviation.empty() && c.params.refine != "mesh") return;
    auto fail = [&](const std::string& why) {
        icp::Logger(icp::LogLevel::Error) << mesh_key(c) << ": " << why;
        std::exit(1);
    };
    if (!cli::is_ply(c.io.target)) fail("the target " + c.io.target + " is not a PLY file: only a PLY holds a mesh");
    cli::load_mesh_ply(c.io.target, m.vertices, m.triangles);
    if (m.triangles.empty()) fail("the target " + c.io.target + " has no faces (element face with a vertex_indices list)");
}
// ... and after the run: the source points the registration saw (the rows of io.alignment), moved by the final pose — the refined one when
// params.refine is set, else the best transform; R9 in glm order, R9[col * 3 + row] — as write_visualization_ply moves them, formed in fp64
// per axis, (R[a][0] x + R[a][1] y) + R[a][2] z + t[a], and rounded to fp32 once; fgoicp_mesh_distance on device 0.  A mesh without area
// is refused by the call: exit code 1, the key named.
static void write_deviation(const cli::Config& c, const DeviationMesh& m, const std::vector<icp::vec3>& src, const float* R9, const float* t3, const std::string& prefix) {
    if (c.io.deviation.empty()) return;
    std::vector<icp::vec3> moved(src.size());
    for (size_t i = 0; i < src.size(); ++i) {
        const double x = src[i].x, y = src[i].y, z = src[i].z;
        float q[3];
        for (int a = 0; a < 3; ++a) q[a] = (float)((((double)R9[a] * x + (double)R9[3 + a] * y) + (double)R9[6 + a] * z) + (double)t3[a]);
        moved[i] = icp::vec3{q[0], q[1], q[2]};
    }
    std::vector<uint32_t> face(src.size());
    std::vector<double> dist2(src.size());
    std::vector<uint8_t> region(src.size());
    std::vector<int8_t> side(src.size());
    fgoicp_mesh_distance_info_t mi{};
    mi.struct_size = sizeof(mi);
    const int rc = fgoicp_mesh_distance(&m.vertices.data()->x, m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, &moved.data()->x, moved.size(), 0u, 0, face.data(),
                                        nullptr, dist2.data(), region.data(), side.data(), &mi);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "io.deviation = \"" << c.io.deviation << "\": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    const cli::DeviationSummary s = cli::summarize_deviation(mi, dist2.data(), side.data());
    cli::write_deviation_txt(c.io.deviation, src, face.data(), dist2.data(), side.data(), region.data(), s);
    icp::Logger(icp::LogLevel::Info) << prefix << "Deviation (source -> target mesh): " << s.points << " points, " << s.triangles << " triangles (" << s.zero_area
                                     << " zero-area), rms " << s.rms << ", max " << s.max;
}

// params.target_voxel / params.source_voxel: the loaded cloud replaced by the centroids of its voxel grid (fgoicp_voxel_downsample on device 0,
// the origin is the cloud's own minimum), once, before any solver exists: everything downstream sees the thinned cloud.  A refused size
// (too small for the cloud's extent, not finite) is an error of the configuration: reported, exit code 1.
static void voxel_thin(std::vector<icp::vec3>& pc, float voxel, const char* which) {
    if (!(voxel > 0.0f)) return;
    std::vector<icp::vec3> out(pc.size());
    fgoicp_voxel_info_t vi{};
    vi.struct_size = sizeof(vi);
    const int rc = fgoicp_voxel_downsample(&pc.data()->x, pc.size(), voxel, nullptr, 0, &out.data()->x, out.size(), nullptr, nullptr, &vi);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_voxel = " << voxel << ": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    out.resize((size_t)vi.voxels);
    icp::Logger(icp::LogLevel::Info) << "Voxel grid (" << which << "): " << pc.size() << " -> " << out.size() << " points, voxel " << voxel;
    pc.swap(out);
}

// params.*_outlier_knn: the cloud replaced by the points fgoicp_remove_outliers keeps (device 0), after the voxel grid and before any solver
// exists: everything downstream sees the filtered cloud, and the indices of io.alignment are those of its rows.  A radius > 0 selects the
// radius filter, otherwise the statistical one runs with the std ratio.  A refused call is an error of the configuration: exit code 1.
static void outlier_filter(std::vector<icp::vec3>& pc, int knn, float std_ratio, float radius, const char* which) {
    if (knn <= 0) return;
    const bool by_radius = radius > 0.0f;
    std::vector<icp::vec3> out(pc.size());
    fgoicp_outlier_info_t oi{};
    oi.struct_size = sizeof(oi);
    const int rc = fgoicp_remove_outliers(&pc.data()->x, pc.size(), by_radius ? FGOICP_OUTLIER_RADIUS : FGOICP_OUTLIER_STATISTICAL, knn, by_radius ? radius : std_ratio, 0,
                                          &out.data()->x, out.size(), nullptr, nullptr, nullptr, nullptr, &oi);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_outlier_knn = " << knn << ": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    out.resize((size_t)oi.kept);
    if (by_radius)
        icp::Logger(icp::LogLevel::Info) << "Outlier filter (" << which << "): " << pc.size() << " -> " << out.size() << " points, " << knn << " neighbours, radius " << radius;
    else
        icp::Logger(icp::LogLevel::Info) << "Outlier filter (" << which << "): " << pc.size() << " -> " << out.size() << " points, " << knn << " neighbours, std ratio "
                                         << std_ratio << ", threshold " << oi.threshold;
    pc.swap(out);
}

// params.*_plane_distance: the cloud without the points of its dominant planes (fgoicp_segment_planes on device 0, refitted planes, the rest
// kept) — after the outlier filter and before the clustering, which a support plane would otherwise join into one component.  A plane needs
// ceil(min_fraction x points) inliers; none of that size leaves the cloud as it is.  A refused call, and a filter that keeps no point, is an
// error of the configuration: exit code 1.
static void plane_filter(std::vector<icp::vec3>& pc, float distance, int iterations, int count, double min_fraction, long long seed, const char* which) {
    if (!(distance > 0.0f)) return;
    const double want = std::ceil(min_fraction * (double)pc.size());
    const size_t min_inliers = want > 0.0 ? (want < 9e18 ? (size_t)want : (size_t)9e18) : 0;
    std::vector<icp::vec3> out(pc.size());
    std::vector<fgoicp_segment_model_t> models(16);
    fgoicp_segment_info_t si{};
    si.struct_size = sizeof(si);
    const int rc = fgoicp_segment_planes(&pc.data()->x, pc.size(), distance, iterations, (uint64_t)seed, count, min_inliers, 1, 0, 0, &out.data()->x, out.size(), nullptr,
                                         nullptr, models.data(), models.size(), sizeof(fgoicp_segment_model_t), &si);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_plane_distance = " << distance << ": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    if (si.kept == 0) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_plane_distance = " << distance << ": the filter keeps no point (" << si.planes << " planes hold all "
                                          << si.on_planes << " points)";
        std::exit(1);
    }
    icp::Logger log(icp::LogLevel::Info);
    log << "Plane filter (" << which << "): " << pc.size() << " -> " << si.kept << " points, distance " << distance << ", " << iterations << " hypotheses: ";
    if (si.planes == 0) {
        log << "no plane of at least " << (min_inliers > 3 ? min_inliers : (size_t)3) << " points: unchanged";
        return;
    }
    log << si.planes << (si.planes == 1 ? " plane of " : " planes of ");
    for (uint64_t j = 0; j < si.planes; ++j) log << (j == 0 ? "" : (j + 1 == si.planes ? " and " : ", ")) << models[(size_t)j].inliers;
    const double* p = models[0].plane;
    auto tidy = [](double v) { return std::fabs(v) < 5e-7 ? 0.0 : v; };  // (six digits are printed: no "-0" and no 1e-09 beside a 1)
    log << " points, normal (" << tidy(p[0]) << " " << tidy(p[1]) << " " << tidy(p[2]) << "), offset " << tidy(p[3]);
    out.resize((size_t)si.kept);
    pc.swap(out);
}

// params.*_cluster_eps: the cloud replaced by the points fgoicp_cluster_dbscan keeps (device 0) — its largest cluster, or with
// params.*_cluster_min_size >= 1 every cluster of at least that many points — after the outlier filter and before the sampling and any solver:
// everything downstream sees the filtered cloud.  A refused call, and a filter that keeps no point, is an error of the configuration: exit code 1.
static void cluster_filter(std::vector<icp::vec3>& pc, float eps, int min_points, int min_size, const char* which) {
    if (!(eps > 0.0f)) return;
    std::vector<icp::vec3> out(pc.size());
    std::vector<uint64_t> sizes(pc.size());
    fgoicp_cluster_info_t ci{};
    ci.struct_size = sizeof(ci);
    const int rc = fgoicp_cluster_dbscan(&pc.data()->x, pc.size(), eps, min_points, (size_t)min_size, 0, &out.data()->x, out.size(), nullptr, nullptr, nullptr, sizes.data(),
                                         sizes.size(), &ci);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_cluster_eps = " << eps << ": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    if (ci.kept == 0) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_cluster_eps = " << eps << ": the filter keeps no point (" << ci.clusters << " clusters, "
                                          << ci.noise_points << " noise points, " << min_points << " neighbours, clusters of at least " << min_size << " points)";
        std::exit(1);
    }
    out.resize((size_t)ci.kept);
    size_t kept_clusters = 0;
    for (uint64_t c = 0; c < ci.clusters; ++c) kept_clusters += sizes[(size_t)c] >= (uint64_t)min_size ? 1 : 0;
    icp::Logger log(icp::LogLevel::Info);
    log << "Cluster filter (" << which << "): " << pc.size() << " -> " << out.size() << " points, eps " << eps << ", " << min_points << " neighbours: " << ci.clusters
        << " clusters, " << ci.noise_points << " noise points, ";
    if (min_size <= 0) log << "kept the largest";
    else log << "kept " << kept_clusters << " clusters of at least " << min_size << " points";
    pc.swap(out);
}

// params.*_points: the cloud replaced by fgoicp_farthest_point_sample's picks (device 0, start_index 0) in pick order, after the outlier filter
// and before any solver exists: everything downstream sees the sampled cloud.  A cloud that has no more points than asked stays as it is,
// order included.  A refused call is an error of the configuration: exit code 1.
static void farthest_sample(std::vector<icp::vec3>& pc, int points, const char* which) {
    if (points <= 0) return;
    if (pc.size() <= (size_t)points) {
        icp::Logger(icp::LogLevel::Info) << "Farthest-point sampling (" << which << "): " << pc.size() << " points, at most " << points << " asked: unchanged";
        return;
    }
    std::vector<icp::vec3> out((size_t)points);
    fgoicp_fps_info_t fi{};
    fi.struct_size = sizeof(fi);
    const int rc = fgoicp_farthest_point_sample(&pc.data()->x, pc.size(), out.size(), 0, 0, &out.data()->x, nullptr, nullptr, nullptr, nullptr, &fi);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params." << which << "_points = " << points << ": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    icp::Logger(icp::LogLevel::Info) << "Farthest-point sampling (" << which << "): " << pc.size() << " -> " << out.size() << " points, cover radius "
                                     << std::sqrt(fi.cover_dist2);
    pc.swap(out);
}

// a robust result as the [refined] table and the log line take it: the fields fgoicp_plane_result_t shares
static void plane_from_robust(const fgoicp_robust_result_t& robust, fgoicp_plane_result_t& refined) {
    std::memcpy(refined.R, robust.R, sizeof(refined.R));
    std::memcpy(refined.t, robust.t, sizeof(refined.t));
    refined.iterations = robust.iterations; refined.rank = robust.rank; refined.correspondences = robust.correspondences;
    refined.plane_rmse = robust.rmse; refined.sse = robust.sse; refined.scaling_factor = robust.scaling_factor;
}
// the refinement's log line (a lone run's, or with a batch's "Pair i: " in front)
// rms_distance: params.refine = "mesh" (the rms of the deviation map at the refined pose; refined.plane_rmse then holds mesh_rmse)
static void log_refinement(const std::string& prefix, const cli::Config& config, const fgoicp_plane_result_t& refined, const fgoicp_robust_result_t* robust,
                           const double* rms_distance = nullptr) {
    const bool gicp = config.params.refine == "gicp";
    icp::mat3 Rr;
    std::memcpy(Rr.data(), refined.R, sizeof(refined.R));
    icp::Logger log(icp::LogLevel::Info);
    log << prefix << (rms_distance ? "Point-to-mesh" : gicp ? "Generalized-ICP" : "Point-to-plane") << " refinement: " << refined.iterations << " iterations, rank " << refined.rank
        << ", " << refined.correspondences << " correspondences, ";
    if (rms_distance) log << "rms distance " << *rms_distance << ", mesh RMSE ";
    else if (gicp) log << "epsilon " << config.params.refine_epsilon << ", plane-to-plane RMSE ";
    else log << "plane RMSE ";
    log << refined.plane_rmse / (double)refined.scaling_factor;
    if (robust)
        log << ", " << config.params.refine_loss << " loss, scale " << robust->scale / (double)robust->scaling_factor << (robust->scale_estimated ? " (estimated)" : " (given)")
            << ", weight " << robust->weight_sum << " of " << robust->correspondences;
    log << "\n\tRotation:\n" << Rr << "\n\tTranslation: " << icp::vec3{refined.t[0], refined.t[1], refined.t[2]};
}

// params.refine = "mesh": the pose near (R9, t3) — the best transform, in the files' frame, which is the mesh's — that minimises the distances
// from the source points the registration saw to the target FILE's triangles (fgoicp_mesh_refine on device 0; params.refine_max_iter,
// refine_distance, refine_loss and refine_loss_scale apply, refine_knn and refine_epsilon do not).  The result as the [refined] table and
// the log line take it: `refined` (plane_rmse holds mesh_rmse; the files' frame is the call's, so the scaling factor is 1) and, with a loss,
// `robust`.  A refusal — a mesh without area among them — ends the run: exit code 1, the key named.
static void refine_to_mesh(const cli::Config& c, const DeviationMesh& m, const std::vector<icp::vec3>& src, const float* R9, const float* t3, const std::string& prefix,
                           fgoicp_plane_result_t& refined, fgoicp_robust_result_t& robust, double& rms_distance) {
    fgoicp_mesh_refine_result_t r{};
    r.struct_size = sizeof(r);
    const int loss = c.params.refine_loss_code();
    const int rc = fgoicp_mesh_refine(&m.vertices.data()->x, m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, &src.data()->x, src.size(), R9, t3,
                                      (size_t)c.params.refine_max_iter, 1e-6f, c.params.refine_distance, loss, c.params.refine_loss_scale, 0u, 0, &r);
    if (rc != FGOICP_OK) {
        icp::Logger(icp::LogLevel::Error) << "params.refine = \"mesh\": status " << rc << ": " << fgoicp_last_error();
        std::exit(1);
    }
    refined = fgoicp_plane_result_t{};
    refined.struct_size = sizeof(refined);
    std::memcpy(refined.R, r.R, sizeof(refined.R));
    std::memcpy(refined.t, r.t, sizeof(refined.t));
    refined.iterations = r.iterations; refined.rank = r.rank; refined.correspondences = r.correspondences;
    refined.plane_rmse = r.mesh_rmse; refined.scaling_factor = 1.0f;
    robust = fgoicp_robust_result_t{};
    robust.struct_size = sizeof(robust);
    robust.correspondences = r.correspondences; robust.weight_sum = r.weight_sum; robust.scaling_factor = 1.0f;
    robust.loss = r.loss; robust.scale_estimated = r.scale_estimated; robust.scale = r.loss_scale;
    rms_distance = r.rms_distance;
    log_refinement(prefix, c, refined, loss > 0 ? &robust : nullptr, &rms_distance);
}

// --batch LIST: every config of the list registered in one fgoicp_batch run; each config's io.output / io.visualization as a lone -c run
// of it writes them (the seconds written are the batch's).  The configs must agree on the schedule and round width; each is trimmed with
// its own params.trim_fraction and refined with its own params.refine* (fgoicp_batch_opts_refine.refine): the refinement's log line, the
// [refined] table and io.information at the refined pose as a lone run of it.
static int run_batch(const std::string& list_file) {
    std::ifstream lf(list_file);
    if (!lf) { icp::Logger(icp::LogLevel::Error) << "Unable to read " << list_file; return 1; }
    const std::filesystem::path dir = std::filesystem::path(list_file).parent_path();
    std::vector<cli::Config> configs;
    for (std::string line; std::getline(lf, line);) {
        line = cli::trim(line);
        if (line.empty() || line[0] == '#') continue;
        const std::filesystem::path p(line);
        try {
            configs.emplace_back((p.is_absolute() ? p : dir / p).string());
        } catch (const std::invalid_argument& e) {
            icp::Logger(icp::LogLevel::Error) << e.what();
            return 1;
        }
    }
    if (configs.empty()) { icp::Logger(icp::LogLevel::Error) << "--batch: " << list_file << " lists no config"; return 1; }
    const cli::Config& c0 = configs[0];
    for (const cli::Config& c : configs) {
        if (c.params.gpus > 1) { icp::Logger(icp::LogLevel::Error) << "--batch: a batch runs on one GPU (params.gpus > 1)"; return 1; }
        if (c.params.schedule != c0.params.schedule || c.params.round_width != c0.params.round_width) {
            icp::Logger(icp::LogLevel::Error) << "--batch: every config of a batch must have the same params.schedule and params.round_width";
            return 1;
        }
    }
    const size_t n = configs.size();
    std::vector<std::vector<icp::vec3>> pct(n), pcs(n);
    std::vector<DeviationMesh> meshes(n);
    for (size_t i = 0; i < n; ++i) load_deviation_mesh(configs[i], meshes[i]);
    std::vector<fgoicp_batch_pair> pairs(n);
    std::vector<float> trim(n);
    for (size_t i = 0; i < n; ++i) {
        const cli::Config& c = configs[i];
        load_input(c.io.target, c.params.target_subsample, c.params.target_mesh_points, c.params.seed, c.params.seed, pct[i], "target");
        load_input(c.io.source, c.params.source_subsample, c.params.source_mesh_points, c.params.seed < 0 ? -1 : c.params.seed + 1, c.params.seed, pcs[i], "source");
        voxel_thin(pct[i], c.params.target_voxel, "target");
        voxel_thin(pcs[i], c.params.source_voxel, "source");
        outlier_filter(pct[i], c.params.target_outlier_knn, c.params.target_outlier_std, c.params.target_outlier_radius, "target");
        outlier_filter(pcs[i], c.params.source_outlier_knn, c.params.source_outlier_std, c.params.source_outlier_radius, "source");
        plane_filter(pct[i], c.params.target_plane_distance, c.params.target_plane_iterations, c.params.target_plane_count, c.params.target_plane_min_fraction,
                     c.params.seed < 0 ? 0 : c.params.seed, "target");
        plane_filter(pcs[i], c.params.source_plane_distance, c.params.source_plane_iterations, c.params.source_plane_count, c.params.source_plane_min_fraction,
                     c.params.seed < 0 ? 1 : c.params.seed + 1, "source");
        cluster_filter(pct[i], c.params.target_cluster_eps, c.params.target_cluster_min_points, c.params.target_cluster_min_size, "target");
        cluster_filter(pcs[i], c.params.source_cluster_eps, c.params.source_cluster_min_points, c.params.source_cluster_min_size, "source");
        farthest_sample(pct[i], c.params.target_points, "target");
        farthest_sample(pcs[i], c.params.source_points, "source");
        icp::Logger(icp::LogLevel::Info) << "Pair " << i << ": target (" << pct[i].size() << ") " << c.io.target << ", source (" << pcs[i].size() << ") " << c.io.source;
        pairs[i] = fgoicp_batch_pair{&pct[i].data()->x, pct[i].size(), &pcs[i].data()->x, pcs[i].size(), c.params.lut_resolution, c.params.mse_threshold};
        trim[i] = c.params.trim_fraction;
    }
    const int schedule = c0.params.schedule == "round" ? FGOICP_SCHEDULE_ROUND : FGOICP_SCHEDULE_SERIAL;
    fgoicp_batch_opts_refine with_refine{};
    fgoicp_batch_opts& o = with_refine.opts;
    o.struct_size = sizeof(with_refine);
    o.solver = fgoicp_solver_opts{schedule, c0.params.round_width, 0u, 0, 0.0f};
    o.trim_fractions = trim.data();
    for (const cli::Config& c : configs) o.alignment |= c.io.alignment.empty() ? 0 : 1;  // the reports are kept only if a config asks for one
    for (const cli::Config& c : configs) {  // ... and the information matrices; a batch has one distance threshold
        if (c.io.information.empty()) continue;
        if (o.information && c.params.information_distance != o.information_max_distance) {
            icp::Logger(icp::LogLevel::Error) << "--batch: every config of a batch that names io.information must have the same params.information_distance";
            return 1;
        }
        o.information = 1;
        o.information_max_distance = c.params.information_distance;
    }
    std::vector<fgoicp_batch_refine_t> refine(n);
    bool any_refine = false;
    for (size_t i = 0; i < n; ++i) {
        const cli::Config& c = configs[i];
        fgoicp_batch_refine_t& r = refine[i];
        r.struct_size = sizeof(r);
        r.model = c.params.refine == "gicp" ? FGOICP_MODEL_GICP : c.params.refine == "plane" ? FGOICP_MODEL_PLANE : -1;
        if (r.model < 0) continue;
        any_refine = true;
        r.k = c.params.refine_knn;
        r.max_iter = (size_t)c.params.refine_max_iter;
        r.conv_thr = 1e-6f;
        r.max_distance = c.params.refine_distance > 0.0f ? c.params.refine_distance : INFINITY;
        r.epsilon = c.params.refine_epsilon;
        r.loss = c.params.refine_loss_code();
        r.loss_scale = c.params.refine_loss_scale;
    }
    if (any_refine) with_refine.refine = refine.data();
    fgoicp_batch* b = nullptr;
    icp::check_status(fgoicp_batch_create(pairs.data(), (int)n, &o, &b), "fgoicp_batch_create");
    std::vector<float> R9(9 * n), t3(3 * n);
    std::vector<int> status(n, 0);
    const auto start = std::chrono::high_resolution_clock::now();
    icp::check_status(fgoicp_batch_run(b, R9.data(), t3.data(), status.data()), "fgoicp_batch_run");
    const std::chrono::duration<double> elapsed = std::chrono::high_resolution_clock::now() - start;
    icp::Logger(icp::LogLevel::Info) << "Fast Go-ICP batch of " << n << " finished, time elapsed: " << std::fixed << std::setprecision(3) << elapsed.count() << " seconds";
    int rc = 0;
    for (size_t i = 0; i < n; ++i) {
        if (status[i]) { icp::Logger(icp::LogLevel::Error) << "Pair " << i << " failed (status " << status[i] << ")"; rc = 1; continue; }
        icp::mat3 R;
        std::memcpy(R.data(), &R9[9 * i], 9 * sizeof(float));
        const icp::vec3 t{t3[3 * i], t3[3 * i + 1], t3[3 * i + 2]};
        float best_error = 0.f;
        fgoicp_run_stats st{};
        icp::check_status(fgoicp_batch_best_error(b, (int)i, &best_error), "fgoicp_batch_best_error");
        icp::check_status(fgoicp_batch_stats(b, (int)i, &st), "fgoicp_batch_stats");
        icp::Logger(icp::LogLevel::Info) << "Pair " << i << ": Best Error: " << best_error << "\n\tRotation:\n" << R << "\n\tTranslation: " << t;
        const cli::Config& c = configs[i];
        fgoicp_plane_result_t refined{};
        fgoicp_robust_result_t robust{};
        // params.refine = "mesh": not one of the batch's own refinements (its specs stay plane / gicp) — the one-shot call, here, as
        // write_deviation below; io.information of such a config stays at the best transform (a batch keeps no context to ask at another pose)
        const bool to_mesh = c.params.refine == "mesh", in_batch = refine[i].model >= 0;
        const bool have_refined = in_batch || to_mesh, have_robust = have_refined && c.params.refine_loss_code() > 0;
        double rms_distance = 0.0;
        if (to_mesh) {
            refine_to_mesh(c, meshes[i], pcs[i], &R9[9 * i], &t3[3 * i], "Pair " + std::to_string(i) + ": ", refined, robust, rms_distance);
        } else if (have_robust) {
            robust.struct_size = sizeof(robust);
            icp::check_status(fgoicp_batch_refined_robust(b, (int)i, &robust), "fgoicp_batch_refined_robust");
            plane_from_robust(robust, refined);
        } else if (have_refined) {
            refined.struct_size = sizeof(refined);
            icp::check_status(fgoicp_batch_refined_plane(b, (int)i, &refined), "fgoicp_batch_refined_plane");
        }
        if (in_batch) log_refinement("Pair " + std::to_string(i) + ": ", c, refined, have_robust ? &robust : nullptr);
        if (!c.io.output.empty())
            cli::write_result_toml(c.io.output, R, t, best_error, pcs[i].size(), elapsed.count(), st, have_refined ? &refined : nullptr,
                                   to_mesh ? "mesh_rmse" : c.params.refine == "gicp" ? "gicp_rmse" : "plane_rmse", have_robust ? &robust : nullptr, c.params.refine_loss.c_str(),
                                   to_mesh ? &rms_distance : nullptr);
        if (!c.io.visualization.empty()) cli::write_visualization_ply(c.io.visualization, pct[i], pcs[i], R, t);
        if (!c.io.alignment.empty()) {
            std::vector<uint32_t> idx(pcs[i].size());
            std::vector<float> d2(pcs[i].size());
            std::vector<uint8_t> inl(pcs[i].size());
            fgoicp_alignment_summary sm{};
            sm.struct_size = sizeof(sm);
            icp::check_status(fgoicp_batch_alignment(b, (int)i, idx.data(), d2.data(), inl.data(), nullptr, &sm), "fgoicp_batch_alignment");
            cli::write_alignment_txt(c.io.alignment, pcs[i], idx.data(), d2.data(), inl.data(), sm);
        }
        if (!c.io.information.empty()) {
            fgoicp_information_t inf{};
            inf.struct_size = sizeof(inf);
            if (in_batch) icp::check_status(fgoicp_batch_refined_information(b, (int)i, &inf), "fgoicp_batch_refined_information");  // as a lone run: at the refined pose
            else icp::check_status(fgoicp_batch_information(b, (int)i, &inf), "fgoicp_batch_information");
            cli::write_information_txt(c.io.information, inf, c.params.information_distance);
        }
        write_deviation(c, meshes[i], pcs[i], have_refined ? refined.R : &R9[9 * i], have_refined ? refined.t : &t3[3 * i], "Pair " + std::to_string(i) + ": ");
    }
    fgoicp_batch_destroy(b);
    return rc;
}

int main(int argc, char* argv[]) {
    std::string config_file, batch_file;
    bool verbose = false;
    int gpus_flag = 0;
    const std::string exe = std::filesystem::path(argv[0]).filename().string();
    auto fail = [&](const std::string& what, int code) {
        icp::Logger(icp::LogLevel::Error) << what;
        icp::Logger(icp::LogLevel::Info) << usage(exe);
        std::exit(code);
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") { std::cout << usage(exe); return 0; }
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "-g" || a == "--gpus") { if (i + 1 >= argc) fail("--gpus: 1 required INT missing", 114); gpus_flag = std::atoi(argv[++i]); }
        else if (a.rfind("--gpus=", 0) == 0) gpus_flag = std::atoi(a.substr(7).c_str());
        else if (a == "-b" || a == "--batch") { if (i + 1 >= argc) fail("--batch: 1 required TEXT missing", 114); batch_file = argv[++i]; }
        else if (a.rfind("--batch=", 0) == 0) batch_file = a.substr(8);
        else if (a == "-c" || a == "--config") { if (i + 1 >= argc) fail("--config: 1 required TEXT missing", 114); config_file = argv[++i]; }
        else if (a.rfind("--config=", 0) == 0) config_file = a.substr(9);
        else if (a.rfind("-c", 0) == 0 && a.size() > 2) config_file = a.substr(2);
        else fail("The following argument was not expected: " + a, 109);
    }
    if (!batch_file.empty()) {
        if (!config_file.empty()) fail("--batch excludes --config", 109);
        if (gpus_flag > 1) fail("--batch runs on one GPU: --gpus > 1 is not allowed with it", 109);
        icp::Logger::set_verbose(verbose);
        return run_batch(batch_file);
    }
    if (config_file.empty()) fail("--config is required", 106);
    icp::Logger::set_verbose(verbose);

    cli::Config config = [&] {
        try {
            return cli::Config(config_file);
        } catch (const std::invalid_argument& e) {
            icp::Logger(icp::LogLevel::Error) << e.what();
            std::exit(1);
        }
    }();
    DeviationMesh deviation_mesh;
    load_deviation_mesh(config, deviation_mesh);
    std::vector<icp::vec3> pct, pcs;
    load_input(config.io.target, config.params.target_subsample, config.params.target_mesh_points, config.params.seed, config.params.seed, pct, "target");
    icp::Logger(icp::LogLevel::Info) << "Target point cloud (" << pct.size() << ") loaded from " << config.io.target;
    load_input(config.io.source, config.params.source_subsample, config.params.source_mesh_points, config.params.seed < 0 ? -1 : config.params.seed + 1, config.params.seed, pcs,
               "source");
    icp::Logger(icp::LogLevel::Info) << "Source point cloud (" << pcs.size() << ") loaded from " << config.io.source;
    voxel_thin(pct, config.params.target_voxel, "target");
    voxel_thin(pcs, config.params.source_voxel, "source");
    outlier_filter(pct, config.params.target_outlier_knn, config.params.target_outlier_std, config.params.target_outlier_radius, "target");
    outlier_filter(pcs, config.params.source_outlier_knn, config.params.source_outlier_std, config.params.source_outlier_radius, "source");
    plane_filter(pct, config.params.target_plane_distance, config.params.target_plane_iterations, config.params.target_plane_count,
                 config.params.target_plane_min_fraction, config.params.seed < 0 ? 0 : config.params.seed, "target");
    plane_filter(pcs, config.params.source_plane_distance, config.params.source_plane_iterations, config.params.source_plane_count,
                 config.params.source_plane_min_fraction, config.params.seed < 0 ? 1 : config.params.seed + 1, "source");
    cluster_filter(pct, config.params.target_cluster_eps, config.params.target_cluster_min_points, config.params.target_cluster_min_size, "target");
    cluster_filter(pcs, config.params.source_cluster_eps, config.params.source_cluster_min_points, config.params.source_cluster_min_size, "source");
    farthest_sample(pct, config.params.target_points, "target");
    farthest_sample(pcs, config.params.source_points, "source");
    const std::vector<icp::vec3> pct_in = pct, pcs_in = pcs;
    for (const auto* pc : {&pct, &pcs}) {  // verbose: the statistics the pre-processing normalises by (TODO.md:7 of the reference)
        fgoicp_cloud_stats_t cs{};
        if (fgoicp_cloud_stats(&pc->data()->x, pc->size(), &cs) == FGOICP_OK)
            icp::Logger(icp::LogLevel::Debug) << (pc == &pct ? "Target" : "Source") << " statistics: centroid " << icp::vec3{cs.centroid[0], cs.centroid[1], cs.centroid[2]}
                                              << ", box [" << cs.min[0] << ", " << cs.max[0] << "] x [" << cs.min[1] << ", " << cs.max[1] << "] x [" << cs.min[2] << ", " << cs.max[2]
                                              << "], largest centred coordinate " << cs.max_abs_centred << ", RMS radius " << cs.rms_radius;
    }

    const int schedule = config.params.schedule == "round" ? FGOICP_SCHEDULE_ROUND : FGOICP_SCHEDULE_SERIAL;
    const int gpus = gpus_flag > 0 ? gpus_flag : config.params.gpus;
    icp::mat3 R;
    icp::vec3 t;
    fgoicp_run_stats st{};
    float best_error = 0.f;
    std::chrono::duration<double> elapsed_seconds{};
    // io.alignment: the report at the best transform, from the solver that ran (rank 0's on several GPUs: every rank holds the same answer)
    auto write_alignment = [&](fgoicp_solver* s) {
        if (config.io.alignment.empty()) return;
        std::vector<uint32_t> idx(pcs_in.size());
        std::vector<float> d2(pcs_in.size());
        std::vector<uint8_t> inl(pcs_in.size());
        fgoicp_alignment_summary sm{};
        sm.struct_size = sizeof(sm);
        icp::check_status(fgoicp_solver_alignment(s, idx.data(), d2.data(), inl.data(), nullptr, &sm), "fgoicp_solver_alignment");
        cli::write_alignment_txt(config.io.alignment, pcs_in, idx.data(), d2.data(), inl.data(), sm);
    };
    // params.refine = "plane" / "gicp": point-to-plane / Generalized-ICP refinement from the best transform, after the search (the search's own result stays as it is)
    fgoicp_plane_result_t refined{};
    bool have_refined = false;
    const bool gicp = config.params.refine == "gicp";
    // params.refine_loss: the same refinement under a robust loss (fgoicp_solver_refine_robust); its pose and counts go into `refined`
    fgoicp_robust_result_t robust{};
    const int loss = config.params.refine_loss_code();
    bool have_robust = false;
    // params.refine = "mesh": from the best transform too, against the target FILE's triangles; once, on the host thread
    const bool to_mesh = config.params.refine == "mesh";
    double rms_distance = 0.0;
    auto refine = [&](fgoicp_solver* s) {
        if (to_mesh) {
            refine_to_mesh(config, deviation_mesh, pcs_in, R.data(), &t.x, "", refined, robust, rms_distance);
            have_refined = true;
            have_robust = loss > 0;
            return;
        }
        if (config.params.refine != "plane" && !gicp) return;
        refined.struct_size = sizeof(refined);
        const float d = config.params.refine_distance > 0.0f ? config.params.refine_distance : INFINITY;
        const int knn = config.params.refine_knn;
        const size_t max_iter = (size_t)config.params.refine_max_iter;
        if (loss > 0) {
            robust.struct_size = sizeof(robust);
            icp::check_status(fgoicp_solver_refine_robust(s, gicp ? FGOICP_MODEL_GICP : FGOICP_MODEL_PLANE, knn, max_iter, 1e-6f, d, config.params.refine_epsilon, loss,
                                                          config.params.refine_loss_scale, &robust), "fgoicp_solver_refine_robust");
            plane_from_robust(robust, refined);
            have_robust = true;
        } else if (gicp) {
            icp::check_status(fgoicp_solver_refine_gicp(s, knn, max_iter, 1e-6f, d, config.params.refine_epsilon, &refined), "fgoicp_solver_refine_gicp");
        } else {
            icp::check_status(fgoicp_solver_refine_plane(s, knn, max_iter, 1e-6f, d, &refined), "fgoicp_solver_refine_plane");
        }
        have_refined = true;
        log_refinement("", config, refined, have_robust ? &robust : nullptr);
    };
    // io.information: the information matrix in the files' frame — at the best transform, or at the refined pose when there is one: then
    // from the context at that pose in the solver's frame (the restored translation taken back, t_s = (t - R offset_pcs + offset_pct) * scale)
    // and converted as fgoicp_solver_information converts (fgoicp_information_from_moments): refined_pose.hpp, the text a batch runs too
    auto write_information = [&](fgoicp_solver* s) {
        if (config.io.information.empty()) return;
        fgoicp_information_t inf{};
        inf.struct_size = sizeof(inf);
        const float d = config.params.information_distance;
        if (!have_refined) {
            icp::check_status(fgoicp_solver_information(s, d > 0.0f ? d : INFINITY, &inf), "fgoicp_solver_information");
        } else {
            float offs[6], scale = 1.0f;
            icp::check_status(fgoicp_solver_preproc(s, offs, &scale, nullptr), "fgoicp_solver_preproc");
            icp::check_status(fgoicp::refined_information(fgoicp_solver_ctx(s), refined.R, refined.t, offs, scale, d, &inf), "fgoicp_information at the refined pose");
        }
        cli::write_information_txt(config.io.information, inf, d);
    };
    if (gpus > 1) {
        // EXTENSION: one host thread + one solver per GPU (include/fgoicp_amd.h, fgoicp_multi_*).  params.schedule = "serial" (the
        // default) keeps the reference's exact trajectory and deals the inner BnBs of every speculative evaluation over the GPUs;
        // "round" deals the children of every expansion round (one RCCL all-gather per round; fastest).
        std::vector<int> devices;
        for (int d = 0; d < gpus; ++d) devices.push_back(d);
        int transport = FGOICP_TRANSPORT_RCCL;
        if (const char* e = std::getenv("FGOICP_MULTI_DEVICES")) {  // e.g. "0,0": rehearse two ranks on one GPU (in-process transport)
            devices.clear();
            for (const char* p = e; *p;) { devices.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p) ++p; }
            transport = FGOICP_TRANSPORT_IN_PROCESS;
        }
        icp::Logger(icp::LogLevel::Info) << "Sharding the search over " << devices.size() << " GPUs (schedule: "
                                         << (schedule == FGOICP_SCHEDULE_ROUND ? "expansion rounds" : "the reference's order, evaluations sharded") << ")";
        fgoicp_solver_opts o{schedule, schedule == FGOICP_SCHEDULE_ROUND ? config.params.round_width : 1, 0u, 0, config.params.trim_fraction};
        fgoicp_multi* m = nullptr;
        icp::check_status(fgoicp_multi_create(&pct.data()->x, pct.size(), &pcs.data()->x, pcs.size(), config.params.lut_resolution, config.params.mse_threshold, &o,
                                              devices.data(), (int)devices.size(), transport, &m), "fgoicp_multi_create");
        // rank 0's log events: every rank holds the same incumbents (SERIAL and the cooperative flow: the same refinements too)
        icp::check_status(fgoicp_solver_set_log(fgoicp_multi_solver(m, 0), &icp::FastGoICP::log_line, nullptr), "fgoicp_solver_set_log");
        auto start = std::chrono::high_resolution_clock::now();
        icp::check_status(fgoicp_multi_run(m, R.data(), &t.x), "fgoicp_multi_run");
        elapsed_seconds = std::chrono::high_resolution_clock::now() - start;
        // ROUND: counters summed over the ranks; SERIAL: every rank holds the whole trajectory's counters (rank 0's are reported).
        // Rank 0's incumbent is every rank's.
        for (int r = 0; r < (schedule == FGOICP_SCHEDULE_ROUND ? (int)devices.size() : 1); ++r) {
            fgoicp_run_stats s1{};
            icp::check_status(fgoicp_solver_stats(fgoicp_multi_solver(m, r), &s1), "fgoicp_solver_stats");
            st.trans_cubes += s1.trans_cubes; st.rot_cubes += s1.rot_cubes; st.icp_runs += s1.icp_runs; st.icp_iters += s1.icp_iters;
            st.bounds_calls += s1.bounds_calls; st.inner_bnb += s1.inner_bnb;
            if (r == 0) { st.rounds = s1.rounds; st.initial_icp_sse = s1.initial_icp_sse; }
        }
        icp::check_status(fgoicp_solver_best_error(fgoicp_multi_solver(m, 0), &best_error), "fgoicp_solver_best_error");
        write_alignment(fgoicp_multi_solver(m, 0));
        refine(fgoicp_multi_solver(m, 0));
        write_information(fgoicp_multi_solver(m, 0));
        fgoicp_multi_destroy(m);
        icp::Logger(icp::LogLevel::Info) << "Searching over! Best Error: " << best_error << "\n\tRotation:\n" << R << "\n\tTranslation: " << t;  // fgoicp.cpp:25-27
    } else {
        icp::FastGoICP fgoicp(std::move(pct), std::move(pcs), config.params.lut_resolution, config.params.mse_threshold, schedule,
                              config.params.round_width, 0, config.params.trim_fraction);
        auto start = std::chrono::high_resolution_clock::now();
        std::tie(R, t) = fgoicp.run();
        elapsed_seconds = std::chrono::high_resolution_clock::now() - start;
        st = fgoicp.stats();
        best_error = fgoicp.get_best_error();
        write_alignment(fgoicp.handle());
        refine(fgoicp.handle());
        write_information(fgoicp.handle());
    }
    icp::Logger(icp::LogLevel::Debug) << "Subcubes: " << st.trans_cubes << ", rotation cubes: " << st.rot_cubes << ", ICP runs: " << st.icp_runs;
    icp::Logger(icp::LogLevel::Info) << "Fast Go-ICP finished, time elapsed: " << std::fixed << std::setprecision(3) << elapsed_seconds.count() << " seconds";
    if (!config.io.output.empty()) cli::write_result_toml(config.io.output, R, t, best_error, pcs_in.size(), elapsed_seconds.count(), st, have_refined ? &refined : nullptr, to_mesh ? "mesh_rmse" : gicp ? "gicp_rmse" : "plane_rmse",
                                                              have_robust ? &robust : nullptr, config.params.refine_loss.c_str(), to_mesh ? &rms_distance : nullptr);
    if (!config.io.visualization.empty()) cli::write_visualization_ply(config.io.visualization, pct_in, pcs_in, R, t);
    write_deviation(config, deviation_mesh, pcs_in, have_refined ? refined.R : R.data(), have_refined ? refined.t : &t.x, "");  // once, on the host thread (rank 0's pose is every rank's)
    return 0;
}
