// The CLI's preparation path: the two clouds of a run from its configuration — loaded (or sampled from a mesh), then thinned and filtered on
// device 0, stage by stage, before any solver exists.  prepare_pair is the one place that knows the order of the stages and the seeds they
// take; a lone -c run and every pair of a --batch go through it.  A stage that refuses its key ends the process: fail_config / fail_status.
#pragma once
#include "config.hpp"

namespace cli {

// An error of the configuration: one Error line, exit code 1 ...
[[noreturn]] inline void fail(const std::string& line) {
    icp::Logger(icp::LogLevel::Error) << line;
    std::exit(1);
}
// ... which starts with the key as the file wrote it when a key is to blame, and carries the status and the library's message after a refused call
[[noreturn]] inline void fail_config(const std::string& key_text, const std::string& why) { fail(key_text + ": " + why); }
[[noreturn]] inline void fail_status(const std::string& key_text, int rc) { fail_config(key_text, "status " + std::to_string(rc) + ": " + fgoicp_last_error()); }

// One cloud on its way through the stages: which side it is, its file, that side's keys and the seeds of its calls (prepare_pair)
struct Side {
    const char* name;  // "target" / "source": the key prefix and the word in the log lines
    const std::string& file;
    const Config::Params::Cloud& keys;
    std::vector<icp::vec3>& pc;
    long long load_seed;  // < 0: std::random_device
    uint64_t plane_seed, mesh_seed;
    template <typename V> std::string key(const char* field, V value) const {  // "params.target_voxel = 0.05", the value as a log line prints it
        std::ostringstream s;
        s << "params." << name << "_" << field << " = " << value;
        return s.str();
    }
};

// One cloud of a run.  params.*_mesh_points off: cli::load_cloud, as ever.  On: the file is read as a triangle mesh (cli::load_mesh_ply) and
// the cloud is that many samples of its surface (fgoicp_mesh_sample), then thinned by *_subsample as a loaded cloud is.  A TXT file, a PLY
// without faces and a mesh without area are errors of the configuration.  The face normals are not carried through the filters:
// params.refine = "plane" / "gicp" keep estimating their own ("mesh" refines against the file's triangles themselves).
inline void load_input(const Side& s) {
    const std::string& path = s.file;
    const int mesh_points = s.keys.mesh_points;
    if (mesh_points <= 0) {
        load_cloud(path, s.keys.subsample, s.pc, s.load_seed);
        return;
    }
    const std::string key = s.key("mesh_points", mesh_points);
    if (!is_ply(path)) fail_config(key, path + " is not a PLY file: only a PLY holds a mesh");
    std::vector<icp::vec3> vertices;
    std::vector<uint32_t> triangles;
    size_t short_faces = 0;
    load_mesh_ply(path, vertices, triangles, &short_faces);
    if (triangles.empty()) fail_config(key, path + " has no faces (element face with a vertex_indices list)");
    s.pc.assign((size_t)mesh_points, icp::vec3{});
    fgoicp_mesh_info_t mi{};
    mi.struct_size = sizeof(mi);
    const int rc = fgoicp_mesh_sample(&vertices.data()->x, vertices.size(), triangles.data(), triangles.size() / 3, s.pc.size(), s.mesh_seed, 0, &s.pc.data()->x, nullptr, nullptr,
                                      nullptr, nullptr, &mi);
    if (rc != FGOICP_OK) fail_status(key, rc);
    icp::Logger log(icp::LogLevel::Info);
    log << "Mesh sampling (" << s.name << "): " << mi.vertices << " vertices, " << mi.triangles << " triangles (" << mi.zero_area << " zero-area, " << mi.unweighted
        << " unweighted), area " << mi.area << " -> " << s.pc.size() << " points";
    if (short_faces) log << "; " << short_faces << " faces of fewer than 3 vertices dropped";
    subsample_cloud(s.pc, s.keys.subsample, s.load_seed);
}

// params.*_voxel: the loaded cloud replaced by the centroids of its voxel grid (fgoicp_voxel_downsample, the origin is the cloud's own
// minimum).  A refused size (too small for the cloud's extent, not finite) is an error of the configuration.
inline void voxel_thin(const Side& s) {
    const float voxel = s.keys.voxel;
    if (!(voxel > 0.0f)) return;
    std::vector<icp::vec3> out(s.pc.size());
    fgoicp_voxel_info_t vi{};
    vi.struct_size = sizeof(vi);
    const int rc = fgoicp_voxel_downsample(&s.pc.data()->x, s.pc.size(), voxel, nullptr, 0, &out.data()->x, out.size(), nullptr, nullptr, &vi);
    if (rc != FGOICP_OK) fail_status(s.key("voxel", voxel), rc);
    out.resize((size_t)vi.voxels);
    icp::Logger(icp::LogLevel::Info) << "Voxel grid (" << s.name << "): " << s.pc.size() << " -> " << out.size() << " points, voxel " << voxel;
    s.pc.swap(out);
}

// params.*_outlier_knn: the cloud replaced by the points fgoicp_remove_outliers keeps; the indices of io.alignment are those of its rows.
// A radius > 0 selects the radius filter, otherwise the statistical one runs with the std ratio.
inline void outlier_filter(const Side& s) {
    const int knn = s.keys.outlier_knn;
    if (knn <= 0) return;
    const float std_ratio = s.keys.outlier_std, radius = s.keys.outlier_radius;
    const bool by_radius = radius > 0.0f;
    std::vector<icp::vec3> out(s.pc.size());
    fgoicp_outlier_info_t oi{};
    oi.struct_size = sizeof(oi);
    const int rc = fgoicp_remove_outliers(&s.pc.data()->x, s.pc.size(), by_radius ? FGOICP_OUTLIER_RADIUS : FGOICP_OUTLIER_STATISTICAL, knn, by_radius ? radius : std_ratio, 0,
                                          &out.data()->x, out.size(), nullptr, nullptr, nullptr, nullptr, &oi);
    if (rc != FGOICP_OK) fail_status(s.key("outlier_knn", knn), rc);
    out.resize((size_t)oi.kept);
    icp::Logger log(icp::LogLevel::Info);
    log << "Outlier filter (" << s.name << "): " << s.pc.size() << " -> " << out.size() << " points, " << knn << " neighbours, ";
    if (by_radius) log << "radius " << radius;
    else log << "std ratio " << std_ratio << ", threshold " << oi.threshold;
    s.pc.swap(out);
}

// params.*_plane_distance: the cloud without the points of its dominant planes (fgoicp_segment_planes, refitted planes, the rest kept) —
// before the clustering, which a support plane would otherwise join into one component.  A plane needs ceil(min_fraction x points)
// inliers; none of that size leaves the cloud as it is.  A filter that keeps no point is an error of the configuration too.
inline void plane_filter(const Side& s) {
    const float distance = s.keys.plane_distance;
    if (!(distance > 0.0f)) return;
    const double want = std::ceil(s.keys.plane_min_fraction * (double)s.pc.size());
    const size_t min_inliers = want > 0.0 ? (want < 9e18 ? (size_t)want : (size_t)9e18) : 0;
    std::vector<icp::vec3> out(s.pc.size());
    std::vector<fgoicp_segment_model_t> models(16);
    fgoicp_segment_info_t si{};
    si.struct_size = sizeof(si);
    const int rc = fgoicp_segment_planes(&s.pc.data()->x, s.pc.size(), distance, s.keys.plane_iterations, s.plane_seed, s.keys.plane_count, min_inliers, 1, 0, 0, &out.data()->x,
                                         out.size(), nullptr, nullptr, models.data(), models.size(), sizeof(fgoicp_segment_model_t), &si);
    if (rc != FGOICP_OK) fail_status(s.key("plane_distance", distance), rc);
    if (si.kept == 0) fail_config(s.key("plane_distance", distance), "the filter keeps no point (" + std::to_string(si.planes) + " planes hold all " + std::to_string(si.on_planes) + " points)");
    icp::Logger log(icp::LogLevel::Info);
    log << "Plane filter (" << s.name << "): " << s.pc.size() << " -> " << si.kept << " points, distance " << distance << ", " << s.keys.plane_iterations << " hypotheses: ";
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
    s.pc.swap(out);
}

// params.*_cluster_eps: the cloud replaced by the points fgoicp_cluster_dbscan keeps — its largest cluster, or with
// params.*_cluster_min_size >= 1 every cluster of at least that many points.  A filter that keeps no point is an error of the configuration too.
inline void cluster_filter(const Side& s) {
    const float eps = s.keys.cluster_eps;
    if (!(eps > 0.0f)) return;
    const int min_points = s.keys.cluster_min_points, min_size = s.keys.cluster_min_size;
    std::vector<icp::vec3> out(s.pc.size());
    std::vector<uint64_t> sizes(s.pc.size());
    fgoicp_cluster_info_t ci{};
    ci.struct_size = sizeof(ci);
    const int rc = fgoicp_cluster_dbscan(&s.pc.data()->x, s.pc.size(), eps, min_points, (size_t)min_size, 0, &out.data()->x, out.size(), nullptr, nullptr, nullptr, sizes.data(),
                                         sizes.size(), &ci);
    if (rc != FGOICP_OK) fail_status(s.key("cluster_eps", eps), rc);
    if (ci.kept == 0)
        fail_config(s.key("cluster_eps", eps), "the filter keeps no point (" + std::to_string(ci.clusters) + " clusters, " + std::to_string(ci.noise_points) + " noise points, " +
                                                   std::to_string(min_points) + " neighbours, clusters of at least " + std::to_string(min_size) + " points)");
    out.resize((size_t)ci.kept);
    size_t kept_clusters = 0;
    for (uint64_t c = 0; c < ci.clusters; ++c) kept_clusters += sizes[(size_t)c] >= (uint64_t)min_size ? 1 : 0;
    icp::Logger log(icp::LogLevel::Info);
    log << "Cluster filter (" << s.name << "): " << s.pc.size() << " -> " << out.size() << " points, eps " << eps << ", " << min_points << " neighbours: " << ci.clusters
        << " clusters, " << ci.noise_points << " noise points, ";
    if (min_size <= 0) log << "kept the largest";
    else log << "kept " << kept_clusters << " clusters of at least " << min_size << " points";
    s.pc.swap(out);
}

// params.*_points: the cloud replaced by fgoicp_farthest_point_sample's picks (start_index 0) in pick order.  A cloud that has no more
// points than asked stays as it is, order included.
inline void farthest_sample(const Side& s) {
    const int points = s.keys.points;
    if (points <= 0) return;
    if (s.pc.size() <= (size_t)points) {
        icp::Logger(icp::LogLevel::Info) << "Farthest-point sampling (" << s.name << "): " << s.pc.size() << " points, at most " << points << " asked: unchanged";
        return;
    }
    std::vector<icp::vec3> out((size_t)points);
    fgoicp_fps_info_t fi{};
    fi.struct_size = sizeof(fi);
    const int rc = fgoicp_farthest_point_sample(&s.pc.data()->x, s.pc.size(), out.size(), 0, 0, &out.data()->x, nullptr, nullptr, nullptr, nullptr, &fi);
    if (rc != FGOICP_OK) fail_status(s.key("points", points), rc);
    icp::Logger(icp::LogLevel::Info) << "Farthest-point sampling (" << s.name << "): " << s.pc.size() << " -> " << out.size() << " points, cover radius " << std::sqrt(fi.cover_dist2);
    s.pc.swap(out);
}

// The clouds of one configuration as the registration sees them.  Stage-major: both files are loaded, then every stage runs on the target
// and on the source before the next one starts — each stage sees what the one before left, and the rows of io.alignment and
// io.visualization are those of the last.  announce_loads: the "loaded from" lines of a lone run (a batch names its pairs itself).
// The seeds: with params.seed absent (< 0) the loaders draw from std::random_device, as the reference does, and the device calls — which
// take a seed always — run as with seed 0.  The source's loader and plane search take the seed after the target's, so that equal files do
// not lose the same points; the mesh sampling takes the same seed on both sides.
inline void prepare_pair(const Config& c, std::vector<icp::vec3>& target, std::vector<icp::vec3>& source, bool announce_loads) {
    const long long seed = c.params.seed;
    const uint64_t fixed = (uint64_t)std::max(seed, 0LL);
    const Side sides[2] = {{"target", c.io.target, c.params.target, target, seed, fixed, fixed}, {"source", c.io.source, c.params.source, source, seed < 0 ? -1 : seed + 1, fixed + 1, fixed}};
    for (const Side& s : sides) {
        load_input(s);
        if (announce_loads) icp::Logger(icp::LogLevel::Info) << (&s == sides ? "Target" : "Source") << " point cloud (" << s.pc.size() << ") loaded from " << s.file;
    }
    for (void (*stage)(const Side&) : {voxel_thin, outlier_filter, plane_filter, cluster_filter, farthest_sample})
        for (const Side& s : sides) stage(s);
}

}  // namespace cli
