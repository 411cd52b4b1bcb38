// fast-go-icp — the reference's CLI (src/main.cpp:8-58) over libfgoicp_amd.so:
//     fast-go-icp -c config.toml [-v]
//     fast-go-icp --batch LIST [-v]      (EXTENSION: every config of LIST as one batch on one GPU, fgoicp_batch_*)
// Same flags, same TOML keys / defaults / clamps, same log lines; the search runs on the MI355X.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <optional>
#include <string>
#include <vector>

#include "../../../include/fgoicp/fgoicp.hpp"
#include "prepare.hpp"
#include "../host/refined_pose.hpp"

static std::string usage(const std::string& exe) {
    return "Fast Go-ICP: an MI355X (HIP) implementation of Go-ICP\nUsage: " + exe + " [OPTIONS]\n\nOptions:\n"
           "  -h,--help                   Print this help message and exit\n"
           "  -c,--config TEXT REQUIRED   Path to the TOML configuration file\n"
           "  -v,--verbose                Enable verbose logging\n"
           "  -g,--gpus N                 Shard the search over N GPUs of this node (default: params.gpus, 1)\n"
           "  -b,--batch LIST             Run every config listed in LIST (one path per line, relative to LIST) as one batch on one GPU\n\nExample Usage:\n  " + exe + " -c config.toml --verbose\n  " + exe + " --config=config.toml\n";
}

// a key the parser refuses: its message, exit code 1 (thrown by cli::Config, not exit(1): the harnesses read the message)
static cli::Config read_config(const std::string& path) try {
    return cli::Config(path);
} catch (const std::invalid_argument& e) {
    cli::fail(e.what());
}

// What a search leaves — on one GPU, on several, or for a pair of a batch: the best transform (R in glm order, R.data()[col * 3 + row]), its
// error, the counters, the seconds and, in a lone run, the solver to ask for more (rank 0's on several GPUs: every rank holds the same answer).
struct Search { icp::mat3 R; icp::vec3 t; fgoicp_run_stats st{}; float best_error = 0.f; double seconds = 0.0; fgoicp_solver* solver = nullptr; };

// params.refine* as the calls take them — a batch as its pair's spec, a lone run as the arguments of fgoicp_solver_refine_plane / _gicp /
// _robust, which the spec lists.  model -1: no refinement on a solver ("" and "mesh").
static fgoicp_batch_refine_t refine_spec(const cli::Config::Params& p) {
    fgoicp_batch_refine_t r{};
    r.struct_size = sizeof(r);
    r.model = p.refine == "gicp" ? FGOICP_MODEL_GICP : p.refine == "plane" ? FGOICP_MODEL_PLANE : -1;
    if (r.model < 0) return r;
    r.k = p.refine_knn;
    r.max_iter = (size_t)p.refine_max_iter;
    r.conv_thr = 1e-6f;
    r.max_distance = p.refine_distance > 0.0f ? p.refine_distance : INFINITY;
    r.epsilon = p.refine_epsilon;
    r.loss = p.refine_loss_code();
    r.loss_scale = p.refine_loss_scale;
    return r;
}

// What params.refine leaves, whichever call made it: fgoicp_solver_refine_plane / _gicp / _robust of a lone run, a batch's own refinement
// (fgoicp_batch_refined_*) or the one-shot fgoicp_mesh_refine.  `plane` is what the [refined] table and the log line read — a robust and a
// mesh result are narrowed into it (plane_rmse then holds their residual) — `robust` what params.refine_loss adds, rms_distance what "mesh"
// adds (the rms of the deviation map at the refined pose).  The search's own result stays as it is.
struct Refinement {
    bool have = false, have_robust = false, to_mesh = false, gicp = false;
    fgoicp_plane_result_t plane{};
    fgoicp_robust_result_t robust{};
    double rms_distance = 0.0;
    explicit Refinement(const cli::Config::Params& p) : to_mesh(p.refine == "mesh"), gicp(p.refine == "gicp") { plane.struct_size = sizeof(plane); }
    const char* rmse_key() const { return to_mesh ? "mesh_rmse" : gicp ? "gicp_rmse" : "plane_rmse"; }
    // the run's final pose: the refined one when there is one, else the best transform
    const float* pose_R(const Search& s) const { return have ? plane.R : s.R.data(); }
    const float* pose_t(const Search& s) const { return have ? plane.t : &s.t.x; }
    void from_robust(const fgoicp_robust_result_t& r) {
        robust = r;
        narrow(r, r.rmse, r.scaling_factor);
        plane.sse = r.sse;
        have = have_robust = true;
    }
    void from_mesh(const fgoicp_mesh_refine_result_t& r) {  // the files' frame is the call's, so the scaling factor is 1
        narrow(r, r.mesh_rmse, 1.0f);
        robust.correspondences = r.correspondences; robust.weight_sum = r.weight_sum; robust.scaling_factor = 1.0f;
        robust.loss = r.loss; robust.scale_estimated = r.scale_estimated; robust.scale = r.loss_scale;
        rms_distance = r.rms_distance;
        have = true; have_robust = r.loss > 0;
    }
private:
    template <typename Wide> void narrow(const Wide& r, double rmse, float scaling_factor) {  // the fields fgoicp_plane_result_t shares with the wider results
        std::memcpy(plane.R, r.R, sizeof(plane.R));
        std::memcpy(plane.t, r.t, sizeof(plane.t));
        plane.iterations = r.iterations; plane.rank = r.rank; plane.correspondences = r.correspondences;
        plane.plane_rmse = rmse; plane.scaling_factor = scaling_factor;
    }
};

// the refinement's log line (a lone run's, or with a batch's "Pair i: " in front)
static void log_refinement(const std::string& prefix, const cli::Config& config, const Refinement& ref) {
    const fgoicp_plane_result_t& refined = ref.plane;
    icp::mat3 Rr;
    std::memcpy(Rr.data(), refined.R, sizeof(refined.R));
    icp::Logger log(icp::LogLevel::Info);
    log << prefix << (ref.to_mesh ? "Point-to-mesh" : ref.gicp ? "Generalized-ICP" : "Point-to-plane") << " refinement: " << refined.iterations << " iterations, rank " << refined.rank
        << ", " << refined.correspondences << " correspondences, ";
    if (ref.to_mesh) log << "rms distance " << ref.rms_distance << ", mesh RMSE ";
    else if (ref.gicp) log << "epsilon " << config.params.refine_epsilon << ", plane-to-plane RMSE ";
    else log << "plane RMSE ";
    log << refined.plane_rmse / (double)refined.scaling_factor;
    if (ref.have_robust)
        log << ", " << config.params.refine_loss << " loss, scale " << ref.robust.scale / (double)ref.robust.scaling_factor << (ref.robust.scale_estimated ? " (estimated)" : " (given)")
            << ", weight " << ref.robust.weight_sum << " of " << ref.robust.correspondences;
    log << "\n\tRotation:\n" << Rr << "\n\tTranslation: " << icp::vec3{refined.t[0], refined.t[1], refined.t[2]};
}

// io.output: the result and, with params.refine, the [refined] table behind it (cli::write_result_toml)
static void write_result(const cli::Config& c, const Search& s, size_t ns, const Refinement& ref) {
    if (c.io.output.empty()) return;
    cli::write_result_toml(c.io.output, s.R, s.t, s.best_error, ns, s.seconds, s.st, ref.have ? &ref.plane : nullptr, ref.rmse_key(), ref.have_robust ? &ref.robust : nullptr,
                           c.params.refine_loss.c_str(), ref.to_mesh ? &ref.rms_distance : nullptr);
}

// io.alignment: the report at the best transform; fill(indices, dist2, inlier, summary) asks the solver or the batch and checks its status
template <typename Fill> static void write_alignment(const cli::Config& c, const std::vector<icp::vec3>& src, Fill fill) {
    if (c.io.alignment.empty()) return;
    std::vector<uint32_t> idx(src.size());
    std::vector<float> d2(src.size());
    std::vector<uint8_t> inl(src.size());
    fgoicp_alignment_summary sm{};
    sm.struct_size = sizeof(sm);
    fill(idx.data(), d2.data(), inl.data(), &sm);
    cli::write_alignment_txt(c.io.alignment, src, idx.data(), d2.data(), inl.data(), sm);
}
// io.information: the information matrix in the files' frame, asked for in the same way
template <typename Fill> static void write_information(const cli::Config& c, Fill fill) {
    if (c.io.information.empty()) return;
    fgoicp_information_t inf{};
    inf.struct_size = sizeof(inf);
    fill(&inf);
    cli::write_information_txt(c.io.information, inf, c.params.information_distance);
}

// io.deviation: the target FILE's mesh — every vertex and face (cli::load_mesh_ply), whether or not params.target_mesh_points sampled it for the
// registration — read before anything runs, so that a TXT target and a PLY without faces end the run at once: exit code 1, the key named.
struct DeviationMesh { std::vector<icp::vec3> vertices; std::vector<uint32_t> triangles; };
// params.refine = "mesh" needs the same mesh, read by the same loader at the same moment: without io.deviation the errors name that key.
static std::string mesh_key(const cli::Config& c) { return c.io.deviation.empty() ? "params.refine = \"mesh\"" : "io.deviation = \"" + c.io.deviation + "\""; }
static void load_deviation_mesh(const cli::Config& c, DeviationMesh& m) {
    if (c.io.deviation.empty() && c.params.refine != "mesh") return;
    if (!cli::is_ply(c.io.target)) cli::fail_config(mesh_key(c), "the target " + c.io.target + " is not a PLY file: only a PLY holds a mesh");
    cli::load_mesh_ply(c.io.target, m.vertices, m.triangles);
    if (m.triangles.empty()) cli::fail_config(mesh_key(c), "the target " + c.io.target + " has no faces (element face with a vertex_indices list)");
}
// ... and after the run: the source points the registration saw (the rows of io.alignment), moved by the final pose (Refinement::pose_R /
// pose_t; R9 in glm order) — as write_visualization_ply moves them, formed in fp64 per axis, (R[a][0] x + R[a][1] y) + R[a][2] z + t[a],
// and rounded to fp32 once; fgoicp_mesh_distance on device 0, once, on the host thread.  A mesh without area is refused by the call:
// exit code 1, the key named.
static void write_deviation(const cli::Config& c, const DeviationMesh& m, const std::vector<icp::vec3>& src, const Search& s, const Refinement& ref, const std::string& prefix) {
    if (c.io.deviation.empty()) return;
    const float *R9 = ref.pose_R(s), *t3 = ref.pose_t(s);
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
    if (rc != FGOICP_OK) cli::fail_status("io.deviation = \"" + c.io.deviation + "\"", rc);
    const cli::DeviationSummary ds = cli::summarize_deviation(mi, dist2.data(), side.data());
    cli::write_deviation_txt(c.io.deviation, src, face.data(), dist2.data(), side.data(), region.data(), ds);
    icp::Logger(icp::LogLevel::Info) << prefix << "Deviation (source -> target mesh): " << ds.points << " points, " << ds.triangles << " triangles (" << ds.zero_area
                                     << " zero-area), rms " << ds.rms << ", max " << ds.max;
}

// params.refine = "mesh": the pose near the best transform — in the files' frame, which is the mesh's — that minimises the distances from
// the source points the registration saw to the target FILE's triangles (fgoicp_mesh_refine on device 0; params.refine_max_iter,
// refine_distance, refine_loss and refine_loss_scale apply, refine_knn and refine_epsilon do not).  A refusal — a mesh without area among
// them — ends the run: exit code 1, the key named.
static void refine_to_mesh(const cli::Config& c, const DeviationMesh& m, const std::vector<icp::vec3>& src, const Search& s, Refinement& ref) {
    fgoicp_mesh_refine_result_t r{};
    r.struct_size = sizeof(r);
    const int rc = fgoicp_mesh_refine(&m.vertices.data()->x, m.vertices.size(), m.triangles.data(), m.triangles.size() / 3, &src.data()->x, src.size(), s.R.data(), &s.t.x,
                                      (size_t)c.params.refine_max_iter, 1e-6f, c.params.refine_distance, c.params.refine_loss_code(), c.params.refine_loss_scale, 0u, 0, &r);
    if (rc != FGOICP_OK) cli::fail_status("params.refine = \"mesh\"", rc);
    ref.from_mesh(r);
}

// params.refine, from the best transform, after the search: "mesh" as above; "plane" / "gicp" as `spec` (refine_spec) says, from whoever ran
// the search — robust(result) under params.refine_loss, else plane(result), each checking its status; then the refinement's log line.
template <typename Robust, typename Plane>
static Refinement refine(const cli::Config& c, const DeviationMesh& m, const std::vector<icp::vec3>& src, const Search& s, const std::string& prefix, const fgoicp_batch_refine_t& spec,
                         Robust robust, Plane plane) {
    Refinement ref(c.params);
    if (ref.to_mesh) {
        refine_to_mesh(c, m, src, s, ref);
    } else if (spec.model >= 0 && spec.loss > 0) {
        fgoicp_robust_result_t r{};
        r.struct_size = sizeof(r);
        robust(&r);
        ref.from_robust(r);
    } else if (spec.model >= 0) {
        plane(&ref.plane);
        ref.have = true;
    }
    if (ref.have) log_refinement(prefix, c, ref);
    return ref;
}

// --batch LIST: every config of the list registered in one fgoicp_batch run; each config's io.output / io.visualization as a lone -c run
// of it writes them (the seconds written are the batch's).  The configs must agree on the schedule and round width; each is trimmed with
// its own params.trim_fraction and refined with its own params.refine* (fgoicp_batch_opts_refine.refine): the refinement's log line, the
// [refined] table and io.information at the refined pose as a lone run of it.
static int run_batch(const std::string& list_file) {
    std::ifstream lf(list_file);
    if (!lf) cli::fail("Unable to read " + list_file);
    const std::filesystem::path dir = std::filesystem::path(list_file).parent_path();
    std::vector<cli::Config> configs;
    for (std::string line; std::getline(lf, line);) {
        line = cli::trim(line);
        if (line.empty() || line[0] == '#') continue;
        const std::filesystem::path p(line);
        configs.push_back(read_config((p.is_absolute() ? p : dir / p).string()));
    }
    if (configs.empty()) cli::fail("--batch: " + list_file + " lists no config");
    const cli::Config& c0 = configs[0];
    for (const cli::Config& c : configs) {
        if (c.params.gpus > 1) cli::fail("--batch: a batch runs on one GPU (params.gpus > 1)");
        if (c.params.schedule != c0.params.schedule || c.params.round_width != c0.params.round_width)
            cli::fail("--batch: every config of a batch must have the same params.schedule and params.round_width");
    }
    const size_t n = configs.size();
    std::vector<std::vector<icp::vec3>> pct(n), pcs(n);
    std::vector<DeviationMesh> meshes(n);
    for (size_t i = 0; i < n; ++i) load_deviation_mesh(configs[i], meshes[i]);
    std::vector<fgoicp_batch_pair> pairs(n);
    std::vector<float> trim(n);
    for (size_t i = 0; i < n; ++i) {
        const cli::Config& c = configs[i];
        cli::prepare_pair(c, pct[i], pcs[i], false);
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
        if (o.information && c.params.information_distance != o.information_max_distance)
            cli::fail("--batch: every config of a batch that names io.information must have the same params.information_distance");
        o.information = 1;
        o.information_max_distance = c.params.information_distance;
    }
    std::vector<fgoicp_batch_refine_t> specs(n);
    for (size_t i = 0; i < n; ++i) {
        specs[i] = refine_spec(configs[i].params);
        if (specs[i].model >= 0) with_refine.refine = specs.data();
    }
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
        const int pair = (int)i;
        const std::string prefix = "Pair " + std::to_string(i) + ": ";
        Search s;
        std::memcpy(s.R.data(), &R9[9 * i], 9 * sizeof(float));
        s.t = icp::vec3{t3[3 * i], t3[3 * i + 1], t3[3 * i + 2]};
        s.seconds = elapsed.count();
        icp::check_status(fgoicp_batch_best_error(b, pair, &s.best_error), "fgoicp_batch_best_error");
        icp::check_status(fgoicp_batch_stats(b, pair, &s.st), "fgoicp_batch_stats");
        icp::Logger(icp::LogLevel::Info) << prefix << "Best Error: " << s.best_error << "\n\tRotation:\n" << s.R << "\n\tTranslation: " << s.t;
        const cli::Config& c = configs[i];
        // params.refine = "mesh": not one of the batch's own refinements (its specs stay plane / gicp) — the one-shot call, here, as
        // write_deviation below; io.information of such a config stays at the best transform (a batch keeps no context to ask at another pose)
        const bool in_batch = specs[i].model >= 0;
        const Refinement ref = refine(c, meshes[i], pcs[i], s, prefix, specs[i],
                                      [&](fgoicp_robust_result_t* r) { icp::check_status(fgoicp_batch_refined_robust(b, pair, r), "fgoicp_batch_refined_robust"); },
                                      [&](fgoicp_plane_result_t* r) { icp::check_status(fgoicp_batch_refined_plane(b, pair, r), "fgoicp_batch_refined_plane"); });
        write_result(c, s, pcs[i].size(), ref);
        if (!c.io.visualization.empty()) cli::write_visualization_ply(c.io.visualization, pct[i], pcs[i], s.R, s.t);
        write_alignment(c, pcs[i], [&](uint32_t* idx, float* d2, uint8_t* inl, fgoicp_alignment_summary* sm) {
            icp::check_status(fgoicp_batch_alignment(b, pair, idx, d2, inl, nullptr, sm), "fgoicp_batch_alignment");
        });
        write_information(c, [&](fgoicp_information_t* inf) {
            if (in_batch) icp::check_status(fgoicp_batch_refined_information(b, pair, inf), "fgoicp_batch_refined_information");  // as a lone run: at the refined pose
            else icp::check_status(fgoicp_batch_information(b, pair, inf), "fgoicp_batch_information");
        });
        write_deviation(c, meshes[i], pcs[i], s, ref, prefix);
    }
    fgoicp_batch_destroy(b);
    return rc;
}

// The search of a lone run on one GPU: icp::FastGoICP, which logs "Searching over!" itself; `owner` keeps the solver for the caller
static Search search_one_gpu(const cli::Config& config, int schedule, const std::vector<icp::vec3>& pct, const std::vector<icp::vec3>& pcs, std::optional<icp::FastGoICP>& owner) {
    owner.emplace(pct, pcs, config.params.lut_resolution, config.params.mse_threshold, schedule, config.params.round_width, 0, config.params.trim_fraction);
    Search s;
    const auto start = std::chrono::high_resolution_clock::now();
    std::tie(s.R, s.t) = owner->run();
    s.seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count();
    s.st = owner->stats();
    s.best_error = owner->get_best_error();
    s.solver = owner->handle();
    return s;
}

// EXTENSION: ... on several: one host thread + one solver per GPU (include/fgoicp_amd.h, fgoicp_multi_*).  params.schedule = "serial" (the
// default) keeps the reference's exact trajectory and deals the inner BnBs of every speculative evaluation over the GPUs; "round" deals the
// children of every expansion round (one RCCL all-gather per round; fastest).  The caller destroys `owner`, then logs "Searching over!".
static Search search_multi_gpu(const cli::Config& config, int schedule, int gpus, const std::vector<icp::vec3>& pct, const std::vector<icp::vec3>& pcs, fgoicp_multi*& owner) {
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
    icp::check_status(fgoicp_multi_create(&pct.data()->x, pct.size(), &pcs.data()->x, pcs.size(), config.params.lut_resolution, config.params.mse_threshold, &o, devices.data(),
                                          (int)devices.size(), transport, &owner), "fgoicp_multi_create");
    Search s;
    s.solver = fgoicp_multi_solver(owner, 0);
    // rank 0's log events: every rank holds the same incumbents (SERIAL and the cooperative flow: the same refinements too)
    icp::check_status(fgoicp_solver_set_log(s.solver, &icp::FastGoICP::log_line, nullptr), "fgoicp_solver_set_log");
    const auto start = std::chrono::high_resolution_clock::now();
    icp::check_status(fgoicp_multi_run(owner, s.R.data(), &s.t.x), "fgoicp_multi_run");
    s.seconds = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - start).count();
    // ROUND: counters summed over the ranks; SERIAL: every rank holds the whole trajectory's counters (rank 0's are reported).
    // Rank 0's incumbent is every rank's.
    for (int r = 0; r < (schedule == FGOICP_SCHEDULE_ROUND ? (int)devices.size() : 1); ++r) {
        fgoicp_run_stats s1{};
        icp::check_status(fgoicp_solver_stats(fgoicp_multi_solver(owner, r), &s1), "fgoicp_solver_stats");
        s.st.trans_cubes += s1.trans_cubes; s.st.rot_cubes += s1.rot_cubes; s.st.icp_runs += s1.icp_runs; s.st.icp_iters += s1.icp_iters;
        s.st.bounds_calls += s1.bounds_calls; s.st.inner_bnb += s1.inner_bnb;
        if (r == 0) { s.st.rounds = s1.rounds; s.st.initial_icp_sse = s1.initial_icp_sse; }
    }
    icp::check_status(fgoicp_solver_best_error(s.solver, &s.best_error), "fgoicp_solver_best_error");
    return s;
}

// -c CONFIG: one registration, on one GPU or sharded over several; what follows the search is the same for both.
static int run_single(const cli::Config& config, int gpus_flag) {
    DeviationMesh deviation_mesh;
    load_deviation_mesh(config, deviation_mesh);
    std::vector<icp::vec3> pct, pcs;
    cli::prepare_pair(config, pct, pcs, true);
    for (const auto* pc : {&pct, &pcs}) {  // verbose: the statistics the pre-processing normalises by (TODO.md:7 of the reference)
        fgoicp_cloud_stats_t cs{};
        if (fgoicp_cloud_stats(&pc->data()->x, pc->size(), &cs) == FGOICP_OK)
            icp::Logger(icp::LogLevel::Debug) << (pc == &pct ? "Target" : "Source") << " statistics: centroid " << icp::vec3{cs.centroid[0], cs.centroid[1], cs.centroid[2]}
                                              << ", box [" << cs.min[0] << ", " << cs.max[0] << "] x [" << cs.min[1] << ", " << cs.max[1] << "] x [" << cs.min[2] << ", " << cs.max[2]
                                              << "], largest centred coordinate " << cs.max_abs_centred << ", RMS radius " << cs.rms_radius;
    }
    const int schedule = config.params.schedule == "round" ? FGOICP_SCHEDULE_ROUND : FGOICP_SCHEDULE_SERIAL;
    const int gpus = gpus_flag > 0 ? gpus_flag : config.params.gpus;
    std::optional<icp::FastGoICP> one;
    fgoicp_multi* multi = nullptr;
    const Search s = gpus > 1 ? search_multi_gpu(config, schedule, gpus, pct, pcs, multi) : search_one_gpu(config, schedule, pct, pcs, one);
    write_alignment(config, pcs, [&](uint32_t* idx, float* d2, uint8_t* inl, fgoicp_alignment_summary* sm) {
        icp::check_status(fgoicp_solver_alignment(s.solver, idx, d2, inl, nullptr, sm), "fgoicp_solver_alignment");
    });
    const fgoicp_batch_refine_t q = refine_spec(config.params);  // "plane" / "gicp": on the solver that ran
    const Refinement ref = refine(config, deviation_mesh, pcs, s, "", q,
        [&](fgoicp_robust_result_t* r) { icp::check_status(fgoicp_solver_refine_robust(s.solver, q.model, q.k, q.max_iter, q.conv_thr, q.max_distance, q.epsilon, q.loss, q.loss_scale, r), "fgoicp_solver_refine_robust"); },
        [&](fgoicp_plane_result_t* r) {
            if (q.model == FGOICP_MODEL_GICP) icp::check_status(fgoicp_solver_refine_gicp(s.solver, q.k, q.max_iter, q.conv_thr, q.max_distance, q.epsilon, r), "fgoicp_solver_refine_gicp");
            else icp::check_status(fgoicp_solver_refine_plane(s.solver, q.k, q.max_iter, q.conv_thr, q.max_distance, r), "fgoicp_solver_refine_plane");
        });
    // io.information at the best transform, or at the refined pose when there is one: then from the context at that pose in the solver's
    // frame (the restored translation taken back, t_s = (t - R offset_pcs + offset_pct) * scale) and converted as fgoicp_solver_information
    // converts (fgoicp_information_from_moments): refined_pose.hpp, the text a batch runs too
    write_information(config, [&](fgoicp_information_t* inf) {
        const float d = config.params.information_distance;
        if (!ref.have) {
            icp::check_status(fgoicp_solver_information(s.solver, d > 0.0f ? d : INFINITY, inf), "fgoicp_solver_information");
        } else {
            float offs[6], scale = 1.0f;
            icp::check_status(fgoicp_solver_preproc(s.solver, offs, &scale, nullptr), "fgoicp_solver_preproc");
            icp::check_status(fgoicp::refined_information(fgoicp_solver_ctx(s.solver), ref.plane.R, ref.plane.t, offs, scale, d, inf), "fgoicp_information at the refined pose");
        }
    });
    if (multi) {
        fgoicp_multi_destroy(multi);
        icp::Logger(icp::LogLevel::Info) << "Searching over! Best Error: " << s.best_error << "\n\tRotation:\n" << s.R << "\n\tTranslation: " << s.t;  // fgoicp.cpp:25-27
    }
    icp::Logger(icp::LogLevel::Debug) << "Subcubes: " << s.st.trans_cubes << ", rotation cubes: " << s.st.rot_cubes << ", ICP runs: " << s.st.icp_runs;
    icp::Logger(icp::LogLevel::Info) << "Fast Go-ICP finished, time elapsed: " << std::fixed << std::setprecision(3) << s.seconds << " seconds";
    write_result(config, s, pcs.size(), ref);
    if (!config.io.visualization.empty()) cli::write_visualization_ply(config.io.visualization, pct, pcs, s.R, s.t);
    write_deviation(config, deviation_mesh, pcs, s, ref, "");
    return 0;
}

struct Args { std::string config_file, batch_file; bool verbose = false; int gpus_flag = 0; };
static Args parse_args(int argc, char* argv[]) {
    Args args;
    const std::string exe = std::filesystem::path(argv[0]).filename().string();
    auto fail = [&](const std::string& what, int code) {
        icp::Logger(icp::LogLevel::Error) << what;
        icp::Logger(icp::LogLevel::Info) << usage(exe);
        std::exit(code);
    };
    auto value = [&](int& i, const char* missing) {  // the word after a flag
        if (i + 1 >= argc) fail(missing, 114);
        return std::string(argv[++i]);
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") { std::cout << usage(exe); std::exit(0); }
        else if (a == "-v" || a == "--verbose") args.verbose = true;
        else if (a == "-g" || a == "--gpus") args.gpus_flag = std::atoi(value(i, "--gpus: 1 required INT missing").c_str());
        else if (a.rfind("--gpus=", 0) == 0) args.gpus_flag = std::atoi(a.substr(7).c_str());
        else if (a == "-b" || a == "--batch") args.batch_file = value(i, "--batch: 1 required TEXT missing");
        else if (a.rfind("--batch=", 0) == 0) args.batch_file = a.substr(8);
        else if (a == "-c" || a == "--config") args.config_file = value(i, "--config: 1 required TEXT missing");
        else if (a.rfind("--config=", 0) == 0) args.config_file = a.substr(9);
        else if (a.rfind("-c", 0) == 0 && a.size() > 2) args.config_file = a.substr(2);
        else fail("The following argument was not expected: " + a, 109);
    }
    if (!args.batch_file.empty()) {
        if (!args.config_file.empty()) fail("--batch excludes --config", 109);
        if (args.gpus_flag > 1) fail("--batch runs on one GPU: --gpus > 1 is not allowed with it", 109);
    } else if (args.config_file.empty()) {
        fail("--config is required", 106);
    }
    return args;
}

int main(int argc, char* argv[]) {
    const Args args = parse_args(argc, argv);
    icp::Logger::set_verbose(args.verbose);
    if (!args.batch_file.empty()) return run_batch(args.batch_file);
    return run_single(read_config(args.config_file), args.gpus_flag);
}
