// CLI-side configuration and cloud loaders — the caller side of the drop-in (reference
// src/utilities.hpp:18-260, test/bunny.toml).  Own minimal parsers: a TOML subset (tables, string /
// bool / integer / float values, comments) and PLY (ascii, binary little/big endian; any scalar
// property types; list properties and foreign elements are skipped, but for the faces' vertex list when
// a mesh is asked for: load_mesh_ply) — the reference vendors toml++,
// CLI11 and tinyply for these, none of which are copied here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/fgoicp/common.hpp"

namespace cli {

// ------------------------------------------------------------------------------------------
// TOML subset
// ------------------------------------------------------------------------------------------
struct TomlValue {
    enum Kind { String, Bool, Number } kind = String;
    std::string s;
    bool b = false;
    double d = 0;
};
using TomlTable = std::map<std::string, std::map<std::string, TomlValue>>;  // [section][key]

inline std::string trim(const std::string& x) {
    size_t a = x.find_first_not_of(" \t\r\n"), b = x.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? "" : x.substr(a, b - a + 1);
}

inline TomlTable parse_toml(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("Error parsing file '" + path + "': could not open file");
    TomlTable t;
    std::string line, section;
    int lineno = 0;
    while (std::getline(f, line)) {
        ++lineno;
        // strip comments outside strings
        bool in_str = false;
        char q = 0;
        std::string clean;
        for (size_t i = 0; i < line.size(); ++i) {
            char ch = line[i];
            if (in_str) {
                clean += ch;
                if (ch == '\\' && q == '"' && i + 1 < line.size()) { clean += line[++i]; continue; }
                if (ch == q) in_str = false;
            } else if (ch == '"' || ch == '\'') { in_str = true; q = ch; clean += ch; }
            else if (ch == '#') break;
            else clean += ch;
        }
        clean = trim(clean);
        if (clean.empty()) continue;
        auto err = [&](const std::string& what) { return std::runtime_error("Error parsing file '" + path + "': line " + std::to_string(lineno) + ": " + what); };
        if (clean.front() == '[') {
            if (clean.back() != ']') throw err("unterminated table header");
            section = trim(clean.substr(1, clean.size() - 2));
            t[section];
            continue;
        }
        size_t eq = clean.find('=');
        if (eq == std::string::npos) throw err("expected key = value");
        std::string key = trim(clean.substr(0, eq)), val = trim(clean.substr(eq + 1));
        if (key.empty() || val.empty()) throw err("expected key = value");
        TomlValue v;
        if (val.front() == '"' || val.front() == '\'') {
            if (val.size() < 2 || val.back() != val.front()) throw err("unterminated string");
            v.kind = TomlValue::String;
            std::string raw = val.substr(1, val.size() - 2), out;
            if (val.front() == '"')
                for (size_t i = 0; i < raw.size(); ++i) {
                    if (raw[i] == '\\' && i + 1 < raw.size()) {
                        char n = raw[++i];
                        out += n == 'n' ? '\n' : n == 't' ? '\t' : n;
                    } else out += raw[i];
                }
            else out = raw;
            v.s = out;
        } else if (val == "true" || val == "false") {
            v.kind = TomlValue::Bool;
            v.b = val == "true";
        } else {
            std::string num;
            for (char ch : val) if (ch != '_') num += ch;
            if (num == "inf" || num == "+inf") v.d = std::numeric_limits<double>::infinity();
            else if (num == "-inf") v.d = -std::numeric_limits<double>::infinity();
            else {
                char* end = nullptr;
                v.d = std::strtod(num.c_str(), &end);
                if (end == num.c_str() || *end != '\0') throw err("unsupported value '" + val + "'");
            }
            v.kind = TomlValue::Number;
        }
        t[section][key] = v;
    }
    return t;
}

// ------------------------------------------------------------------------------------------
// Config — src/utilities.hpp:18-107 (same keys, defaults and clamps; `seed` is an addition)
// ------------------------------------------------------------------------------------------
struct Config {
    struct IO { std::string target, source, output, visualization, alignment, information, deviation; } io;  // alignment, information, deviation: EXTENSION, optional (write_alignment_txt, write_information_txt, write_deviation_txt)
    struct Params {
        bool trim = false;
        float lut_resolution = 0.005f, mse_threshold = 1e-3f;
        long long seed = -1;       // < 0: std::random_device, as the reference (utilities.hpp:149-150)
        std::string schedule = "serial";
        int round_width = 1;
        float trim_fraction = 0.0f;  // EXTENSION: > 0 enables trimmed Go-ICP; `trim` itself stays parsed-and-ignored as upstream
        int gpus = 1;                // EXTENSION: > 1 shards the outer BnB over that many GPUs of this node (one host thread each, RCCL)
        float information_distance = 0.0f;  // EXTENSION: distance threshold of io.information in the files' units (absent or 0: none)
        std::string refine;          // EXTENSION: "plane" = point-to-plane refinement after the search (fgoicp_solver_refine_plane), "gicp" = Generalized ICP (fgoicp_solver_refine_gicp), "mesh" = point-to-mesh refinement against the target FILE's triangles (fgoicp_mesh_refine; refine_knn and refine_epsilon are ignored); absent or "": none; anything else is refused
        int refine_knn = 16;         // ... neighbours per target point for its normal (4 .. 32)
        int refine_max_iter = 30;
        float refine_distance = 0.0f;  // ... distance threshold in the files' units (absent or 0: none)
        double refine_epsilon = 1e-3;  // ... "gicp" only: the smallest eigenvalue of the regularised covariances, in (0, 1]
        std::string refine_loss = "none";  // EXTENSION: the robust loss of the refinement (fgoicp_solver_refine_robust): "none", "huber", "cauchy", "geman_mcclure", "tukey"; anything else, or a loss without params.refine, is refused
        double refine_loss_scale = 0.0;    // ... its scale in the files' units; absent or <= 0: estimated at the best transform
        int refine_loss_code() const {     // FGOICP_LOSS_*
            static const char* const names[] = {"none", "huber", "cauchy", "geman_mcclure", "tukey"};
            for (int k = 0; k < 5; ++k)
                if (refine_loss == names[k]) return k;
            return -1;
        }
        // The keys a cloud has of its own: params.target_<field> and params.source_<field>, read by the same rules (cloud_keys in the
        // constructor) and applied in the stage order of csrc/cli/prepare.hpp.
        struct Cloud {
            float subsample = 1.0f;  // utilities.hpp:101-104: clamped to [1e-5, 1], the source's to [1e-5, 0.5]
            // EXTENSION: mesh input (fgoicp_mesh_sample).  *_mesh_points: the cloud becomes that many samples of the SURFACE of the file's triangle
            // mesh (a PLY with faces) in place of its vertices, before everything that sees the loaded cloud, *_subsample included; absent or <= 0:
            // off.  A value that is not an integer is refused.
            int mesh_points = 0;
            float voxel = 0.0f;  // EXTENSION: voxel size in the files' units; the cloud is replaced by its voxel grid's centroids (fgoicp_voxel_downsample) after loading; absent or <= 0: off, NaN is refused
            // EXTENSION: outlier removal per cloud after the voxel grid (fgoicp_remove_outliers).  *_outlier_knn: the neighbours, absent or <= 0: off;
            // *_outlier_std: the statistical filter's std ratio; *_outlier_radius (the files' units) > 0: the radius filter in place of the statistical one.
            // A value that is not a number is refused.
            int outlier_knn = 0;
            float outlier_std = 2.0f, outlier_radius = 0.0f;
            // EXTENSION: the dominant planes of a cloud removed after the outlier filter and before the clustering (fgoicp_segment_planes: the table
            // under the object, the floor of the room).  *_plane_distance: the inlier distance in the files' units, absent or <= 0: off;
            // *_plane_iterations: the hypotheses per plane; *_plane_count: the planes at most; *_plane_min_fraction: a plane needs at least
            // ceil(fraction x points) inliers.  A value that is not a number is refused.
            float plane_distance = 0.0f;
            int plane_iterations = 1000, plane_count = 1;
            double plane_min_fraction = 0.1;
            // EXTENSION: density clustering per cloud after the outlier filter and before the sampling (fgoicp_cluster_dbscan).  *_cluster_eps: the
            // radius in the files' units, absent or <= 0: off; *_cluster_min_points: the neighbours (the point included) that make a point core;
            // *_cluster_min_size: 0 keeps the largest cluster, >= 1 every cluster of at least that many points.  A value that is not a number is refused.
            float cluster_eps = 0.0f;
            int cluster_min_points = 10, cluster_min_size = 0;
            // EXTENSION: farthest-point sampling per cloud after the outlier filter (fgoicp_farthest_point_sample, start_index 0): the number of points the
            // cloud is brought down to; absent or <= 0: off; a cloud that has no more points stays as it is.  A value that is not an integer is refused.
            int points = 0;
        } target, source;
    } params;

    explicit Config(const std::string& toml_filepath) {
        std::string base = toml_filepath.substr(toml_filepath.find_last_of("/\\") + 1);
        icp::Logger(icp::LogLevel::Info) << "Reading configurations from " << base;
        TomlTable tbl;
        try {
            tbl = parse_toml(toml_filepath);
        } catch (const std::exception& e) {
            icp::Logger(icp::LogLevel::Error) << e.what() << "\n";
            std::exit(1);  // utilities.hpp:69-78
        }
        auto str = [&](const char* sec, const char* key, const std::string& def) {
            auto s = tbl.find(sec);
            if (s == tbl.end()) return def;
            auto k = s->second.find(key);
            return (k == s->second.end() || k->second.kind != TomlValue::String) ? def : k->second.s;
        };
        auto num = [&](const char* sec, const char* key, double def) {
            auto s = tbl.find(sec);
            if (s == tbl.end()) return def;
            auto k = s->second.find(key);
            return (k == s->second.end() || k->second.kind != TomlValue::Number) ? def : k->second.d;
        };
        auto boolean = [&](const char* sec, const char* key, bool def) {
            auto s = tbl.find(sec);
            if (s == tbl.end()) return def;
            auto k = s->second.find(key);
            return (k == s->second.end() || k->second.kind != TomlValue::Bool) ? def : k->second.b;
        };
        io.target = str("io", "target", "");
        io.source = str("io", "source", "");
        io.output = str("io", "output", "");                // declared in test/bunny.toml:10, unparsed upstream
        io.visualization = str("io", "visualization", "");  // declared in test/bunny.toml:11, unparsed upstream
        io.alignment = str("io", "alignment", "");          // EXTENSION: where the alignment report goes ("" = none; not part of the printed summary)
        io.information = str("io", "information", "");      // EXTENSION: where the information matrix goes ("" = none; not part of the printed summary)
        io.deviation = str("io", "deviation", "");          // EXTENSION: where the deviation map against the target's mesh goes ("" = none; not part of the printed summary)
        auto clampf0 = [](float x) { return x < 0.0f ? 0.0f : (x > 0.9f ? 0.9f : x); };
        if (tbl.count("params")) {
            params.trim = boolean("params", "trim", false);
            params.lut_resolution = (float)num("params", "lut_resolution", 0.005);
            params.mse_threshold = (float)num("params", "mse_threshold", 1e-3);
            params.seed = (long long)num("params", "seed", -1);
            params.schedule = str("params", "schedule", "serial");
            params.round_width = (int)num("params", "round_width", 1);
            params.trim_fraction = clampf0((float)num("params", "trim_fraction", 0.0));
            params.gpus = std::max(1, (int)num("params", "gpus", 1));
            params.information_distance = (float)num("params", "information_distance", 0.0);
            if (!(params.information_distance > 0.0f)) params.information_distance = 0.0f;
            params.refine = str("params", "refine", "");
            params.refine_knn = (int)num("params", "refine_knn", 16);
            params.refine_max_iter = std::max(0, (int)num("params", "refine_max_iter", 30));
            params.refine_distance = (float)num("params", "refine_distance", 0.0);
            if (!(params.refine_distance > 0.0f)) params.refine_distance = 0.0f;
            params.refine_epsilon = num("params", "refine_epsilon", 1e-3);
            if (!params.refine.empty() && params.refine != "plane" && params.refine != "gicp" && params.refine != "mesh")  // (thrown, not exit(1): the callers report it; a typo must not silently skip the refinement)
                throw std::invalid_argument("params.refine = \"" + params.refine + "\" is not supported: the refinements are \"plane\", \"gicp\" and \"mesh\"");
            if (!params.refine.empty() && params.refine != "mesh" && (params.refine_knn < 4 || params.refine_knn > 32)) throw std::invalid_argument("params.refine_knn must lie in [4, 32]");
            if (params.refine == "gicp" && !(params.refine_epsilon > 0.0 && params.refine_epsilon <= 1.0)) throw std::invalid_argument("params.refine_epsilon must lie in (0, 1]");
            params.refine_loss = str("params", "refine_loss", "none");
            params.refine_loss_scale = num("params", "refine_loss_scale", 0.0);
            if (!(params.refine_loss_scale > 0.0) || !std::isfinite(params.refine_loss_scale)) params.refine_loss_scale = 0.0;
            if (params.refine_loss_code() < 0)
                throw std::invalid_argument("params.refine_loss = \"" + params.refine_loss + "\" is not supported: the losses are \"none\", \"huber\", \"cauchy\", \"geman_mcclure\" and \"tukey\"");
            if (params.refine_loss_code() > 0 && params.refine.empty()) throw std::invalid_argument("params.refine_loss needs params.refine (\"plane\", \"gicp\" or \"mesh\")");
            auto strict = [&](const std::string& key, double def) {  // as num, but a key that is present and not a number is an error of the configuration
                auto k = tbl["params"].find(key);
                if (k != tbl["params"].end() && k->second.kind != TomlValue::Number) throw std::invalid_argument("params." + key + " must be a number");
                const double v = num("params", key.c_str(), def);
                if (std::isnan(v)) throw std::invalid_argument("params." + key + " must not be NaN");
                return v;
            };
            auto knn = [](double v) { return v >= 1.0 ? (v > 1e6 ? 1000000 : (int)v) : 0; };
            auto count = [&](const std::string& key) {  // as strict, and the number must be an integer; <= 0: off
                const double v = strict(key, 0.0);
                if (v != std::floor(v)) throw std::invalid_argument("params." + key + " must be an integer");
                return v >= 1.0 ? (v > 2147483647.0 ? 2147483647 : (int)v) : 0;
            };
            auto whole = [&](const std::string& key, double def) {  // as strict, and the number must be an integer; the call judges its range
                const double v = strict(key, def);
                if (v != std::floor(v)) throw std::invalid_argument("params." + key + " must be an integer");
                return v > 2147483647.0 ? 2147483647 : (v < -2147483647.0 ? -2147483647 : (int)v);
            };
            auto cloud_keys = [&](const std::string& side, Params::Cloud& c) {  // side: "target_" / "source_"
                c.subsample = (float)num("params", (side + "subsample").c_str(), 1.0);
                c.voxel = (float)num("params", (side + "voxel").c_str(), 0.0);
                c.outlier_knn = knn(strict(side + "outlier_knn", 0.0));
                c.outlier_std = (float)strict(side + "outlier_std", 2.0);
                c.outlier_radius = (float)strict(side + "outlier_radius", 0.0);
                c.points = count(side + "points");
                c.mesh_points = count(side + "mesh_points");
                c.cluster_eps = (float)strict(side + "cluster_eps", 0.0);
                c.cluster_min_points = whole(side + "cluster_min_points", 10.0);
                c.cluster_min_size = count(side + "cluster_min_size");
                c.plane_distance = (float)strict(side + "plane_distance", 0.0);
                c.plane_iterations = whole(side + "plane_iterations", 1000.0);
                c.plane_count = whole(side + "plane_count", 1.0);
                c.plane_min_fraction = strict(side + "plane_min_fraction", 0.1);
            };
            cloud_keys("target_", params.target);
            cloud_keys("source_", params.source);
            if (std::isnan(params.target.voxel) || std::isnan(params.source.voxel)) throw std::invalid_argument("params.target_voxel and params.source_voxel must not be NaN");
            auto clampf = [](float x, float lo, float hi) { return x < hi ? (x > lo ? x : lo) : hi; };
            params.target.subsample = clampf(params.target.subsample, 1e-5f, 1.0f);  // utilities.hpp:101-104
            params.source.subsample = clampf(params.source.subsample, 1e-5f, 1.0f);
            params.source.subsample = clampf(params.source.subsample, 1e-5f, 0.5f);
            params.mse_threshold = clampf(params.mse_threshold, 1e-12f, INFINITY);
        }
        icp::Logger(icp::LogLevel::Info) << *this;
    }

    friend std::ostream& operator<<(std::ostream& os, const Config& c) {  // utilities.hpp:45-58
        os << "Fast Go-ICP Configurations\n"
           << "\tIO Configuration:\n"
           << "\t\tTarget: " << c.io.target << "\n"
           << "\t\tSource: " << c.io.source << "\n"
           << "\tParameters:\n"
           << "\t\tTrim: " << (c.params.trim ? "true" : "false") << "\n"
           << "\t\tTarget Subsample: " << c.params.target.subsample << "\n"
           << "\t\tSource Subsample: " << c.params.source.subsample << "\n"
           << "\t\tLUT Resolution: " << c.params.lut_resolution << "\n"
           << "\t\tMSE Threshold: " << c.params.mse_threshold;
        return os;
    }
};

// ------------------------------------------------------------------------------------------
// Loaders — src/utilities.hpp:113-260
// ------------------------------------------------------------------------------------------
struct Subsampler {  // keep each point with probability `subsample` until floor(total*subsample) are kept
    std::mt19937 gen;
    std::uniform_real_distribution<float> dis{0.0f, 1.0f};
    float subsample;
    size_t budget, kept = 0;
    Subsampler(size_t total, float s, long long seed) : subsample(s), budget(static_cast<size_t>(total * s)) {
        if (seed < 0) { std::random_device rd; gen.seed(rd()); } else gen.seed((uint32_t)seed);
    }
    bool keep() { return dis(gen) <= subsample; }
};

inline size_t load_cloud_txt(const std::string& path, float subsample, std::vector<icp::vec3>& cloud, long long seed) {
    std::ifstream f(path);
    if (!f.is_open()) throw std::runtime_error("Error reading TXT file: Unable to open TXT file: " + path);
    int total = 0;
    f >> total;
    if (total <= 0) throw std::runtime_error("Error reading TXT file: Invalid number of points in the TXT file: " + path);
    Subsampler ss((size_t)total, subsample, seed);
    cloud.reserve(ss.budget);
    for (int i = 0; i < total; ++i) {
        float x, y, z;
        if (!(f >> x >> y >> z)) throw std::runtime_error("Error reading TXT file: Error reading point data from TXT file: " + path);
        if (ss.keep() && ss.kept < ss.budget) {  // utilities.hpp:217 — the RNG is drawn for every point
            cloud.emplace_back(x, y, z);
            ++ss.kept;
        }
    }
    return ss.kept;
}

namespace ply {
struct Property { std::string name, type, count_type; bool is_list = false; };
struct Element { std::string name; size_t count = 0; std::vector<Property> props; };
inline size_t type_size(const std::string& t) {
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    throw std::runtime_error("unsupported PLY property type '" + t + "'");
}
inline double read_scalar(std::istream& f, const std::string& t, bool swap) {
    unsigned char b[8];
    const size_t n = type_size(t);
    f.read(reinterpret_cast<char*>(b), (std::streamsize)n);
    if (!f) throw std::runtime_error("unexpected end of PLY data");
    if (swap) std::reverse(b, b + n);
    if (t == "char" || t == "int8") { int8_t v; std::memcpy(&v, b, 1); return v; }
    if (t == "uchar" || t == "uint8") { uint8_t v; std::memcpy(&v, b, 1); return v; }
    if (t == "short" || t == "int16") { int16_t v; std::memcpy(&v, b, 2); return v; }
    if (t == "ushort" || t == "uint16") { uint16_t v; std::memcpy(&v, b, 2); return v; }
    if (t == "int" || t == "int32") { int32_t v; std::memcpy(&v, b, 4); return v; }
    if (t == "uint" || t == "uint32") { uint32_t v; std::memcpy(&v, b, 4); return v; }
    if (t == "float" || t == "float32") { float v; std::memcpy(&v, b, 4); return v; }
    double v; std::memcpy(&v, b, 8); return v;
}
// the header of an opened file, up to and including end_header: the elements in file order and how the data behind them is written
struct Header { std::vector<Element> elements; bool ascii = false, swap = false; };
inline Header read_header(std::ifstream& f, const std::string& path) {
    if (!f) throw std::runtime_error("Unable to open file: " + path);
    std::string line;
    std::getline(f, line);
    if (trim(line) != "ply") throw std::runtime_error("not a PLY file");
    std::string format;
    Header h;
    while (std::getline(f, line)) {
        std::istringstream ls(trim(line));
        std::string tok;
        ls >> tok;
        if (tok == "format") ls >> format;
        else if (tok == "element") { Element e; ls >> e.name >> e.count; h.elements.push_back(e); }
        else if (tok == "property") {
            if (h.elements.empty()) throw std::runtime_error("property before element");
            Property p;
            std::string t;
            ls >> t;
            if (t == "list") { p.is_list = true; ls >> p.count_type >> p.type >> p.name; }
            else { p.type = t; ls >> p.name; }
            h.elements.back().props.push_back(p);
        } else if (tok == "end_header") break;
    }
    h.ascii = format == "ascii";
    const bool big = format == "binary_big_endian";
    if (!h.ascii && !big && format != "binary_little_endian") throw std::runtime_error("unsupported PLY format '" + format + "'");
    const uint16_t probe = 1;
    const bool host_little = *reinterpret_cast<const uint8_t*>(&probe) == 1;
    h.swap = !h.ascii && (big == host_little);
    return h;
}
}  // namespace ply

inline size_t load_cloud_ply(const std::string& path, float subsample, std::vector<icp::vec3>& cloud, long long seed) {
    try {
        std::ifstream f(path, std::ios::binary);
        const ply::Header header = ply::read_header(f, path);
        const bool ascii = header.ascii, swap = header.swap;
        for (const ply::Element& e : header.elements) {
            const bool is_vertex = e.name == "vertex";
            int ix = -1, iy = -1, iz = -1;
            for (size_t k = 0; k < e.props.size(); ++k) {
                if (e.props[k].name == "x") ix = (int)k;
                if (e.props[k].name == "y") iy = (int)k;
                if (e.props[k].name == "z") iz = (int)k;
            }
            if (is_vertex && (ix < 0 || iy < 0 || iz < 0)) throw std::runtime_error("PLY file missing 'x', 'y', or 'z' vertex properties.");
            if (is_vertex && e.count == 0) throw std::runtime_error("No vertices found in the PLY file.");
            Subsampler ss(e.count, subsample, seed);
            if (is_vertex) cloud.reserve(ss.budget);
            std::vector<double> vals(e.props.size());
            for (size_t i = 0; i < e.count; ++i) {
                if (is_vertex && ss.kept >= ss.budget) return ss.kept;  // utilities.hpp:154 — the PLY loop ends early
                for (size_t k = 0; k < e.props.size(); ++k) {
                    const ply::Property& p = e.props[k];
                    if (p.is_list) {
                        double n;
                        if (ascii) { if (!(f >> n)) throw std::runtime_error("unexpected end of PLY data"); }
                        else n = ply::read_scalar(f, p.count_type, swap);
                        for (long long j = 0; j < (long long)n; ++j) {
                            double dummy;
                            if (ascii) { if (!(f >> dummy)) throw std::runtime_error("unexpected end of PLY data"); }
                            else (void)ply::read_scalar(f, p.type, swap);
                        }
                    } else if (ascii) {
                        if (!(f >> vals[k])) throw std::runtime_error("unexpected end of PLY data");
                    } else {
                        vals[k] = ply::read_scalar(f, p.type, swap);
                    }
                }
                if (is_vertex && ss.keep()) {
                    cloud.emplace_back((float)vals[ix], (float)vals[iy], (float)vals[iz]);
                    ++ss.kept;
                }
            }
            if (is_vertex) return ss.kept;
        }
        throw std::runtime_error("No vertices found in the PLY file.");
    } catch (const std::exception& err) {
        throw std::runtime_error(std::string("Error reading PLY file: ") + err.what());
    }
}

// EXTENSION (params.*_mesh_points): the PLY as a triangle mesh — every vertex (no subsampling here) and the faces of `element face`, read
// from its list property vertex_indices or vertex_index, any integer count and index type, in the three formats.  A polygon of k > 3
// vertices is fan-triangulated as (i0, ij, ij+1); a face of fewer than 3 is dropped and counted in *short_faces.  Every other list, element
// and property is passed over as load_cloud_ply passes over it.  A file without faces returns no triangles: the caller judges that.
inline void load_mesh_ply(const std::string& path, std::vector<icp::vec3>& vertices, std::vector<uint32_t>& triangles, size_t* short_faces = nullptr) {
    try {
        std::ifstream f(path, std::ios::binary);
        const ply::Header header = ply::read_header(f, path);
        const bool ascii = header.ascii, swap = header.swap;
        auto scalar = [&](const std::string& type) {
            double v;
            if (ascii) { if (!(f >> v)) throw std::runtime_error("unexpected end of PLY data"); }
            else v = ply::read_scalar(f, type, swap);
            return v;
        };
        size_t dropped = 0;
        bool have_vertices = false;
        std::vector<uint32_t> poly;
        for (const ply::Element& e : header.elements) {
            const bool is_vertex = e.name == "vertex", is_face = e.name == "face";
            int ix = -1, iy = -1, iz = -1;
            for (size_t k = 0; k < e.props.size(); ++k) {
                if (e.props[k].name == "x") ix = (int)k;
                if (e.props[k].name == "y") iy = (int)k;
                if (e.props[k].name == "z") iz = (int)k;
            }
            if (is_vertex && (ix < 0 || iy < 0 || iz < 0)) throw std::runtime_error("PLY file missing 'x', 'y', or 'z' vertex properties.");
            if (is_vertex && e.count == 0) throw std::runtime_error("No vertices found in the PLY file.");
            if (is_vertex) { vertices.reserve(e.count); have_vertices = true; }
            std::vector<double> vals(e.props.size());
            for (size_t i = 0; i < e.count; ++i) {
                for (size_t k = 0; k < e.props.size(); ++k) {
                    const ply::Property& p = e.props[k];
                    if (!p.is_list) { vals[k] = scalar(p.type); continue; }
                    const bool corners = is_face && (p.name == "vertex_indices" || p.name == "vertex_index");
                    const long long n = (long long)scalar(p.count_type);
                    poly.clear();
                    for (long long j = 0; j < n; ++j) {
                        const double v = scalar(p.type);
                        if (!corners) continue;
                        if (!(v >= 0.0 && v <= 4294967295.0)) throw std::runtime_error("face " + std::to_string(i) + " has a vertex index outside [0, 2^32)");
                        poly.push_back((uint32_t)v);
                    }
                    if (!corners) continue;
                    if (poly.size() < 3) { ++dropped; continue; }
                    for (size_t j = 1; j + 1 < poly.size(); ++j) {
                        triangles.push_back(poly[0]); triangles.push_back(poly[j]); triangles.push_back(poly[j + 1]);
                    }
                }
                if (is_vertex) vertices.emplace_back((float)vals[ix], (float)vals[iy], (float)vals[iz]);
            }
        }
        if (!have_vertices) throw std::runtime_error("No vertices found in the PLY file.");
        if (short_faces) *short_faces = dropped;
    } catch (const std::exception& err) {
        throw std::runtime_error(std::string("Error reading PLY file: ") + err.what());
    }
}

// params.*_subsample over a cloud that was not thinned while it was read (a sampled mesh): load_cloud_txt's rule — the RNG is drawn for
// every point, a point is kept with probability `subsample` until floor(total * subsample) are kept
inline void subsample_cloud(std::vector<icp::vec3>& cloud, float subsample, long long seed) {
    Subsampler ss(cloud.size(), subsample, seed);
    std::vector<icp::vec3> out;
    out.reserve(ss.budget);
    for (const icp::vec3& p : cloud)
        if (ss.keep() && ss.kept < ss.budget) {
            out.push_back(p);
            ++ss.kept;
        }
    cloud.swap(out);
}

inline bool is_ply(const std::string& filepath) {
    const auto dot = filepath.find_last_of('.');
    if (dot == std::string::npos) return false;
    std::string ext = filepath.substr(dot + 1);
    std::transform(ext.begin(), ext.end(), ext.begin(), ::tolower);
    return ext == "ply";
}

inline size_t load_cloud(const std::string& filepath, float subsample, std::vector<icp::vec3>& cloud, long long seed = -1) {
    auto dot = filepath.find_last_of('.');
    if (dot == std::string::npos) throw std::runtime_error("Filepath does not have a valid extension: " + filepath);
    std::string ext = filepath.substr(dot + 1);
    std::transform(ext.begin(), ext.end(), ext.begin(), ::tolower);
    if (ext == "ply") return load_cloud_ply(filepath, subsample, cloud, seed);
    if (ext == "txt") return load_cloud_txt(filepath, subsample, cloud, seed);
    throw std::runtime_error("Unsupported file extension: " + ext);
}

// io.output / io.visualization (declared by test/bunny.toml:10-11, unimplemented upstream)
// refined (optional, EXTENSION: params.refine): a [refined] table behind the existing keys, which stay as they are; rmse_key names its
// residual — plane_rmse for "plane", gicp_rmse for "gicp".  robust (optional, EXTENSION: params.refine_loss): loss, loss_scale (the files'
// units) and weight_sum behind the table's keys.  rms_distance (optional, EXTENSION: params.refine = "mesh"): the rms of the deviation map at
// the refined pose, behind the residual (whose key is then mesh_rmse)
inline void write_result_toml(const std::string& path, const icp::mat3& R, const icp::vec3& t, float sse, size_t ns, double seconds,
                              const fgoicp_run_stats& st, const fgoicp_plane_result_t* refined = nullptr, const char* rmse_key = "plane_rmse",
                              const fgoicp_robust_result_t* robust = nullptr, const char* loss_name = "", const double* rms_distance = nullptr) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("Unable to write " + path);
    f.precision(9);
    f << "# Fast Go-ICP result (fgoicp_amd)\n[result]\n";
    f << "rotation = [\n";
    for (int r = 0; r < 3; ++r) f << "  [" << R[0][r] << ", " << R[1][r] << ", " << R[2][r] << "],\n";
    f << "]\ntranslation = [" << t.x << ", " << t.y << ", " << t.z << "]\n";
    f << "sse = " << sse << "\nmse = " << sse / (float)ns << "\nseconds = " << seconds << "\n";
    f << "\n[stats]\nsubcubes = " << st.trans_cubes << "\nrotation_cubes = " << st.rot_cubes << "\nicp_runs = " << st.icp_runs
      << "\nicp_iterations = " << st.icp_iters << "\nrounds = " << st.rounds << "\n";
    if (!refined) return;
    const float* Q = refined->R;  // glm order: Q[col * 3 + row]
    f << "\n[refined]\nrotation = [\n";
    for (int r = 0; r < 3; ++r) f << "  [" << Q[r] << ", " << Q[3 + r] << ", " << Q[6 + r] << "],\n";
    f << "]\ntranslation = [" << refined->t[0] << ", " << refined->t[1] << ", " << refined->t[2] << "]\n";
    f << rmse_key << " = " << refined->plane_rmse / (double)refined->scaling_factor;
    if (rms_distance) f << "\nrms_distance = " << *rms_distance;
    f << "\niterations = " << refined->iterations << "\nrank = " << refined->rank
      << "\ncorrespondences = " << refined->correspondences << "\n";
    if (!robust) return;
    f << "loss = \"" << loss_name << "\"\nloss_scale = " << robust->scale / (double)robust->scaling_factor << "\nweight_sum = " << robust->weight_sum << "\n";
}

// io.alignment (EXTENSION): the alignment report of the run (fgoicp_solver_alignment / fgoicp_batch_alignment).  Two '#' lines — the summary,
// the column names — then one line per registered source point, in the order the cloud was loaded (after source_subsample): its coordinates
// as loaded, the index of its nearest target point (into the target as loaded), its distance to it in the files' units
// (sqrt(dist2) / scaling_factor) and 1 if the optimum counts it as an inlier.  Points and indices refer to the clouds AS REGISTERED: with
// params.source_voxel / params.target_voxel those are the voxel grids' centroids in their row order, not the points of the files, and with params.*_outlier_knn, params.*_plane_distance or params.*_cluster_eps the rows the filter kept, in their order;
// with params.source_points / params.target_points the sampled points in pick order.
inline void write_alignment_txt(const std::string& path, const std::vector<icp::vec3>& src, const uint32_t* idx, const float* dist2, const uint8_t* inlier,
                                const fgoicp_alignment_summary& s) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("Unable to write " + path);
    f.precision(9);
    const double scale = (double)s.scaling_factor;
    f << "# alignment: points = " << s.points << ", inliers = " << s.inliers << ", targets_hit = " << s.targets_hit << ", sse = " << s.sse
      << ", max_inlier_dist2 = " << s.max_inlier_dist2 << ", scaling_factor = " << s.scaling_factor
      << ", fitness = " << (s.points ? (double)s.inliers / (double)s.points : 0.0)
      << ", inlier_rmse = " << (s.inliers ? std::sqrt((double)s.sse / (double)s.inliers) / scale : 0.0) << "\n";
    f << "# x y z target_index distance inlier\n";
    for (size_t i = 0; i < src.size(); ++i)
        f << src[i].x << " " << src[i].y << " " << src[i].z << " " << idx[i] << " " << std::sqrt((double)dist2[i]) / scale << " " << (int)inlier[i] << "\n";
}

// io.information (EXTENSION): the information matrix of the run (fgoicp_solver_information / fgoicp_batch_information) in the files' frame.
// One '#' line — correspondences, fitness, inlier_rmse and the distance used (inf: none) — then the six rows of the matrix, six numbers each
// at precision 17 (a double read back from it is the double written), twist order (wx, wy, wz, vx, vy, vz).
inline void write_information_txt(const std::string& path, const fgoicp_information_t& s, float distance) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("Unable to write " + path);
    f.precision(9);
    f << "# information: correspondences = " << s.correspondences << ", fitness = " << (s.points ? (double)s.correspondences / (double)s.points : 0.0)
      << ", inlier_rmse = " << (s.correspondences ? std::sqrt(s.sum_dist2 / (double)s.correspondences) / (double)s.scaling_factor : 0.0)
      << ", distance = " << (distance > 0.0f ? distance : INFINITY) << "\n";
    f.precision(17);
    for (int r = 0; r < 6; ++r)
        for (int k = 0; k < 6; ++k) f << s.info[6 * r + k] << (k == 5 ? "\n" : " ");
}

// io.deviation (EXTENSION): the distance of every registered source point, moved by the run's final pose, from the SURFACE of the target
// file's mesh (fgoicp_mesh_distance).  Two '#' lines — the summary, the column names — then one line per source point in the rows of
// io.alignment: its coordinates as loaded, the nearest face (an index into the file's triangles after fan triangulation), its distance in
// the files' units, the side of that face's plane (-1, 0, 1) and the region of the closest point (0 interior, 1 - 3 edge, 4 - 6 vertex).
// The sums are plain fp64 loops in row order.
struct DeviationSummary {
    uint64_t points = 0, triangles = 0, zero_area = 0, negative = 0, on_plane = 0, positive = 0;
    double mean = 0.0, rms = 0.0, max = 0.0;
};
inline DeviationSummary summarize_deviation(const fgoicp_mesh_distance_info_t& mi, const double* dist2, const int8_t* side) {
    DeviationSummary s;
    s.points = mi.queries; s.triangles = mi.triangles; s.zero_area = mi.zero_area;
    double sum = 0.0, sum2 = 0.0;
    for (uint64_t i = 0; i < s.points; ++i) {
        const double d = std::sqrt(dist2[i]);
        sum += d;
        sum2 += dist2[i];
        if (d > s.max) s.max = d;
        (side[i] < 0 ? s.negative : side[i] > 0 ? s.positive : s.on_plane) += 1;
    }
    s.mean = s.points ? sum / (double)s.points : 0.0;
    s.rms = s.points ? std::sqrt(sum2 / (double)s.points) : 0.0;
    return s;
}
inline void write_deviation_txt(const std::string& path, const std::vector<icp::vec3>& src, const uint32_t* face, const double* dist2, const int8_t* side, const uint8_t* region,
                                const DeviationSummary& s) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("Unable to write " + path);
    f.precision(9);
    f << "# deviation: points = " << s.points << ", triangles = " << s.triangles << ", zero_area = " << s.zero_area << ", mean = " << s.mean << ", rms = " << s.rms
      << ", max = " << s.max << ", negative = " << s.negative << ", on_plane = " << s.on_plane << ", positive = " << s.positive << "\n";
    f << "# x y z face distance side region\n";
    for (size_t i = 0; i < src.size(); ++i)
        f << src[i].x << " " << src[i].y << " " << src[i].z << " " << face[i] << " " << std::sqrt(dist2[i]) << " " << (int)side[i] << " " << (int)region[i] << "\n";
}

inline void write_visualization_ply(const std::string& path, const std::vector<icp::vec3>& tgt, const std::vector<icp::vec3>& src,
                                    const icp::mat3& R, const icp::vec3& t) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("Unable to write " + path);
    f << "ply\nformat ascii 1.0\ncomment target = blue, registered source = red\nelement vertex " << tgt.size() + src.size()
      << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    for (const auto& p : tgt) f << p.x << " " << p.y << " " << p.z << " 40 90 220\n";
    for (const auto& p : src) { icp::vec3 q = R * p + t; f << q.x << " " << q.y << " " << q.z << " 220 60 40\n"; }
}

}  // namespace cli
