// ============================================================================
// goicp_oracle — CPU restatement of solemnwind/fast-go-icp's hot path.
//
// THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, bench.py's
// `cpu_baseline` leg and __graft_entry__.smoke() may build, load or call it.
// The product (fast-go-icp_amd/) never includes, links or dlopens anything
// under oracle/.
//
// PARITY UNPINNED: the reference (CUDA + Thrust + GLM + Eigen + CUDA texture
// unit) cannot be built in this image, and it ships no unit tests, golden
// vectors or published outputs.  This file restates the
// reference's arithmetic line by line (each function cites the file:line it
// follows, paths relative to the reference checkout) and is pinned only by
// analytic known-answer tests and by an independent numpy restatement
// (oracle/np_restatement.py), not by reference outputs.
//
// Conventions that the reference inherits from CUDA/GLM/Thrust and that are
// therefore *chosen* here (documented in DESIGN.md §Oracle):
//   * device code (nvcc -fmad=true): a*x + b*y + c*z is evaluated as
//     fma(c, z, fma(b, y, a*x)); host code (fgoicp.cpp, the host half of
//     icp3d.cu) uses plain mul/add, left to right;
//   * Thrust reductions (unspecified fp32 tree order) are restated as a
//     double-precision serial sum rounded once to fp32;
//   * CUDA linear texture filtering: sample at x-0.5, i=floor, weight held in
//     1.8 fixed point (round-to-nearest), clamp addressing, lerp x→y→z;
//   * Eigen::JacobiSVD<Matrix3d> restated from its published algorithm.
// Each of these has a switch in `Conventions` below; tools/convention_flips.py
// runs the golden cases under every flip and DESIGN.md §2 tabulates what moves.
// ============================================================================
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <tuple>
#include <utility>
#include <vector>

namespace goicp_oracle {

// fgoicp/common.hpp:17-19
constexpr float kPi = 3.141592653589793f;
constexpr float kInf = 1E+10f;
constexpr float kSqrt3 = 1.732050807568877f;

// The conventions this restatement CHOOSES where the reference inherits behaviour from nvcc (-fmad=true contraction),
// the CUDA texture unit, Thrust's reduction tree, libdevice's sinf and Eigen.  Value 0/the default is the choice the
// fixtures are generated with; every other value is a FLIP for tools/convention_flips.py (process-global, set before use).
struct Conventions {
    // a*x + b*y + c*z in device code (R*p at registration.cu:20,34, icp3d.cu:35; squared distances at :159, :255 and
    // glm::distance's dot at icp3d.cu:20; the squared norm at :39-41):
    //   1 = fma(c,z, fma(b,y, a*x)) [default]   0 = no contraction   2 = fma(c,z, fma(a,x, b*y)) (the first product fused)
    int fma_matvec = 1;
    int fma_dist = 1;
    int fma_rot_sub = 0;    // distance -= 2*radius*sin (registration.cu:43,51): 0 = product rounded, then subtracted; 1 = fma(-(2*radius), sin, distance)
    int fma_trans_sub = 0;  // distance - M_SQRT3*span (:33, :57): 0 = product rounded; 1 = fma(-M_SQRT3, span, distance)
    int tex_weight = 0;     // 1.8 fixed-point filter weight: 0 = round to nearest, 1 = truncate, 2 = not quantised
    int tex_blend = 0;      // 0 = nested lerps x->y->z as fma(w, b-a, a); 1 = the CUDA programming guide's 8-term weighted sum
    int sum_mode = 0;       // Thrust reductions (registration.cu:80,126,134; icp3d.cu:152,153,166): 0 = fp64 sum rounded once,
                            // 1 = fp32 pairwise tree, 2 = fp32 serial in index order
    int sin_ulps = 0;       // device sin(float) (registration.cu:43) moved by this many ulps (CUDA documents sinf within 2 ulp)
    int svd_r2_two_sided = 0;  // 0 = Eigen's JacobiSVD algorithm; 1 = round 2's own two-sided Jacobi
};
Conventions& conventions();

struct Vec3 { float x, y, z; };
// glm::mat3 layout: c[col][row], 36 B, column-major.
struct Mat3 { float c[3][3]; };

Mat3 mat3_identity();
Vec3 dev_mul(const Mat3& m, const Vec3& v);   // device R*p   (fma convention)
Vec3 host_mul(const Mat3& m, const Vec3& v);  // host   R*p   (plain)
Mat3 host_mul(const Mat3& a, const Mat3& b);  // host   A*B   (plain)

// fgoicp/common.hpp:30-69
struct Rotation {
    float x, y, z, r;
    Mat3 R;
    Rotation() : Rotation(0.f, 0.f, 0.f) {}
    Rotation(float x, float y, float z);
    bool in_SO3() const { return r <= 1.0f; }
};

// fgoicp/common.hpp:75-104
struct RotNode {
    Rotation q;
    float span, lb, ub;
    RotNode(float x, float y, float z, float span, float lb, float ub)
        : q(x, y, z), span(span), lb(lb), ub(ub) {}
    friend bool operator<(const RotNode& a, const RotNode& b) {
        if (a.lb == b.lb) return a.span < b.span;
        return a.lb > b.lb;
    }
    bool overlaps_SO3() const;
};

// fgoicp/common.hpp:110-128
struct TransNode {
    Vec3 t;
    float span, lb, ub;
    TransNode(float x, float y, float z, float span, float lb, float ub)
        : t{x, y, z}, span(span), lb(lb), ub(ub) {}
    friend bool operator<(const TransNode& a, const TransNode& b) {
        if (a.lb == b.lb) return a.span < b.span;
        return a.lb > b.lb;
    }
};

using PointCloud = std::vector<Vec3>;
using Bounds = std::array<std::pair<float, float>, 3>;

// fgoicp/registration.cu:180-207, 258-328 (+ CUDA texture semantics)
struct NearestNeighborLUT {
    float resolution = 0.f;
    int dims[3] = {0, 0, 0};
    float scale = 0.f;
    Vec3 offset{0, 0, 0};
    std::vector<float> data;  // x fastest: (z*dy + y)*dx + x
    bool quantize_weights = true;  // 1.8 fixed-point interpolation weights

    NearestNeighborLUT() = default;
    NearestNeighborLUT(float resolution, const Bounds& target_bounds, const PointCloud& pc, bool build_now = true);
    void build(const PointCloud& pc);
    float search(const Vec3& q) const;
    size_t size() const { return (size_t)dims[0] * dims[1] * dims[2]; }
};

// CPU-BASELINE ONLY (bench.py's cpu_baseline leg; off by default, the restatement's searches stay the literal O(n*m) loops).
// The reference's README names a nanoflann kd-tree for the CPU nearest-neighbour queries but its code never calls one
// (SURVEY fact 2); this uniform grid over the target's bounding box stands in for it.  Results are those of the brute-force
// loops bit for bit (same fp32 distance expression, min is order-independent, the first-index rule of icp3d.cu:20-25 is
// applied on the sqrt-tie set) — tests/test_oracle_kat.py checks that.
struct GridNN {
    Vec3 lo{0, 0, 0}, hi{0, 0, 0};
    float h = 1.f;
    int n[3] = {1, 1, 1};
    std::vector<int> start, items;
    const PointCloud* pc = nullptr;
    void build(const PointCloud& cloud);
    float min_d2(const Vec3& q) const;            // brute_force_find_nearest_neighbor
    int first_min_sqrt_index(const Vec3& q) const; // kernFindNearestNeighbor's index
private:
    template <class F> void rings(const Vec3& q, F& visit_and_bound) const;
};

// fgoicp/registration.hpp:49-98, registration.cu:14-174
class Registration {
public:
    Registration(const PointCloud& pct, const PointCloud& pcs, const Bounds& bounds, float lut_resolution,
                 bool build_lut = true);
    float compute_sse_error(const Mat3& R, const Vec3& t) const;
    // returns {lower, upper} — lower first, registration.cu:151
    std::tuple<std::vector<float>, std::vector<float>>
    compute_sse_error(const RotNode& rnode, const std::vector<TransNode>& tnodes, bool fix_rot) const;

    const PointCloud& pct;
    const PointCloud& pcs;
    NearestNeighborLUT nnlut;
    // EXTENSION (no reference behaviour: `params.trim` is parsed but never used upstream).
    // Trimmed Go-ICP as in Yang et al.'s Go-ICP: every sum over source points becomes the sum of the
    // `inliers` smallest per-point terms (0 = no trimming).
    size_t inliers = 0;
    std::shared_ptr<GridNN> grid;   // CPU baseline only: exact NN through a uniform grid instead of the O(n*m) loops (same results)
    void use_grid(bool on);
};
// sum of the k smallest values (fp64 accumulation in ascending order, rounded once); k = 0 or k >= n: plain sum in index order
float trimmed_sum(std::vector<float>& values, size_t k);

float brute_force_find_nearest_neighbor(const Vec3& q, const PointCloud& pct);  // registration.cu:162-174

// fgoicp/icp3d.hpp / icp3d.cu
Mat3 closest_orthogonal_approximation(const Mat3& ABt);  // icp3d.cu:110-138
struct ProcrustesDebug { Vec3 src_centroid, cor_centroid; Mat3 ABt; };
class IterativeClosestPoint3D {
public:
    IterativeClosestPoint3D(const Registration& reg, const PointCloud& pct, const PointCloud& pcs,
                            size_t max_iter, float conv_thr, const Mat3& R, const Vec3& t);
    std::tuple<float, Mat3, Vec3> run();
    std::tuple<Mat3, Vec3> procrustes(ProcrustesDebug* dbg = nullptr);
    size_t iterations() const { return iters_; }
    PointCloud& working() { return pcs_buf_; }
    void move_working(const Mat3& R, const Vec3& t);  // run()'s rotate_translate_inplace on working() (:85, :100)
    std::vector<int>& last_corr_index() { return corr_idx_; }
private:
    const Registration& reg_;
    const PointCloud& pct_;
    PointCloud pcs_buf_;
    Mat3 R_;
    Vec3 t_;
    size_t max_iter_;
    float thr_;
    size_t iters_ = 0;
    std::vector<int> corr_idx_;
};

// fgoicp/fgoicp.hpp, fgoicp.cpp
struct RunStats {
    uint64_t trans_cubes = 0;     // `count` of fgoicp.cpp:108,132 summed over all inner BnBs
    uint64_t bounds_calls = 0;    // Registration::compute_sse_error(batch) calls
    uint64_t rot_cubes = 0;       // rotation children that went through branch_and_bound_R3
    uint64_t icp_runs = 0;
    uint64_t icp_iters = 0;
    uint64_t inner_bnb = 0;
};

class FastGoICP {
public:
    FastGoICP(PointCloud pct, PointCloud pcs, float lut_resolution, float mse_threshold, float trim_fraction = 0.0f);
    std::tuple<Mat3, Vec3> run();
    float get_best_error() const { return best_sse; }
    std::tuple<Mat3, Vec3> get_best_transform() const { return {best_rotation, best_translation}; }
    const RunStats& stats() const { return stats_; }

    // pre-processing results exposed for tests (fgoicp.cpp:176-287)
    PointCloud pcs, pct;
    size_t ns, nt;
    Vec3 offset_pcs, offset_pct;
    float scaling_factor;
    Bounds target_bounds;
    Registration registration;
    float best_sse;
    Mat3 best_rotation;
    Vec3 best_translation;
    float mse_threshold, sse_threshold;

    Vec3 restore_translation(const Mat3& R, const Vec3& t) const;  // fgoicp.hpp:87-90
    std::tuple<float, Vec3> branch_and_bound_R3(RotNode& rnode, bool fix_rot);
    float branch_and_bound_SO3();
private:
    RunStats stats_;
};

Vec3 center_point_cloud(PointCloud& pc);                  // fgoicp.cpp:176-195
float get_scaling_factor(const PointCloud& pc);            // fgoicp.cpp:197-220
float scale_point_clouds(PointCloud& pct, PointCloud& pcs);  // fgoicp.cpp:271-287
Bounds get_point_cloud_ranges(const PointCloud& pc);       // fgoicp.cpp:222-268

}  // namespace goicp_oracle
