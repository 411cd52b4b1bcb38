/*
 * fgoicp_amd.h — C ABI of the MI355X-native Go-ICP hot path (libfgoicp_amd.so).
 *
 * The reference (solemnwind/fast-go-icp) has no FFI layer: its boundary is the C++ class
 * interface in namespace icp.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  Plain pointers and sizes
 * only; every function returns an fgoicp_status (0 = OK) and never throws across the ABI.
 *
 * Conventions
 *   - points:    float xyz triples, tightly packed (glm::vec3 / icp::Point3D, common.hpp:130).
 *   - matrices:  9 floats in glm::mat3 memory order = COLUMN-major, m[col*3 + row]
 *                (common.hpp:50-54).
 *   - all pointers are HOST pointers unless a parameter says "device".
 *   - a context is bound to one HIP device and one stream; it is not thread-safe.
 *   - there is NO CPU fallback: without a usable HIP device every create call fails with
 *     FGOICP_ERR_NO_DEVICE.
 */
#ifndef FGOICP_AMD_H
#define FGOICP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fgoicp_status {
    FGOICP_OK = 0,
    FGOICP_ERR_INVALID_ARG = 1,
    FGOICP_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime error at init            */
    FGOICP_ERR_HIP = 3,         /* a HIP call failed (see fgoicp_last_error)             */
    FGOICP_ERR_OOM = 4,
    FGOICP_ERR_TOO_LARGE = 5,   /* batch larger than the context was sized for          */
    FGOICP_ERR_EXCHANGE = 6     /* the multi-GPU exchange callback reported a failure   */
} fgoicp_status;

/* Thread-local description of the last failure on the calling thread ("" if none). */
const char* fgoicp_last_error(void);
const char* fgoicp_version(void);
/* 1 = this is the development build (-DFGOICP_DEV_KNOBS, libfgoicp_amd_dev.so): it reads the FGOICP_* tuning / A-B variables of
 * NOTES.md from the environment and carries the kernel variants that were measured and rejected.  0 = the shipped build: it reads
 * FGOICP_HOST_THREADS / FGOICP_HOST_SPIN only and no stray variable can change its code path. */
int fgoicp_dev_knobs(void);
/* The ABI revision of this header.  2 (round 4): fgoicp_exchange and fgoicp_ctx_info start with `struct_size` (members may be appended
 * from now on without breaking callers built against this revision); fgoicp_solver_set_log, fgoicp_rccl_create_ex added.  A caller
 * built against revision 1 (no struct_size) must be rebuilt: INTEGRATION.md "ABI revisions". */
#define FGOICP_ABI_VERSION 2
int fgoicp_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Operator level: icp::Registration + icp::NearestNeighborLUT + icp::IterativeClosestPoint3D
 * ------------------------------------------------------------------------------------------ */
typedef struct fgoicp_ctx fgoicp_ctx;

enum {
    FGOICP_FLAG_NO_WEIGHT_QUANT = 1u << 0, /* trilinear weights in full fp32 instead of CUDA's 1.8 fixed point */
    FGOICP_FLAG_NO_MORTON       = 1u << 1, /* keep the source cloud in caller order on the device             */
    FGOICP_FLAG_PROFILE         = 1u << 2, /* bracket every bounds kernel with HIP events (fgoicp_ctx_profile) */
    FGOICP_FLAG_BRUTE_FORCE_NN  = 1u << 3, /* O(n*m) brute-force kernels for LUT build / SSE / ICP instead of the exact BVH */
    FGOICP_FLAG_CURVE_ORDER     = 1u << 4  /* source cloud along the Hilbert curve instead of in k-d order on the device: for sources with outliers
                                              spread through the volume (trimmed runs; fgoicp_solver_create sets it when trim_fraction > 0).  Locality only:
                                              results do not depend on the order */
};

/*
 * Replaces icp::Registration::Registration(pct, pcs, target_bounds, lut_resolution)
 * (fgoicp/registration.hpp:68-80) together with icp::NearestNeighborLUT::NearestNeighborLUT /
 * build (fgoicp/registration.cu:180-207, 258-318): uploads both clouds, builds the
 * nearest-squared-distance LUT on the device.  bounds6 = {minx,maxx,miny,maxy,minz,maxz} of the
 * target (std::array<std::pair<float,float>,3>).  Clouds are copied; the caller keeps ownership.
 */
int fgoicp_ctx_create(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, const float* bounds6,
                      float lut_resolution, int device, unsigned flags, fgoicp_ctx** out);
/* Replaces ~Registration / ~NearestNeighborLUT (registration.hpp:82-87, registration.cu:209-248). */
void fgoicp_ctx_destroy(fgoicp_ctx* ctx);

/* LUT geometry / contents in the reference's layout, index (z*dy + y)*dx + x
 * (registration.cu:186-188, :276).  Used by tests and by INTEGRATION.md's façade. */
int fgoicp_lut_dims(const fgoicp_ctx* ctx, int* dims3);
int fgoicp_lut_read(fgoicp_ctx* ctx, float* out, size_t capacity_floats);
/* What the context derived from the clouds' statistics for its own scaling decisions (the reference's open item "compute point
 * clouds' stats, normalize (For scalability)", TODO.md:7): LUT size in every layout it keeps, source points per voxel of the LUT's
 * faces (the density that picks the packed layout and the points per work item), work items per evaluation. */
typedef struct fgoicp_ctx_info {
    size_t struct_size;          /* IN: sizeof(fgoicp_ctx_info) as the CALLER was compiled (ABI 2).  fgoicp_ctx_get_info writes no byte beyond it, so a caller
                                    built against an older, shorter struct is not overrun when members are appended; 0 is refused */
    int lut_dims[3];
    int lut_layout;              /* next to the plain fp32 LUT: 1 = z-pair copy (8 B per node), 2 = yz-quad copy (16 B per node), 4 = apron-bricked yz-quad copy (21.3 B per node),
                                    6 = z-pair apron bricks (14.2 B per node; sparse clouds whose quad copy would exceed 256 MiB) */
    uint64_t lut_nodes;
    uint64_t lut_bytes;          /* plain LUT (padded) + packed copy, device memory */
    double source_points_per_face_voxel;
    int points_per_item;         /* 256 .. 2048 */
    int items_per_evaluation;    /* ceil(ns / points_per_item) */
    int max_subcubes_per_window;
    int source_order;            /* order of the source cloud on the device: 0 = caller / Z-order, 1 = Hilbert curve, 2 = k-d cells of 64 points, 3 = density split */
    int tree_order;              /* leaves of the target tree: 1 = k-d cells of 32 points, 0 = runs of the space-filling curve */
    int chunks_per_item_with_thresholds; /* fgoicp_bounds_submit_cut: a work item of such a submission spans this many chunks of points_per_item points (1 or 2).  Appended within revision 2: a caller built with the shorter struct is served as before (struct_size) */
} fgoicp_ctx_info;
int fgoicp_ctx_get_info(const fgoicp_ctx* ctx, fgoicp_ctx_info* out);
/* n single nodes of the LUT: out[i] = node (x, y, z) = xyz[3i..3i+2] (the value buildLUTKernel, registration.cu:258-278, stores at
 * index (z*dy + y)*dx + x).  For LUTs too large to read back whole (test/bunny.toml: 923 x 906 x 711 nodes). */
int fgoicp_lut_nodes(fgoicp_ctx* ctx, const int* xyz, size_t n, float* out);
/* Device evaluation of NearestNeighborLUT::search (registration.cu:320-328; CUDA tex3D linear
 * filtering restated in software) at n query points. */
int fgoicp_lut_search(fgoicp_ctx* ctx, const float* q_xyz, size_t n, float* out);

/*
 * Replaces Registration::compute_sse_error(RotNode&, std::vector<TransNode>&, bool, StreamPool&)
 * (registration.hpp:97, registration.cu:88-152; kernel kernComputeBounds :27-60).
 * tnodes4 = B x {t.x, t.y, t.z, span}.  Outputs: lb_out[B], ub_out[B] (the reference returns
 * {lower, upper}, registration.cu:151).  B may exceed the reference's 32.
 */
int fgoicp_bounds_batch(fgoicp_ctx* ctx, const float* R9, float rot_span, const float* tnodes4, int B, int fix_rot,
                        float* lb_out, float* ub_out);
/*
 * The same operator for G rotation nodes in one submission (one host<->device round trip):
 * group g uses R9[g*9..], rot_span[g], fix_rot[g] and the translation nodes
 * tnodes4[offsets[g]*4 .. offsets[g+1]*4).  lb_out/ub_out are indexed like tnodes.
 */
int fgoicp_bounds_multi(fgoicp_ctx* ctx, int G, const float* R9, const float* rot_span, const int* fix_rot,
                        const int* offsets, const float* tnodes4, float* lb_out, float* ub_out);

/*
 * Asynchronous form of fgoicp_bounds_multi on one of two slots (0, 1), each with its own buffers (the
 * kernels of both queue on the context's stream and run back to back): submit returns once the work is queued, collect waits for it and returns the bounds in
 * submission order.  Lets the host prepare the next submission of one slot while the device works on
 * the other.  A slot must be collected before it is submitted again.
 */
int fgoicp_bounds_submit(fgoicp_ctx* ctx, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot,
                         const int* offsets, const float* tnodes4);
/*
 * The same with a hint: twin[i] = j (and twin[j] = i) says that subcubes i and j of this submission are the SAME translation
 * node under the SAME rotation, once in a fix_rot group and once in a non-fix_rot group — what the UB and the LB inner
 * branch-and-bound of one rotation cube (fgoicp.cpp:69, :90) produce while they walk the top of the same translation tree.
 * Such a pair is evaluated with one LUT lookup per point and both variants of the bound formulae (registration.cu:39-58);
 * the four sums are bit-identical to two separate evaluations.  twin[i] = -1 (or twin = NULL): no twin.  The hint is
 * validated (rotation, span, node and fix_rot are compared), a wrong hint only costs the saving.
 */
int fgoicp_bounds_submit_twins(fgoicp_ctx* ctx, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot,
                               const int* offsets, const float* tnodes4, const int* twin);
/*
 * The same with what the caller does NOT need to know: cut_above[g] = T (one per group; +inf, or cut_above = NULL: everything) says
 * that for a subcube of group g whose lower bound is >= T the exact bounds do not matter — the inner branch-and-bound drops such a node
 * whatever they are (fgoicp.cpp:151, with T = its running best error) and its result takes part in comparisons only (:74, :92;
 * csrc/host/driver.hpp InnerTask::cut_above).  Such a row comes back as lb = ub = T.  All terms of the lower-bound sum are >= 0 and the
 * evaluation of a subcube is spread over many work items (chunks of source points), so the kernel stops evaluating a subcube once the
 * sums of its finished items have reached T: on a certify run two thirds of all point evaluations belong to such subcubes
 * (profiles/r04_early_exit_*).  Rows below their threshold are bit-identical to fgoicp_bounds_submit_twins; the answer for a row at or
 * above it is {T, T} whether the kernel got to cut it short or not (deterministic).  Trimmed contexts ignore cut_above: they are the only
 * case in which rows at or above their threshold come back exact.
 */
int fgoicp_bounds_submit_cut(fgoicp_ctx* ctx, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot,
                             const int* offsets, const float* tnodes4, const int* twin, const float* cut_above);
/*
 * The same with one more hint: ub_below_span[g] = S (one per group; 0, or ub_below_span = NULL: none — the call is then
 * fgoicp_bounds_submit_cut) says that a subcube of group g whose translation span is below S is TERMINAL for the caller: it is never split,
 * so its lower bound takes part in no decision of the caller's, and its upper bound only where it is below T = cut_above[g] (a leaf of the
 * inner branch-and-bound, span < 0.1: fgoicp.cpp:139-145, :151, :155; csrc/host/driver.hpp InnerTask::leaf_below).  For such a row the
 * exact bounds do not matter once its UPPER bound is >= T: it comes back as lb = ub = T.  Every term of the upper-bound sum is >= 0 and
 * >= the lower-bound term of the same point, so the kernel stops evaluating a terminal subcube once the UPPER-bound sums of its finished
 * items have reached T — much earlier than the lower-bound sums would, which for a leaf that survives often never do.
 * One rule per row, deterministic either way: a terminal row is {T, T} if its upper bound is >= T (which subsumes "lower bound >= T"),
 * cut short or not; every other row follows fgoicp_bounds_submit_cut; a row that is not answered {T, T} is bit-identical to
 * fgoicp_bounds_submit_twins.  The two rows of a twin pair are the same node: each follows the rule of its own group.  Without cut_above
 * the hint has no effect; trimmed contexts ignore it as they ignore cut_above.
 */
int fgoicp_bounds_submit_leaf(fgoicp_ctx* ctx, int slot, int G, const float* R9, const float* rot_span, const int* fix_rot,
                              const int* offsets, const float* tnodes4, const int* twin, const float* cut_above, const float* ub_below_span);
int fgoicp_bounds_collect(fgoicp_ctx* ctx, int slot, float* lb_out, float* ub_out);
/* Work items (subcube x chunk of source points) of the submissions that carried thresholds since the last reset, and how many of them
 * the early exit did not evaluate (measurement: bench.py prices the kernel on the items it evaluated).  Call between submissions. */
int fgoicp_ctx_cut_stats(fgoicp_ctx* ctx, uint64_t* items_offered, uint64_t* items_cut, int reset);

/* Replaces float Registration::compute_sse_error(glm::mat3 R, glm::vec3 t)
 * (registration.hpp:96, registration.cu:62-86; kernels :14-25, :154-174): exact nearest
 * neighbour SSE of R*src + t against the target. */
int fgoicp_sse(fgoicp_ctx* ctx, const float* R9, const float* t3, float* sse_out);

/*
 * EXTENSION — the alignment report (no reference counterpart: the reference ends in (R, t) and the best error).  For R*src + t: per
 * source point the exact nearest target point (index into the target as handed to the create call; the tie rule of icp3d.cu:20-25 —
 * square roots compared, lowest index) and its squared distance, the inlier mask (all ones; on a trimmed context the `inliers` smallest
 * squared distances, ties at the cut to the lowest source indices), and per target point whether it is the neighbour of an inlier.
 * Every output pointer may be NULL; arrays are in the caller's point order (corr_idx_ns, dist2_ns, inlier_ns: ns entries;
 * target_hit_nt: nt).  On a trimmed context the outliers get their true neighbour too.  Distances are in the frame of the clouds the
 * context holds (a solver's are centred and scaled: scaling_factor).  The call leaves the context as it found it.
 */
typedef struct fgoicp_alignment_summary {
    uint32_t struct_size;      /* IN: sizeof(fgoicp_alignment_summary) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, inliers;  /* ns; ns or the trimmed k */
    uint64_t targets_hit;      /* distinct target points that are the neighbour of an inlier */
    float sse;                 /* == fgoicp_sse(ctx, R, t), bit for bit */
    float max_inlier_dist2;
    float scaling_factor;      /* 1 for a bare context; the solver's (fgoicp_solver_preproc) otherwise: sqrt(dist2) / scaling_factor is in the callers' units */
} fgoicp_alignment_summary;
int fgoicp_alignment(fgoicp_ctx* ctx, const float* R9, const float* t3, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns,
                     uint8_t* target_hit_nt, fgoicp_alignment_summary* out);

/*
 * EXTENSION — the information matrix of a registration (no reference counterpart; Open3D: get_information_matrix_from_point_clouds), the
 * weight of a pose-graph edge.  For a transform (R, t) the COUNTED correspondences are the source points i that
 *   - the alignment report marks an inlier (every point; on a trimmed context the k smallest),
 *   - have dist2[i] <= max_dist2 (+inf: no threshold; NaN and negative values are refused before any device work), and
 *   - have corr_idx[i] < nt.
 * With q_i the target point corr_idx[i] names and G_i = [ -[q_i]x | I3 ]:
 *   info = sum G_i^T G_i = [ (sum |q|^2) I - sum q q^T   [sum q]x ]
 *                          [ -[sum q]x                   N I      ]
 * 6 x 6, row-major, twist order rotation first (wx, wy, wz, vx, vy, vz).  The device computes N, sum q, sum q q^T (xx xy xz yy yz zz) and
 * sum dist2 over the counted set behind the report's device half, with every addition in a fixed order (two calls return the same bytes);
 * the host forms the matrix in fp64.  fitness = correspondences / points, inlier_rmse = sqrt(sum_dist2 / correspondences) / scaling_factor.
 * The call leaves the context as it found it, as fgoicp_alignment does.
 * Frame: fgoicp_information answers in the frame of the clouds the context holds.  fgoicp_solver_information and fgoicp_batch_information
 * answer in the CALLERS' frame, q as handed to the create call: the context holds q_s = (q - c) * s (c = the target's centroid, MINUS the target offset of
 * fgoicp_solver_preproc, which follows the reference's sign; s = its scale) and the host converts, sum q = sum q_s / s + N c and sum q q^T = sum q_s q_s^T / s^2 + (c sum q_s^T + sum q_s c^T) / s
 * + N c c^T (fgoicp_information_from_moments).  Their threshold is a DISTANCE in the callers' units; the library forms, in fp32,
 *   ds = (float)max_distance * scale;  max_dist2 = ds * ds;
 * and counts dist2[i] <= max_dist2 against the report's dist2 (fgoicp_solver_alignment), so a caller can reproduce the set.  sum_dist2 and
 * max_dist2 stay in the context's frame whichever call filled them (scaling_factor converts, as for fgoicp_alignment_summary).
 * (The struct is fgoicp_information_t, as fgoicp_cloud_stats_t: C has one name space for a typedef and a function.)
 */
typedef struct fgoicp_information_t {
    uint32_t struct_size;            /* IN: sizeof(fgoicp_information_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, correspondences; /* ns; the counted correspondences N */
    double   sum_dist2;              /* over the counted set, context frame */
    double   sum_q[3], sum_qq[6];    /* frame as defined above; sum_qq in the order xx xy xz yy yz zz */
    double   info[36];
    float    max_dist2, scaling_factor; /* the threshold the device compared with (context frame); 1 for a bare context, the solver's scale otherwise */
} fgoicp_information_t;
int fgoicp_information(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, fgoicp_information_t* out);
/* The host half of the three calls, no device needed: moments of n points in one frame -> the moments in the frame q = q_s / scale + offset
 * and the matrix.  offset3 = NULL, scale = 1: no change of frame.  info36, sum_q3_out and sum_qq6_out may each be NULL; the outputs may
 * alias the inputs.  Refuses null inputs and a scale that is not a positive finite number. */
int fgoicp_information_from_moments(uint64_t n, const double* sum_q3, const double* sum_qq6, const float* offset3, float scale, double* info36,
                                    double* sum_q3_out, double* sum_qq6_out);

/*
 * EXTENSION — point-to-plane refinement with target normals (no reference counterpart; what a multiway-registration pipeline runs from the
 * global result before it takes the pose-graph edge).
 *
 * Target normals.  fgoicp_ctx_set_target_normals with a pointer takes the caller's normals (nt triples, caller order), normalised on upload;
 * a non-finite or zero vector is refused (FGOICP_ERR_INVALID_ARG) before any device work; k is ignored.  With NULL the normals are ESTIMATED
 * on the device: per target point the unit direction of least variance of its k nearest target points, the point itself included
 * (4 <= k <= 32, k <= nt; needs the search tree, so a FGOICP_FLAG_BRUTE_FORCE_NN context is refused).  The neighbours are exact: the k
 * smallest of the fp32 squared distances the scans compute, ordered by (distance, caller index) — ties at the cut go to the lowest index.
 * The SIGN of an estimated normal is left as it falls: everything below is even in n (r n = (-r)(-n), J^T J and J^T r likewise), so
 * normals need not be oriented.  A degenerate neighbourhood (all k points equal) gets the zero vector, which takes its point out of the
 * counted set below.  The array is 16 bytes per target point, allocated by the first call; a context that never asks allocates nothing.
 * fgoicp_target_normals reads them back (nt triples, caller order; refused before they are set).  fgoicp_target_knn returns the
 * neighbour sets themselves: nt rows of k, rows and indices in caller order, each row sorted by (distance, index); either output may be NULL.
 *
 * The normal equations.  For (R, t) the COUNTED correspondences are the source points i that the alignment report marks an inlier, with
 * dist2[i] <= max_dist2 (+inf: no threshold; NaN and negative values refused), corr_idx[i] < nt and a non-zero normal at corr_idx[i].  With
 * x = R p_i + t (fp32, as the report's scan forms it), q the target point, n its normal: r = n.(x - q), J = [ (x cross n)^T, n^T ], twist
 * order (wx, wy, wz, vx, vy, vz).  m[28] = the upper triangle of sum J^T J row by row (21), sum J^T r (6), sum r^2 (1), every term formed in
 * fp64 and added in a fixed order (two calls return the same bytes).  Context frame.
 */
typedef struct fgoicp_plane_moments_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_plane_moments_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, correspondences; /* ns; the counted correspondences N */
    double   m[28];
    float    max_dist2;               /* the threshold the device compared with */
} fgoicp_plane_moments_t;
typedef struct fgoicp_plane_result_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_plane_result_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    float    R[9], t[3];              /* the refined pose (fgoicp_solver_refine_plane: t restored to the callers' frame) */
    int      iterations;              /* steps taken */
    int      rank;                    /* of the last solve (6: well posed; 0 when max_iter = 0 or nothing was counted) */
    uint64_t correspondences;         /* counted at the returned pose */
    double   plane_rmse;              /* sqrt(sum r^2 / N) at the returned pose, context frame (0 when N = 0); / scaling_factor: callers' units
                                       * (fgoicp_icp_gicp, fgoicp_solver_refine_gicp: sqrt(sum d^T M d / N)) */
    float    sse;                     /* == fgoicp_sse(ctx, R, t) at the returned pose, bit for bit (context frame) */
    float    scaling_factor;          /* 1 for a bare context; the solver's scale otherwise */
} fgoicp_plane_result_t;
int fgoicp_ctx_set_target_normals(fgoicp_ctx* ctx, const float* normals_nt3_or_NULL, int k);
int fgoicp_target_normals(fgoicp_ctx* ctx, float* out_nt3);
int fgoicp_target_knn(fgoicp_ctx* ctx, int k, uint32_t* idx_ntk, float* d2_ntk);
/* One evaluation at a fixed pose: the report's device half, then the reduction.  Refused when the normals are not set.  Leaves the
 * context as it found it, as fgoicp_alignment does. */
int fgoicp_plane_moments(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, fgoicp_plane_moments_t* out);
/* Host only, no device needed: solves (sum J^T J) xi = -sum J^T r in fp64 by a symmetric eigen-decomposition (6 x 6 Jacobi).  rank = the
 * number of eigenvalues above 1e-9 x the largest; with rank < 6 the solution lies in the span of the kept eigenvectors (a planar target:
 * rank 3, the in-plane motions stay zero).  Refuses null arguments, n = 0 and a non-finite moment. */
int fgoicp_plane_step_from_moments(uint64_t n, const double* m28, double* xi6, int* rank);
/* Host only: the pose update of a step, R' = Rod(w) R, t' = Rod(w) t + v with Rod = Rodrigues' formula in fp64; R' is rounded to fp32
 * once and then replaced by the rotation nearest to it (closest_orthogonal_approximation).  The outputs may alias the inputs. */
int fgoicp_plane_apply_step(const float* R9, const float* t3, const double* xi6, float* R_out9, float* t_out3);
/* The loop from (R0, t0): moments at (R, t), the step, the update; it ends after the step with |w| + |v| < conv_thr, after the first
 * step when that solve had rank < 6 (the unconstrained motions would drift), when nothing is counted, or after max_iter steps.
 * max_iter = 0 evaluates and returns the start.  On a trimmed context the inliers are the report's, selected anew in every iteration.
 * Refused when the normals are not set.  Leaves the context as it found it: a later fgoicp_icp, fgoicp_sse or solver run returns the
 * bits it returns without this call. */
int fgoicp_icp_plane(fgoicp_ctx* ctx, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, fgoicp_plane_result_t* out);

/*
 * EXTENSION — Generalized-ICP refinement with source normals (no reference counterpart; Segal et al., "Generalized-ICP": the plane-to-plane
 * error, for two clouds that are both noisy samples of one surface).
 *
 * Regularised covariances.  GICP replaces the eigenvalues of a neighbourhood covariance by (1, 1, epsilon); with n the unit direction of
 * least variance that is C = I - (1 - epsilon) n n^T, so a normal per point of BOTH clouds is all the state.  epsilon must be finite and lie
 * in (0, 1] (1e-3 is the usual choice); anything else is refused.
 *
 * Source normals follow the rule of the target's: fgoicp_ctx_set_source_normals with a pointer takes ns triples in caller order, normalised
 * on upload, a zero or non-finite one refused with its index before any device work (the stored normals stay), k ignored.  With NULL they
 * are estimated from every source point's k nearest SOURCE points, itself included (4 <= k <= 32, k <= ns; neighbours by (bits of the fp32
 * squared distance, caller index); covariance and eigenvector in fp64; sign as it falls; a neighbourhood without extent gets the zero
 * vector), in the frame of the source as the context holds it, through a search tree over the source that the call builds and frees.  A
 * FGOICP_FLAG_BRUTE_FORCE_NN context is refused for estimation, as for the target.  16 bytes per source point, allocated by the first
 * call; a context that never asks allocates nothing.  fgoicp_source_normals reads them back (ns triples, caller order; refused before
 * they are set).
 *
 * The normal equations.  COUNTED at (R, t) are the correspondences fgoicp_plane_moments counts whose own source normal is non-zero too.
 * Per counted point, in fp64 from the fp32 values: x = R p + t (as the report's scan forms it), q the target point and n_q its normal,
 * m = R n_p with n_p the source normal, S = 2 I - (1 - epsilon)(n_q n_q^T + m m^T), M = adj(S) / det(S) (S >= 2 epsilon I), d = x - q,
 * J = [ -[x]x | I ] (3 x 6, twist order wx wy wz vx vy vz).  m[28] = the upper triangle of sum J^T M J row by row (21), sum J^T M d (6),
 * sum d^T M d (1): the layout of fgoicp_plane_moments_t, so fgoicp_plane_step_from_moments and fgoicp_plane_apply_step serve unchanged
 * (with M = n n^T the terms are the point-to-plane ones).  Every term is even in n_q and in n_p; the sums are added in
 * fgoicp_plane_moments' fixed order (two calls return the same bytes).  Context frame.
 */
int fgoicp_ctx_set_source_normals(fgoicp_ctx* ctx, const float* normals_ns3_or_NULL, int k);
int fgoicp_source_normals(fgoicp_ctx* ctx, float* out_ns3);
/* One evaluation at a fixed pose, as fgoicp_plane_moments.  Refused unless both normal sets are set (the message names the missing
 * setter), for a NaN or negative max_dist2 and for an epsilon outside (0, 1] — all before any device work. */
int fgoicp_gicp_moments(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, double epsilon, fgoicp_plane_moments_t* out);
/* fgoicp_icp_plane's loop, term for term, over fgoicp_gicp_moments.  HERE out->plane_rmse HOLDS sqrt(sum d^T M d / N) at the returned
 * pose — the root mean squared plane-to-plane (Mahalanobis) residual, context frame — not the point-to-plane one.  Leaves the context
 * as it found it. */
int fgoicp_icp_gicp(fgoicp_ctx* ctx, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, double epsilon,
                    fgoicp_plane_result_t* out);
/* Host only, no device needed: the arithmetic of ONE pair, the text the device kernel runs.  x3, q3, nq3, np3: the moved source point, the
 * target point, its normal, the source point's normal (source frame); R9 in glm order.  M6 (optional): M as xx xy xz yy yz zz; v28
 * (optional): the pair's 28 terms.  Refuses null inputs and an epsilon outside (0, 1]. */
int fgoicp_gicp_terms(const float* x3, const float* q3, const float* nq3, const float* np3, const float* R9, double epsilon, double* M6_or_NULL, double* v28_or_NULL);

/*
 * EXTENSION — robust losses for the two refinements (no reference counterpart; Open3D: registration.HuberLoss, CauchyLoss, GMLoss,
 * TukeyLoss): iteratively reweighted least squares.  Every term a counted correspondence contributes to the normal equations is multiplied
 * by w(s), s the correspondence's residual: s = r = n.(x - q) for FGOICP_MODEL_PLANE, s = sqrt(max(d^T M d, 0)) for FGOICP_MODEL_GICP.  The
 * scale c > 0 is fixed for a whole loop.  All arithmetic is fp64 with one rounding per operation, a = |s|:
 *   FGOICP_LOSS_NONE           w = 1
 *   FGOICP_LOSS_HUBER          w = a <= c ? 1 : c / a
 *   FGOICP_LOSS_CAUCHY         u = s / c;  w = 1 / (1 + u * u)
 *   FGOICP_LOSS_GEMAN_MCCLURE  c2 = c * c;  g = c2 / (c2 + s * s);  w = g * g
 *   FGOICP_LOSS_TUKEY          w = a <= c ? (v = 1 - (s / c) * (s / c), v * v) : 0
 * Only + - * / and one sqrt: the host function, the kernel and a float64 restatement agree in every bit.  The rho values are not computed.
 * The counted set, the 28 unweighted terms and the order of every addition are those of fgoicp_plane_moments / fgoicp_gicp_moments; with
 * FGOICP_LOSS_NONE m[28] has the bits of the plain call and weight_sum == correspondences.  Context frame.
 */
enum { FGOICP_LOSS_NONE = 0, FGOICP_LOSS_HUBER = 1, FGOICP_LOSS_CAUCHY = 2, FGOICP_LOSS_GEMAN_MCCLURE = 3, FGOICP_LOSS_TUKEY = 4 };
enum { FGOICP_MODEL_PLANE = 0, FGOICP_MODEL_GICP = 1 };
typedef struct fgoicp_robust_moments_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_robust_moments_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, correspondences; /* ns; the counted correspondences N (a zero weight still counts) */
    double   m[28];                   /* the layout of fgoicp_plane_moments_t, every term times its pair's w */
    double   weight_sum;              /* sum w over the counted */
    float    max_dist2;               /* the threshold the device compared with */
    int      loss;
    double   scale;                   /* as given */
} fgoicp_robust_moments_t;
typedef struct fgoicp_robust_result_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_robust_result_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    float    R[9], t[3];              /* the refined pose (fgoicp_solver_refine_robust: t restored to the callers' frame) */
    int      iterations;              /* steps taken */
    int      rank;                    /* of the last solve (0 when max_iter = 0, nothing was counted or every weight was zero) */
    uint64_t correspondences;         /* counted at the returned pose */
    double   weight_sum;              /* sum w at the returned pose */
    double   rmse;                    /* sqrt(sum w s^2 / sum w) at the returned pose, context frame (0 when the weight sum is 0) */
    float    sse;                     /* == fgoicp_sse(ctx, R, t) at the returned pose, bit for bit (context frame) */
    float    scaling_factor;          /* 1 for a bare context; the solver's scale otherwise */
    int      loss;
    int      scale_estimated;         /* 1: the scale was estimated at the start pose (fgoicp_robust_scale), 0: it was given */
    double   scale;                   /* the scale the loop ran with, context frame (/ scaling_factor: callers' units) */
} fgoicp_robust_result_t;
/* Host only, no device: *w = w(s).  Refuses a null w, an unknown loss, a non-finite s and, except for FGOICP_LOSS_NONE, a scale that is
 * not finite and positive; a refusal leaves *w untouched. */
int fgoicp_robust_weight(int loss, double s, double scale, double* w);
/* One evaluation at a fixed pose, as fgoicp_plane_moments (model 0) / fgoicp_gicp_moments (model 1; epsilon is ignored by model 0).
 * Refuses what those refuse and an unknown loss or model and a bad scale (FGOICP_LOSS_NONE ignores the scale), all before any device
 * work.  Leaves the context as it found it.  Two calls return the same bytes. */
int fgoicp_robust_moments(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, int model, double epsilon, int loss, double scale,
                          fgoicp_robust_moments_t* out);
/* The same evaluation per point, caller order, ns entries each: residual s, weight w(s), counted 0 / 1; an uncounted point gets 0, 0, 0.
 * Any of the arrays may be NULL. */
int fgoicp_robust_residuals(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, int model, double epsilon, int loss, double scale,
                            double* residual_ns, double* weight_ns, unsigned char* counted_ns);
/* The automatic scale at (R, t): 1.4826 * sorted(|s| over the N counted)[(N - 1) / 2] — the lower median, one fp64 product.  Refused
 * (FGOICP_ERR_INVALID_ARG, the message says to pass a scale) when nothing is counted or that median is 0. */
int fgoicp_robust_scale(fgoicp_ctx* ctx, const float* R9, const float* t3, float max_dist2, int model, double epsilon, double* scale);
/* fgoicp_icp_plane's / fgoicp_icp_gicp's loop, term for term, over fgoicp_robust_moments: the stop band, the rank-deficient first
 * step, the evaluation at the returned pose.  scale <= 0: estimated once at (R0, t0).  It also ends when the weight sum is 0 (every
 * counted pair beyond a Tukey scale): the pose is then the one that evaluation was made at.  With FGOICP_LOSS_NONE R, t, iterations, rank
 * and sse are the plain loop's.  Leaves the context as it found it. */
int fgoicp_icp_robust(fgoicp_ctx* ctx, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float max_dist2, int model, double epsilon,
                      int loss, double scale, fgoicp_robust_result_t* out);

/* Replaces IterativeClosestPoint3D(reg, pct, pcs, max_iter, thr, R, t) + run()
 * (fgoicp/icp3d.hpp:30-35, icp3d.cu:55-108).  Returns the reference's Result_t {sse, R, t}
 * plus the number of loop iterations executed. */
int fgoicp_icp(fgoicp_ctx* ctx, const float* R0_9, const float* t0_3, size_t max_iter, float conv_thr, float* sse_out,
               float* R_out9, float* t_out3, int* iters_out);
/* n IterativeClosestPoint3D objects (fgoicp.cpp:76-77 creates and runs one per promising rotation cube) run at once.  Run i starts from R0s_9[9i..], t0s_3[3i..] and is exactly the run
 * fgoicp_icp would do; runs share the device through per-run scratch and streams (an ICP iteration is a chain of small
 * kernels: below ~100k points one run fills a fraction of the device). */
int fgoicp_icp_batch(fgoicp_ctx* ctx, int n, const float* R0s_9, const float* t0s_3, size_t max_iter, float conv_thr, float* sse_out,
                     float* R_out9s, float* t_out3s, int* iters_out);
/* One IterativeClosestPoint3D::procrustes() step (icp3d.cu:140-172) on an explicit working cloud
 * (ns x xyz, caller order).  Test hook: optional outputs may be NULL.  In trimmed mode corr_idx is 0x7fffffff for points
 * that provably lie outside the inlier set (they take no part in the step and their exact neighbour is not searched). */
int fgoicp_procrustes(fgoicp_ctx* ctx, const float* working_xyz, float* R_out9, float* t_out3, float* centroids6,
                      float* ABt9, int* corr_idx);

/*
 * EXTENSION — trimmed Go-ICP.  The reference parses `params.trim` (src/utilities.hpp:94) but never uses it, so
 * there is no reference behaviour; this follows Yang et al.'s Go-ICP: with k inliers every sum over source
 * points (bounds, SSE, the Procrustes means) runs over the k smallest per-point terms.  k = 0 or k >= ns: off.
 */
int fgoicp_ctx_set_inliers(fgoicp_ctx* ctx, size_t k);

/*
 * Trimmed mode only (diagnostic): the per-point quantity behind one subcube's bounds, in caller order —
 * e_i = max(d_i, 0) with d_i the value of `distance` at registration.cu:48-52 (after the rotation-uncertainty term when
 * fix_rot == 0); the reference's per-point outputs are ub_i = e_i^2 (:54) and lb_i = max(e_i - sqrt3*span, 0)^2 (:57-58).
 */
int fgoicp_bounds_point_distances(fgoicp_ctx* ctx, const float* R9, float rot_span, const float* tnode4, int fix_rot, float* e_out);

/* Sorted ticks so far and how many of them had to be repeated because the on-device check found that the locality sort had not
 * produced a permutation of the work items (then the context switches to device-scope atomics for good). */
int fgoicp_ctx_sort_fallbacks(const fgoicp_ctx* ctx, uint64_t* sorted_ticks, uint64_t* fallbacks);
/* TEST HOOK, not part of the drop-in surface: spoils the nth_tick-th sorted tick from now (0 = off) so that the permutation check
 * above has something to find.  (Round 2 read this from the environment of the shipped library) */
int fgoicp_ctx_test_sort_fault(fgoicp_ctx* ctx, int nth_tick);
/* TEST HOOK, not part of the drop-in surface: what the library's owning handles hold in this process right now — out4 = {device
 * allocations, pinned host allocations, streams, events}.  Contexts, batches and the one-shot calls release through those handles, so the
 * counts return to where they were once an object is destroyed or a call has returned.  Needs no device. */
int fgoicp_test_live_resources(uint64_t out4[4]);

/* Accumulated HIP-event timing of the bounds kernel since the last reset (FGOICP_FLAG_PROFILE):
 * kernel_ms = sum of launch durations, launches = kernel launches, subcubes = (rot, trans) pairs. */
int fgoicp_ctx_profile(fgoicp_ctx* ctx, double* kernel_ms, uint64_t* launches, uint64_t* subcubes, int reset);
/* Evaluations behind those subcubes since the last reset: a twin pair (fgoicp_bounds_submit_twins) is two subcubes and one
 * evaluation.  Read it before the fgoicp_ctx_profile call that resets. */
int fgoicp_ctx_profile_evaluations(fgoicp_ctx* ctx, uint64_t* evaluations);
/* Trimmed mode: accumulated duration of the selection kernel (one launch per window, next to the bounds kernel) since the last
 * reset by fgoicp_ctx_profile — read it before that call. */
int fgoicp_ctx_profile_select_ms(fgoicp_ctx* ctx, double* select_ms);
/* Trimmed mode (EXTENSION): how the per-row selections of the bounds went since the last reset — out3 = {rows selected, rows whose
 * sampled bracket failed its exact check and that were done again in two passes, bracket members gathered}.  No submission may
 * be in flight. */
int fgoicp_ctx_trim_stats(fgoicp_ctx* ctx, uint64_t* out3, int reset);
/* Multi-rank runs: from how many source points a cooperative refinement (fgoicp_exchange.allgather_device) splits its exact scans over the
 * ranks instead of running replicated on every rank.  Defaults: untrimmed never ((size_t)-1: measured no faster at 437k points on 8 ranks),
 * trimmed contexts from 262 144 points (their iterations are long: 8-rank replay 1.84x -> 2.69x).  A deployment choice (it trades an
 * in-place device all-gather of 4 B per source point, twice per ICP iteration, against the replicated scan), hence an option, not a knob. */
int fgoicp_ctx_set_coop_split(fgoicp_ctx* ctx, size_t min_points_untrimmed, size_t min_points_trimmed);
/* Turns the HIP-event bracketing on or off at run time (events are created on first use). */
int fgoicp_ctx_set_profile(fgoicp_ctx* ctx, int enabled);
size_t fgoicp_ctx_ns(const fgoicp_ctx* ctx);
size_t fgoicp_ctx_nt(const fgoicp_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Driver level: icp::FastGoICP (fgoicp/fgoicp.hpp:13-43, fgoicp/fgoicp.cpp:10-287)
 * ------------------------------------------------------------------------------------------ */
typedef struct fgoicp_solver fgoicp_solver;

typedef enum fgoicp_schedule {
    FGOICP_SCHEDULE_SERIAL = 0, /* the reference's exact exploration order (fgoicp.cpp:32-174)       */
    FGOICP_SCHEDULE_ROUND  = 1  /* expansion rounds: pop K cubes, evaluate all children concurrently  */
} fgoicp_schedule;

/*
 * Exchange hook for the sharded outer BnB (one process per GPU).  Called once per expansion
 * round on every rank, from the thread that called fgoicp_solver_run:
 *   allreduce_min(buf, n, user)            — in-place element-wise MIN over ranks (RCCL all-reduce)
 *   allgather(send, recv, n_per_rank, user)— recv[r*n .. (r+1)*n) = rank r's send[0..n)
 * Both return 0 on success.
 */
typedef struct fgoicp_exchange {
    size_t struct_size;  /* sizeof(fgoicp_exchange) as the caller was compiled (ABI 2): members beyond it are taken as NULL / 0, so a struct from an older
                            header (without allgather_device, say) never hands the library a garbage pointer; 0 is refused */
    int rank;
    int world_size;
    int (*allreduce_min)(float* buf, size_t n, void* user);
    int (*allgather)(const float* send, float* recv, size_t n_per_rank, void* user);
    void* user;
    /* Optional (NULL = off).  In-place all-gather on DEVICE memory of the calling rank's context: on return
     * device_buf[r * bytes_per_rank .. (r + 1) * bytes_per_rank) holds rank r's chunk, for every r (RCCL: ncclAllGather with
     * sendbuff = recvbuff + rank * count).  With it a round's refinements become COOPERATIVE: the child bounds are exchanged first,
     * every rank applies the trigger rule of fgoicp.cpp:74-88 to ALL children in the single-GPU order, and each triggered
     * IterativeClosestPoint3D::run() is executed by all ranks together — every rank scans 1/world of the source for the two exact
     * nearest-neighbour passes of an iteration, the per-query results (4 B each) are all-gathered through this hook, the sums and the
     * SVD are replicated.  Results are the single-GPU bits on every rank.  Called twice per ICP iteration, from the thread that
     * called fgoicp_solver_run; the context's streams are idle during the call. */
    int (*allgather_device)(void* device_buf, size_t bytes_per_rank, void* user);
} fgoicp_exchange;

typedef struct fgoicp_solver_opts {
    int schedule;        /* fgoicp_schedule                                            */
    int round_width;     /* ROUND: rotation cubes popped per expansion round (K >= 1); 0 = adaptive: 32 per rank,
                            doubled after every round that does not improve the incumbent, reset when one does */
    unsigned ctx_flags;  /* FGOICP_FLAG_*                                              */
    int device;          /* HIP device ordinal                                         */
    float trim_fraction; /* EXTENSION: fraction of source points treated as outliers (0 = the reference's behaviour) */
} fgoicp_solver_opts;

typedef struct fgoicp_run_stats {
    uint64_t trans_cubes;   /* (rot, trans) subcubes evaluated = `count` of fgoicp.cpp:108,132 */
    uint64_t bounds_calls;  /* bounds-operator submissions                                      */
    uint64_t rot_cubes;     /* rotation cubes that went through branch_and_bound_R3             */
    uint64_t icp_runs;
    uint64_t icp_iters;
    uint64_t inner_bnb;
    uint64_t rounds;        /* expansion rounds (ROUND) / popped rotation nodes (SERIAL)        */
    double   seconds_total; /* wall-clock of run()                                              */
    double   seconds_bnb;   /* of which: outer BnB phase                                        */
    double   seconds_icp;   /* of which: inside ICP                                             */
    double   initial_icp_sse; /* error of the initial ICP from identity (fgoicp.cpp:12-17)        */
} fgoicp_run_stats;

/* Replaces FastGoICP::FastGoICP(pct, pcs, lut_resolution, mse_threshold) (fgoicp.hpp:13-25):
 * centre, scale, bounds (fgoicp.cpp:176-287), then the Registration constructor. */
int fgoicp_solver_create(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, float lut_resolution,
                         float mse_threshold, const fgoicp_solver_opts* opts, fgoicp_solver** out);
void fgoicp_solver_destroy(fgoicp_solver* s);
/* Installs the multi-GPU exchange (NULL = single process). */
int fgoicp_solver_set_exchange(fgoicp_solver* s, const fgoicp_exchange* ex);
/* The log lines FastGoICP::run() and branch_and_bound_SO3 emit while they run (fgoicp.cpp:15-17, :85-87), as a callback on the thread
 * that called fgoicp_solver_run:
 *   FGOICP_LOG_INITIAL_ICP  once, after the initial ICP: its (sse, R, t) as it returned them (t in the solver's scaled frame, as the
 *                           reference prints it);
 *   FGOICP_LOG_NEW_BEST     after EVERY refinement the search triggers (improved or not, as the reference): the incumbent's error and
 *                           rotation and its translation RESTORED to the callers' frame (restore_translation, fgoicp.hpp:87-90).
 * Under FGOICP_SCHEDULE_SERIAL the events come in the reference's order.  cb = NULL removes the hook.  icp::FastGoICP (include/fgoicp/
 * fgoicp.hpp) installs one that prints the reference's lines through icp::Logger. */
enum { FGOICP_LOG_INITIAL_ICP = 0, FGOICP_LOG_NEW_BEST = 1 };
typedef void (*fgoicp_log_fn)(int event, float sse, const float* R9, const float* t3, void* user);
int fgoicp_solver_set_log(fgoicp_solver* s, fgoicp_log_fn cb, void* user);
/* on = 1 (default): the inner branch-and-bounds hand their thresholds to the bounds operator (fgoicp_bounds_submit_cut); 0: every
 * subcube is evaluated in full, as the reference does.  Same trajectory, counters and result either way. */
int fgoicp_solver_set_early_exit(fgoicp_solver* s, int on);
/* Replaces FastGoICP::run() (fgoicp.cpp:10-30): returns R and the restored translation
 * (fgoicp.hpp:87-90). */
int fgoicp_solver_run(fgoicp_solver* s, float* R_out9, float* t_out3);
/* Replaces get_best_error / get_best_transform / get_last_transform (fgoicp.hpp:33-43);
 * translations here are in the solver's scaled frame, as in the reference. */
int fgoicp_solver_best_error(const fgoicp_solver* s, float* sse_out);
int fgoicp_solver_best_transform(const fgoicp_solver* s, float* R9, float* t3);
int fgoicp_solver_last_transform(const fgoicp_solver* s, float* R9, float* t3);
int fgoicp_solver_stats(const fgoicp_solver* s, fgoicp_run_stats* out);
/* EXTENSION: fgoicp_alignment at the best transform the solver holds (the normalised one, before restore_translation), after a
 * successful fgoicp_solver_run — before that the call is refused (FGOICP_ERR_INVALID_ARG).  Indices and masks refer to the clouds as
 * handed to fgoicp_solver_create; distances are in the solver's centred and scaled frame, out->scaling_factor is its scale.  A later
 * fgoicp_solver_run returns what it returned before.  On a multi-GPU run every rank answers from its own context. */
int fgoicp_solver_alignment(fgoicp_solver* s, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns, uint8_t* target_hit_nt,
                            fgoicp_alignment_summary* out);
/* EXTENSION: fgoicp_information at the best transform the solver holds, in the callers' frame, after a successful fgoicp_solver_run —
 * before that the call is refused (FGOICP_ERR_INVALID_ARG).  max_distance: callers' units, +inf = no threshold, NaN and negative values
 * refused.  A later fgoicp_solver_run returns what it returned before. */
int fgoicp_solver_information(fgoicp_solver* s, float max_distance, fgoicp_information_t* out);
/* EXTENSION: fgoicp_icp_plane from the best transform the solver holds, after a successful fgoicp_solver_run — before that the call is
 * refused (FGOICP_ERR_INVALID_ARG).  If the context has no normals yet they are estimated with k neighbours (normals are invariant under
 * the solver's centring and uniform scale).  max_distance: callers' units, converted as fgoicp_solver_information converts it
 * (ds = (float)max_distance * scale; max_dist2 = ds * ds); +inf = no threshold.  out->R and out->t: the refined pose in the CALLERS' frame
 * (the translation restored as fgoicp_solver_run restores it); plane_rmse and sse stay in the solver's frame (scaling_factor converts).
 * The solver's own best transform, best error and a later fgoicp_solver_run are untouched.  On a multi-GPU run every rank answers from
 * its own context. */
int fgoicp_solver_refine_plane(fgoicp_solver* s, int k, size_t max_iter, float conv_thr, float max_distance, fgoicp_plane_result_t* out);
/* EXTENSION: fgoicp_icp_gicp from the best transform the solver holds, after a successful fgoicp_solver_run — before that the call is
 * refused (FGOICP_ERR_INVALID_ARG).  Whichever normal set the context lacks is estimated with k neighbours (normals are invariant under
 * the solver's centring and uniform scale).  max_distance, R, t and scaling_factor as fgoicp_solver_refine_plane; plane_rmse holds
 * sqrt(sum d^T M d / N) in the solver's frame.  The solver's own result is untouched. */
int fgoicp_solver_refine_gicp(fgoicp_solver* s, int k, size_t max_iter, float conv_thr, float max_distance, double epsilon, fgoicp_plane_result_t* out);
/* EXTENSION: fgoicp_icp_robust from the best transform, as the two calls above (model FGOICP_MODEL_PLANE / FGOICP_MODEL_GICP; normals
 * estimated with k where they are not set).  max_distance and loss_scale are in the CALLERS' units (x scaling_factor inwards;
 * loss_scale <= 0: estimated); t is restored to the callers' frame; rmse, sse and scale stay in the solver's frame (scaling_factor
 * converts).  The solver's best transform is left alone. */
int fgoicp_solver_refine_robust(fgoicp_solver* s, int model, int k, size_t max_iter, float conv_thr, float max_distance, double epsilon, int loss, double loss_scale,
                                fgoicp_robust_result_t* out);
/* Pre-processing results (tests): offs6 = {offset_pcs, offset_pct}, bounds6 as in ctx_create. */
int fgoicp_solver_preproc(const fgoicp_solver* s, float* offs6, float* scale, float* bounds6);
/* Statistics of a raw cloud, host side, no device needed (TODO.md:7 of the reference: "compute point clouds' stats"): what the
 * pre-processing (fgoicp.cpp:176-287) derives its centring and scaling from, plus the spread.  Sums in double. */
typedef struct fgoicp_cloud_stats_t {
    uint64_t n;
    float centroid[3];
    float min[3], max[3];        /* axis-aligned bounding box */
    float max_abs_centred;       /* max_i max(|x_i - c_x|, |y_i - c_y|, |z_i - c_z|): 1 / this is the scale of fgoicp.cpp:205-220 when taken over the source */
    float rms_radius;            /* sqrt(mean |p_i - c|^2) */
} fgoicp_cloud_stats_t;
int fgoicp_cloud_stats(const float* xyz, size_t n, fgoicp_cloud_stats_t* out);
/*
 * EXTENSION — voxel-grid downsampling on the device (no reference counterpart: the reference thins a cloud only in its loaders, keeping each
 * point with probability p; Open3D: voxel_down_sample, PCL: VoxelGrid).  The first step of a registration pipeline: one point per occupied
 * cell of a regular grid, so the cloud comes to an even density, reproducibly.
 *
 * Inputs: n points (fp32 xyz triples), voxel_size v > 0, optionally an origin o of 3 floats; with NULL, o is the per-axis minimum of the cloud.
 *   cell of a point   per axis c = floor(((double)p - (double)o) / (double)v), the subtraction and the division in IEEE fp64 (no reciprocal,
 *                     no fp32, no fast-math: numpy's float64 arithmetic names the same cell for every point, those on a cell face included)
 *   key               (cz << 42) | (cy << 21) | cx
 *   output rows       one per occupied cell in ascending key order (z-major, then y, then x): count_per_voxel = the members, out_xyz = the
 *                     centroid — fp64 sums of the member coordinates (fp32 -> fp64 is exact) divided by the count in fp64 and rounded to
 *                     fp32 once.  The sums are a function of the input array alone (a fixed order, no floating-point atomics, no dependence
 *                     on timing): two calls on the same input return the same bytes
 *   voxel_of_point_n  per input point, the output row it fell into
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (a host pass over the cloud, as fgoicp_cloud_stats): a null xyz or n == 0,
 * n >= 2^31, a v that is not a positive finite number, a non-finite coordinate or origin, a null `out` or a struct_size that ends before
 * max_points_per_voxel, and any c outside [0, 2^21) — a point below a given origin, or an extent of more than 2^21 cells: the voxel size is
 * too small for the extent.  No usable device: FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure: FGOICP_ERR_OOM.
 * out_xyz (3 floats per row) and count_per_voxel hold capacity_points rows; each of the three arrays may be NULL (all NULL: count only).  If
 * out_xyz or count_per_voxel is given and capacity_points < voxels the call returns FGOICP_ERR_TOO_LARGE with `out` filled, so a second call
 * can be sized, and writes nothing to the arrays; a capacity of n always suffices.
 * The call owns its stream and its device memory (about 70 bytes per point) and frees both before it returns; it touches no fgoicp_ctx and
 * no global state and may be called from several threads.
 */
typedef struct fgoicp_voxel_info_t {
    uint32_t struct_size;          /* IN: sizeof(fgoicp_voxel_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, voxels;       /* n; occupied cells */
    uint64_t max_points_per_voxel;
    float    origin[3], voxel_size;/* the origin actually used */
} fgoicp_voxel_info_t;
int fgoicp_voxel_downsample(const float* xyz, size_t n, float voxel_size, const float* origin3_or_NULL, int device,
                            float* out_xyz, size_t capacity_points,
                            uint32_t* voxel_of_point_n, uint32_t* count_per_voxel,
                            fgoicp_voxel_info_t* out);
/*
 * EXTENSION — outlier removal on the device (no reference counterpart; Open3D: remove_statistical_outlier(nb_neighbors, std_ratio) and
 * remove_radius_outlier(nb_points, radius), PCL: StatisticalOutlierRemoval and RadiusOutlierRemoval).  The step of a registration pipeline
 * between downsampling and normals / registration: stray points of a TARGET cannot be trimmed away later.
 *
 * The list L_i of point i (caller order): the k smallest keys (bits(d2_ij) << 32) | j over ALL j, i itself included (the convention of
 * fgoicp_target_knn and of Open3D's search_knn), d2_ij the scans' fp32 dist_sq(p_i, p_j) = fma(dz, dz, fma(dy, dy, dx * dx)); a tie at the
 * cut goes to the lowest caller index.  2 <= k <= 32, k <= n.
 *   kth_dist2[i]  the fp32 d2 of the last entry of L_i
 *   mean_dist[i]  (the sum over L_i, in list order, of sqrt((double)d2)) / (double)k: IEEE fp64 square roots, additions and one division
 * FGOICP_OUTLIER_STATISTICAL (param = std_ratio, finite and >= 0): mean = (sum_i mean_dist[i]) / n, stddev = sqrt(sum_i (mean_dist[i] - mean)^2
 *   / (n - 1)) (the sample form, as Open3D; 0 for n == 1), both fp64 with every addition in an order that is a function of n alone (no
 *   floating-point atomics); threshold = mean + (double)param * stddev, formed on the host, unfused; keep[i] = mean_dist[i] <= threshold,
 *   compared with the very value `out` reports.
 * FGOICP_OUTLIER_RADIUS (param = the radius, finite and > 0): radius2 = param * param in fp32; keep[i] = kth_dist2[i] <= radius2 — a point
 *   stays when at least k points of the cloud, itself included, lie within the radius.
 * Output rows: the kept points in caller order, bits verbatim; kept_index[r] = the caller index of row r.  keep_n (n bytes, 0 / 1),
 * mean_dist_n (n doubles) and kth_dist2_n (n floats) are per input point.  Every array pointer may be NULL (all NULL: count only).
 * out_xyz (3 floats per row) and kept_index hold capacity_points rows; if either is given and capacity_points < kept the call returns
 * FGOICP_ERR_TOO_LARGE with `out` filled, so a second call can be sized, and writes nothing to the arrays; a capacity of n always suffices.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (a host pass over the cloud): a null xyz or n == 0, n >= 2^31, an unknown mode,
 * k outside [2, 32] or above n, a bad param, a non-finite coordinate, a null `out` or a struct_size that ends before radius2.  No usable
 * device: FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure: FGOICP_ERR_OOM.
 * Two calls on the same input return the same bytes in every output.  The call owns its stream and its device memory (about 70 bytes per
 * point) and frees both before it returns; it touches no fgoicp_ctx and no global state and may be called from several threads.
 */
enum { FGOICP_OUTLIER_STATISTICAL = 0, FGOICP_OUTLIER_RADIUS = 1 };
typedef struct fgoicp_outlier_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_outlier_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, kept;       /* n; rows of the output */
    int      mode, k;
    double   mean, stddev;       /* STATISTICAL: of mean_dist over the cloud; RADIUS: 0 */
    double   threshold;          /* STATISTICAL: the value mean_dist was compared with; RADIUS: 0 */
    float    radius2;            /* RADIUS: the fp32 value kth_dist2 was compared with; STATISTICAL: 0 */
} fgoicp_outlier_info_t;
int fgoicp_remove_outliers(const float* xyz, size_t n, int mode, int k, float param, int device,
                           float* out_xyz, size_t capacity_points, uint32_t* kept_index,
                           uint8_t* keep_n, double* mean_dist_n, float* kth_dist2_n,
                           fgoicp_outlier_info_t* out);
/*
 * EXTENSION — farthest-point sampling on the device (no reference counterpart: the reference thins a cloud only in its loaders; Open3D:
 * farthest_point_down_sample(num_samples, start_index), PCL: FarthestPointSampling).  Sets the NUMBER of points of a cloud — what the run time
 * of a search is proportional to — where the voxel grid sets a density: exactly m points, spread as evenly as m points can be, and every
 * prefix of the result is the sampling of that size.
 *
 * Inputs: n points (fp32 xyz triples, caller order), 1 <= m <= n, 0 <= start_index < n.
 *   d2(i, j)      the scans' fp32 dist_sq(p_i, p_j) = fma(dz, dz, fma(dy, dy, dx * dx)), the differences formed in fp32
 *   D_0[i] = +inf, c_0 = start_index; after pick c_t: D_{t+1}[i] = min(D_t[i], d2(i, c_t)), and owner[i] = t whenever that minimum strictly
 *                 decreased at step t (a tie keeps the earlier sample; owner starts at 0)
 *   c_{t+1}       the point not picked so far with the largest D_{t+1}, a tie to the lowest caller index — the largest 64-bit key
 *                 (bits(D) << 32) | (0xFFFFFFFF - i) over the unpicked points.  A picked point never wins, also when every remaining point
 *                 is a copy of a picked one (D = 0 everywhere): the call returns m distinct indices, and m = n a permutation of the cloud
 * Outputs, every array pointer may be NULL (all NULL: `out` alone); all m rows are always written, there is no capacity argument:
 *   sample_index_m  the picks c_0 .. c_{m-1} in pick order         out_xyz_m3    those points, bits verbatim, in pick order
 *   pick_dist2_m    D_t[c_t] at the moment of the pick, +inf for the first; non-increasing
 *   min_dist2_n     the final D: squared distance to the nearest sample, +0.0 for a sample itself
 *   owner_n         the position in sample_index of that nearest sample
 *   out             cover_dist2 = max_i min_dist2[i], the squared cover radius; next_index = the point that attains it under the tie rule, what
 *                   pick m + 1 would be.  m == n: next_index = n, cover_dist2 = 0
 * Nothing is summed: the outputs are a function of the input alone, two calls return the same bytes.
 * Cost: m DEPENDENT steps over the n points, one kernel launch each (each reads 16 bytes per point); device memory 16 bytes per point, plus
 * 4 for each of min_dist2_n and owner_n when asked.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (one host pass over the cloud): a null xyz or n == 0, n >= 2^31, m == 0 or m > n,
 * start_index >= n, a non-finite coordinate (the message names its index), a null `out` or a struct_size that ends before cover_dist2 or is
 * above 4096.  No usable device: FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure: FGOICP_ERR_OOM.
 * The call owns its stream and its one device allocation and frees both before it returns; it touches no fgoicp_ctx, no global state and no
 * knob and may be called from several threads.
 */
typedef struct fgoicp_fps_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_fps_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points, samples;    /* n, m */
    uint64_t start_index;
    uint64_t next_index;         /* what pick m + 1 would be; n when m == n */
    float    cover_dist2;        /* max_i min_dist2[i] */
} fgoicp_fps_info_t;
int fgoicp_farthest_point_sample(const float* xyz, size_t n, size_t m, size_t start_index, int device,
                                 float* out_xyz_m3, uint32_t* sample_index_m, float* pick_dist2_m,
                                 float* min_dist2_n, uint32_t* owner_n, fgoicp_fps_info_t* out);
/*
 * EXTENSION — density clustering on the device (no reference counterpart; Open3D: cluster_dbscan(eps, min_points) followed by "keep the
 * largest label", PCL: EuclideanClusterExtraction, which is the min_points = 1 case).  Removes what the outlier filter cannot: a detached
 * CLUMP of points — a piece of the fixture, a second object, a blob of ghost returns — whose members are each other's close neighbours.
 *
 * Inputs: n points (fp32 xyz triples, caller order), eps finite and > 0, min_points >= 1, keep_min_size.
 *   d2(i, j)       the scans' fp32 dist_sq(p_i, p_j) = fma(dz, dz, fma(dy, dy, dx * dx)), the differences formed in fp32: symmetric in its
 *                  arguments and 0 on the diagonal, both to the bit.  eps2 = eps * eps in fp32
 *   neighbours[i]  #{ j : d2(i, j) <= eps2 }, the point itself counted; the comparison is <= on fp32
 *   core[i]        neighbours[i] >= min_points
 *   cluster        a connected component of the graph on the CORE points with an edge wherever d2 <= eps2.  Clusters are numbered
 *                  0 .. clusters - 1 in ascending order of their lowest caller index among core members
 *   border point   a point that is not core and has at least one core neighbour: it gets the label of the core neighbour with the smallest key
 *                  (bits(d2) << 32) | caller index — the total order of fgoicp_target_knn, a tie goes to the lowest index
 *   noise          every other point: label -1
 *   cluster_size[c]  the number of points labelled c, core and border together; the LARGEST cluster is the one of greatest size, a tie going
 *                  to the lowest label
 *   kept           keep_min_size == 0: the points of the largest cluster; keep_min_size >= 1: the points of every cluster of at least that
 *                  many points (1: all but noise).  Noise is never kept; no cluster at all keeps nothing (kept = 0, FGOICP_OK)
 * min_points = 1 makes every point core: plain Euclidean cluster extraction.
 * DIFFERS from Open3D and scikit-learn in the border points only: they give a border point to whichever cluster reaches it first, which
 * depends on the order of their scan; here the nearest core neighbour decides, so the result is a function of the input alone and two calls
 * return the same bytes in every output.  (The components come out of concurrent integer atomics on the device, yet their fixed point —
 * every component's root is its lowest caller index — does not depend on how those interleave; `rounds` may.)
 * Outputs, every array pointer may be NULL (all NULL: `out` alone):
 *   out_xyz / kept_index  the kept points in caller order, bits verbatim, and their caller indices; both hold capacity_points rows
 *   label_n (n int32)     neighbours_n (n uint32)     cluster_size (capacity_clusters uint64, `clusters` of them written)
 * If out_xyz or kept_index is given and capacity_points < kept, or cluster_size is given and capacity_clusters < clusters, the call returns
 * FGOICP_ERR_TOO_LARGE with `out` filled, so a second call can be sized, and writes nothing to any array; n always suffices for either.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (one host pass over the cloud): a null xyz or n == 0, n >= 2^31, a non-finite
 * coordinate (the message names the point), eps not finite or not > 0, min_points < 1, a null `out` or a struct_size that is 0, ends before
 * `rounds` or is above 4096, a device ordinal out of range.  No usable device: FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure:
 * FGOICP_ERR_OOM.  The call owns its stream and its one device allocation (about 100 bytes per point) and frees both before it returns; it
 * touches no fgoicp_ctx, no global state and no knob and may be called from several threads.
 */
typedef struct fgoicp_cluster_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_cluster_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points;             /* n */
    uint64_t core_points, border_points, noise_points;
    uint64_t clusters;
    int64_t  largest_label;      /* -1: no cluster */
    uint64_t largest_size;
    uint64_t kept;               /* rows of the output */
    uint64_t keep_min_size;
    int      min_points;
    float    eps2;               /* the fp32 value every d2 was compared with */
    uint32_t rounds;             /* hook-and-compress rounds of the connected-components pass, the last one (which changed nothing) included */
} fgoicp_cluster_info_t;
int fgoicp_cluster_dbscan(const float* xyz, size_t n, float eps, int min_points, size_t keep_min_size, int device,
                          float* out_xyz, size_t capacity_points, uint32_t* kept_index,
                          int32_t* label_n, uint32_t* neighbours_n, uint64_t* cluster_size, size_t capacity_clusters,
                          fgoicp_cluster_info_t* out);
/*
 * EXTENSION — plane segmentation on the device by RANSAC (no reference counterpart; Open3D: segment_plane(distance_threshold, ransac_n = 3,
 * num_iterations), PCL: SACSegmentation with SACMODEL_PLANE).  Removes what makes the cluster filter useless on a real scan: the SUPPORT
 * PLANE — the table under an object, the floor of a room — which joins everything that stands on it into one connected component.
 * ("segment": fgoicp_plane_* is the point-to-plane refinement.)
 *
 * Inputs: n points (fp32 xyz triples, caller order), distance_threshold finite and > 0, K = iterations in [1, 65536], seed, max_planes in
 * [1, 16], min_inliers, refit, keep_planes.  ALL arithmetic is IEEE fp64 on the fp32 coordinates converted to double, every operation rounded
 * on its own in the order written — no contraction, no reciprocal — so numpy's float64 names the same inlier set for every point, those
 * exactly at the threshold included.  T = (double)distance_threshold.  Every point starts with label -1.
 *   peel j         j = 0, 1, ... < max_planes works on the candidates R_j: the caller indices whose label is still -1, ascending, m_j of
 *                  them.  Peeling stops with no plane j when m_j < 3
 *   hypothesis h   h = 0 .. K - 1 of peel j draws three numbers, s = 0, 1, 2, everything mod 2^64:
 *                    u_s = mix64(seed + 0x9E3779B97F4A7C15 * ((j * K + h) * 3 + s + 1))
 *                    mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *                  (the splitmix64 finaliser) and its sample s is R_j[((u_s >> 32) * m_j) >> 32] (the product is below 2^63: n < 2^31).
 *                  Counter based: any hypothesis can be formed alone
 *   plane          a, b, c = the three sample points;  e1 = b - a, e2 = c - a;
 *                  N = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);  L2 = (Nx*Nx + Ny*Ny) + Nz*Nz;
 *                  (nx, ny, nz) = N / sqrt(L2), three divisions;  d = -((nx*ax + ny*ay) + nz*az).  The sign is the cross product's
 *   degenerate     two of the three samples are the same index, or L2 is not a positive finite number: the hypothesis counts 0 inliers,
 *                  never wins, and its plane is reported as four +0.0
 *   score          r_i = ((nx*x_i + ny*y_i) + nz*z_i) + d;  count_h = #{ i in R_j : |r_i| <= T }, the comparison is <= on fp64.  The winner
 *                  has the largest count, a tie goes to the lowest h.  Peeling stops with no plane j when the winner's count is below
 *                  max(min_inliers, 3)
 *   refit          (refit != 0) pivot = the winner's first sample a; for every inlier of the winner u = p - a; nine sums, sum_u[3] and
 *                  sum_uu[6] in the order xx xy xz yy yz zz, in the fixed order of the moment kernels: the term of caller index i sits at
 *                  position i of an n-vector, every other position adds +0.0, blocks of 256 (oracle/np_restatement.py fixed_order_sum).
 *                  The host forms mean = sum_u / count, C = sum_uu / count - mean mean^T, the unit eigenvector of C's smallest eigenvalue by
 *                  symmetric Jacobi sweeps in fp64, flipped so that its dot product with the hypothesis normal is >= 0, and
 *                  d = -((nx*qx + ny*qy) + nz*qz) with q = a + mean (fgoicp_segment_fit_from_moments).  The final inliers of plane j are
 *                  the i in R_j with |r_i| <= T under the refitted plane.  refit == 0: the hypothesis plane and its inliers are final, the
 *                  sums are reported as zero
 *   label          the final inliers of plane j get label j
 *   rows           keep_planes == 0: the points with label -1 (the rest: what a pipeline wants); keep_planes != 0: those with label >= 0.
 *                  Caller order, bits verbatim
 * The counts are integers and the sums have one order, so the outputs are a function of the input and the seed alone: two calls return the
 * same bytes.  n < 3 is a valid call that finds no plane.
 * Outputs, every array pointer may be NULL (all NULL: `out` alone):
 *   out_xyz / kept_index  the rows and their caller indices; both hold capacity_points rows
 *   label_n (n int32)     models (capacity_models entries of model_size bytes each, `planes` of them written)
 * model_size = sizeof(fgoicp_segment_model_t) as the CALLER was compiled: entry j starts at byte j * model_size and no byte beyond
 * min(model_size, the library's size) of it is written.  If out_xyz or kept_index is given and capacity_points < kept, or models is given
 * and capacity_models < planes, the call returns FGOICP_ERR_TOO_LARGE with `out` filled, so a second call can be sized, and writes nothing to
 * any array; n points and max_planes models always suffice.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (one host pass over the cloud): a null xyz or n == 0, n >= 2^31, a non-finite
 * coordinate (the message names the point), a threshold that is not finite or not > 0, iterations or max_planes out of range, a null `out`
 * or a struct_size that is 0, ends before `distance_threshold` ends or is above 4096, models given with model_size 0, a device ordinal out
 * of range.  No usable device: FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure: FGOICP_ERR_OOM.  The call owns its stream and its
 * one device allocation (about 40 bytes per point and 36 per hypothesis) and frees both before it returns; it touches no fgoicp_ctx, no
 * global state and no knob and may be called from several threads.
 */
typedef struct fgoicp_segment_model_t {
    uint64_t candidates;                   /* m_j */
    uint32_t sample[3];                    /* the winner's three caller indices; sample[0] is the refit's pivot */
    uint32_t hypothesis;                   /* the winning h */
    uint64_t hypothesis_inliers, inliers;  /* the counts under the hypothesis plane and under the final one */
    double   hypothesis_plane[4], plane[4]; /* nx ny nz d */
    double   pivot[3];
    double   sum_u[3], sum_uu[6];          /* the refit's sums over the hypothesis inliers (refit == 0: zero) */
} fgoicp_segment_model_t;
typedef struct fgoicp_segment_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_segment_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t points;             /* n */
    uint64_t planes;             /* the planes found */
    uint64_t on_planes;          /* the points with label >= 0 */
    uint64_t kept;               /* rows of the output */
    int      iterations, max_planes, refit, keep_planes;  /* as given; refit and keep_planes as 0 / 1 */
    uint64_t min_inliers, seed;
    double   distance_threshold; /* T: the double every |r| was compared with */
} fgoicp_segment_info_t;
int fgoicp_segment_planes(const float* xyz, size_t n, float distance_threshold, int iterations, uint64_t seed,
                          int max_planes, size_t min_inliers, int refit, int keep_planes, int device,
                          float* out_xyz, size_t capacity_points, uint32_t* kept_index, int32_t* label_n,
                          fgoicp_segment_model_t* models, size_t capacity_models, size_t model_size,
                          fgoicp_segment_info_t* out);
/* The two host halves of the call, no device needed (the call itself runs these).  fgoicp_segment_hypotheses: the table of one peel —
 * sample_K3 (3 caller indices per hypothesis), plane_K4 (nx ny nz d), degenerate_K (0 / 1) for h = 0 .. iterations - 1; candidates = the m
 * ascending caller indices of R_peel, NULL = the identity list, m = n; every output may be NULL.  Refuses what the call refuses of the
 * cloud, an m outside [1, n], iterations outside [1, 65536], a peel outside [0, 16) and candidates that are not ascending indices below n.
 * fgoicp_segment_fit_from_moments: the refit — count, pivot, sum_u, sum_uu -> plane4, the normal flipped towards toward4's (NULL: as the
 * iteration leaves it).  Refuses null pointers, count < 3 and moments that are not finite. */
int fgoicp_segment_hypotheses(const float* xyz, size_t n, const uint32_t* candidates_or_NULL, size_t m, int iterations, uint64_t seed, int peel,
                              uint32_t* sample_K3, double* plane_K4, uint8_t* degenerate_K);
int fgoicp_segment_fit_from_moments(uint64_t count, const double* pivot3, const double* sum_u3, const double* sum_uu6, const double* toward4_or_NULL,
                                    double* plane4);
/*
 * EXTENSION — surface sampling of a triangle mesh on the device (no reference counterpart: its loaders keep a mesh's vertices only; Open3D:
 * sample_points_uniformly, and with fgoicp_farthest_point_sample behind it sample_points_poisson_disk).  Turns a CAD or reconstructed model
 * into the point cloud the rest of the pipeline takes: points spread over the FACES in proportion to their area, each with the exact normal
 * of its face.
 *
 * Inputs: nv vertices (fp32 xyz triples), nf triangles (three uint32 vertex indices each), m samples, a seed.  ALL arithmetic is IEEE fp64 on
 * the fp32 coordinates converted to double, every operation rounded on its own in the order written — no contraction, no reciprocal.
 *   face f         a, b, c = its vertices;  e1 = b - a, e2 = c - a;
 *                  n = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x);  n2 = (nx*nx + ny*ny) + nz*nz;  area_f = 0.5 * sqrt(n2)
 *   weight         A_max = the largest area;  q_f = (uint64) floor(area_f / A_max * 4294967296.0);  Q = the inclusive 64-bit integer scan of q in
 *                  face order, weight_total = Q[nf - 1].  Integer weights: the scan is exact however it is associated.  A face more than 2^32
 *                  times smaller than the largest has weight 0 and is never sampled (counted in `unweighted`, as the faces of area 0 are)
 *   draws          h(k, s) = mix64(seed + 0x9E3779B97F4A7C15 * (3k + s + 1)) mod 2^64, s = 0, 1, 2, mix64 the splitmix64 finaliser of
 *                  fgoicp_segment_planes.  Counter based: any sample can be formed alone
 *   sample k       r = the high 64 bits of h(k, 0) * weight_total;  face_k = the first f with Q[f] > r;
 *                  u = (h(k, 1) >> 11) * 2^-53, v = (h(k, 2) >> 11) * 2^-53;  if u + v > 1.0 then u = 1 - u, v = 1 - v (no square root);
 *                  point_k = (a + u*e1) + v*e2 per axis, rounded to fp32 once;  normal_k = n / sqrt(n2), three divisions, rounded to fp32:
 *                  its direction follows the winding;  uv_k = (u, v)
 * Sample k depends on (mesh, seed, k) alone: two calls return the same bytes, and every prefix of a result is the sampling of that size.
 * Outputs: points_m3 is required; normals_m3, face_m (uint32), uv_m2 (doubles) per sample and face_area_nf (doubles) per face may be NULL.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (one host pass over the mesh): null or empty vertices or triangles, a null
 * points_m3, nv, nf or m at or above 2^31, m == 0, a non-finite vertex coordinate (the message names the vertex), a triangle index >= nv
 * (the message names the face and the index), a null `info` or a struct_size that is 0, ends before `area` ends or is above 4096, a device
 * ordinal out of range; and once the areas are known: A_max == 0, "the mesh has no area".  No usable device: FGOICP_ERR_NO_DEVICE (no CPU
 * fallback); allocation failure: FGOICP_ERR_OOM.  The call owns its stream and its one device allocation (12 bytes per vertex, 36 per face
 * and 12 to 44 per sample) and frees both before it returns; it touches no fgoicp_ctx, no global state and no knob and may be called from
 * several threads.
 */
typedef struct fgoicp_mesh_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_mesh_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint64_t vertices, triangles, samples;  /* nv, nf, m */
    uint64_t zero_area;          /* faces with area == 0 */
    uint64_t unweighted;         /* faces with weight 0, the zero_area ones included */
    uint64_t weight_total;
    double   max_area;
    double   area;               /* = max_area * (double)weight_total / 2^32: the area the samples are spread over */
} fgoicp_mesh_info_t;
int fgoicp_mesh_sample(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, size_t m, uint64_t seed, int device,
                       float* points_m3, float* normals_m3_or_NULL, uint32_t* face_m_or_NULL, double* uv_m2_or_NULL,
                       double* face_area_nf_or_NULL, fgoicp_mesh_info_t* info);
/*
 * EXTENSION — the distance from points to a triangle mesh on the device (no reference counterpart; Open3D: RaycastingScene
 * compute_closest_points / compute_distance, CloudCompare: cloud-to-mesh distance).  After a registration against a model's samples this
 * is the deviation of every scan point from the model's SURFACE, not from its nearest sample.
 *
 * Inputs: nv vertices (fp32 xyz), nf triangles (uint32 triples), nq query points (fp32 xyz).  ALL arithmetic is IEEE fp64 on the fp32 values
 * converted to double, every operation rounded once in the order written, nothing contracted, divisions are divisions.
 * dot(x, y) = (x0*y0 + x1*y1) + x2*y2.
 *   closest point of (a, b, c) to p — the seven regions of Ericson (Real-Time Collision Detection 5.1.5), in his order:
 *     1  ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 && d2 <= 0: vertex a
 *     2  bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp);  d3 >= 0 && d4 <= d3: vertex b
 *     3  vc = d1*d4 - d3*d2;  vc <= 0 && d1 >= 0 && d3 <= 0: edge ab at a + (d1 / (d1 - d3)) * ab
 *     4  cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp);  d6 >= 0 && d5 <= d6: vertex c
 *     5  vb = d5*d2 - d1*d6;  vb <= 0 && d2 >= 0 && d6 <= 0: edge ac at a + (d2 / (d2 - d6)) * ac
 *     6  va = d3*d6 - d5*d4;  va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0: edge bc at b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
 *     7  s = (va + vb) + vc, v = vb / s, w = vc / s;  s > 0 && v >= 0 && w >= 0 && v + w <= 1: the interior at (a + v*ab) + w*ac
 *     A quotient of steps 3, 5, 6 whose denominator is 0 is taken as 0 (the edge's first vertex).  When step 7's condition fails — a
 *     sliver whose va, vb, vc are rounding noise: s <= 0, a quotient that is not finite or weights outside the triangle — the answer is
 *     the nearest of the three edges taken as segments x -> y, in the order ab, bc, ca: e = y - x, num = dot(e, p - x), den = dot(e, e);
 *     not (num > 0): vertex x; not (num < den): vertex y; otherwise x + (num / den) * e on the edge; the smallest dist2 wins, a tie goes to
 *     the lowest region code.  Every branch returns a point whose computed weights lie inside the triangle.
 *   region   0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c
 *   dist2    (dx*dx + dy*dy) + dz*dz of p - closest, with the fp64 closest point;  closest is returned rounded to fp32 once per axis
 *   side     the sign (-1, 0, +1) of dot(n, p - closest), n = ab x ac as fgoicp_mesh_sample forms it.  This is the side of the WINNING
 *            FACE'S PLANE, not an inside / outside test of the mesh: where region != 0 (the closest point lies on an edge or a vertex) the
 *            face's plane says little about the surface around it and the sign is weak
 *   faces left out   a face whose n2 is 0 under fgoicp_mesh_sample's formula takes no part (counted in zero_area); a mesh without any
 *            other face is refused, "the mesh has no area"
 *   winner   per query the smallest (dist2, face index) over the participating faces: among equal dist2 — a query on a shared edge or
 *            vertex, or midway between two faces — the lowest face index.  A total order: the result is a function of the inputs alone,
 *            two calls return the same bytes, and FGOICP_MESH_DISTANCE_BRUTE (every query against every face, no tree) returns them too
 * Outputs per query, every array may be NULL: face_nq, closest_nq3, dist2_nq, region_nq, side_nq.  info->max_dist2 is the largest dist2
 * and max_dist2_index the lowest query index that attains it.
 * Refused with FGOICP_ERR_INVALID_ARG before any device work (one host pass over the inputs): null or empty vertices, triangles or
 * queries, nv, nf or nq at or above 2^31, a null `info` or a struct_size that is 0, ends before `max_dist2` ends or is above 4096, an
 * unknown flag bit, a non-finite vertex or query coordinate (the message names it), a triangle index >= nv (the message names the face
 * and the index), a device ordinal out of range; and once the device is chosen: "the mesh has no area".  No usable device:
 * FGOICP_ERR_NO_DEVICE (no CPU fallback); allocation failure: FGOICP_ERR_OOM.  The call owns its stream and its one device allocation (40
 * bytes per participating face, 6 to 12 per face for the tree's boxes, 36 to 54 per query plus the sort's storage; no vertex array) and frees both before it returns; it touches no
 * fgoicp_ctx, no global state and no knob and may be called from several threads.
 */
enum { FGOICP_MESH_DISTANCE_BRUTE = 1 };  /* flags bit 0: no tree — the on-device checker of the walk and the baseline of its timings */
typedef struct fgoicp_mesh_distance_info_t {
    uint32_t struct_size;        /* IN: sizeof(fgoicp_mesh_distance_info_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint32_t flags;              /* as given */
    uint64_t vertices, triangles, queries;  /* nv, nf, nq */
    uint64_t faces;              /* the faces that take part: triangles - zero_area */
    uint64_t zero_area;          /* faces with n2 == 0 */
    uint32_t tree_depth;         /* levels below the root: 2^tree_depth >= the number of leaves */
    uint32_t leaf_faces;         /* faces per leaf */
    uint64_t max_dist2_index;
    double   max_dist2;
} fgoicp_mesh_distance_info_t;
int fgoicp_mesh_distance(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* queries_nq3, size_t nq,
                         uint32_t flags, int device, uint32_t* face_nq, float* closest_nq3, double* dist2_nq, uint8_t* region_nq, int8_t* side_nq,
                         fgoicp_mesh_distance_info_t* info);
/* The arithmetic the kernel runs on one (point, triangle) pair, on the host (no device needed; csrc/device/point_triangle.hpp is the one
 * text of both).  Every output may be NULL.  Refuses null inputs and a coordinate that is not finite. */
int fgoicp_point_triangle(const float* p3, const float* a3, const float* b3, const float* c3, float* closest3, double* dist2, int* region, int* side);
/*
 * EXTENSION — point-to-mesh refinement on the device (no reference counterpart; CloudCompare: fine registration of a cloud against a
 * mesh): the pose that minimises the deviation map of fgoicp_mesh_distance itself.  The refinements above minimise residuals against the
 * nearest SAMPLE of a model, with normals estimated from samples; this one takes the exact closest point of the nearest triangle and the
 * exact direction of the distance field there, so the number minimised is the number the deviation map reports.
 *
 * Everything is IEEE fp64 on the fp32 inputs converted to double, every operation rounded once in the order written, nothing contracted;
 * dot is fgoicp_mesh_distance's.  For a source point p and a pose (R9 in glm order, R[a][b] = R9[3 b + a]; t3), both in the mesh's frame:
 *   moved point   x[a] = (float)((((double)R[a][0] px + (double)R[a][1] py) + (double)R[a][2] pz) + (double)t[a]) — rounded to fp32 once, so
 *                 face, closest, dist2 and region of the point are, byte for byte, what fgoicp_mesh_distance returns for the query x
 *   winner        fgoicp_mesh_distance's smallest (dist2, face index) over the faces with area; c = its fp64 closest point, d = x - c
 *   direction g   region != 0 and dist2 > 0 (off an edge or a vertex): g = d / sqrt(dist2) per axis, the gradient of the distance field;
 *                 otherwise g = n / sqrt(n2) per axis, n = ab x ac and n2 = (nx nx + ny ny) + nz nz as fgoicp_mesh_sample forms them: the
 *                 face's unit normal
 *   residual      s = dot(g, d); for an interior closest point s = +- sqrt(dist2) up to rounding
 *   counted       max_distance <= 0: every point; otherwise the points with dist2 <= (double)max_distance * (double)max_distance.  No
 *                 trimming, no context
 *   weight        w = the w(s) of fgoicp_robust_weight at (loss, scale); with FGOICP_LOSS_NONE w = 1 and nothing is multiplied by it
 *   terms         J = [ (x cross g)^T, g^T ] with the fp64 value of the fp32 x; the 28 terms in the layout and order of
 *                 fgoicp_plane_moments_t::m — the upper triangle of J^T J row by row (21), J^T s (6), s s (1) — each times w when weighted;
 *                 so fgoicp_plane_step_from_moments and fgoicp_plane_apply_step serve unchanged
 *   sums          the 28 terms, weight_sum = sum w and sum_dist2 = sum dist2 over the counted points, each added in a fixed order: the
 *                 points sorted once by (a 30-bit Z-order code of the SOURCE point inside the source's box, caller index) — the stable sort
 *                 of fgoicp_mesh_distance, a function of the source alone — then the order of fgoicp_plane_moments over those slots.  Two
 *                 calls return the same bytes, and FGOICP_MESH_DISTANCE_BRUTE (flags bit 0: no tree) returns them too.
 */
/* Host only, no device: the arithmetic of ONE (moved point, triangle) pair, the text the kernel runs.  x3: the moved point; every output may
 * be NULL: closest3 (fp64), dist2, region, g3, s, w, v28 (the 28 terms, times w unless the loss is FGOICP_LOSS_NONE).  Refuses null inputs, a
 * coordinate that is not finite, an unknown loss, a scale that is not finite and > 0 (FGOICP_LOSS_NONE ignores the scale) and a triangle
 * without area (n2 == 0: it takes no part in a mesh). */
int fgoicp_mesh_pair_terms(const float* x3, const float* a3, const float* b3, const float* c3, int loss, double scale, double* closest3, double* dist2, int* region,
                           double* g3, double* s, double* w, double* v28);
typedef struct fgoicp_mesh_moments_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_mesh_moments_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    uint32_t flags;                   /* as given */
    uint64_t points, correspondences; /* ns; the counted points N (a zero weight still counts) */
    double   m[28];                   /* the layout of fgoicp_plane_moments_t */
    double   weight_sum;              /* sum w over the counted (FGOICP_LOSS_NONE: == correspondences) */
    double   sum_dist2;               /* sum dist2 over the counted */
    double   max_dist2;               /* the fp64 threshold the device compared dist2 with; +inf: none */
    int      loss;
    double   scale;                   /* as given */
    uint64_t vertices, triangles;     /* nv, nf */
    uint64_t faces, zero_area;        /* as fgoicp_mesh_distance_info_t */
    uint32_t tree_depth, leaf_faces;
} fgoicp_mesh_moments_t;
/* One evaluation at (R9, t3).  Optional per-point outputs in caller order, ns entries each, any may be NULL: face, closest (fp32, 3 per
 * point), dist2, region, direction (3 doubles per point), residual, weight, counted (0 / 1); order_ns: the sorted order — slot k of the
 * sums holds the caller's point order_ns[k].  An uncounted point gets residual, weight and counted 0; its other outputs are still its own.
 * Refuses what fgoicp_mesh_distance refuses (the source points are its queries) and a non-finite pose, max_distance or scale, an unknown
 * loss, a loss with a scale that is not finite and > 0 — all before any device work.  One-shot as fgoicp_mesh_distance: its own stream and
 * one device allocation (that call's for the mesh; 28 bytes per point, 248 per 256 points, 66 more per point when a per-point output is asked
 * for; the sort's storage), nothing left behind. */
int fgoicp_mesh_moments(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* points_ns3, size_t ns, const float* R9, const float* t3,
                        float max_distance, int loss, double scale, uint32_t flags, int device, uint32_t* face_ns, float* closest_ns3, double* dist2_ns, uint8_t* region_ns,
                        double* direction_ns3, double* residual_ns, double* weight_ns, unsigned char* counted_ns, uint32_t* order_ns, fgoicp_mesh_moments_t* out);
typedef struct fgoicp_mesh_refine_result_t {
    uint32_t struct_size;             /* IN: sizeof(fgoicp_mesh_refine_result_t) as the CALLER was compiled; no byte beyond it is written, 0 is refused */
    float    R[9], t[3];              /* the refined pose, in the mesh's frame */
    int      iterations;              /* steps taken */
    int      rank;                    /* of the last solve (0 when max_iter = 0, nothing was counted or every weight was zero) */
    uint64_t points, correspondences; /* ns; counted at the returned pose */
    double   weight_sum;              /* sum w at the returned pose */
    double   mesh_rmse;               /* sqrt(sum w s^2 / sum w) at the returned pose (0 when the weight sum is 0) */
    double   rms_distance;            /* sqrt(sum_dist2 / correspondences) there (0 when nothing is counted): the rms of the deviation map */
    int      loss;
    int      scale_estimated;         /* 1: the scale was estimated at the start pose, 0: it was given (or there is no loss) */
    double   loss_scale;              /* the scale the loop ran with (0 without a loss) */
    uint64_t triangles, faces, zero_area;
} fgoicp_mesh_refine_result_t;
/* The loop of fgoicp_icp_plane / fgoicp_icp_robust, term for term, over these moments: evaluate, fgoicp_plane_step_from_moments,
 * fgoicp_plane_apply_step; it ends after a step with |w| + |v| < conv_thr, after the first step when that solve had rank < 6, when nothing
 * is counted or the weights sum to 0, or after max_iter steps; the result's sums are those of one more evaluation at the pose returned.
 * The tree is built, the points are uploaded and sorted ONCE per call; an iteration is one kernel, one fold and one 248-byte copy.
 * loss_scale <= 0 with a loss: estimated once at the start pose, 1.4826 * the lower median of |s| over the counted points (as
 * fgoicp_robust_scale); refused, the message saying to pass a scale, when nothing is counted or that median is 0.  Refuses what
 * fgoicp_mesh_moments refuses (a scale <= 0 asks for the estimate) and a non-finite conv_thr. */
int fgoicp_mesh_refine(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* points_ns3, size_t ns, const float* R0_9, const float* t0_3,
                       size_t max_iter, float conv_thr, float max_distance, int loss, double loss_scale, uint32_t flags, int device, fgoicp_mesh_refine_result_t* out);
/* EXTENSION: given normals at solver level — fgoicp_ctx_set_target_normals / fgoicp_ctx_set_source_normals with the pointer, on the solver's
 * context (nt / ns triples in the order the clouds were passed to fgoicp_solver_create, normalised on upload; normals are invariant under
 * the solver's centring and uniform scale).  A mesh knows its normals exactly (fgoicp_mesh_sample).  fgoicp_solver_refine_plane / _gicp /
 * _robust estimate only what is not set: with both sets given they ignore k.  Refusals carry the context call's message. */
int fgoicp_solver_set_target_normals(fgoicp_solver* s, const float* normals_nt3);
int fgoicp_solver_set_source_normals(fgoicp_solver* s, const float* normals_ns3);
/* The operator context the solver drives (borrowed; valid until solver_destroy). */
fgoicp_ctx* fgoicp_solver_ctx(fgoicp_solver* s);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU inside the library (no reference counterpart: the reference is single-GPU).
 * The rotation cubes of every expansion round are dealt round-robin to the ranks; per round ONE all-reduce(MIN) of the
 * best error and ONE small all-gather keep every rank's queue and incumbent identical.
 * ------------------------------------------------------------------------------------------ */
typedef struct fgoicp_rccl fgoicp_rccl;
/* RCCL transport of the exchange, one communicator per rank (one process per GPU, or one thread per GPU): rank 0 draws the
 * 128-byte id (ncclGetUniqueId) and hands it to the others by whatever channel the launcher has; every rank then calls
 * fgoicp_rccl_create (ncclCommInitRank — blocks until all ranks have joined) and installs fgoicp_rccl_exchange's struct with
 * fgoicp_solver_set_exchange.  The collectives run on device buffers over xGMI, on a stream of their own. */
int fgoicp_rccl_unique_id(unsigned char* id128);
/* Which librccl the transport runs on (loads it on first use): the instance already mapped into the process — PyTorch-ROCm brings its own
 * librccl.so + librocm_smi64.so, and a second copy next to it makes the process abort in its exit handlers (two librocm_smi64 destroying
 * the same globals) — or the system's librccl.so.1, loaded RTLD_LOCAL | RTLD_DEEPBIND.  Returns a description (or the load error). */
const char* fgoicp_rccl_library(void);
int fgoicp_rccl_create(int rank, int world_size, const unsigned char* id128, int device, fgoicp_rccl** out);
/* The same with the kind of communicator chosen: nonblocking != 0 creates it with ncclConfig_t.blocking = 0 (what fgoicp_multi_create
 * does for its rank threads, so that a rank can abandon the set-up when a peer fails); every collective on such a communicator may
 * return ncclInProgress and is polled (ncclCommGetAsyncError) until it is on the stream before anything else is enqueued. */
int fgoicp_rccl_create_ex(int rank, int world_size, const unsigned char* id128, int device, int nonblocking, fgoicp_rccl** out);
/* TEST HOOK, not part of the drop-in surface: the next n collectives of x report ncclInProgress once before their real status (the
 * polling path on a box where RCCL answers at once); settled_out (optional) = polls of ncclCommGetAsyncError made so far. */
int fgoicp_rccl_test_inprogress(fgoicp_rccl* x, int n, uint64_t* settled_out);
int fgoicp_rccl_exchange(fgoicp_rccl* x, fgoicp_exchange* out);   /* `out` borrows x: keep x alive while a solver uses it */
int fgoicp_rccl_calls(const fgoicp_rccl* x, uint64_t* collectives);
/* Ranks the communicator itself reports (ncclCommCount) — printed by bench.py so that a scaling run shows RCCL joined N ranks. */
int fgoicp_rccl_comm_count(fgoicp_rccl* x, int* count);
/* A PEER rank has failed: the collective in flight on x and every later one must end instead of waiting for it for ever.  Any
 * thread, once or more — it only raises a flag; the thread that runs x's collectives polls it while it waits and aborts the
 * communicator itself (ncclCommAbort frees it: it must not be called under a running collective's feet).  x stays valid until
 * fgoicp_rccl_destroy but cannot be used for another run. */
int fgoicp_rccl_abort(fgoicp_rccl* x);
void fgoicp_rccl_destroy(fgoicp_rccl* x);

/* One process, one host thread + one solver per device — what `fast-go-icp --gpus N` runs.  devices[r] = HIP ordinal of rank r.
 * FGOICP_TRANSPORT_RCCL needs distinct devices; FGOICP_TRANSPORT_IN_PROCESS (a shared-memory rendezvous of the rank threads)
 * takes any list, e.g. {0, 0, 0, 0}: four ranks rehearsed on one GPU.  opts->schedule selects what is sharded (opts == NULL:
 * ROUND, adaptive width): FGOICP_SCHEDULE_ROUND deals the children of an expansion round over the ranks (fastest; an epsilon-optimal
 * result reached in another order than the reference's); FGOICP_SCHEDULE_SERIAL keeps the reference's exact trajectory
 * (fgoicp.cpp:32-100: same pops, pushes, counters and result as the one-GPU SERIAL run, bit for bit, on every rank) and deals the
 * inner BnBs of every speculative evaluation over the ranks — one all-gather per evaluation, cooperative refinements. */
typedef struct fgoicp_multi fgoicp_multi;
enum { FGOICP_TRANSPORT_RCCL = 0, FGOICP_TRANSPORT_IN_PROCESS = 1 };
int fgoicp_multi_create(const float* tgt_xyz, size_t nt, const float* src_xyz, size_t ns, float lut_resolution, float mse_threshold,
                        const fgoicp_solver_opts* opts, const int* devices, int ndev, int transport, fgoicp_multi** out);
void fgoicp_multi_destroy(fgoicp_multi* m);
/* FastGoICP::run() on all ranks at once; R, t as fgoicp_solver_run (every rank ends with the same incumbent — checked).
 * If a rank fails, the exchange is aborted for all of them (nobody waits for the failed rank) and the call returns that rank's
 * status and message; with the RCCL transport the object cannot run again afterwards. */
int fgoicp_multi_run(fgoicp_multi* m, float* R_out9, float* t_out3);
/* One IterativeClosestPoint3D::run() (icp3d.cu:80-108) executed by ALL ranks together: each scans 1/world of the source for the two
 * exact nearest-neighbour passes of an iteration, the per-query results are all-gathered on device memory, sums and SVD are
 * replicated.  Same (sse, R, t, iterations) as fgoicp_icp on one GPU, bit for bit, on every rank (checked).  This is what every
 * refinement of a multi-rank run is (fgoicp_exchange.allgather_device). */
int fgoicp_multi_icp(fgoicp_multi* m, const float* R0, const float* t0, size_t max_iter, float convergence_threshold, float* sse_out, float* R_out9, float* t_out3,
                     int* iterations_out);
int fgoicp_multi_world(const fgoicp_multi* m);
fgoicp_solver* fgoicp_multi_solver(fgoicp_multi* m, int rank);     /* borrowed: stats, getters */
int fgoicp_multi_seconds(const fgoicp_multi* m, int rank, double* seconds);   /* wall-clock of that rank's last run() */
/* Scaling rehearsal on fewer GPUs than ranks: record what every exchange returned during a run, then run ONE rank alone
 * against the recording — the time that rank would need on a GPU of its own, without the collectives' latency. */
int fgoicp_multi_set_record(fgoicp_multi* m, int on);
/* What the last recorded run exchanged: the host-side collectives of `rank` and the device all-gathers of the cooperative ICP runs. */
int fgoicp_multi_recorded(const fgoicp_multi* m, int rank, uint64_t* host_exchanges, uint64_t* device_allgathers);
/* TEST HOOK, not part of the drop-in surface: the call-th exchange of `rank` in the next run fails, once. */
int fgoicp_multi_test_fault(fgoicp_multi* m, int rank, long call);
int fgoicp_multi_replay_rank(fgoicp_multi* m, int rank, double* seconds_out);

/* ------------------------------------------------------------------------------------------
 * Batches: many registrations on one device (no reference counterpart).  Each pair of a batch returns exactly what
 * fgoicp_solver_run returns for it alone with the same options — R, the restored t, the best error and the counters trans_cubes,
 * rot_cubes, inner_bnb, icp_runs, icp_iters, rounds, initial_icp_sse, bit for bit, under both schedules — whatever the other pairs,
 * their order or the grouping of requests into launches.  bounds_calls and the timings are not part of that.  Every live pair runs
 * its own search; the bounds requests of all of them are evaluated in fused launches (one per LUT class present in a tick; a class of more than 2^24 work items is split) and their
 * ICP runs are advanced in lock-step, so the host turn-arounds are paid once for all live pairs.  Trimming is per
 * pair (fgoicp_batch_opts.trim_fractions): a trimmed pair returns what fgoicp_solver_run returns for it alone with that trim_fraction.
 * Its bounds rows go through the batch's e-row arena (fused trimmed launches per LUT class, then one selection launch per arena fill)
 * and its ICP runs are not stepped: each runs its whole loop while the other pairs wait.
 * ------------------------------------------------------------------------------------------ */
typedef struct fgoicp_batch fgoicp_batch;
typedef struct fgoicp_batch_pair {
    const float* tgt_xyz; size_t nt; const float* src_xyz; size_t ns;
    float lut_resolution; float mse_threshold;           /* per pair, as fgoicp_solver_create takes them */
} fgoicp_batch_pair;
/* EXTENSION: how one pair of a batch is refined after its search (fgoicp_batch_opts_refine.refine) — the arguments of fgoicp_solver_refine_plane /
 * _gicp / _robust, in the callers' units.  model = -1: this pair is not refined.  loss = FGOICP_LOSS_NONE: the plain (unweighted)
 * refinement, served by fgoicp_batch_refined_plane; any other loss: fgoicp_solver_refine_robust's, served by fgoicp_batch_refined_robust. */
typedef struct fgoicp_batch_refine_t {
    uint32_t struct_size;        /* sizeof(fgoicp_batch_refine_t) as the caller was compiled */
    int      model;              /* -1, FGOICP_MODEL_PLANE or FGOICP_MODEL_GICP */
    int      k;                  /* neighbours per normal, 4 .. 32 */
    size_t   max_iter;
    float    conv_thr;
    float    max_distance;       /* >= 0, +inf: no threshold */
    double   epsilon;            /* FGOICP_MODEL_GICP: in (0, 1] */
    int      loss;               /* FGOICP_LOSS_* */
    double   loss_scale;         /* finite; <= 0: estimated at the search's pose */
} fgoicp_batch_refine_t;
typedef struct fgoicp_batch_opts {
    size_t struct_size;          /* sizeof(fgoicp_batch_opts) as the caller was compiled (ABI 2): members beyond it are taken as 0 */
    fgoicp_solver_opts solver;   /* schedule, round_width, ctx_flags, device; trim_fraction must be 0 (trimming is per pair: trim_fractions) */
    int max_live;                /* pairs whose device state (context: LUT, tree, source order) exists at once; 0 = as many as device memory allows, at most 16 */
    const float* trim_fractions; /* n entries, pair i trimmed as fgoicp_solver_create trims with solver.trim_fraction = trim_fractions[i] (0 = untrimmed);
                                    NULL, or a struct_size that ends before this member: no pair is trimmed.  Read by fgoicp_batch_create only */
    int alignment;               /* != 0: the run keeps every pair's alignment report (fgoicp_batch_alignment) on the host: 9 bytes per source point, 1 per target
                                    point.  Appended within revision 2: 0 for a caller built with the shorter struct (struct_size) */
    int reserved0;               /* the tail padding of the struct as first published with `alignment` (48 bytes): a caller built against it may leave anything
                                    here, so it is never read and the members below start behind it */
    int information;             /* != 0: the run keeps every pair's information matrix (fgoicp_batch_information): under 200 bytes per pair.  Appended within
                                    revision 2: 0 for a caller built with a shorter struct (struct_size) */
    float information_max_distance; /* its distance threshold in the callers' units, as fgoicp_solver_information takes it; <= 0: none.  NaN is refused */
} fgoicp_batch_opts;
/* EXTENSION: the options of a batch that refines.  fgoicp_batch_create reads its options as struct_size bytes, so what is appended to them
 * lies behind fgoicp_batch_opts, whose own 56 bytes stay as published (callers and bindings hold that size): fill this struct, set
 * opts.struct_size = sizeof(fgoicp_batch_opts_refine) and pass &opts. */
typedef struct fgoicp_batch_opts_refine {
    fgoicp_batch_opts opts;      /* every member as above; struct_size covers this whole struct */
    const fgoicp_batch_refine_t* refine; /* n entries, pair i refined after its search as entry i says; NULL, or a struct_size that ends before this member: no
                                    pair is refined and the run takes no new path.  Appended within revision 2.  Read by fgoicp_batch_create only */
} fgoicp_batch_opts_refine;
/* Copies the clouds and pre-processes every pair on the host (centre, scale, bounds, inlier count, as fgoicp_solver_create); creates no
 * device state.  Refuses n <= 0, a null or empty cloud, solver.trim_fraction != 0, a trim_fractions entry that is NaN, negative or >= 1,
 * and a struct_size shorter than the solver options.  Every refine entry is refused as the solo entry points refuse their arguments, the message
 * naming the pair: a bad struct_size, an unknown model or loss, k outside 4 .. 32, a negative or NaN max_distance, an epsilon outside (0, 1]
 * for FGOICP_MODEL_GICP, a loss_scale that is not finite. */
int fgoicp_batch_create(const fgoicp_batch_pair* pairs, int n, const fgoicp_batch_opts* opts, fgoicp_batch** out);
/* Runs every pair: pairs enter a window of at most max_live live pairs in index order; a pair's context is created when it enters
 * and destroyed when it finishes.  Returns FGOICP_OK when the batch ran; status_n[i] is pair i's own status (a pair that cannot be
 * served — LUT dims above 4094: FGOICP_ERR_INVALID_ARG; FGOICP_ERR_OOM only if it does not fit with no other pair live — leaves
 * the others untouched).  R_out9n / t_out3n: 9 / 3 floats per pair, as fgoicp_solver_run; untouched for a failed pair. */
int fgoicp_batch_run(fgoicp_batch* b, float* R_out9n, float* t_out3n, int* status_n);
int fgoicp_batch_best_error(const fgoicp_batch* b, int i, float* sse_out);
int fgoicp_batch_stats(const fgoicp_batch* b, int i, fgoicp_run_stats* out);
/* Pair i's alignment report as fgoicp_solver_alignment gives it for that pair alone, bit for bit, whatever the window, the order or the
 * other pairs: computed when the pair finished, before its context was released, and kept on the host.  Refused (FGOICP_ERR_INVALID_ARG)
 * when fgoicp_batch_opts.alignment was 0, before fgoicp_batch_run, and for a pair whose status is not FGOICP_OK. */
int fgoicp_batch_alignment(const fgoicp_batch* b, int i, uint32_t* corr_idx_ns, float* dist2_ns, uint8_t* inlier_ns, uint8_t* target_hit_nt,
                           fgoicp_alignment_summary* out);
/* Pair i's information matrix as fgoicp_solver_information(s, information_max_distance) gives it for that pair alone, byte for byte: taken
 * when the pair finished, next to the report (one pass of the report's device half serves both when both options are on).  Refused
 * (FGOICP_ERR_INVALID_ARG) when fgoicp_batch_opts.information was 0, before fgoicp_batch_run, and for a pair whose status is not FGOICP_OK. */
int fgoicp_batch_information(const fgoicp_batch* b, int i, fgoicp_information_t* out);
/* Launches of the last run: fused bounds launches (one per LUT class per tick, more for a class of more than 2^24 work items, and per
 * arena fill for trimmed pairs; neither the finalize nor the trimmed selection counted) and lock-step ICP iterations (one host
 * turn-around each, shared by every active ICP run). */
int fgoicp_batch_launches(const fgoicp_batch* b, uint64_t* bounds_launches, uint64_t* icp_launches);
/* EXTENSION: refinement inside a batch (fgoicp_batch_opts_refine.refine).  A pair with a refine entry is refined from its
 * search's pose before its context is released, and returns, byte for byte, what fgoicp_solver_refine_plane / _gicp (loss none) or
 * fgoicp_solver_refine_robust returns for that pair alone with the same arguments — t restored, scaling_factor the pair's — whatever the
 * other pairs, their order, their entries, the window or the grouping into launches: the loops of all refining pairs advance one
 * evaluation per tick, their moments reduced by one fused launch per class (model x weighted) over per-pair blocks, rows and folds, the
 * host turn-around shared.  What the batch returns otherwise (R, t, errors, counters, fgoicp_batch_alignment, fgoicp_batch_information at
 * the SEARCH's pose) is unchanged, bit for bit.  Both getters refuse (FGOICP_ERR_INVALID_ARG) the other kind, a pair without an entry, a
 * call before fgoicp_batch_run and a pair whose search failed; a refinement that was itself refused (no scale to estimate: "pass a scale")
 * or failed left the pair's search result and status alone, and the getter returns that refinement's own status and message. */
int fgoicp_batch_refined_plane(const fgoicp_batch* b, int i, fgoicp_plane_result_t* out);
int fgoicp_batch_refined_robust(const fgoicp_batch* b, int i, fgoicp_robust_result_t* out);
/* The information matrix at pair i's REFINED pose (needs fgoicp_batch_opts.information and a refined pair): the restored translation taken
 * back into the solver's frame, fgoicp_information there, fgoicp_information_from_moments — the bytes the command-line tool writes for that
 * pair alone (one text of that arithmetic serves both: csrc/host/refined_pose.hpp). */
int fgoicp_batch_refined_information(const fgoicp_batch* b, int i, fgoicp_information_t* out);
/* Of the last run: fused moment launches (one per class present in a tick) and evaluations (one per refining pair per tick). */
int fgoicp_batch_refine_launches(const fgoicp_batch* b, uint64_t* fused_launches, uint64_t* evaluations);
void fgoicp_batch_destroy(fgoicp_batch* b);
/* TEST HOOK, not part of the drop-in surface: one tick of the batch's bounds path over contexts the caller made (fgoicp_ctx_create;
 * borrowed, not destroyed).  Request q goes to ctxs[req_ctx[q]] (a context may be named by several requests) with req_G[q] groups; R9,
 * rot_span, fix_rot, offsets (req_G[q] + 1 entries per request, each run starting at 0), tn4, lb_out and ub_out are laid out as
 * fgoicp_bounds_multi takes them, the requests' arrays concatenated.  All requests share the fused launches of one tick;
 * launches_out (optional) = fused bounds launches the tick made.  Refuses (FGOICP_ERR_INVALID_ARG, before any device work) null
 * arguments, nreq < 0, an index out of range, bad offsets, a trimmed context (fgoicp_ctx_set_inliers), a context without the packed
 * LUT and contexts on different devices. */
int fgoicp_batch_test_bounds(fgoicp_ctx* const* ctxs, int nctx, int nreq, const int* req_ctx, const int* req_G, const float* R9, const float* rot_span,
                             const int* fix_rot, const int* offsets, const float* tn4, float* lb_out, float* ub_out, uint64_t* launches_out);
/* TEST HOOK, not part of the drop-in surface: fgoicp_batch_test_bounds for trimmed contexts (fgoicp_ctx_set_inliers) and untrimmed ones
 * mixed in one tick.  A trimmed row is evaluated into the batch's e-row arena and selected there; the trimmed rows of the tick run in
 * sub-ticks of at most arena_rows rows (0 = as many as the batch's own arena budget holds), each one fused trimmed bounds launch per LUT
 * class and one selection launch.  launches_out (optional) = fused bounds launches, selection_launches_out (optional) = selection
 * launches.  Refuses what fgoicp_batch_test_bounds refuses, trimmed contexts excepted, before any device work. */
int fgoicp_batch_test_trim_bounds(fgoicp_ctx* const* ctxs, int nctx, int nreq, const int* req_ctx, const int* req_G, const float* R9, const float* rot_span,
                                  const int* fix_rot, const int* offsets, const float* tn4, float* lb_out, float* ub_out, uint64_t* launches_out,
                                  size_t arena_rows, uint64_t* selection_launches_out);
/* TEST HOOK, not part of the drop-in surface: n ICP runs stepped as a batch steps them, run i on ctxs[i] (borrowed; each context once,
 * all on one device).  Pass p starts the runs whose start_pass is p, then advances every active run by one iteration; contexts that
 * cannot be stepped (more than 262144 source points, brute force) run their whole loop when they start.  Outputs as fgoicp_icp, one
 * run after the other (9 / 3 floats per run). */
int fgoicp_batch_test_icp(fgoicp_ctx* const* ctxs, int n, const int* start_pass, const float* R0s_9, const float* t0s_3, const size_t* max_iter,
                          const float* thr, float* sse_out, float* R_out9, float* t_out3, int* iters_out);
/* TEST HOOK, not part of the drop-in surface: n refinement loops stepped as a batch steps them, run i on ctxs[i] (borrowed; each context
 * once, all on one device; the normals must be set).  specs[i] in the CONTEXT frame: max_distance holds max_dist2, loss_scale the scale,
 * k is not read; loss none runs fgoicp_icp_plane's / fgoicp_icp_gicp's loop, another loss fgoicp_icp_robust's.  Pass p starts the runs whose
 * start_pass is p, then advances every active run by one evaluation in the fused launches of a batch tick.  out_n[i]: run i's
 * fgoicp_robust_result_t, or (loss none) an fgoicp_plane_result_t in the slot's first bytes, the rest zero — the bytes of the solo call.
 * status_n[i] / messages_n256 (optional, 256 chars per run): a run's own refusal or failure, with the solo call's message; the other
 * runs go on.  fused_launches_out (optional): fused moment launches made. */
int fgoicp_batch_test_refine(fgoicp_ctx* const* ctxs, int n, const fgoicp_batch_refine_t* specs, const int* start_pass, const float* R0s_9, const float* t0s_3,
                             fgoicp_robust_result_t* out_n, int* status_n, char* messages_n256, uint64_t* fused_launches_out);

#ifdef __cplusplus
}
#endif
#endif /* FGOICP_AMD_H */
