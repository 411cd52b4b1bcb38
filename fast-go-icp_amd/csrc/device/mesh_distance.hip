// Point-to-mesh distance (fgoicp_mesh_distance, fgoicp_point_triangle; include/fgoicp_amd.h has the definition, DESIGN.md section 22 the
// pruning argument and the launch chain).  A one-shot call: the frame every such call shares is one_shot.hpp.
//
// The tree, the keys and the walk are mesh_tree.hpp's (one text with mesh_refine.hip).
//
//   host      the refusals (they need no device); then the tree (md_build)
//   keys      md_key_kernel, one thread per query: a 30-bit Z-order code inside the queries' own box
//   sort      rocPRIM radix sort of (code, caller index): a wave's 64 consecutive queries are neighbours
//   walk      md_kernel<false>, one wave per 64 sorted queries: md_walk, then the winner's face once more for the outputs (md_store)
//   brute     md_kernel<true> (flags bit 0): md_brute, the same leaves, the same leaf code, every leaf for every lane, no boxes
//   host      the largest dist2 and the lowest index that attains it
//
// The winner of a query is the smallest (dist2, face index) — a total order — so it does not depend on the order in which the faces are
// met, and a box is skipped only when every face inside it loses STRICTLY (md_box_d2): the walk returns the bytes of the brute search.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mesh_tree.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

struct MdOut {  // caller order; nullptr = not asked for (dist2 is always written)
    uint32_t* face;
    float* closest;
    double* dist2;
    uint8_t* region;
    int8_t* side;
};

// the winner's face once more, now for everything the caller asked for (the same text gives the same dist2)
__device__ __forceinline__ void md_store(const MdTree& t, const MdOut& out, uint32_t qi, double px, double py, double pz, const MdBest& best) {
    const float* c = t.leaf_v + 9 * (size_t)best.slot;
    const double ax = c[0], ay = c[1], az = c[2], bx = c[3], by = c[4], bz = c[5], cx = c[6], cy = c[7], cz = c[8];
    const PtResult r = point_triangle(px, py, pz, ax, ay, az, bx, by, bz, cx, cy, cz);
    out.dist2[qi] = r.d2;
    if (out.face) out.face[qi] = best.face;
    if (out.closest) {
        float* o = out.closest + 3 * (size_t)qi;
        o[0] = (float)r.cx; o[1] = (float)r.cy; o[2] = (float)r.cz;
    }
    if (out.region) out.region[qi] = (uint8_t)r.region;
    if (out.side) out.side[qi] = (int8_t)pt_side(px, py, pz, ax, ay, az, bx, by, bz, cx, cy, cz, r);
}

template <bool kBrute>
__global__ __launch_bounds__(kMdBlock) void md_kernel(MdTree t, const float* __restrict__ q, const uint32_t* __restrict__ order, uint32_t nq, double slack, MdOut out) {
    __shared__ uint32_t s_stack[kMdBlock / 64][kMdStack];
    const int wave = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * kMdBlock + threadIdx.x;
    const bool active = i < nq;
    const uint32_t qi = active ? order[i] : 0u;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (active) {
        const float* p = q + 3 * (size_t)qi;
        px = (double)p[0]; py = (double)p[1]; pz = (double)p[2];
    }
    const MdBest best = kBrute ? md_brute(t, px, py, pz, active) : md_walk(t, px, py, pz, slack, s_stack[wave], active);
    if (active) md_store(t, out, qi, px, py, pz, best);
}

int mesh_distance_impl(const float* vtx, size_t nv, const uint32_t* tri, size_t nf, const float* qry, size_t nq, uint32_t flags, int device, uint32_t* face, float* closest,
                       double* dist2, uint8_t* region, int8_t* side, fgoicp_mesh_distance_info_t* out) {
    const char* const call = "fgoicp_mesh_distance";
    constexpr size_t kLimit = (size_t)1 << 31;
    if (!vtx || nv == 0) return refuse(call, "the vertices must not be null or empty");
    if (!tri || nf == 0) return refuse(call, "the triangles must not be null or empty");
    if (!qry || nq == 0) return refuse(call, "the queries must not be null or empty");
    if (nv >= kLimit) return refuse(call, "more than 2^31 - 1 vertices");
    if (nf >= kLimit) return refuse(call, "more than 2^31 - 1 triangles");
    if (nq >= kLimit) return refuse(call, "more than 2^31 - 1 points");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_mesh_distance_info_t, max_dist2) + sizeof(double), "fgoicp_mesh_distance_info_t")) return rc;
    if (flags & ~(uint32_t)FGOICP_MESH_DISTANCE_BRUTE) return refuse(call, "unknown flag bits " + std::to_string(flags & ~(uint32_t)FGOICP_MESH_DISTANCE_BRUTE));
    float big = 0.0f;  // M: the largest |coordinate| of the call
    for (size_t i = 0; i < nv; ++i)
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(vtx[3 * i + a])) return refuse(call, "vertex " + std::to_string(i) + " has a non-finite coordinate");
            big = std::max(big, std::fabs(vtx[3 * i + a]));
        }
    float lo[3] = {qry[0], qry[1], qry[2]}, hi[3] = {qry[0], qry[1], qry[2]};
    for (size_t i = 0; i < nq; ++i)
        for (int a = 0; a < 3; ++a) {
            const float c = qry[3 * i + a];
            if (!std::isfinite(c)) return refuse_non_finite(call, i);
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
            big = std::max(big, std::fabs(c));
        }
    for (size_t f = 0; f < nf; ++f)
        for (int c = 0; c < 3; ++c)
            if (tri[3 * f + c] >= nv)
                return refuse(call, "face " + std::to_string(f) + " has vertex index " + std::to_string(tri[3 * f + c]) + ": the mesh has " + std::to_string(nv) + " vertices");
    if (const int rc = select_device(call, device)) return rc;

    const MdHostTree h = md_build(vtx, tri, nf);
    if (h.faces == 0) return refuse(call, "the mesh has no area");
    float ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    if (!(ext > 0.0f) || !std::isfinite(ext)) ext = 1.0f;  // one point, or a box wider than fp32 holds: every code 0 or clamped, the order stays the callers'

    std::vector<double> own;  // max_dist2 needs every dist2, asked for or not; declared before the stream: it outlives every copy in flight
    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t nq32 = (uint32_t)nq;
    size_t sort_bytes = 0;
    ONECHK(call, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, nq, 0u, 30u, d.stream));
    float *d_box, *d_leaf_v, *d_qry, *d_closest;
    uint32_t *d_leaf_f, *key_a, *key_b, *idx_a, *idx_b, *d_face;
    double* d_dist2;
    uint8_t* d_region;
    int8_t* d_side;
    char* tmp;
    Arena plan;
    plan.take(d_box, h.box.size()); plan.take(d_leaf_v, h.leaf_v.size()); plan.take(d_leaf_f, h.leaf_f.size()); plan.take(d_qry, 3 * nq);
    plan.take(key_a, nq); plan.take(key_b, nq); plan.take(idx_a, nq); plan.take(idx_b, nq); plan.take(tmp, sort_bytes);
    plan.take(d_dist2, nq); plan.take(d_face, face ? nq : 0); plan.take(d_closest, closest ? 3 * nq : 0); plan.take(d_region, region ? nq : 0); plan.take(d_side, side ? nq : 0);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);

    ONECHK(call, hipMemcpyAsync(d_box, h.box.data(), 4 * h.box.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(d_leaf_v, h.leaf_v.data(), 4 * h.leaf_v.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(d_leaf_f, h.leaf_f.data(), 4 * h.leaf_f.size(), hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(d_qry, qry, 12 * nq, hipMemcpyHostToDevice, d.stream));
    const dim3 block(kMdBlock), grid((unsigned)((nq + kMdBlock - 1) / kMdBlock));
    hipLaunchKernelGGL(md_key_kernel, grid, block, 0, d.stream, d_qry, nq32, lo[0], lo[1], lo[2], ext, key_a, idx_a);
    ONECHK(call, rocprim::radix_sort_pairs(tmp, sort_bytes, key_a, key_b, idx_a, idx_b, nq, 0u, 30u, d.stream));
    const MdTree t{d_box, d_leaf_v, d_leaf_f, h.nleaves, h.depth};
    const MdOut o{d_face, d_closest, d_dist2, d_region, d_side};
    const double slack = kMdSlack * (double)big;
    if (flags & FGOICP_MESH_DISTANCE_BRUTE) hipLaunchKernelGGL(md_kernel<true>, grid, block, 0, d.stream, t, d_qry, idx_b, nq32, slack, o);
    else hipLaunchKernelGGL(md_kernel<false>, grid, block, 0, d.stream, t, d_qry, idx_b, nq32, slack, o);
    double* h_dist2 = dist2;
    if (!h_dist2) {
        own.resize(nq);
        h_dist2 = own.data();
    }
    ONECHK(call, hipMemcpyAsync(h_dist2, d_dist2, 8 * nq, hipMemcpyDeviceToHost, d.stream));
    if (face) ONECHK(call, hipMemcpyAsync(face, d_face, 4 * nq, hipMemcpyDeviceToHost, d.stream));
    if (closest) ONECHK(call, hipMemcpyAsync(closest, d_closest, 12 * nq, hipMemcpyDeviceToHost, d.stream));
    if (region) ONECHK(call, hipMemcpyAsync(region, d_region, nq, hipMemcpyDeviceToHost, d.stream));
    if (side) ONECHK(call, hipMemcpyAsync(side, d_side, nq, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());

    fgoicp_mesh_distance_info_t full{};
    full.flags = flags;
    full.vertices = nv;
    full.triangles = nf;
    full.queries = nq;
    full.faces = h.faces;
    full.zero_area = h.zero_area;
    full.tree_depth = (uint32_t)h.depth;
    full.leaf_faces = (uint32_t)kMdLeaf;
    full.max_dist2 = h_dist2[0];
    for (size_t i = 1; i < nq; ++i)
        if (h_dist2[i] > full.max_dist2) {  // strict: the lowest index that attains it
            full.max_dist2 = h_dist2[i];
            full.max_dist2_index = i;
        }
    write_info(out, full);
    return FGOICP_OK;
}

int point_triangle_impl(const float* p, const float* a, const float* b, const float* c, float* closest, double* dist2, int* region, int* side) {
    const char* const call = "fgoicp_point_triangle";
    if (!p || !a || !b || !c) return refuse(call, "p3, a3, b3 and c3 must not be null");
    for (const float* x : {p, a, b, c})
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(x[k])) return refuse(call, "a coordinate is not finite");
    const PtResult r = point_triangle(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
    if (closest) {
        closest[0] = (float)r.cx; closest[1] = (float)r.cy; closest[2] = (float)r.cz;
    }
    if (dist2) *dist2 = r.d2;
    if (region) *region = r.region;
    if (side) *side = pt_side(p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], r);
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_mesh_distance(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, const float* queries_nq3, size_t nq, uint32_t flags, int device,
                                    uint32_t* face_nq, float* closest_nq3, double* dist2_nq, uint8_t* region_nq, int8_t* side_nq, fgoicp_mesh_distance_info_t* info) {
    return fgoicp::abi_guard("fgoicp_mesh_distance", [&] {
        return fgoicp::mesh_distance_impl(vertices_nv3, nv, triangles_nf3, nf, queries_nq3, nq, flags, device, face_nq, closest_nq3, dist2_nq, region_nq, side_nq, info);
    });
}

extern "C" int fgoicp_point_triangle(const float* p3, const float* a3, const float* b3, const float* c3, float* closest3, double* dist2, int* region, int* side) {
    return fgoicp::abi_guard("fgoicp_point_triangle", [&] { return fgoicp::point_triangle_impl(p3, a3, b3, c3, closest3, dist2, region, side); });
}
