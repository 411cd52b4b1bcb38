// Surface sampling of a triangle mesh (fgoicp_mesh_sample; include/fgoicp_amd.h has the definition, DESIGN.md section 21 the launch chain).
// A one-shot call: the frame every such call shares — what it owns, the common refusals, the arena — is one_shot.hpp.
//
//   host      the refusals (they need no device): the vertices are finite, every index names a vertex
//   areas     mesh_area_kernel, one thread per face: area_f in fp64 and the largest of them, A_max — a wave reduction of the bit patterns
//             (a non-negative double orders as its bits do), one slot per wave in LDS, one integer atomicMax per block
//   weights   mesh_weight_kernel: q_f = floor(area_f / A_max * 2^32) and the two counts (zero-area faces, faces of weight 0), one integer
//             atomicAdd per wave; then rocprim::inclusive_scan over the 64-bit q: integer sums, exact however the device associates them
//   host      reads A_max, weight_total and the counts back; A_max == 0 ends the call here
//   samples   mesh_sample_kernel, one thread per sample k: three counter-based hashes, a binary search over the scan for the face
//             (ceil(log2 nf) dependent 8-byte loads), the gather of the face and the outputs
//
// Nothing is summed in floating point and no draw depends on another: sample k is a function of (mesh, seed, k), the outputs of the inputs alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../host/segment.hpp"
#include "one_shot.hpp"

namespace fgoicp {
namespace {

constexpr int kMeshBlock = 256;
constexpr double kMeshTwo32 = 4294967296.0;

struct MeshFace {  // the face as every kernel sees it: corner a, the two edges from it and their cross product, all fp64 (fp32 -> fp64 is exact)
    double ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz, n2;
};

// three index loads, three 12-byte gathers; every operation rounds once (the build passes -ffp-contract=off)
__device__ __forceinline__ MeshFace mesh_face(const float* __restrict__ vtx, const uint32_t* __restrict__ tri, size_t f) {
    const uint32_t ia = tri[3 * f], ib = tri[3 * f + 1], ic = tri[3 * f + 2];
    const float *pa = vtx + 3 * (size_t)ia, *pb = vtx + 3 * (size_t)ib, *pc = vtx + 3 * (size_t)ic;
    MeshFace m;
    m.ax = (double)pa[0]; m.ay = (double)pa[1]; m.az = (double)pa[2];
    m.e1x = (double)pb[0] - m.ax; m.e1y = (double)pb[1] - m.ay; m.e1z = (double)pb[2] - m.az;
    m.e2x = (double)pc[0] - m.ax; m.e2y = (double)pc[1] - m.ay; m.e2z = (double)pc[2] - m.az;
    m.nx = m.e1y * m.e2z - m.e1z * m.e2y;
    m.ny = m.e1z * m.e2x - m.e1x * m.e2z;
    m.nz = m.e1x * m.e2y - m.e1y * m.e2x;
    m.n2 = (m.nx * m.nx + m.ny * m.ny) + m.nz * m.nz;
    return m;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// area[f] and *max_bits = the bits of the largest area (zeroed before the launch).  The vertices are finite fp32, so every area is a finite
// double >= +0.0 (|n|^2 stays below 1e157): its bits order as the values do.
__global__ __launch_bounds__(kMeshBlock) void mesh_area_kernel(const float* __restrict__ vtx, const uint32_t* __restrict__ tri, uint32_t nf, double* __restrict__ area,
                                                              unsigned long long* __restrict__ max_bits) {
    __shared__ unsigned long long s_max[kMeshBlock / 64];
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    unsigned long long bits = 0ull;
    if (f < nf) {
        const MeshFace m = mesh_face(vtx, tri, f);
        const double a = 0.5 * sqrt(m.n2);
        area[f] = a;
        bits = (unsigned long long)__double_as_longlong(a);
    }
    bits = wave_max_u64(bits);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = s_max[0];
#pragma unroll
        for (int w = 1; w < kMeshBlock / 64; ++w) r = s_max[w] > r ? s_max[w] : r;
        if (r != 0ull) atomicMax(max_bits, r);
    }
}

// q[f] and counts = {faces of area 0, faces of weight 0}.  A_max == 0 (the host then refuses the mesh) gives every face the weight 0.
__global__ __launch_bounds__(kMeshBlock) void mesh_weight_kernel(const double* __restrict__ area, uint32_t nf, const unsigned long long* __restrict__ max_bits,
                                                                unsigned long long* __restrict__ q, unsigned long long* __restrict__ counts) {
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const double amax = __longlong_as_double((long long)*max_bits);
    bool zero = false, unweighted = false;
    if (f < nf) {
        const double a = area[f];
        const unsigned long long w = amax > 0.0 ? (unsigned long long)floor(a / amax * kMeshTwo32) : 0ull;
        q[f] = w;
        zero = a == 0.0;
        unweighted = w == 0ull;
    }
    const unsigned long long nz = __popcll(__ballot(zero)), nu = __popcll(__ballot(unweighted));
    if ((threadIdx.x & 63) == 0) {
        if (nz) atomicAdd(&counts[0], nz);
        if (nu) atomicAdd(&counts[1], nu);
    }
}

// Sample k.  scan[f] = Q[f], total = Q[nf - 1] > 0.  normals, face, uv: nullptr = not asked for (the same way for the whole grid).
__global__ __launch_bounds__(kMeshBlock) void mesh_sample_kernel(const float* __restrict__ vtx, const uint32_t* __restrict__ tri, uint32_t nf,
                                                                const unsigned long long* __restrict__ scan, unsigned long long total, uint64_t seed, uint32_t m,
                                                                float* __restrict__ points, float* __restrict__ normals, uint32_t* __restrict__ face, double* __restrict__ uv) {
    const size_t k = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (k >= m) return;
    const uint64_t c = 3ull * (uint64_t)k;
    const uint64_t h0 = seg_mix64(seed + 0x9E3779B97F4A7C15ull * (c + 1ull)), h1 = seg_mix64(seed + 0x9E3779B97F4A7C15ull * (c + 2ull)),
                   h2 = seg_mix64(seed + 0x9E3779B97F4A7C15ull * (c + 3ull));
    const unsigned long long r = __umul64hi(h0, total);  // < total = scan[nf - 1]: the search ends on a face
    uint32_t lo = 0u, hi = nf - 1u;
    while (lo < hi) {  // the first f with scan[f] > r; lo <= mid < hi <= nf - 1
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (scan[mid] > r) hi = mid;
        else lo = mid + 1u;
    }
    const MeshFace t = mesh_face(vtx, tri, lo);
    double u = (double)(h1 >> 11) * 0x1p-53, v = (double)(h2 >> 11) * 0x1p-53;
    if (u + v > 1.0) {
        u = 1.0 - u;
        v = 1.0 - v;
    }
    float* p = points + 3 * k;
    p[0] = (float)((t.ax + u * t.e1x) + v * t.e2x);
    p[1] = (float)((t.ay + u * t.e1y) + v * t.e2y);
    p[2] = (float)((t.az + u * t.e1z) + v * t.e2z);
    if (normals) {
        const double len = sqrt(t.n2);
        float* o = normals + 3 * k;
        o[0] = (float)(t.nx / len); o[1] = (float)(t.ny / len); o[2] = (float)(t.nz / len);
    }
    if (face) face[k] = lo;
    if (uv) {
        uv[2 * k] = u;
        uv[2 * k + 1] = v;
    }
}

int mesh_sample_impl(const float* vtx, size_t nv, const uint32_t* tri, size_t nf, size_t m, uint64_t seed, int device, float* points, float* normals, uint32_t* face, double* uv,
                     double* face_area, fgoicp_mesh_info_t* out) {
    const char* const call = "fgoicp_mesh_sample";
    constexpr size_t kLimit = (size_t)1 << 31;
    if (!vtx || nv == 0) return refuse(call, "the vertices must not be null or empty");
    if (!tri || nf == 0) return refuse(call, "the triangles must not be null or empty");
    if (nv >= kLimit) return refuse(call, "more than 2^31 - 1 vertices");
    if (nf >= kLimit) return refuse(call, "more than 2^31 - 1 triangles");
    if (m == 0 || m >= kLimit) return refuse(call, "the sample count must lie in [1, 2^31 - 1]");
    if (!points) return refuse(call, "points_m3 must not be null");
    if (const int rc = refuse_info(call, out, offsetof(fgoicp_mesh_info_t, area) + sizeof(double), "fgoicp_mesh_info_t")) return rc;
    for (size_t i = 0; i < nv; ++i)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(vtx[3 * i + a])) return refuse(call, "vertex " + std::to_string(i) + " has a non-finite coordinate");
    for (size_t f = 0; f < nf; ++f)
        for (int c = 0; c < 3; ++c)
            if (tri[3 * f + c] >= nv)
                return refuse(call, "face " + std::to_string(f) + " has vertex index " + std::to_string(tri[3 * f + c]) + ": the mesh has " + std::to_string(nv) + " vertices");
    if (const int rc = select_device(call, device)) return rc;

    OneShot d(call);
    ONECHK(call, d.stream.create(hipStreamNonBlocking));
    const uint32_t nf32 = (uint32_t)nf, m32 = (uint32_t)m;
    size_t scan_bytes = 0;
    ONECHK(call, rocprim::inclusive_scan(nullptr, scan_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, nf, rocprim::plus<unsigned long long>(), d.stream));
    float *d_vtx, *d_pts, *d_nrm;  // d_nrm, d_face, d_uv: nullptr unless asked for
    uint32_t *d_tri, *d_face;
    double *d_area, *d_uv;
    unsigned long long *d_q, *d_scan, *d_head;  // d_head = {bits of A_max, zero-area faces, faces of weight 0}
    char* tmp;
    Arena plan;
    plan.take(d_vtx, 3 * nv); plan.take(d_tri, 3 * nf); plan.take(d_area, nf); plan.take(d_q, nf); plan.take(d_scan, nf); plan.take(d_head, 3); plan.take(tmp, scan_bytes);
    plan.take(d_pts, 3 * m); plan.take(d_nrm, normals ? 3 * m : 0); plan.take(d_face, face ? m : 0); plan.take(d_uv, uv ? 2 * m : 0);
    const size_t total = plan.total();
    ONECHK(call, d.arena.alloc(total));
    plan.place(d.arena);

    ONECHK(call, hipMemcpyAsync(d_vtx, vtx, 12 * nv, hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemcpyAsync(d_tri, tri, 12 * nf, hipMemcpyHostToDevice, d.stream));
    ONECHK(call, hipMemsetAsync(d_head, 0, 24, d.stream));
    const dim3 block(kMeshBlock), per_face((unsigned)((nf + kMeshBlock - 1) / kMeshBlock)), per_sample((unsigned)((m + kMeshBlock - 1) / kMeshBlock));
    hipLaunchKernelGGL(mesh_area_kernel, per_face, block, 0, d.stream, d_vtx, d_tri, nf32, d_area, d_head);
    hipLaunchKernelGGL(mesh_weight_kernel, per_face, block, 0, d.stream, d_area, nf32, d_head, d_q, d_head + 1);
    ONECHK(call, rocprim::inclusive_scan(tmp, scan_bytes, d_q, d_scan, nf, rocprim::plus<unsigned long long>(), d.stream));
    unsigned long long h_head[3] = {0ull, 0ull, 0ull}, h_total = 0ull;
    ONECHK(call, hipMemcpyAsync(h_head, d_head, 24, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipMemcpyAsync(&h_total, d_scan + (nf - 1), 8, hipMemcpyDeviceToHost, d.stream));
    if (face_area) ONECHK(call, hipMemcpyAsync(face_area, d_area, 8 * nf, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());
    double max_area;
    std::memcpy(&max_area, &h_head[0], 8);
    if (!(max_area > 0.0)) return refuse(call, "the mesh has no area");
    if (h_total < (1ull << 32) || h_total > (unsigned long long)nf << 32 || h_head[1] > h_head[2] || h_head[2] >= nf) {  // the largest face alone weighs 2^32
        set_error("fgoicp_mesh_sample: the device returned inconsistent weights");
        return FGOICP_ERR_HIP;
    }

    hipLaunchKernelGGL(mesh_sample_kernel, per_sample, block, 0, d.stream, d_vtx, d_tri, nf32, d_scan, h_total, seed, m32, d_pts, d_nrm, d_face, d_uv);
    ONECHK(call, hipMemcpyAsync(points, d_pts, 12 * m, hipMemcpyDeviceToHost, d.stream));
    if (normals) ONECHK(call, hipMemcpyAsync(normals, d_nrm, 12 * m, hipMemcpyDeviceToHost, d.stream));
    if (face) ONECHK(call, hipMemcpyAsync(face, d_face, 4 * m, hipMemcpyDeviceToHost, d.stream));
    if (uv) ONECHK(call, hipMemcpyAsync(uv, d_uv, 16 * m, hipMemcpyDeviceToHost, d.stream));
    ONECHK(call, hipStreamSynchronize(d.stream));
    ONECHK(call, hipGetLastError());

    fgoicp_mesh_info_t full{};
    full.vertices = nv;
    full.triangles = nf;
    full.samples = m;
    full.zero_area = h_head[1];
    full.unweighted = h_head[2];
    full.weight_total = h_total;
    full.max_area = max_area;
    full.area = max_area * (double)h_total / kMeshTwo32;
    write_info(out, full);
    return FGOICP_OK;
}

}  // namespace
}  // namespace fgoicp

extern "C" int fgoicp_mesh_sample(const float* vertices_nv3, size_t nv, const uint32_t* triangles_nf3, size_t nf, size_t m, uint64_t seed, int device, float* points_m3,
                                  float* normals_m3_or_NULL, uint32_t* face_m_or_NULL, double* uv_m2_or_NULL, double* face_area_nf_or_NULL, fgoicp_mesh_info_t* info) {
    return fgoicp::abi_guard("fgoicp_mesh_sample", [&] {
        return fgoicp::mesh_sample_impl(vertices_nv3, nv, triangles_nf3, nf, m, seed, device, points_m3, normals_m3_or_NULL, face_m_or_NULL, uv_m2_or_NULL, face_area_nf_or_NULL, info);
    });
}
