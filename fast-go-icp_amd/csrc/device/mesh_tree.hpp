// The face tree of a triangle mesh and the wave-uniform walk over it (mesh_distance.hip, mesh_refine.hip; DESIGN.md section 22 has the
// pruning argument).  ONE text for both calls: the tree a mesh gets, the boxes that are entered and the faces that are tested do not depend
// on which of them asks.
//
//   host      md_build: the faces whose n2 is not 0, sorted along the curve of morton.hpp by their centroid, in leaves of kMdLeaf faces
//             (their nine coordinates expanded, so a leaf is one run of memory) under an implicit heap-ordered binary tree of fp32 boxes
//             (min and max round nothing)
//   keys      md_key_kernel, one thread per point: a 30-bit Z-order code inside the points' own box
//   walk      md_walk, one wave per 64 sorted points: a wave-uniform depth-first walk, the nearer child (by the lanes' vote) first; a node
//             is entered when ANY lane cannot rule its box out, a leaf's faces are tested by the lanes that cannot.  The stack (at most
//             depth + 1 nodes) is per wave, in LDS; no loop waits on another wave
//   brute     md_brute: the same leaves, the same leaf code, every leaf for every lane, no boxes
//
// The winner of a point is the smallest (dist2, face index) — a total order — so it does not depend on the order in which the faces are
// met, and a box is skipped only when every face inside it loses STRICTLY (md_box_d2): the walk returns the bytes of the brute search.
// Everything here has internal linkage, as one_shot.hpp: each translation unit carries its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "morton.hpp"
#include "point_triangle.hpp"

namespace fgoicp {
namespace {

constexpr int kMdBlock = 256;
constexpr int kMdLeaf = 8;     // faces per leaf: 288 bytes of coordinates and 32 of indices, read through wave-uniform addresses
constexpr int kMdStack = 32;   // nf < 2^31 and 8 faces per leaf: at most 2^28 leaves, depth <= 28, and the walk holds at most depth + 1 nodes
constexpr uint32_t kMdNone = 0xFFFFFFFFu;  // the face index of an unused slot of the last leaf
// The pruning margins (DESIGN.md section 22 derives them).  A point returned by point_triangle lies within 21 u M of its face (u = 2^-53,
// M = the largest |coordinate| of the call), and the subtractions in front of a gap add 4 u M: kMdSlack * M = 64 u M is taken off every
// axis gap of a box.  The squared distances on the two sides of the comparison carry ten roundings between them: the box's is shrunk
// by 32 u.
constexpr double kMdSlack = 0x1p-47;
constexpr double kMdShrink = 1.0 - 0x1p-48;

struct MdTree {
    const float* box;         // 6 floats per node, lo then hi; node i has the children 2 i + 1 and 2 i + 2, the leaves start at (1 << depth) - 1
    const float* leaf_v;      // 9 floats per slot: a, b, c
    const uint32_t* leaf_f;   // the caller's face index per slot, kMdNone beyond the last face
    uint32_t nleaves;         // leaves 0 .. nleaves - 1 hold faces
    int depth;
};

__device__ __forceinline__ uint32_t md_expand10(uint32_t v) {
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x030000FF;
    v = (v | (v << 8)) & 0x0300F00F;
    v = (v | (v << 4)) & 0x030C30C3;
    v = (v | (v << 2)) & 0x09249249;
    return v;
}

// lo3 / ext: the points' box and its longest side (ext > 0; a single point sorts as it stands).  Only locality depends on the code.
__global__ __launch_bounds__(kMdBlock) void md_key_kernel(const float* __restrict__ q, uint32_t nq, float lox, float loy, float loz, float ext, uint32_t* __restrict__ key,
                                                         uint32_t* __restrict__ idx) {
    const size_t i = (size_t)blockIdx.x * kMdBlock + threadIdx.x;
    if (i >= nq) return;
    const float* p = q + 3 * i;
    const uint32_t cx = (uint32_t)fminf(1023.0f, fmaxf(0.0f, (p[0] - lox) / ext * 1023.0f));
    const uint32_t cy = (uint32_t)fminf(1023.0f, fmaxf(0.0f, (p[1] - loy) / ext * 1023.0f));
    const uint32_t cz = (uint32_t)fminf(1023.0f, fmaxf(0.0f, (p[2] - loz) / ext * 1023.0f));
    key[i] = md_expand10(cx) | (md_expand10(cy) << 1) | (md_expand10(cz) << 2);
    idx[i] = (uint32_t)i;
}

// The squared distance from p to the box, every axis gap first reduced by `slack` (>= the distance a computed closest point may lie from
// its face): a lower bound, after the factor kMdShrink, of the dist2 point_triangle computes for ANY face inside the box.
__device__ __forceinline__ double md_box_d2(const float* __restrict__ b, double px, double py, double pz, double slack) {
    const double dx = fmax(fmax((double)b[0] - px, px - (double)b[3]) - slack, 0.0);
    const double dy = fmax(fmax((double)b[1] - py, py - (double)b[4]) - slack, 0.0);
    const double dz = fmax(fmax((double)b[2] - pz, pz - (double)b[5]) - slack, 0.0);
    return (dx * dx + dy * dy) + dz * dz;
}

struct MdBest {
    double d2;
    uint32_t face, slot;
};

// the faces of leaf l (wave-uniform) for the lanes that need it
__device__ __forceinline__ void md_leaf(const MdTree& t, uint32_t l, bool need, double px, double py, double pz, MdBest& best) {
    const float* __restrict__ v = t.leaf_v + (size_t)l * (kMdLeaf * 9);
    const uint32_t* __restrict__ f = t.leaf_f + (size_t)l * kMdLeaf;
    for (int k = 0; k < kMdLeaf; ++k) {
        const uint32_t face = f[k];
        if (face == kMdNone) break;  // the same for the whole wave
        if (need) {
            const float* c = v + 9 * k;
            const PtResult r = point_triangle(px, py, pz, (double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4], (double)c[5], (double)c[6], (double)c[7],
                                              (double)c[8]);
            if (r.d2 < best.d2 || (r.d2 == best.d2 && face < best.face)) {
                best.d2 = r.d2;
                best.face = face;
                best.slot = l * kMdLeaf + (uint32_t)k;
            }
        }
    }
}

__device__ __forceinline__ MdBest md_none() { return MdBest{__longlong_as_double(0x7FF0000000000000ll), kMdNone, 0u}; }  // +inf: no box is ruled out before the first leaf

// every leaf for every active lane, no boxes
__device__ __forceinline__ MdBest md_brute(const MdTree& t, double px, double py, double pz, bool active) {
    MdBest best = md_none();
    for (uint32_t l = 0; l < t.nleaves; ++l) md_leaf(t, l, active, px, py, pz, best);
    return best;
}

// The walk of one wave; every lane of the wave calls this, `stack` is the wave's own kMdStack words of LDS.  An inactive lane (one beyond
// the points) votes for nothing and tests nothing.
__device__ __forceinline__ MdBest md_walk(const MdTree& t, double px, double py, double pz, double slack, uint32_t* stack, bool active) {
    MdBest best = md_none();
    const uint32_t first_leaf = (1u << t.depth) - 1u;
    // whether node (at `level`) holds any face: its first leaf is the node's position in its level shifted down to the leaves
    auto empty = [&](uint32_t node, int level) { return ((node + 1u - (1u << level)) << (t.depth - level)) >= t.nleaves; };
    int sp = 0;
    stack[sp++] = 0u;  // every lane writes the same word: each lane later reads what it wrote itself
    while (sp > 0) {  // every node is pushed at most once: at most 2^(depth + 1) - 1 turns
        const uint32_t node = (uint32_t)__builtin_amdgcn_readfirstlane((int)stack[--sp]);
        const double d = md_box_d2(t.box + 6 * (size_t)node, px, py, pz, slack);
        const bool need = active && !(d * kMdShrink > best.d2);  // strict: a face that would tie is never skipped
        if (!__any(need)) continue;
        if (node >= first_leaf) {
            md_leaf(t, node - first_leaf, need, px, py, pz, best);
            continue;
        }
        const uint32_t c0 = 2u * node + 1u, c1 = c0 + 1u;
        const int level = 32 - __clz((int)(node + 1u));  // of the children
        if (empty(c1, level)) {  // the tree is filled from the left: c0 holds faces whenever its parent does
            stack[sp++] = c0;
            continue;
        }
        const double d0 = md_box_d2(t.box + 6 * (size_t)c0, px, py, pz, slack), d1 = md_box_d2(t.box + 6 * (size_t)c1, px, py, pz, slack);
        const bool first0 = 2 * __popcll(__ballot(need && d0 <= d1)) >= __popcll(__ballot(need));  // the nearer child for most lanes: popped first
        stack[sp++] = first0 ? c1 : c0;
        stack[sp++] = first0 ? c0 : c1;
    }
    return best;
}

struct MdHostTree {
    std::vector<float> box, leaf_v;
    std::vector<uint32_t> leaf_f;
    uint64_t faces = 0, zero_area = 0;
    uint32_t nleaves = 0;
    int depth = 0;
};

// n2 of fgoicp_mesh_sample's area formula: the faces where it is 0 take no part
double md_n2(const float* a, const float* b, const float* c) {
    const double ax = a[0], ay = a[1], az = a[2];
    const double e1x = (double)b[0] - ax, e1y = (double)b[1] - ay, e1z = (double)b[2] - az;
    const double e2x = (double)c[0] - ax, e2y = (double)c[1] - ay, e2z = (double)c[2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    return (nx * nx + ny * ny) + nz * nz;
}

MdHostTree md_build(const float* vtx, const uint32_t* tri, size_t nf) {
    MdHostTree h;
    std::vector<uint32_t> part;  // the participating faces, ascending
    part.reserve(nf);
    for (size_t f = 0; f < nf; ++f) {
        if (md_n2(vtx + 3 * (size_t)tri[3 * f], vtx + 3 * (size_t)tri[3 * f + 1], vtx + 3 * (size_t)tri[3 * f + 2]) == 0.0) ++h.zero_area;
        else part.push_back((uint32_t)f);
    }
    h.faces = part.size();
    if (part.empty()) return h;
    std::vector<float> centre(3 * part.size());
    for (size_t k = 0; k < part.size(); ++k)
        for (int a = 0; a < 3; ++a) {
            const size_t f = part[k];
            centre[3 * k + a] = (float)(((double)vtx[3 * (size_t)tri[3 * f] + a] + (double)vtx[3 * (size_t)tri[3 * f + 1] + a] + (double)vtx[3 * (size_t)tri[3 * f + 2] + a]) / 3.0);
        }
    const std::vector<uint32_t> perm = morton_order(centre.data(), part.size(), 3);  // stable: a function of the mesh alone
    h.nleaves = (uint32_t)((part.size() + kMdLeaf - 1) / kMdLeaf);
    while (((size_t)1 << h.depth) < h.nleaves) ++h.depth;
    const size_t cap = (size_t)1 << h.depth, first_leaf = cap - 1, nodes = 2 * cap - 1;
    const float inf = std::numeric_limits<float>::infinity();
    h.box.resize(6 * nodes);
    for (size_t n = 0; n < nodes; ++n)
        for (int a = 0; a < 3; ++a) {
            h.box[6 * n + a] = inf;
            h.box[6 * n + 3 + a] = -inf;
        }
    h.leaf_v.assign((size_t)h.nleaves * kMdLeaf * 9, 0.0f);
    h.leaf_f.assign((size_t)h.nleaves * kMdLeaf, kMdNone);
    for (size_t k = 0; k < perm.size(); ++k) {
        const size_t f = part[perm[k]];
        float* b = &h.box[6 * (first_leaf + k / kMdLeaf)];
        h.leaf_f[k] = (uint32_t)f;
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) {
                const float x = vtx[3 * (size_t)tri[3 * f + c] + a];
                h.leaf_v[9 * k + 3 * c + a] = x;
                b[a] = std::min(b[a], x);
                b[3 + a] = std::max(b[3 + a], x);
            }
    }
    for (size_t n = first_leaf; n-- > 0;)
        for (int a = 0; a < 3; ++a) {
            h.box[6 * n + a] = std::min(h.box[6 * (2 * n + 1) + a], h.box[6 * (2 * n + 2) + a]);
            h.box[6 * n + 3 + a] = std::max(h.box[6 * (2 * n + 1) + 3 + a], h.box[6 * (2 * n + 2) + 3 + a]);
        }
    return h;
}

}  // namespace
}  // namespace fgoicp
