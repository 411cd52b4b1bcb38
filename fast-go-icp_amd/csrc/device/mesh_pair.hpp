// What one (moved point, winning triangle) pair contributes to the point-to-mesh normal equations (fgoicp_mesh_moments, fgoicp_mesh_refine,
// fgoicp_mesh_pair_terms; include/fgoicp_amd.h has the definition, DESIGN.md section 23 the launch chain).  One text: the kernel of
// mesh_refine.hip compiles it for the device, fgoicp_mesh_pair_terms for the host.  IEEE fp64, every operation rounded once in the order
// written (the build passes -ffp-contract=off), real divisions and one correctly rounded sqrt per pair.
#pragma once
#include <cmath>

#include "../host/robust.hpp"
#include "point_triangle.hpp"

namespace fgoicp {

struct MeshPair {
    PtResult r;     // closest point, dist2, region
    double g[3];    // the direction
    double s, w;    // the residual and its weight (1 without a loss)
};

// v[0 .. 27] = the pair's 28 terms, times w unless loss is FGOICP_LOSS_NONE; v may be longer (the kernel's row carries two more sums).
// The triangle has area (n2 != 0): faces without take no part in a mesh.
template <int K>
FGOICP_PT_HD inline MeshPair mesh_pair_terms(double x, double y, double z, double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz, int loss,
                                             double scale, double (&v)[K]) {
    static_assert(K >= 28, "28 terms");
    MeshPair o;
    o.r = point_triangle(x, y, z, ax, ay, az, bx, by, bz, cx, cy, cz);
    const double dx = x - o.r.cx, dy = y - o.r.cy, dz = z - o.r.cz;
    if (o.r.region != 0 && o.r.d2 > 0.0) {  // off an edge or a vertex: the gradient of the distance field
        const double len = sqrt(o.r.d2);
        o.g[0] = dx / len; o.g[1] = dy / len; o.g[2] = dz / len;
    } else {  // the face's unit normal, n and n2 as fgoicp_mesh_sample forms them
        const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        o.g[0] = nx / len; o.g[1] = ny / len; o.g[2] = nz / len;
    }
    o.s = pt_dot(o.g[0], o.g[1], o.g[2], dx, dy, dz);
    const double J[6] = {y * o.g[2] - z * o.g[1], z * o.g[0] - x * o.g[2], x * o.g[1] - y * o.g[0], o.g[0], o.g[1], o.g[2]};
    int m = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) v[m++] = J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * o.s;
    v[27] = o.s * o.s;
    o.w = 1.0;
    if (loss != FGOICP_LOSS_NONE) {  // wave-uniform on the device
        o.w = robust_weight(loss, o.s, scale);
#pragma unroll
        for (int k = 0; k < 28; ++k) v[k] *= o.w;
    }
    return o;
}

}  // namespace fgoicp
