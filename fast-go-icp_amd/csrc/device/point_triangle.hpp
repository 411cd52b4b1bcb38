// The closest point of a triangle to a point (fgoicp_mesh_distance, fgoicp_point_triangle; include/fgoicp_amd.h has the definition).
// One text: the kernels of mesh_distance.hip compile it for the device, fgoicp_point_triangle for the host.  IEEE fp64 on fp32 inputs, every
// operation rounded once in the order written (the build passes -ffp-contract=off), real divisions.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FGOICP_PT_HD __host__ __device__
#else
#define FGOICP_PT_HD
#endif

namespace fgoicp {

struct PtResult {
    double cx, cy, cz;  // the closest point, fp64
    double d2;          // |p - closest|^2
    int region;         // 0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c
};

FGOICP_PT_HD inline double pt_dot(double x, double y, double z, double u, double v, double w) { return (x * u + y * v) + z * w; }

FGOICP_PT_HD inline PtResult pt_at(double px, double py, double pz, double cx, double cy, double cz, int region) {
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    return PtResult{cx, cy, cz, pt_dot(dx, dy, dz, dx, dy, dz), region};
}

// the segment x -> y, for the fall-back of the interior branch: t = e.w / e.e clamped, an end of the segment returned as the vertex itself
FGOICP_PT_HD inline PtResult pt_segment(double px, double py, double pz, double xx, double xy, double xz, double yx, double yy, double yz, int edge, int vx, int vy) {
    const double ex = yx - xx, ey = yy - xy, ez = yz - xz;
    const double num = pt_dot(ex, ey, ez, px - xx, py - xy, pz - xz), den = pt_dot(ex, ey, ez, ex, ey, ez);
    if (!(num > 0.0)) return pt_at(px, py, pz, xx, xy, xz, vx);
    if (!(num < den)) return pt_at(px, py, pz, yx, yy, yz, vy);
    const double t = num / den;
    return pt_at(px, py, pz, xx + t * ex, xy + t * ey, xz + t * ez, edge);
}

// Ericson's seven regions in his order (Real-Time Collision Detection 5.1.5).  A quotient whose denominator is 0 is taken as 0 (the edge's
// first vertex).  The interior is accepted when s > 0 and v = vb / s, w = vc / s satisfy v >= 0, w >= 0, v + w <= 1; otherwise (a sliver
// whose va, vb, vc are rounding noise) the answer is the nearest of the three edges as segments, ab, bc, ca, a tie going to the lowest
// region code.  Every branch therefore returns a + v ab + w ac with computed weights inside the triangle: the returned point is never
// farther than rounding from the face, which is what the pruning argument of mesh_distance.hip rests on.
FGOICP_PT_HD inline PtResult point_triangle(double px, double py, double pz, double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz,
                                            bool* fell_back = nullptr) {
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double d1 = pt_dot(abx, aby, abz, apx, apy, apz), d2 = pt_dot(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0 && d2 <= 0.0) return pt_at(px, py, pz, ax, ay, az, 4);
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double d3 = pt_dot(abx, aby, abz, bpx, bpy, bpz), d4 = pt_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0 && d4 <= d3) return pt_at(px, py, pz, bx, by, bz, 5);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double den = d1 - d3, t = den == 0.0 ? 0.0 : d1 / den;
        return pt_at(px, py, pz, ax + t * abx, ay + t * aby, az + t * abz, 1);
    }
    const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
    const double d5 = pt_dot(abx, aby, abz, cpx, cpy, cpz), d6 = pt_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0 && d5 <= d6) return pt_at(px, py, pz, cx, cy, cz, 6);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double den = d2 - d6, t = den == 0.0 ? 0.0 : d2 / den;
        return pt_at(px, py, pz, ax + t * acx, ay + t * acy, az + t * acz, 3);
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
        const double den = (d4 - d3) + (d5 - d6), t = den == 0.0 ? 0.0 : (d4 - d3) / den;
        return pt_at(px, py, pz, bx + t * (cx - bx), by + t * (cy - by), bz + t * (cz - bz), 2);
    }
    const double s = (va + vb) + vc;
    if (s > 0.0) {
        const double v = vb / s, w = vc / s;
        if (v >= 0.0 && w >= 0.0 && v + w <= 1.0) return pt_at(px, py, pz, (ax + v * abx) + w * acx, (ay + v * aby) + w * acy, (az + v * abz) + w * acz, 0);
    }
    if (fell_back) *fell_back = true;
    PtResult best = pt_segment(px, py, pz, ax, ay, az, bx, by, bz, 1, 4, 5);
    const PtResult r2 = pt_segment(px, py, pz, bx, by, bz, cx, cy, cz, 2, 5, 6), r3 = pt_segment(px, py, pz, cx, cy, cz, ax, ay, az, 3, 6, 4);
    if (r2.d2 < best.d2 || (r2.d2 == best.d2 && r2.region < best.region)) best = r2;
    if (r3.d2 < best.d2 || (r3.d2 == best.d2 && r3.region < best.region)) best = r3;
    return best;
}

// side: the sign of n.(p - closest), n = ab x ac as fgoicp_mesh_sample forms it
FGOICP_PT_HD inline int pt_side(double px, double py, double pz, double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz,
                                const PtResult& r) {
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double h = pt_dot(nx, ny, nz, px - r.cx, py - r.cy, pz - r.cz);
    return h > 0.0 ? 1 : h < 0.0 ? -1 : 0;
}

}  // namespace fgoicp
