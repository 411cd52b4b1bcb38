// The host state of IterativeClosestPoint3D::run() (fgoicp/icp3d.cu:80-108), ONE text for every driver of the loop (ctx.hip: lane_icp,
// lane_icp_dual, ctx_icp_coop, ctx_icp_step) and for the CPU harness that runs it over the oracle's operators.  No device, no HIP headers.
//     begin(R0, t0, max_iter, thr);                  // :88-93 (the caller moves its working cloud by (R0, t0), :85)
//     while (next()) {                               // :94-97
//         (Rn, tn) = procrustes();  move the working cloud by (Rn, tn);   // :98-100, the caller's
//         compose(Rn, tn);                           // :101-102
//         took(compute_sse_error(R, t));             // :103
//     }
//     result(...);                                   // :106-107
// rides(), between compose() and took(): the loop can make another iteration, so its correspondence pass may be enqueued next to this
// iteration's SSE (speculative: the loop may still end on that SSE).  `cur` names the correspondence buffer the last pass wrote; a pass
// that rides along writes the other one (flip()) — a pass never seeds from the buffer it writes.
#pragma once
#include <cstddef>
#include <cstring>

#include "math3.hpp"

namespace fgoicp {

struct IcpLoop {
    Mat3f R = Mat3f::identity(), last_R = Mat3f::identity();
    Vec3f t{0, 0, 0}, last_t{0, 0, 0};
    float sse = 1E+10f, last_sse = 2.0f * 1E+10f, thr = 0.f;  // M_INF, fgoicp/common.hpp:18
    size_t iter = 0, max_iter = 0;
    int iters = 0, cur = 0;

    void begin(const float* R0, const float* t0, size_t max_iter_, float thr_) {
        *this = IcpLoop();
        R = Mat3f::from(R0);
        t = Vec3f{t0[0], t0[1], t0[2]};
        max_iter = max_iter_;
        thr = thr_;
    }
    bool next() {
        if (!(iter++ < max_iter && (last_sse - sse) > thr * last_sse)) return false;  // :94
        last_sse = sse;
        last_R = R;
        last_t = t;
        return true;
    }
    void compose(const Mat3f& Rn, Vec3f tn) {
        R = Rn * R;       // :101
        t = Rn * t + tn;  // :102
    }
    bool rides() const { return iter < max_iter; }
    void took(float sse_now) {
        sse = sse_now;
        ++iters;
    }
    int flip() { return cur ^= 1; }
    void result(float* sse_out, float* R_out9, float* t_out3, int* iters_out) const {
        const bool cur_best = sse < last_sse;  // :106-107
        *sse_out = cur_best ? sse : last_sse;
        const Mat3f& Ro = cur_best ? R : last_R;
        const Vec3f& to = cur_best ? t : last_t;
        std::memcpy(R_out9, Ro.m, sizeof(Ro.m));
        t_out3[0] = to.x; t_out3[1] = to.y; t_out3[2] = to.z;
        if (iters_out) *iters_out = iters;
    }
};

}  // namespace fgoicp
