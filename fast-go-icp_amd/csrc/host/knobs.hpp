// Development knobs.  Rounds 1-3 grew environment variables that select layouts, schedules, work sizes and thresholds for A/B runs;
// every default is the measured best (NOTES.md).  A shipped library must not change its code path because a stray variable is set
// (VERDICT r03 #7), so the DEFAULT build reads none of them: dev_env() is a constant nullptr there — the variable names do not even
// reach the binary.  The kernel variants that were measured and rejected have been retired from the tree (NOTES.md).  The development build
// (fgoicp_amd.build.build(dev=True): -DFGOICP_DEV_KNOBS -> libfgoicp_amd_dev.so, loaded with FGOICP_LIB) reads them as before; the
// A/B scripts under tools/ and the tests marked `dev_knobs` use it.
// What the default build does read from the environment: FGOICP_HOST_THREADS, FGOICP_HOST_SPIN (host-thread deployment of the driver's
// worker pool) and, in the CLI, FGOICP_MULTI_DEVICES (the device list of --gpus).
#pragma once
#include <climits>
#include <cstdlib>

namespace fgoicp {
#ifdef FGOICP_DEV_KNOBS
constexpr bool kDevKnobs = true;
inline const char* dev_env(const char* name) { return std::getenv(name); }
// An integer development knob: the variable's value where it lies in [lo, hi], `outside` where it does not, `unset` where the
// variable is not set.  The rules of the knobs differ in what a value out of range means (the default, or 0 = off): each call says so.
inline int dev_int(const char* name, int unset, int lo = INT_MIN, int hi = INT_MAX, int outside = 0) {
    const char* e = dev_env(name);
    if (!e) return unset;
    const int v = std::atoi(e);
    return v >= lo && v <= hi ? v : outside;
}
#else
constexpr bool kDevKnobs = false;
constexpr const char* dev_env(const char*) { return nullptr; }
constexpr int dev_int(const char*, int unset, int = INT_MIN, int = INT_MAX, int = 0) { return unset; }
#endif
}  // namespace fgoicp
