// pose_mask_gate.h -- the depth gate of masks from poses (include/roft_engine.h, section 3e): WHICH frame's depth a silhouette is
// compared with.  Host only, no HIP: tests/cpp/pose_mask_gate_check.cpp builds against this header alone.
//
// A pose that arrives on frame k was computed on an older image; the mask chain says how much older by the flows it chases the new
// mask through.  n = the buffered flows that chase will use -- n_flows - start of oracle/ro_mask.c:44-48, 0 under the first-mask
// rule --, and the gate frame is the object's frame just before the frame that delivered the oldest of those n flows: frame k - n
// with a complete flow stream, the frame the chase itself starts from with dropped flow frames.  n == 0: frame k's own depth.
#pragma once

#include <cmath>

namespace roft {
namespace host {

// keep(R, D) of the contract, as the kernels evaluate it (floats; each bound rounded once; built without contraction)
inline bool pose_mask_gate_keep(float R, float D, float tf, float tb)
{
    const float lo = R - tf, hi = R + tb;
    return !(D > 0.0f && D < lo) && !(tb > 0.0f && D > hi);
}

// The flows the chase of a new mask uses.  buffered: flows in the source's buffer with this frame's own flow counted in
// (decide_mode's n_avail, roft_device.h); frames_between: roft_config::mask_frames_between (<= 0: unknown, all of them);
// n_hist: the entries the history can supply (the device clamps to it as well).
inline int pose_mask_chase_flows(int n_hist, int frames_between, int buffered, bool first_mask)
{
    if (first_mask) return 0;
    int n = buffered;
    if (frames_between > 0 && n > frames_between) n = frames_between;
    if (n > n_hist) n = n_hist;
    return n < 0 ? 0 : n;
}

// The history entry (Sched::hist, newest first) whose FlowEntry::depth_before is the gate image; -1: the frame's own depth.
inline int pose_mask_gate_entry(int n_hist, int frames_between, int buffered, bool first_mask)
{
    return pose_mask_chase_flows(n_hist, frames_between, buffered, first_mask) - 1;
}

// the tolerances an engine or the operator accepts (section 3e): front finite and > 0, behind finite (<= 0: that test is off)
inline bool pose_mask_gate_valid(float front_tolerance, float behind_tolerance)
{
    return std::isfinite(front_tolerance) && front_tolerance > 0.0f && std::isfinite(behind_tolerance);
}

}  // namespace host
}  // namespace roft
