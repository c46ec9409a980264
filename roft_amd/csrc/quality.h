// quality.h -- track quality (include/roft_engine.h, section 3d): what k_quality.hip leaves per (frame, object) pair and how it is
// launched.  The kernel reads engine state -- the pair's control block, its object plane, its depth, the mesh, the log row -- and
// writes only its own records.
#pragma once

#include "raster_shape.h"
#include "roft_device.h"

namespace roft {

// The record as the kernel leaves it: the counts of roft_quality_record and the exact sum of |e| as the two integers of a
// LikelihoodSum; the host forms depth_err = LikelihoodSum::value(hi, lo) / n_depth (quality_record below).
struct QualityRaw {
    int32_t frame, n_mask, n_render, n_both, n_depth, n_front, n_behind, reserved;
    long long hi, lo;
};

struct QualityArgs {
    QualityRaw* ring;        // [cap][n_obj]: the record of (frame, object) lies in row frame % cap
    int cap;
    unsigned frames_packed;  // four bits per frame index: the frames of the batch that get a record (grid.y of them)
    float depth_tolerance;
    double depth_maximum;
    int vcache_cap;          // vertices the LDS cache holds (0: every triangle projects its own)
    int win_cap;             // pixels of the LDS depth window (a larger window is drawn in strips)
};

// One workgroup per (object, listed frame) of the batch a.ctrl describes; a.out_log must hold the frames' rows.  window_pixels > 0
// caps the LDS depth window (operator level: forces strips).  start / stop: events bound to the dispatch.
void launch_quality(const EngineArrays& a, QualityRaw* ring, int cap, unsigned frames_packed, int n_frames, float depth_tolerance,
                    double depth_maximum, int window_pixels, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// false: the render target is wider than the LDS window can be (nothing is launched then)
bool quality_fits(const EngineArrays& a);
// (The LDS of a workgroup that runs quality_body.h: quality_window_shape, raster_shape.h; shared with the pose hypotheses' launcher.)

inline roft_quality_record quality_record(const QualityRaw& r)
{
    roft_quality_record o;
    o.frame = r.frame; o.n_mask = r.n_mask; o.n_render = r.n_render; o.n_both = r.n_both;
    o.n_depth = r.n_depth; o.n_front = r.n_front; o.n_behind = r.n_behind; o.reserved = 0;
    o.depth_err = r.n_depth > 0 ? LikelihoodSum::value(r.hi, r.lo) / (double)r.n_depth : 1.7976931348623157e308;
    return o;
}

}  // namespace roft
