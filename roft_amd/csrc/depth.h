// depth.h -- argument blocks of the raw-depth kernels (k_depth.hip): the sensor's 16-bit frame -> the float depth image in metres
// the engine's kernels read, converted (and, for a depth camera of its own, registered to the colour camera) on the device.
// Contract: include/roft_engine.h section 3c.  A launch serves a chunk of at most kDepthChunk images whose pointers travel in the
// kernel arguments, as the optical-flow producer's do (opticalflow.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/roft_engine.h"

namespace roft {

constexpr int kDepthChunk = 16;
constexpr unsigned kDepthNoKey = 0xffffffffu;   // key of a colour pixel no reading covers

struct DepthJobs {
    int n;
    const uint16_t* raw[kDepthChunk];   // device, 4-byte aligned
    float* out[kDepthChunk];            // device, 16-byte aligned: the product (during an alignment: its keys, one word per pixel)
};

// the two cameras and the transform between them, in float (converted from the caller's doubles once)
struct DepthAlignGeom {
    int Wd, Hd, Wc, Hc;
    float fxd, fyd, cxd, cyd;
    float fxc, fyc, cxc, cyc;
    float R[9], t[3];
    float scale;
};

// ROFT_OK, or ROFT_ERR_INVALID with the reason set: what roft_engine_enable_raw_depth and the stand-alone operators refuse
int depth_check_scale(float scale);
int depth_check_camera(const roft_camera& cam, const char* which);
int depth_check_transform(const roft_depth_source& src);
void depth_align_geometry(DepthAlignGeom& g, const roft_depth_source& src, const roft_camera& colour);

// out = (float)raw * scale for npix readings per image
void launch_depth_convert(const DepthJobs& jobs, size_t npix, float scale, hipStream_t s);
// the three phases of an alignment: clear the keys, scatter the readings (integer minimum), resolve the keys to metres in place
void launch_depth_align(const DepthJobs& jobs, const DepthAlignGeom& g, hipStream_t s);

}  // namespace roft
