// rectify.h -- argument blocks of the rectification kernel (k_rectify.hip): the sensor's distorted frames -> the images of the
// engine's pinhole camera, resampled on the device.  Contract: include/roft_engine.h section 3g.  A launch serves a chunk of at most
// kRectChunk jobs whose pointers travel in the kernel arguments, as the raw-depth kernels' do (depth.h); all jobs of a launch share
// one lens, so a thread evaluates the map once for its pixels and serves every job from it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/roft_engine.h"

namespace roft {

constexpr int kRectChunk = ROFT_RECTIFY_CHUNK;
constexpr int kRectTargetBlocks = 2048;   // workgroups a launch aims for (256 CUs x 8): its jobs are dealt to that many slices of the grid
// kinds the engine adds to ROFT_RECTIFY_*: the gray image of a colour camera image, the conversion fused into the bilinear taps
// (integer arithmetic: the bits of a conversion pass in front of ROFT_RECTIFY_GRAY8)
constexpr int kRectGrayOfBgr8 = 6, kRectGrayOfRgb8 = 7;

struct RectJobs {
    int n;
    const void* src[kRectChunk];    // device, aligned to the element of the kind
    void* dst[kRectChunk];          // device, 16-byte aligned
    unsigned char kind[kRectChunk];
};

// the two cameras and the coefficients, in float (converted from the caller's doubles once)
struct RectGeom {
    int W, H, Ws, Hs;               // target, source
    float fx, fy, cx, cy;           // target
    float fxs, fys, cxs, cys;       // source
    float k1, k2, k3, p1, p2;
    float two_p1, two_p2;           // (exact)
};

// bytes of one source / product pixel of a kind
inline size_t rect_src_pixel_bytes(int kind)
{
    switch (kind) {
        case ROFT_RECTIFY_RGB8: case kRectGrayOfBgr8: case kRectGrayOfRgb8: return 3;
        case ROFT_RECTIFY_U16: return 2;
        case ROFT_RECTIFY_F32: return 4;
        default: return 1;
    }
}
inline size_t rect_dst_pixel_bytes(int kind)
{
    switch (kind) {
        case ROFT_RECTIFY_RGB8: return 3;
        case ROFT_RECTIFY_U16: return 2;
        case ROFT_RECTIFY_F32: return 4;
        default: return 1;
    }
}

// ROFT_OK, or ROFT_ERR_INVALID with the reason set: what roft_engine_enable_rectification and the stand-alone operators refuse
int rect_check_lens(const roft_lens& lens);
int rect_check_camera(const roft_camera& cam, const char* which);
void rect_geometry(RectGeom& g, const roft_lens& lens, const roft_camera& target);

void launch_rectify(const RectJobs& jobs, const RectGeom& g, hipStream_t s);
void launch_rectify_map(const RectGeom& g, float* map_out, hipStream_t s);

}  // namespace roft
