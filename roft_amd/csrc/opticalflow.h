// opticalflow.h -- argument blocks of the optical-flow producer kernels (k_opticalflow.hip)
//
// The producer is two stages.  PER IMAGE: level 0 of its pyramid (u8 gray, or 8-bit colour through OpenCV's fixed-point gray
// conversion, -> float) and the levels below it by 2 x 2 means.  PER PAIR: the Lucas-Kanade levels, coarse to fine, over the
// pyramids of the previous and the current image, and the CV_16SC2 quantisation where that is the product.  An image that is
// the `cur` of one pair and the `prev` of the next (a camera stream) has its pyramid built once.  A launch serves a chunk of at
// most kOfChunk images / pairs whose pointers travel in the kernel arguments: no pointer table in memory, nothing to copy or to
// wait for before a launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace roft {

struct OfLevel {
    int w, h;
    size_t off;   // offset (floats) of this level inside one image's pyramid
};

// what depends on the image size and the parameters only
struct OfGeom {
    int levels, radius, iterations;
    float det_min;
    OfLevel lv[6];
    size_t pyr_stride;     // floats per image pyramid
    size_t flow_off[6];    // offset (floats) of level l's flow field inside one pair's coarse-flow workspace (l >= 1)
    size_t flow_stride;    // floats of coarse-flow workspace per pair
};

constexpr int kOfChunk = 8;

// image_type of OfImages: the ROFT_IMAGE_* values of include/roft_engine.h
constexpr int kOfGray8 = 1, kOfBgr8 = 2, kOfRgb8 = 3;

struct OfImages {
    int n;
    int type[kOfChunk];
    const void* src[kOfChunk];   // device, 4-byte aligned
    float* pyr[kOfChunk];        // [pyr_stride]
};

struct OfPairs {
    int n;
    const float* pyr0[kOfChunk];   // pyramid of the previous image
    const float* pyr1[kOfChunk];   // ... of the current one
    float* coarse[kOfChunk];       // [flow_stride] workspace
    float* field[kOfChunk];        // level-0 field (H x W x 2), always written: the CV_32FC2 product
    int16_t* out_s16[kOfChunk];    // CV_16SC2 grid 4 product, or null
};

inline void of_geometry(OfGeom& g, int W, int H, int levels, int radius, int iterations, float det_min)
{
    g.levels = levels; g.radius = radius; g.iterations = iterations; g.det_min = det_min;
    size_t off = 0, foff = 0;
    for (int l = 0; l < 6; ++l) { g.lv[l] = OfLevel{0, 0, 0}; g.flow_off[l] = 0; }
    for (int l = 0; l < levels; ++l) {
        g.lv[l].w = W >> l; g.lv[l].h = H >> l; g.lv[l].off = off;
        off += (size_t)g.lv[l].w * g.lv[l].h;
        off = (off + 3) & ~(size_t)3;
        g.flow_off[l] = foff;
        if (l >= 1) foff += 2 * (size_t)g.lv[l].w * g.lv[l].h;
    }
    g.pyr_stride = off;
    g.flow_stride = foff > 2 ? foff : 2;
}

void launch_of_pyramids(const OfGeom& g, const OfImages& im, hipStream_t s);
void launch_of_pairs(const OfGeom& g, const OfPairs& pr, hipStream_t s);   // (quantises when out_s16[0] is set: a chunk has one product)
// 8-bit colour -> 8-bit gray, any W x H (the stand-alone operator)
void launch_image_to_gray(const uint8_t* src, int type, size_t npix, uint8_t* dst, hipStream_t s);

}  // namespace roft
