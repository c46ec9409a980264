// opticalflow_args.h -- the argument blocks of the optical-flow producer kernels and the host arithmetic that fills them
// (geometry of the pyramids, slots of a checked chunk).  Host-only: C library headers alone, so that tests/cpp/of_check_plan_check.cpp
// compiles it without HIP.  opticalflow.h adds the launchers.
#pragma once

#include <cstddef>
#include <cstdint>

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

// The forward-backward check (include/roft_engine.h section 3f).  With the check on, a chunk of n <= kOfCheckChunk pairs is
// 2 n Lucas-Kanade problems in ONE OfPairs: slot k is the forward problem of pair k, slot n + k its backward problem -- the two
// pyramid pointers swapped, a coarse workspace and a level-0 field of its own -- so that both directions are z-slices of the
// same launches.  of_check_kernel then rewrites the forward fields in place.
constexpr int kOfCheckChunk = kOfChunk / 2;

struct OfCheck {
    int n;
    float* fwd[kOfCheckChunk];          // level-0 forward field (H x W x 2): invalid pixels are overwritten, the others not touched
    const float* bwd[kOfCheckChunk];    // level-0 field of the swapped pair
    float tol_abs, tol_rel;
};

// pair k of a checked chunk -> its two slots of `pr` (pr.n counts the PAIRS while the chunk is filled; of_check_close makes it
// the number of LK problems and moves the backward slots behind the forward ones)
inline void of_check_put(OfPairs& pr, OfCheck& ck, const float* pyr_prev, const float* pyr_cur, float* field, float* coarse_fwd,
                         float* coarse_bwd, float* field_bwd)
{
    const int k = pr.n++;
    pr.pyr0[k] = pyr_prev; pr.pyr1[k] = pyr_cur; pr.coarse[k] = coarse_fwd; pr.field[k] = field; pr.out_s16[k] = nullptr;
    const int b = kOfCheckChunk + k;
    pr.pyr0[b] = pyr_cur; pr.pyr1[b] = pyr_prev; pr.coarse[b] = coarse_bwd; pr.field[b] = field_bwd; pr.out_s16[b] = nullptr;
    ck.fwd[k] = field; ck.bwd[k] = field_bwd;
    ck.n = pr.n;
}

inline void of_check_close(OfPairs& pr)
{
    const int n = pr.n;
    for (int k = 0; k < n; ++k) {
        const int b = kOfCheckChunk + k;
        pr.pyr0[n + k] = pr.pyr0[b]; pr.pyr1[n + k] = pr.pyr1[b]; pr.coarse[n + k] = pr.coarse[b]; pr.field[n + k] = pr.field[b];
        pr.out_s16[n + k] = nullptr;
    }
    pr.n = 2 * n;
}

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

}  // namespace roft
