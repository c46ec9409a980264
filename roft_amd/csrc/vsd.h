// vsd.h -- BOP's Visible Surface Discrepancy (include/roft_engine.h, section 3i): what k_vsd.hip is given and what it leaves.
// The kernel reads the mesh, the pose pairs and the depth images and adds only to the pairs' own integer rows.
#pragma once

#include "raster.h"

namespace roft {

constexpr int kVsdMaxTaus = ROFT_VSD_MAX_TAUS;
constexpr int kVsdCounts = 4 + kVsdMaxTaus;   // a pair's row: n_union, n_inter, n_gt, n_est, fail[0 .. 16)

struct VsdArgs {
    MeshView mesh;
    const double* est;      // [n][7] x y z, w x y z of the launch's pairs
    const double* ref;
    const float* depth;     // the launch's depth images
    size_t depth_stride;    // floats between the images of two pairs (0: one image under every pair)
    int32_t* counts;        // [n][kVsdCounts], zero before the first launch adds to it
    int W, H;
    float fx, fy, cx, cy;   // the camera as the render contract rounds it (divider 1)
    double dfx, dfy, dcx, dcy;   // ... and as the distance images read it
    float delta;
    int n_taus;
    double taus[kVsdMaxTaus];
    double diameter;        // 0: distances are not normalised
    int vcache_cap;         // vertices the LDS cache holds (0: every triangle projects its own)
    int win_alloc;          // pixels EACH of the two LDS depth windows has room for (at least one row of the target) ...
    int win_cap;            // ... and how many of them a strip may use (<= win_alloc; a strip holds at least one row all the same)
    int parts;              // workgroups per pair: they deal the strips out in turn
};

// n pairs (grid: n * a.parts workgroups) add their counts to a.counts; a.vcache_cap / win_alloc / win_cap and `lds` from vsd_shape
// (raster_shape.h), which refuses a target of which not even one row fits the two windows: nothing may be launched then
void launch_vsd(const VsdArgs& a, int n, size_t lds, hipStream_t s);
// counts[n][kVsdCounts] -> errors[n][n_taus] and rows[n][4 + n_taus]
void launch_vsd_finish(const int32_t* counts, int n, int n_taus, double* errors, int32_t* rows, hipStream_t s);

}  // namespace roft
