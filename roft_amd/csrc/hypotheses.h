// hypotheses.h -- pose hypotheses (include/roft_engine.h, section 3j): what k_hypotheses.hip is given and what it leaves.  One launch
// scores n candidate poses of one mesh against one object plane and one depth image, each with the body of a track-quality record
// (quality_body.h).  The kernel reads the plane, the depth, the mesh and the poses and writes only the poses' own records.
#pragma once

#include "quality.h"
#include "raster.h"

namespace roft {

constexpr int kHypothesesMax = 1 << 20;      // poses of one call
constexpr int kHypothesesChunk = 1 << 16;    // poses of one launch: what the resident pose and record buffers hold

struct HypothesesArgs {
    const uint32_t* plane;   // the object plane M (wpr words per row, plane_words in all)
    size_t plane_words;
    const float* depth;      // D
    MeshView mesh;           // as ObjParams describes it: walk order, flip bits of a closed mesh (n_tris == 0: nothing is drawn)
    DevCamera cam;           // with the divider the records are made under
    int tile_w, tile_h;
    const double* poses;     // [n][7] x y z, w x y z of the launch's hypotheses
    QualityRaw* out;         // [n]
    int* n_mask;             // one word: the plane's bit count, made by the launch's first kernel and read by its second
    int frame;               // what the records carry as `frame`
    float depth_tolerance;
    double depth_maximum;
    int vcache_cap;          // vertices the LDS cache holds (0: every triangle projects its own)
    int win_cap;             // pixels of the LDS depth window (a larger window is drawn in strips)
};

// n hypotheses (n <= kHypothesesChunk): the plane's bit count once, then one workgroup per hypothesis.  a.vcache_cap / win_cap and lds
// from quality_window_shape (raster_shape.h): the two kernels of quality_body.h share the shape and refuse the same targets.
void launch_hypotheses(const HypothesesArgs& a, int n, size_t lds, hipStream_t s);

}  // namespace roft
