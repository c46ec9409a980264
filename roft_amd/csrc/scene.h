// scene.h -- what the scene renderer's kernels (k_scene.hip) and its host side (scene.hip) share.
//
// Contract of the image (stated for callers in include/roft_engine.h, restated in float32 numpy by tests/scene_ref.py):
//   visibility   per pixel the smallest 64-bit key (float bits of eye-space z) << 32 | instance << 24 | triangle over every
//                fragment the render contract (raster.h, oracle/ro_render.c) produces for the frame's valid instances; the
//                triangle index is the caller's.  A closed mesh (mesh_class.h) loses the triangles that face away while all
//                of its vertices are in front of the near plane, as in the outlier test.
//   shading      eye-space corners P_k = (X, Y, Z) as project_vertex computes them (eye_vertex below);
//                n = (P1 - P0) x (P2 - P0);  s = |n_z| / sqrt((n_x^2 + n_y^2) + n_z^2), 0 when the length is 0 or not finite;
//                level = ambient + (1 - ambient) s;  per channel c = opacity (tint_c level) + (1 - opacity) bg_c;
//                out = (uint8) min(max(floorf(c + 0.5f), 0), 255).  All float, this order, -ffp-contract=off.
//   background   the camera image, or its gray (R 4899 + G 9617 + B 1868 + 8192) >> 14 in all three channels, or zeros.
#pragma once

#include "raster.h"

namespace roft {

constexpr int kSceneThreads = 1024;            // visibility: one workgroup per (frame, instance, part)
constexpr int kSceneMaxInstances = 256;        // 8 bits of the key
constexpr uint64_t kSceneKeyEmpty = ~0ull;     // nothing drawn (a key's depth word is below 0x7F800000 when it is a surface)
constexpr int kResolvePixels = 4;              // pixels per thread of the resolve pass: 12 bytes of RGB = three dwords

struct SceneStyle {
    float tint[3], opacity, ambient;
};

// the float pose of a (frame, instance), written by the visibility pass and read back by the resolve pass
struct ScenePose {
    float R[9], t[3];
};

struct SceneArgs {
    int W, H, n_frames, n_instances;
    float fx, fy, cx, cy;
    const MeshView* meshes;        // tris in the caller's order: a key's triangle index is the caller's
    const int* mesh_index;         // [n_instances]
    const double* poses;           // [n_frames][n_instances][7]
    const uint8_t* valid;          // [n_frames][n_instances] or nullptr
    uint64_t* keys;                // [n_frames][W * H] (+ padding to kResolvePixels)
    ScenePose* pose_table;         // [n_frames][n_instances]
    // visibility launch shape
    int parts;                     // workgroups per (frame, instance): they deal out the strips of its window
    int vcache_cap;                // vertices whose projections are kept in LDS (0: projected per triangle)
    int win_cap;                   // keys of the LDS window
    // resolve
    const SceneStyle* styles;      // [n_instances]
    const uint8_t* background;     // RGB or nullptr
    int background_frames;         // n_frames or 1
    int gray_background;
    uint8_t* rgb;                  // outputs, any may be nullptr; flat over the frames of the call
    float* depth;
    int32_t* instance;
    int32_t* triangle;
};

void launch_scene_visibility(const SceneArgs& a, size_t lds_bytes, hipStream_t s);
void launch_scene_resolve(const SceneArgs& a, hipStream_t s);

}  // namespace roft
