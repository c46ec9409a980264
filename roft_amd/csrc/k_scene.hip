// k_scene.hip -- batched scene renderer (gfx950): the meshes of a scene drawn at the poses of many frames, several instances
// per frame hiding each other, into per-pixel depth / instance / triangle maps and a flat-shaded overlay on the camera image.
//
// Reference (behaviour only): the evaluation's `video` and `thumbnail` heads, evaluation/results_renderer.py:591-778, and the
// renderer they call, tools/object_renderer/src/renderer.cpp (the mesh at every estimated pose over the grayed camera frame).
//
// Two passes over a visibility buffer of 64-bit keys, one buffer per frame of the call (scene.h states the contract):
//   scene_visibility_kernel   one workgroup per (frame, instance, part).  It draws the instance by raster.h's draw contract into
//       a window of KEYS in LDS (an LDS 64-bit min; draw_triangles hands the store the triangle's index), in strips of at most
//       win_cap pixels -- whole rows while a row fits, else a row is cut into column runs as well --, and merges the keys that were
//       drawn into the frame's buffer in memory with a 64-bit atomic min (global_atomic_umin_x2, a vector instruction).  The
//       `parts` workgroups of an instance deal the strips out in turn.
//   scene_resolve_kernel      streams the keys once, four pixels per thread, and writes the outputs that were asked for:
//       16-byte stores for the maps, three dwords of RGB.  A covered pixel is shaded from its key: the winning triangle's
//       corners are transformed again with the float pose the visibility pass left in the pose table.
// Determinism: a pixel's key is the minimum over a set of fragments that depends on the frame's poses, flags and meshes only.
// Which workgroup draws a fragment, in which strip, and when it reaches memory changes the order of the min operations and
// nothing else; the resolve pass is a pure function of a pixel's key, its background pixel and the tables.  No other atomic
// touches a pixel.
#include "raster.h"
#include "scene.h"

namespace roft {

// the eye-space point project_vertex divides: the same three expressions
__device__ __forceinline__ void eye_vertex(const float* v, const ScenePose& P, float& X, float& Y, float& Z)
{
    X = ((P.R[0] * v[0] + P.R[1] * v[1]) + P.R[2] * v[2]) + P.t[0];
    Y = ((P.R[3] * v[0] + P.R[4] * v[1]) + P.R[5] * v[2]) + P.t[1];
    Z = ((P.R[6] * v[0] + P.R[7] * v[1]) + P.R[8] * v[2]) + P.t[2];
}

// grid: n_frames * n_instances * parts.  dynamic LDS: [3 * vcache_cap floats] | [win_cap keys]
__global__ __launch_bounds__(kSceneThreads) void scene_visibility_kernel(SceneArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ MeshBoxShared s_mb;
    const int tid = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)a.parts), fi = (int)(blockIdx.x / (unsigned)a.parts);   // fi = frame * n_instances + instance
    const int inst = fi % a.n_instances, frame = fi / a.n_instances;
    if (a.valid && !a.valid[fi]) return;
    const double* pose = a.poses + (size_t)fi * 7;
    if (!pose_is_finite(pose)) return;   // (uniform over the workgroup) draws nothing
    const RenderPose P = make_pose(pose, pose + 3);
    if (part == 0 && tid == 0) {
        ScenePose& o = a.pose_table[fi];
        for (int i = 0; i < 9; ++i) o.R[i] = P.R[i];
        for (int i = 0; i < 3; ++i) o.t[i] = P.t[i];
    }
    const MeshView m = a.meshes[a.mesh_index[inst]];
    const int W = a.W, H = a.H;
    const bool cached = m.n_verts <= a.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    uint64_t* s_k = reinterpret_cast<uint64_t*>(smem + vertex_cache_bytes(a.vcache_cap));
    box_reset(s_mb);
    __syncthreads();
    auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, P, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
    project_mesh<kSceneThreads, 1>(m.verts, m.n_verts, cached, s_v, W, H, s_mb.box, &s_mb.behind, project);
    __syncthreads();
    const MeshBox box = box_read(s_mb, W, H);
    if (!box.drawable()) return;   // nothing on the screen
    // strips of the window: whole rows while a row fits the LDS window, else a row is cut into column runs as well
    const int win_w = box.width(), cw = min(win_w, a.win_cap), rows = strip_rows(a.win_cap, cw);
    const int n_cols = (win_w + cw - 1) / cw, n_rows = (box.j1 - box.j0 + rows) / rows;
    const uint8_t* const flips = cull_table(m.flip, s_mb.behind);
    ROFT_LDS uint64_t* const zk = (ROFT_LDS uint64_t*)pin_lds(reinterpret_cast<uint32_t*>(s_k));
    uint64_t* const keys = a.keys + (size_t)frame * W * H;
    for (int strip = part; strip < n_cols * n_rows; strip += a.parts) {
        const Strip st = strip_at(box, cw, rows, n_cols, strip);   // (st.npx <= win_cap)
        const int is = st.i0, js = st.js, je = st.je, sw = st.win_w, npx = st.npx;
        for (int i = tid; i < npx; i += kSceneThreads) s_k[i] = kSceneKeyEmpty;
        __syncthreads();
        draw_triangles<kSceneThreads>(m, s_v, cached, flips, project, W, H, js, je, [zk, is, js, sw, inst](int i, int j, float z, int t) {
            const unsigned ci = (unsigned)(i - is);   // (the strip's column run)
            const uint64_t low = ((uint64_t)(uint32_t)inst << 24) | (uint32_t)t;
            if (ci < (unsigned)sw)
                (void)__hip_atomic_fetch_min(zk + ((j - js) * sw + (int)ci), ((uint64_t)__float_as_uint(z) << 32) | low, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        __syncthreads();
        // the strip's drawn keys -> the frame's buffer (other instances and other strips of this one merge into the same buffer)
        for (int i = tid; i < npx; i += kSceneThreads) {
            const uint64_t key = s_k[i];
            if (key != kSceneKeyEmpty)
                (void)__hip_atomic_fetch_min(keys + ((size_t)(js + i / sw) * W + (is + i % sw)), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();   // the next strip clears the window
    }
}

// shade of the key's triangle: scene.h, operation by operation
__device__ __forceinline__ float scene_shade(const SceneArgs& a, int frame, int inst, int tri_id)
{
    const MeshView& m = a.meshes[a.mesh_index[inst]];
    const ScenePose& P = a.pose_table[(size_t)frame * a.n_instances + inst];
    const int32_t* tri = m.tris + (size_t)3 * tri_id;
    float p[3][3];
    for (int k = 0; k < 3; ++k) eye_vertex(m.verts + (size_t)3 * tri[k], P, p[k][0], p[k][1], p[k][2]);
    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    return (len > 0.0f && len < INFINITY) ? fabsf(nz) / len : 0.0f;
}

__device__ __forceinline__ uint32_t scene_level(float c)
{
    return (uint32_t)fminf(fmaxf(floorf(c + 0.5f), 0.0f), 255.0f);
}

// grid: ceil(n_frames * W * H / (kResolvePixels * 256)); the pixels of the call as one flat array (a thread's four may span
// two frames).  Every array is padded to a multiple of kResolvePixels pixels.
__global__ __launch_bounds__(256) void scene_resolve_kernel(SceneArgs a)
{
    const size_t WH = (size_t)a.W * a.H, total = WH * a.n_frames;
    const size_t g0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * kResolvePixels;
    if (g0 >= total) return;
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(a.keys + g0), k23 = *reinterpret_cast<const ulonglong2*>(a.keys + g0 + 2);
    const uint64_t key[kResolvePixels] = {k01.x, k01.y, k23.x, k23.y};
    int frame = (int)(g0 / WH);
    size_t p = g0 - (size_t)frame * WH;
    float dep[kResolvePixels];
    int ins[kResolvePixels], tri[kResolvePixels];
    uint32_t bytes[3 * kResolvePixels];
#pragma unroll
    for (int k = 0; k < kResolvePixels; ++k) {
        const bool in_range = g0 + k < total;
        const uint32_t zb = (uint32_t)(key[k] >> 32);
        const bool covered = in_range && zb < kDepthEmpty;   // (an infinite depth is background, as the contract's `z < +inf`)
        dep[k] = covered ? __uint_as_float(zb) : 0.0f;
        ins[k] = covered ? (int)((key[k] >> 24) & 0xFFu) : -1;
        tri[k] = covered ? (int)(key[k] & 0xFFFFFFu) : -1;
        if (a.rgb) {
            uint32_t r = 0, g = 0, b = 0;
            if (a.background && in_range) {
                const uint8_t* px = a.background + ((a.background_frames == 1 ? 0 : (size_t)frame * WH) + p) * 3;
                r = px[0]; g = px[1]; b = px[2];
                if (a.gray_background) r = g = b = (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14;
            }
            if (covered) {
                const SceneStyle st = a.styles[ins[k]];
                const float s = scene_shade(a, frame, ins[k], tri[k]);
                const float level = st.ambient + (1.0f - st.ambient) * s;
                r = scene_level(st.opacity * (st.tint[0] * level) + (1.0f - st.opacity) * (float)r);
                g = scene_level(st.opacity * (st.tint[1] * level) + (1.0f - st.opacity) * (float)g);
                b = scene_level(st.opacity * (st.tint[2] * level) + (1.0f - st.opacity) * (float)b);
            }
            bytes[3 * k] = r; bytes[3 * k + 1] = g; bytes[3 * k + 2] = b;
        }
        if (++p == WH) { p = 0; ++frame; }
    }
    if (a.rgb) {
        uint32_t* out = reinterpret_cast<uint32_t*>(a.rgb) + 3 * (g0 / kResolvePixels);
#pragma unroll
        for (int d = 0; d < 3; ++d)
            out[d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
    }
    if (a.depth) *reinterpret_cast<float4*>(a.depth + g0) = make_float4(dep[0], dep[1], dep[2], dep[3]);
    if (a.instance) *reinterpret_cast<int4*>(a.instance + g0) = make_int4(ins[0], ins[1], ins[2], ins[3]);
    if (a.triangle) *reinterpret_cast<int4*>(a.triangle + g0) = make_int4(tri[0], tri[1], tri[2], tri[3]);
}

void launch_scene_visibility(const SceneArgs& a, size_t lds_bytes, hipStream_t s)
{
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(scene_visibility_kernel), (int)kRasterLdsBudget);
    const size_t groups = (size_t)a.n_frames * a.n_instances * a.parts;
    hipLaunchKernelGGL(scene_visibility_kernel, dim3((unsigned)groups), dim3(kSceneThreads), (uint32_t)lds_bytes, s, a);
}

void launch_scene_resolve(const SceneArgs& a, hipStream_t s)
{
    const size_t total = (size_t)a.W * a.H * a.n_frames;
    const size_t threads = (total + kResolvePixels - 1) / kResolvePixels;
    hipLaunchKernelGGL(scene_resolve_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace roft
