// k_render.hip -- the outlier test: depth render of the object mesh under both pose alternatives + masked depth likelihood
// (gfx950).  The decision itself is taken by the pose chain segment that follows (ukf_chain_kernel, k_ukf.hip).
//
// Reference:
//   ROFTFilter::correct_outlier_rejection / pick_best_alternative
//                                               src/roft-lib/src/ROFTFilter.cpp:467-621
//   SICAD::superimpose (OpenGL) contract         src/roft-lib/src/SICAD.cpp:924-1066,1601-1656,
//                                               src/roft-lib/shader/shader_model.frag:30-52
//
// What is here.
//  * outlier_fused_kernel<GL>, the engine's test: one launch draws an alternative into an LDS window by the pieces of raster.h's
//    draw contract (the box, the strips, DepthWindow) and sums the likelihood over the buffered features (k_features.hip) where
//    the window lies.  No OpenGL, no z-buffer in memory.  What this file adds: an alternative is shared by `parts` workgroups as
//    bands of the box's rows x groups of its triangles (band_split, merge_slabs), and each render mode walks the triangles its way:
//      - the contract (GL = false, the hot path): a wave projects and draws one 64-triangle cluster at a time (draw_clusters over
//        mesh_clusters.h), and the box comes from the corners of the mesh's box (box_from_corners) instead of a vertex pass;
//      - ROFT_RENDER_GL (GL = true, opt-in, twice the time): raster_gl.h's arithmetic, every triangle of `tris` in the caller's
//        order over a vertex cache in LDS (draw_triangles_gl), the window holds (depth, triangle) keys (GlWindow).
//    The stages: job, window box, band split; per strip clear, draw, merge, dump, score; band sums.
//  * launch_outlier: the launch shape (OutlierShape) and the split override.
//  * outlier_kernel, the operator-level likelihood and decision over z-buffers in memory (roft_depth_likelihood).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>

#include "mesh_clusters.h"
#include "raster.h"
#include "raster_gl.h"

namespace roft {

namespace host { int fail(int code, const std::string& msg); }   // (engine.hip: sets the thread's error string, returns `code`)

// Operator level (roft_depth_likelihood): likelihood of both alternatives over the buffered features from z-buffers in
// HBM (EngineArrays::zbuf), decision, and the selected belief becomes the corrected belief (ROFTFilter.cpp:581-583,
// 670-675).  One workgroup per object.  The engine's own test is outlier_fused_kernel below.
constexpr int kOutlierThreads = 1024;

__global__ __launch_bounds__(kOutlierThreads) void outlier_kernel(EngineArrays a, int lin)
{
    __shared__ double s_err[2][kOutlierThreads / 64];
    __shared__ double s_cnt[2][kOutlierThreads / 64];
    __shared__ int s_sel;
    const int obj = blockIdx.x;
    ObjState& st = a.state[obj];
    PoseLane& pl = st.lane[lin];
    if (pl.pending_frame < 0) return;
    const FrameCtrl& c = frame_ctrl(a, pl.pending_frame, obj);
    const int d = a.cam.divider, tw = a.tile_w;
    const int fslot = (c.feat_read >= 0) ? c.feat_read : 0;
    const uint32_t* fpix = a.feat_pix + ((size_t)obj * kFeatRing + fslot) * a.feat_cap;
    const float* fdep = a.feat_depth + ((size_t)obj * kFeatRing + fslot) * a.feat_cap;
    const uint32_t* z0 = a.zbuf + (((size_t)lin * a.n_obj + obj) * 2) * a.tile_w * a.tile_h;
    const uint32_t* z1 = z0 + (size_t)a.tile_w * a.tile_h;
    double err[2] = {0.0, 0.0}, cnt[2] = {0.0, 0.0};
    const int n = st.n_feat[fslot];
    // kBatch feature slots per thread and iteration: their loads are independent and go out together (one iteration
    // covers 16 k features; per-thread accumulation order is the slot order either way)
    constexpr int kBatch = 16;
    for (int i0 = threadIdx.x; i0 < n; i0 += kBatch * blockDim.x) {
        float dep[kBatch];
        uint32_t pix[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int i = i0 + k * blockDim.x;
            dep[k] = (i < n) ? fdep[i] : 0.0f;
            pix[k] = (i < n) ? fpix[i] : 0u;
        }
        uint32_t b0[kBatch], b1[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int v = (int)(pix[k] >> 16), u = (int)(pix[k] & 0xFFFFu);
            const size_t ti = (size_t)(v / d) * tw + (u / d);
            b0[k] = z0[ti];
            b1[k] = z1[ti];
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (!((dep[k] > 0) && ((double)dep[k] < 2.0))) continue;  // hard-coded 2.0 (ROFTFilter.cpp:561)
            if (b0[k] != kDepthEmpty) { err[0] += (double)fabsf(dep[k] - __uint_as_float(b0[k])); cnt[0] += 1.0; }
            if (b1[k] != kDepthEmpty) { err[1] += (double)fabsf(dep[k] - __uint_as_float(b1[k])); cnt[1] += 1.0; }
        }
    }
    for (int k = 0; k < 2; ++k) {
        double e = err[k], n2 = cnt[k];
        for (int off = 32; off > 0; off >>= 1) { e += __shfl_down(e, off, 64); n2 += __shfl_down(n2, off, 64); }
        if ((threadIdx.x & 63) == 0) { s_err[k][threadIdx.x >> 6] = e; s_cnt[k][threadIdx.x >> 6] = n2; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double L[2];
        for (int k = 0; k < 2; ++k) {
            double e = 0.0, n2 = 0.0;
            for (int w = 0; w < kOutlierThreads / 64; ++w) { e += s_err[k][w]; n2 += s_cnt[k][w]; }
            L[k] = (n2 == 0.0) ? 1.7976931348623157e308 : (e / n2) / 1.0;  // gain is a bool -> 1.0 (ROFTFilter.h:64)
        }
        const int sel = (L[0] > 2.0 * L[1]) ? 1 : 0;
        pl.outlier_selected = sel;
        pl.outlier_L[0] = L[0];
        pl.outlier_L[1] = L[1];
        for (int k = 0; k < 2; ++k) {
            double n2 = 0.0;
            for (int w = 0; w < kOutlierThreads / 64; ++w) n2 += s_cnt[k][w];
            pl.outlier_cnt[k] = n2;
        }
        s_sel = sel;
    }
    __syncthreads();
    const PoseBelief& src = st.belief[b_alt(lin, s_sel ? 1 : 0)];
    PoseBelief& dst = st.belief[c.cur_slot];
    for (int i = threadIdx.x; i < 144; i += blockDim.x) dst.cov[i] = src.cov[i];
    if (threadIdx.x < 13) dst.mean[threadIdx.x] = src.mean[threadIdx.x];
    if (roft_object_output* row = log_row(a, c, obj)) {
        if (threadIdx.x < 13) row->pose[threadIdx.x] = src.mean[threadIdx.x];
        if (threadIdx.x == 0) {
            row->outlier_selected = s_sel;
            row->outlier_L[0] = pl.outlier_L[0];
            row->outlier_L[1] = pl.outlier_L[1];
        }
    }
}

// ---- the engine's outlier test: depth render + likelihood of ONE alternative per workgroup, all in LDS ------------------
// The render is only ever sampled at the buffered feature pixels, and the object covers a small window of the render
// target (about 70 x 90 of 320 x 240 pixels at the metric shape).  So: the pixel box of the mesh is the z window -- in LDS,
// resolved with LDS atomicMin, +inf = empty --, and the likelihood reads it in place.  No z-buffer in HBM, no clear
// pass, no global atomics, one launch instead of three.  A window that does not fit the LDS is rendered in horizontal strips
// (every strip walks all triangles and all features).  The per-pixel arithmetic is raster_projected's, whatever the strips and
// bands: the depths are bit-identical to oracle/ro_render.c in every configuration (tests/test_parity_gpu.py and
// tests/test_outlier_clusters_gpu.py drive this kernel through roft_render_depth and roft_outlier_test).
// The contract render (GL = false) has no vertex pass: the mesh goes up cut into clusters of at most 64 triangles over at most 64
// vertices (mesh_clusters.h), and a wave projects and draws one cluster at a time.  Before, every workgroup of an alternative
// projected ALL vertices into a 98 KB LDS cache in a phase of its own in front of everything else (7 of 37 us at 64 objects),
// and every triangle fetched three 32-bit indices and gathered nine floats from that cache.  Why the bits stay what they were:
//   * every triangle the walk over `tris` drew is drawn, with the same corner coordinates -- a slot holds the bits of the mesh's
//     vertex and goes through the same project_vertex -- in the triangle's own corner order and with the same cull code; the
//     clusters the cone test skips hold only triangles raster_projected's sign-of-area rule culls (cluster_faces_away);
//   * every window pixel is an order-free atomicMin, so it does not matter which wave draws a triangle, or when;
//   * the window box from the corners of the mesh's box CONTAINS the vertices' box (corner_box_settles, raster.h): the same
//     depths at the same pixels, the added pixels stay empty, and an empty pixel is neither dumped nor sampled; `behind` is
//     the vertices' own flag (settled by the corners only with a tenfold margin, else by the vertex pass);
//   * the band sums are exact integers (LikelihoodSum): rows may fall to other bands or strips than before.
// The GL render mode keeps the vertex pass and its cache (project_mesh / fetch_triangle, as the other rasteriser kernels).
// With CUs to spare an alternative is shared by `parts` workgroups, as R bands of the window's rows x G groups of its
// triangles (round 4; R G = parts, R = the fewest bands that fit the LDS in one piece -- 1 for most objects).  The G workgroups of
// a band each draw THEIR triangles (runs of 64, dealt out in turn) into a window of their own, write it through to a slab in
// memory (agent-coherent stores, EngineArrays::zmerge), count themselves in; the one that arrives last reads the other slabs
// back (agent-coherent loads), keeps the nearest depth per pixel -- the same minimum, so the same bits, as one window would
// hold -- and scores the band.  Every band leaves its partial sums; the pose chain segment that follows adds them up in band
// order and decides.  (G = 1: the row split of rounds 2 - 3, every workgroup walks all triangles; the launch falls back to it
// when the slabs do not cover objects x parts, roft_debug_outlier_split(0) forces it.)  The launch lasts as long as its slowest
// workgroup, which in the row split is the middle band of the largest object (49 - 56 us of triangles at 8 and 16 objects against
// 25 - 30 with the triangles dealt out: 60 - 66 -> 45 - 46 us per launch).
// grid: (2 alternatives x parts, n_obj).  dynamic LDS: [win_cap z values]; GL: [3 * vcache_cap floats] | [win_cap keys]
// GL = true: render mode ROFT_RENDER_GL (raster_projected_gl).  The window is then a visibility buffer: a pixel holds the 64-bit key
// (quantised window z << 32 | triangle index in the caller's order) resolved with LDS atomicMin -- the nearest fragment, the first
// drawn among equal depths, whatever order the threads draw in --, and the depth of the winning triangle is evaluated again where it
// is read (dump, samples).  The workgroups of an alternative split only the rows of its window (launch_outlier passes split_tris 0).
constexpr int kFusedThreads = 1024;

// ---- stages of outlier_fused_kernel.  Every one is called by ALL threads of the workgroup; each says what it reads, what it
// leaves and which barrier the caller owes. -----------------------------------------------------------------------------------

// What a workgroup works on: the alternative `alt` of object `obj`, as workgroup `part` of the alternative's `parts`.
struct FusedJob {
    int obj, bx, alt, part;   // bx = alt * parts + part: the workgroup's index within the object
    ObjState* st;
    PoseLane* pl;
    const FrameCtrl* c;
    const ObjParams* prm;
    RenderPose P;             // the alternative's pose
    int d, tw, th;            // divider, render target
    float fx, fy, cx, cy;     // intrinsics at the divider
};

// job.  Reads the block index and the lane's pending test; leaves `job`.  False: nothing to do, the whole workgroup returns (an
// object slot past n_obj, or no outlier test pending between the pose chain segments).  No barrier.
__device__ __forceinline__ bool fused_job(const EngineArrays& a, int lin, int parts, FusedJob& job)
{
    // Workgroups are handed to the XCDs round robin by their linear index; the 2 x parts workgroups of an object read the
    // same mesh (246 clusters of 1 KB at the bench's 15.5 k triangles): with the grid laid out as
    // [group of 8 objects][workgroup of the object][object within the group] they share one XCD and one L2.
    const int per = 2 * parts, lin_id = (int)blockIdx.x;
    job.obj = (lin_id / (8 * per)) * 8 + (lin_id & 7);
    job.bx = (lin_id >> 3) % per;
    if (job.obj >= a.n_obj) return false;
    job.alt = job.bx / parts;
    job.part = job.bx % parts;
    job.st = &a.state[job.obj];
    job.pl = &job.st->lane[lin];
    if (job.pl->pending_frame < 0) return false;
    job.c = &frame_ctrl(a, job.pl->pending_frame, job.obj);
    job.prm = &a.params[job.obj];
    const PoseBelief& bl = job.st->belief[b_alt(lin, job.alt)];
    job.P = make_pose(bl.mean + 6, bl.mean + 9);
    job.d = a.cam.divider; job.tw = a.tile_w; job.th = a.tile_h;
    const int d = job.d;
    job.fx = (float)(a.cam.fx / d); job.fy = (float)(a.cam.fy / d); job.cx = (float)(a.cam.cx / d); job.cy = (float)(a.cam.cy / d);
    return true;
}

// The window of a render mode, in dynamic LDS: what a pixel holds, what "empty" is, how the rasteriser stores into it and how a
// depth is read back, strip by strip (Strip, raster.h).  clear / the stores / the reads each need a barrier between them; the
// stages below say which.  The contract's window is raster.h's DepthWindow.

// project_mesh's / fetch_triangle's `project` under the GL numerics
struct GlProject {
    const FusedJob& job;
    __device__ __forceinline__ void operator()(const float* v, float& sx, float& sy, float& z) const
    {
        project_vertex_gl(v, job.P, job.fx, job.fy, job.cx, job.cy, sx, sy, z);
    }
};

// The GL mode's window, a visibility buffer behind the vertex cache: a pixel is the key (quantised window z << 32 | triangle index in
// the caller's order), kGlKeyClear where nothing was drawn (depth word kGlDepthClear).
struct GlWindow {
    uint64_t* k;     // [win_cap]
    float* s_v;      // [3 * vcache_cap] projected vertices (box_from_vertices fills them when `cached`)
    bool cached;
    const FusedJob& job;
    __device__ __forceinline__ void clear(int npx, int threads) const { for (int i = threadIdx.x; i < npx; i += threads) k[i] = kGlKeyClear; }
    // `store(i, j, key)`: the nearest fragment, the first drawn among equal depths, whatever order the threads draw in
    __device__ __forceinline__ auto store(const Strip& s) const
    {
        ROFT_LDS uint64_t* const zk = (ROFT_LDS uint64_t*)pin_lds(reinterpret_cast<uint32_t*>(k));
        const int i0 = s.i0, js = s.js, win_w = s.win_w;
        return [zk, i0, js, win_w](int i, int j, uint64_t key) {
            (void)__hip_atomic_fetch_min(zk + ((j - js) * win_w + (i - i0)), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
    }
    __device__ __forceinline__ bool covered(int i) const { return (uint32_t)(k[i] >> 32) != kGlDepthClear; }
    // gl_resolve: eye-space depth at pixel (pi, pj) of the triangle whose key won it: raster_projected_gl's arithmetic again, so
    // the window z it drew with
    __device__ __forceinline__ float depth(int i, int pi, int pj) const
    {
        const ObjParams& prm = *job.prm;
        const int32_t* tri = prm.tris + (size_t)3 * (uint32_t)k[i];
        const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
        float x0, y0, z0, x1, y1, z1, x2, y2, z2;
        fetch_triangle(s_v, cached, prm.verts, v0, v1, v2, GlProject{job}, x0, y0, z0, x1, y1, z1, x2, y2, z2);
        return gl_linear_depth(gl_pixel_window_z(x0, y0, x1, y1, x2, y2, gl_vertex_window_z(z0), gl_vertex_window_z(z1),
                                                 gl_vertex_window_z(z2), (float)pi + 0.5f, (float)pj + 0.5f));
    }
};

// The mode's window over the kernel's dynamic LDS: [win_cap depths], GL: [3 * vcache_cap floats] | [win_cap keys].
// (the contract render keeps no projected vertices: its dynamic LDS is the window alone)
template <bool GL>
__device__ __forceinline__ auto open_window(unsigned char* smem, int vcache_cap, const FusedJob& job)
{
    if constexpr (GL)
        return GlWindow{reinterpret_cast<uint64_t*>(smem + vertex_cache_bytes(vcache_cap)), reinterpret_cast<float*>(smem),
                        job.prm->n_verts <= vcache_cap, job};
    else
        return DepthWindow{reinterpret_cast<uint32_t*>(smem)};
}

// window box, both modes: leave `sh` as project_mesh does (raster.h), behind a barrier of their own.  They write shared memory
// first: the caller has no other use of sh / s_settled in flight.

// window box, contract.  The box and the `behind` flag from the eight corners of the mesh's box, by the whole first wave (lane l
// takes corner l & 7: corner_box_settles votes and reduces across the wave); the vertex pass only where the corners do not settle them.
__device__ __forceinline__ void box_from_corners(const FusedJob& job, MeshBoxShared& sh, int* s_settled)
{
    const int tid = threadIdx.x;
    const ObjParams& prm = *job.prm;
    box_reset(sh);
    __syncthreads();
    if (tid < 64 && prm.n_clusters > 0) {
        const int k = tid & 7;
        const float vc[3] = {prm.box_corners[3 * k], prm.box_corners[3 * k + 1], prm.box_corners[3 * k + 2]};
        int box[4];
        const bool settled = corner_box_settles(vc, job.P, job.fx, job.fy, job.cx, job.cy, job.tw, job.th, box);
        if (tid == 0) {
            *s_settled = settled ? 1 : 0;
            if (settled) { sh.box[0] = box[0]; sh.box[1] = box[1]; sh.box[2] = box[2]; sh.box[3] = box[3]; }
        }
    } else if (tid == 0) {
        *s_settled = 1;   // (no mesh: the empty box)
    }
    __syncthreads();
    if (!*s_settled) {
        auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, job.P, job.fx, job.fy, job.cx, job.cy, sx, sy, z); };
        project_mesh<kFusedThreads, 4>(prm.verts, prm.n_verts, false, nullptr, job.tw, job.th, sh.box, &sh.behind, project);
        __syncthreads();
    }
}

// window box, GL.  vertices -> screen and the pixel box of everything that can be drawn (raster.h), four vertices per thread fetched
// together; the projected vertices stay in the window's cache when they fit it.
__device__ __forceinline__ void box_from_vertices(const FusedJob& job, const GlWindow& win, MeshBoxShared& sh)
{
    box_reset(sh);
    __syncthreads();
    project_mesh<kFusedThreads, 4>(job.prm->verts, job.prm->n_verts, win.cached, win.s_v, job.tw, job.th, sh.box, &sh.behind, GlProject{job});
    __syncthreads();
}

// band split.  The `parts` workgroups of the alternative share its work as R bands of the window's rows x G groups of its triangles
// (R G = parts).  Rows only (G = 1): every workgroup walks all triangles and draws the rows of its band.  With triangle
// groups, the G workgroups of a band each draw their share of the triangles into a window of their own, the windows are
// merged in memory and the workgroup that arrives last scores the band: R is the smallest divisor of `parts` whose bands
// fit the LDS in one piece (1 for most objects: set-up and walk are divided by `parts`, nothing is done twice but the
// projection).  This is a pure function of its arguments, the same in every workgroup of the alternative but for `part`: every
// workgroup sees the same box and decides alike.  `all`: box_read behind the box stage's barrier.
struct BandSplit {
    int R, G, band, grp;   // this workgroup: band `band` of R, triangle group `grp` of G
    MeshBox box;           // the band's columns and rows (nothing to draw: not drawable())
};
__device__ __forceinline__ BandSplit band_split(int parts, int split_tris, int part, const MeshBox& all, int win_cap)
{
    BandSplit b;
    b.box = all;
    b.R = parts;
    if (split_tris && parts > 1 && all.drawable()) {
        const long long w_all = all.width(), rows_all = all.j1 - all.j0 + 1;
        for (b.R = 1; b.R < parts; ++b.R)
            if (parts % b.R == 0 && ((rows_all + b.R - 1) / b.R) * w_all <= (long long)win_cap) break;
    }
    b.G = parts / b.R;
    b.band = part / b.G;
    b.grp = part % b.G;
    if (all.j1 >= all.j0 && b.R > 1) {
        const int rows_all = all.j1 - all.j0 + 1;
        b.box.j0 = all.j0 + (int)((long long)rows_all * b.band / b.R);
        b.box.j1 = all.j0 + (int)((long long)rows_all * (b.band + 1) / b.R) - 1;
    }
    return b;
}

// draw, contract.  Reads the cleared window (the caller's barrier after clear), leaves this workgroup's triangles in it; the
// caller owes a barrier before anything reads the window.  `behind`: the box stage's flag.
// One wave, one cluster at a time (mesh_clusters.h).  The clusters are dealt out in turn to the G workgroups that share
// the band's triangles and to their waves -- neighbouring clusters, which cost alike, go to different workgroups.
// First every lane looks at ONE cluster of the wave's list: while the back-face rule is on it reads the cluster's
// header and asks its cone whether all of it faces away (cluster_faces_away: only clusters of which raster_projected
// would cull every triangle) -- such a cluster is neither fetched, projected nor drawn.  Then the wave walks the
// clusters that are left: lane v projects vertex slot v, lane t takes the corners of triangle t from the lanes that
// own them and draws it, with the next cluster's slots and words (coalesced loads, no address depends on a header) in
// flight meanwhile.  A spare word names slot 0 three times: zero area, nothing drawn.
__device__ __forceinline__ void draw_clusters(const FusedJob& job, const DepthWindow& win, const Strip& s, int G, int grp, int behind)
{
    const ObjParams& prm = *job.prm;
    const RenderPose& P = job.P;
    const float fx = job.fx, fy = job.fy, cx = job.cx, cy = job.cy;
    const int tid = threadIdx.x;
    const auto store = win.store(s);
    const bool rule_on = cull_table(prm.tri_flip, behind) != nullptr;
    const bool cones = rule_on && fx > 0.0f && fy > 0.0f && pose_is_rotation(P.R);   // (a quaternion as given may not be a unit one)
    const float f_lo = fminf(fx, fy), f_hi = fmaxf(fx, fy), c_abs = fabsf(cx) + fabsf(cy);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nc = prm.n_clusters, n_waves = kFusedThreads / 64;
    auto cluster_of = [=](int i) { return (i * n_waves + wave) * G + grp; };   // the wave's i-th cluster
    auto fetch = [&](int c, float (&v)[3], uint32_t& w) {
        const float* sl = prm.cl_slots + (size_t)c * 3 * kClusterSize + lane;
        v[0] = sl[0]; v[1] = sl[kClusterSize]; v[2] = sl[2 * kClusterSize];
        w = prm.cl_words[(size_t)c * kClusterSize + lane];
    };
    for (int base = 0; cluster_of(base) < nc; base += 64) {
        const int mine = cluster_of(base + lane);
        bool live = mine < nc;
        if (live && cones) {
            const uint4* hp = reinterpret_cast<const uint4*>(prm.cl_headers + (size_t)mine * kClusterWords);
            const uint4 h0 = hp[0], h1 = hp[1], h2 = hp[2], h3 = hp[3];
            static_assert(kCwCone == 2 && kCwAxis == 4 && kCwCos == 7 && kCwSin == 8 && kCwCenter == 9 && kCwRadius == 12 &&
                          kCwAreaMin == 13 && kCwEdgeMax == 14, "the header words as they are unpacked here");
            if (h0.z && cluster_faces_away(__uint_as_float(h1.x), __uint_as_float(h1.y), __uint_as_float(h1.z), __uint_as_float(h1.w),
                                           __uint_as_float(h2.x), __uint_as_float(h2.y), __uint_as_float(h2.z), __uint_as_float(h2.w),
                                           __uint_as_float(h3.x), __uint_as_float(h3.y), __uint_as_float(h3.z), P.R, P.t, f_lo, f_hi, c_abs))
                live = false;
        }
        unsigned long long todo = __ballot(live);
        if (!todo) continue;
        float v[3];
        uint32_t w;
        fetch(cluster_of(base + (int)__builtin_ctzll(todo)), v, w);
        while (todo) {
            todo &= todo - 1;
            float v_n[3] = {v[0], v[1], v[2]};
            uint32_t w_n = w;
            if (todo) fetch(cluster_of(base + (int)__builtin_ctzll(todo)), v_n, w_n);
            float sx, sy, z;
            project_vertex(v, P, fx, fy, cx, cy, sx, sy, z);
            const int a0 = (int)(w & 63u), a1 = (int)((w >> 6) & 63u), a2 = (int)((w >> 12) & 63u);
            const float x0 = __shfl(sx, a0, 64), y0 = __shfl(sy, a0, 64), z0 = __shfl(z, a0, 64);
            const float x1 = __shfl(sx, a1, 64), y1 = __shfl(sy, a1, 64), z1 = __shfl(z, a1, 64);
            const float x2 = __shfl(sx, a2, 64), y2 = __shfl(sy, a2, 64), z2 = __shfl(z, a2, 64);
            raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, job.tw, job.th, s.js, s.je, rule_on ? 1 + (int)((w >> 18) & 1u) : 0, store);
            v[0] = v_n[0]; v[1] = v_n[1]; v[2] = v_n[2];
            w = w_n;
        }
    }
}

// draw, GL.  Reads the cleared window (the caller's barrier after clear) and the vertex cache, leaves every triangle's fragments in
// the window; the caller owes a barrier before anything reads it.
// Every triangle in the caller's order (tris are uploaded unsorted in this mode; the key's low word is that index), kTB per thread
// whose vertex indices are fetched together.
__device__ __forceinline__ void draw_triangles_gl(const FusedJob& job, const GlWindow& win, const Strip& s)
{
    const ObjParams& prm = *job.prm;
    const int tid = threadIdx.x, nt = prm.n_tris;
    const auto store_key = win.store(s);
    constexpr int kTB = 8;
    for (int tb = tid; tb < nt; tb += kTB * kFusedThreads) {
        int idx[kTB][3];
#pragma unroll
        for (int k = 0; k < kTB; ++k) {
            const int32_t* tri = prm.tris + (size_t)3 * min(tb + k * kFusedThreads, nt - 1);
            idx[k][0] = tri[0]; idx[k][1] = tri[1]; idx[k][2] = tri[2];
        }
#pragma unroll
        for (int k = 0; k < kTB; ++k) {
            if (tb + k * kFusedThreads >= nt) break;
            float x0, y0, z0, x1, y1, z1, x2, y2, z2;
            fetch_triangle(win.s_v, win.cached, prm.verts, idx[k][0], idx[k][1], idx[k][2], GlProject{job}, x0, y0, z0, x1, y1, z1, x2, y2, z2);
            const uint64_t t = (uint32_t)(tb + k * kFusedThreads);
            raster_projected_gl(x0, y0, z0, x1, y1, z1, x2, y2, z2, job.tw, job.th, s.js, s.je,
                                [&](int i, int j, uint32_t qz) { store_key(i, j, ((uint64_t)qz << 32) | t); });
        }
    }
}

// merge (contract with G > 1 only).  Reads this workgroup's drawn window behind the caller's barrier after the draw.  True: this
// workgroup arrived last of the band's G, the window now holds the minimum over all G windows, behind a barrier of the function's
// own, and the workgroup goes on alone: dump, samples, sums.  False: another workgroup will; the caller returns, all threads alike
// (the answer is workgroup-uniform: it goes through *s_last and a barrier).
// This workgroup's window -> its slab in memory, written through (agent-coherent stores: the workgroups of an
// alternative may sit on different XCDs, each behind an L2 of its own); the workgroup that arrives last reads all
// slabs back with agent-coherent loads and keeps the nearest depth of every pixel.  No atomics on the pixels, nothing to clear
// afterwards: every slab is rewritten whole by the next test.
__device__ __forceinline__ bool merge_slabs(const EngineArrays& a, int lin, const FusedJob& job, const BandSplit& bs, int parts, uint32_t* s_z,
                                            int npx, int* s_last)
{
    const int tid = threadIdx.x, G = bs.G, grp = bs.grp;
    const size_t slab0 = (((size_t)lin * a.zmerge_slabs + (size_t)job.obj * parts + (size_t)bs.band * G) * 2 + job.alt) * a.zmerge_stride;   // the band's first slab
    uint32_t* mine = a.zmerge + slab0 + (size_t)grp * 2 * a.zmerge_stride;
    int* arrivals = a.zcount + (((size_t)lin * a.n_obj + job.obj) * 2 + job.alt) * kMaxOutlierParts + bs.band;
    for (int i = tid; i < npx; i += kFusedThreads)
        __hip_atomic_store(&mine[i], s_z[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0);   // every store of this wave acknowledged
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __syncthreads();
    if (tid == 0) {
        const int before = __hip_atomic_fetch_add(arrivals, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_last = (before == G - 1) ? 1 : 0;
        if (before == G - 1) __hip_atomic_store(arrivals, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!*s_last) return false;
    // (agent-coherent loads, a pixel's G - 1 of them in flight together: as atomic loads the compiler waits for each one)
    static_assert(kMaxOutlierParts <= 8, "eight slabs per pixel");
    const uint32_t* others = a.zmerge + slab0;
    const size_t slab_step = 2 * a.zmerge_stride;
    // the other groups' slabs, compacted (G - 1 pointers); the loads and the wait that makes them valid are ONE asm
    // statement per pixel with early-clobber outputs (round 5, ADVICE: as separate statements the compiler was free to
    // move, spill or reuse the destination registers between the load and the s_waitcnt)
    const uint32_t* op[7];
    {
        int k = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p)
            if (p < G && p != grp && k < 7) op[k++] = others + (size_t)p * slab_step;
        for (; k < 7; ++k) op[k] = others;
    }
    for (int i = tid; i < npx; i += kFusedThreads) {
        uint32_t m = s_z[i];
        uint32_t v0, v1, v2, v3, v4, v5, v6;
        switch (G - 1) {   // (uniform)
        case 1:
            asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v0) : "v"(op[0] + i) : "memory");
            m = min(m, v0);
            break;
        case 2:
            asm volatile("global_load_dword %0, %2, off sc1\n\tglobal_load_dword %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(v0), "=&v"(v1) : "v"(op[0] + i), "v"(op[1] + i) : "memory");
            m = min(m, min(v0, v1));
            break;
        case 3:
            asm volatile("global_load_dword %0, %3, off sc1\n\tglobal_load_dword %1, %4, off sc1\n\tglobal_load_dword %2, %5, off sc1\n\t"
                         "s_waitcnt vmcnt(0)"
                         : "=&v"(v0), "=&v"(v1), "=&v"(v2) : "v"(op[0] + i), "v"(op[1] + i), "v"(op[2] + i) : "memory");
            m = min(min(m, v0), min(v1, v2));
            break;
        case 4:
            asm volatile("global_load_dword %0, %4, off sc1\n\tglobal_load_dword %1, %5, off sc1\n\tglobal_load_dword %2, %6, off sc1\n\t"
                         "global_load_dword %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3) : "v"(op[0] + i), "v"(op[1] + i), "v"(op[2] + i), "v"(op[3] + i) : "memory");
            m = min(m, min(min(v0, v1), min(v2, v3)));
            break;
        default:   // 5 .. 7 others: seven loads (the spare pointers repeat the first slab: harmless under min)
            asm volatile("global_load_dword %0, %7, off sc1\n\tglobal_load_dword %1, %8, off sc1\n\tglobal_load_dword %2, %9, off sc1\n\t"
                         "global_load_dword %3, %10, off sc1\n\tglobal_load_dword %4, %11, off sc1\n\tglobal_load_dword %5, %12, off sc1\n\t"
                         "global_load_dword %6, %13, off sc1\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(v5), "=&v"(v6)
                         : "v"(op[0] + i), "v"(op[1] + i), "v"(op[2] + i), "v"(op[3] + i), "v"(op[4] + i), "v"(op[5] + i), "v"(op[6] + i) : "memory");
            m = min(min(m, v0), min(min(v1, v2), min(min(v3, v4), min(v5, v6))));
            break;
        case 0: break;
        }
        s_z[i] = m;
    }
    __syncthreads();
    return true;
}

// dump.  Operator level (roft_render_depth / roft_outlier_test): the strip of the window as this workgroup drew it -> the caller's
// (zero-filled) render tile of the alternative, 0 = background as the reference reads it back.  Reads the window behind the draw's
// (or the merge's) barrier; writes memory only.
template <class Window>
__device__ __forceinline__ void dump_strip(const Window& win, const Strip& s, float* tile, int tw)
{
    for (int i = threadIdx.x; i < s.npx; i += kFusedThreads) {
        const int pi = s.i0 + i % s.win_w, pj = s.js + i / s.win_w;
        tile[(size_t)pj * tw + pi] = win.covered(i) ? win.depth(i, pi, pj) : 0.0f;
    }
}

// The buffered features the lane's test reads (k_features.hip): (v << 16 | u) and depth per slot
struct FeatureList {
    const uint32_t* pix;
    const float* dep;
    int n;
};
__device__ __forceinline__ FeatureList pending_features(const EngineArrays& a, const FusedJob& job)
{
    const int fslot = (job.c->feat_read >= 0) ? job.c->feat_read : 0;
    return {a.feat_pix + ((size_t)job.obj * kFeatRing + fslot) * a.feat_cap, a.feat_depth + ((size_t)job.obj * kFeatRing + fslot) * a.feat_cap,
            job.st->n_feat[fslot]};
}

// score.  The likelihood samples of this strip into the thread's sums (feature slots in ascending order per thread, as
// outlier_kernel adds them; the sums are exact integers, so the order is free anyway).  Reads the window behind the draw's (or the
// merge's) barrier; the caller owes a barrier before the next strip clears the window.
template <class Window>
__device__ __forceinline__ void score_strip(const Window& win, const Strip& s, const FeatureList& ft, int d, LikelihoodSum& err, int& cnt)
{
    constexpr int kBatch = 16;
    for (int f0 = threadIdx.x; f0 < ft.n; f0 += kBatch * kFusedThreads) {
        float dep[kBatch];
        uint32_t pix[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int i = f0 + k * kFusedThreads;
            dep[k] = (i < ft.n) ? ft.dep[i] : 0.0f;
            pix[k] = (i < ft.n) ? ft.pix[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (!((dep[k] > 0) && ((double)dep[k] < 2.0))) continue;  // hard-coded 2.0 (ROFTFilter.cpp:561)
            const int v = (int)(pix[k] >> 16), u = (int)(pix[k] & 0xFFFFu);
            const int tj = v / d, ti = u / d;
            if (tj < s.js || tj > s.je || ti < s.i0 || ti > s.i1) continue;
            const int i = (tj - s.js) * s.win_w + (ti - s.i0);
            if (win.covered(i)) { err.add(fabsf(dep[k] - win.depth(i, ti, tj))); cnt += 1; }
        }
    }
}

// band sums.  The threads' sums -> the band's partial sums in the lane (the pose chain segment that follows adds them up in band
// order and decides).  One workgroup per band gets here -- with triangle groups the one that merged the band -- with the sums of
// its rows.  Barrier inside; nothing owed.
__device__ __forceinline__ void band_sums(LikelihoodSum err, int cnt, long long* s_hi, long long* s_lo, int* s_cnt, PoseLane& pl, int alt, int band, int R)
{
    const int tid = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) {
        err.hi += __shfl_down(err.hi, off, 64);
        err.lo += __shfl_down(err.lo, off, 64);
        cnt += __shfl_down(cnt, off, 64);
    }
    if ((tid & 63) == 0) { s_hi[tid >> 6] = err.hi; s_lo[tid >> 6] = err.lo; s_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        long long hi = 0, lo = 0;
        int n2 = 0;
        for (int w = 0; w < kFusedThreads / 64; ++w) { hi += s_hi[w]; lo += s_lo[w]; n2 += s_cnt[w]; }
        pl.part_hi[alt][band] = hi;
        pl.part_lo[alt][band] = lo;
        pl.part_cnt[alt][band] = (double)n2;
        if (band == 0) pl.n_parts[alt] = R;
    }
}

// phase stamps (-DROFT_FUSED_PROFILE; PHASES=fused tools/k1_phase_profile.py): 100 MHz ticks -> ObjState::dbg[alt * 8 + phase]:
// 0 box, 1 clear, 2 draw, 3 merge + dump + score; words 4 - 6: strips, window width x 100, band rows x 100
#ifdef ROFT_FUSED_PROFILE
#define UTICK(i) do { __syncthreads(); if (threadIdx.x == 0 && job.bx < 4) { long long _t = wall_clock64(); job.st->dbg[job.bx * 8 + (i)] += _t - u_t0; u_t0 = _t; } } while (0)
#else
#define UTICK(i) do {} while (0)
#endif

template <bool GL>
__global__ __launch_bounds__(kFusedThreads) void outlier_fused_kernel(EngineArrays a, int lin, int vcache_cap, int win_cap, int parts,
                                                                     int split_tris, float* tile_dump)
{
    ROFT_RESIDENT(a, RK_OUTLIER);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ long long s_hi[kFusedThreads / 64], s_lo[kFusedThreads / 64];
    __shared__ int s_cnt[kFusedThreads / 64];
    __shared__ MeshBoxShared s_mb;
    __shared__ int s_last;
    __shared__ int s_settled;
    FusedJob job;
    if (!fused_job(a, lin, parts, job)) return;
#ifdef ROFT_FUSED_PROFILE
    long long u_t0 = wall_clock64();
    if (threadIdx.x < 8 && job.bx < 4) job.st->dbg[job.bx * 8 + threadIdx.x] = 0;
#endif
    const auto win = open_window<GL>(smem, vcache_cap, job);
    if constexpr (GL) box_from_vertices(job, win, s_mb);
    else box_from_corners(job, s_mb, &s_settled);
    UTICK(0);
    const BandSplit bs = band_split(parts, GL ? 0 : split_tris, job.part, box_read(s_mb, job.tw, job.th), win_cap);
    const FeatureList ft = pending_features(a, job);
    LikelihoodSum err;
    int cnt = 0;
    if (bs.box.drawable()) {
        const int rows = strip_rows(win_cap, bs.box.width());   // (win_cap >= the target's width: a strip holds at least one row)
        for (int js = bs.box.j0; js <= bs.box.j1; js += rows) {
            const Strip s = strip_from(bs.box, js, rows);
            win.clear(s.npx, kFusedThreads);
            __syncthreads();
            UTICK(1);
            if constexpr (GL) draw_triangles_gl(job, win, s);
            else draw_clusters(job, win, s, bs.G, bs.grp, s_mb.behind);
            __syncthreads();
            UTICK(2);
            if constexpr (!GL)
                if (bs.G > 1 && !merge_slabs(a, lin, job, bs, parts, win.z, s.npx, &s_last)) return;
            if (tile_dump) dump_strip(win, s, tile_dump + (size_t)job.alt * job.tw * job.th, job.tw);
            score_strip(win, s, ft, job.d, err, cnt);
            __syncthreads();   // the next strip clears the window
            UTICK(3);
#ifdef ROFT_FUSED_PROFILE
            if (threadIdx.x == 0 && job.bx < 4) job.st->dbg[job.bx * 8 + 4] += 1;
            if (threadIdx.x == 0 && job.bx < 4) job.st->dbg[job.bx * 8 + 5] = (long long)bs.box.width() * 100;
            if (threadIdx.x == 0 && job.bx < 4) job.st->dbg[job.bx * 8 + 6] = (long long)(bs.box.j1 - bs.box.j0 + 1) * 100;
#endif
        }
    }
    band_sums(err, cnt, s_hi, s_lo, s_cnt, *job.pl, job.alt, bs.band, bs.R);
}

// ---- the launcher -----------------------------------------------------------------------------------------------------------------

// The split switch: several workgroups per alternative share its TRIANGLES (1) or only its window's rows (0).  Three overrides, in
// this order: the caller's OutlierLaunchOpts::split, the process-wide roft_debug_outlier_split, the environment's
// ROFT_OUTLIER_SPLIT (experiments; read once, at first use); else triangles.
static std::atomic<int> g_outlier_split{-1};   // roft_debug_outlier_split
void set_outlier_split(int mode) { g_outlier_split.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }

static int outlier_split_wanted(const OutlierLaunchOpts* opts)
{
    static const int env = getenv("ROFT_OUTLIER_SPLIT") ? atoi(getenv("ROFT_OUTLIER_SPLIT")) : -1;
    if (opts && opts->split >= 0) return opts->split;
    const int debug = g_outlier_split.load(std::memory_order_relaxed);
    if (debug >= 0) return debug;
    return env >= 0 ? env : 1;
}

// The shape of one launch, derived once from (a, opts, gl).
struct OutlierShape {
    int parts;        // workgroups per alternative
    int split;        // the kernel's split_tris
    int vcache_cap;   // GL: vertices the cache holds (0: none)
    int win_cap;      // pixels the window holds
    size_t lds;       // dynamic LDS of a workgroup
};

static OutlierShape outlier_shape(const EngineArrays& a, const OutlierLaunchOpts* opts, bool gl)
{
    OutlierShape sh;
    const size_t lds_total = kRasterLdsBudget;
    // render mode: the GL numerics keep an 8-byte key per window pixel (GlWindow), the contract a 4-byte depth (DepthWindow)
    const size_t zb = gl ? 8 : 4;
    // GL: cache the projected vertices when they leave room for a window of 8 k pixels (a window that large or larger is
    // rendered in strips) and for the widest row of the target.  The contract render walks clusters and caches nothing: its
    // LDS is the window alone.
    const size_t vbytes = vertex_cache_bytes(a.max_verts);
    const size_t min_win = zb * std::max(8192, a.tile_w);
    const bool cache = gl && vbytes + min_win <= lds_total && !(opts && opts->no_vertex_cache);
    const size_t cache_bytes = cache ? vbytes : 0;
    sh.vcache_cap = cache ? a.max_verts : 0;
    // bands per alternative: as many workgroups as the chip has CUs to spare
    sh.parts = std::max(1, std::min(kMaxOutlierParts, device_cu_count() / (2 * std::max(a.n_obj, 1))));
    if (a.outlier_parts > 0) sh.parts = std::min(a.outlier_parts, kMaxOutlierParts);
    if (opts && opts->parts > 0) sh.parts = std::min(opts->parts, kMaxOutlierParts);
    if (opts && opts->parts < 0) sh.parts = std::max(1, sh.parts / -opts->parts);
    // Several workgroups per alternative share its TRIANGLES (R bands x G triangle groups, decided per alternative inside the
    // kernel from the size of its window: band_split) unless the caller asks for rows only -- or the structure rules it out:
    sh.split = outlier_split_wanted(opts);
    if (sh.parts <= 1) sh.split = 0;                                                            // nothing to share
    if (!a.zmerge || (size_t)a.n_obj * sh.parts > a.zmerge_slabs) sh.split = 0;                 // no slabs, or too few
    if (gl) sh.split = 0;   // (GL: the workgroups of an alternative split only the rows of its window; its slabs would be 64-bit)
    // (a band is a fraction of the window: request only the LDS it can need, so that other chains' workgroups fit next to it)
    const int lds_parts = sh.split ? 1 : sh.parts;
    const size_t win_need = zb * std::max((size_t)a.tile_w, ((size_t)a.tile_w * a.tile_h + lds_parts - 1) / lds_parts + (size_t)a.tile_w);
    sh.lds = std::min(lds_total, ((cache_bytes + win_need + 15) & ~(size_t)15));
    sh.win_cap = std::min((int)((lds_total - cache_bytes) / zb), (int)((sh.lds - cache_bytes) / zb));
    // (operator level: a smaller window forces the strip path)
    if (opts && opts->window_pixels > 0) sh.win_cap = std::max(a.tile_w, std::min(sh.win_cap, opts->window_pixels));
    return sh;
}

int launch_outlier(const EngineArrays& a, int lin, hipStream_t s, hipEvent_t stop, const OutlierLaunchOpts* opts)
{
    const bool gl = opts && opts->render_mode == ROFT_RENDER_GL;
    // (the contract kernel walks clusters only: a mesh without them would be drawn as nothing, silently)
    if (!gl && a.meshes_without_clusters > 0)
        return host::fail(ROFT_ERR_STATE, "outlier test: a mesh went up without clusters (MeshLayout::kWalkClusters)");
    // objects that do not test this frame return immediately; the decision (ROFTFilter.cpp:581-583) is taken by the
    // pose chain segment that follows (ukf_chain_kernel)
    const OutlierShape sh = outlier_shape(a, opts, gl);
    const dim3 grid(2 * sh.parts * ((a.n_obj + 7) / 8) * 8);   // (fused_job: objects in groups of eight)
    const auto launch = [&](auto kernel) {
        (void)set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)kRasterLdsBudget);
        hipExtLaunchKernelGGL(kernel, grid, dim3(kFusedThreads), (uint32_t)sh.lds, s, nullptr, stop, 0, a, lin, sh.vcache_cap, sh.win_cap, sh.parts,
                              sh.split, opts ? opts->tile_dump : nullptr);
    };
    if (gl) launch(outlier_fused_kernel<true>);
    else launch(outlier_fused_kernel<false>);
    return ROFT_OK;
}

void launch_outlier_only(const EngineArrays& a, hipStream_t s)
{
    hipLaunchKernelGGL(outlier_kernel, dim3(a.n_obj), dim3(kOutlierThreads), 0, s, a, 0);
}

}  // namespace roft
