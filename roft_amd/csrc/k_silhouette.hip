// k_silhouette.hip -- masks from poses (gfx950): the silhouette of an object's mesh at a delivered pose, drawn straight into the
// bit planes a delivered mask would have been ingested into (include/roft_engine.h, section 3e).
//
// The mask is M(p) = roft_render_depth(mesh, pose_x, pose_q, cam, 1)(p) > 0 ? 255 : 0: the render contract at full resolution
// (raster.h: make_pose / project_vertex / raster_projected unchanged, the back-face rule for closed meshes as k_quality.hip and
// outlier_fused_kernel apply it), of which only "some triangle covers the pixel with z > 0" is kept -- one bit.  So the store of
// the rasteriser is an LDS atomicOr, the result is an order-free OR, and no band count, strip height or triangle order changes it.
//
// One workgroup = one band of image rows of one (delivering frame, enrolled object) pair; ONE launch covers every pair of a batch
// (grid z: the batch's delivering frames, four bits each in frames_packed; a pair that is not enrolled, or whose mask arrived
// another way, leaves at once).  The workgroup projects the vertices once -- into LDS where the mesh fits, else again per triangle --
// and takes the row box of everything that can be drawn from them; it clears a bit window of its rows in LDS, walks the triangles
// over [j_lo, j_hi] = band x box (a band the box misses walks none), and flushes the window: EVERY word of BOTH planes of slot
// slot0 + t is written, zeros included (the slot holds stale words; a silhouette has no pixel of value 1: nz == obj, new_ones
// stays 0), consecutive threads consecutive words, and the population count goes to mrec[t + 1][obj].new_count behind a wave
// reduction, as label_ingest_kernel does.  A band taller than the window is drawn in strips.
// Built with -ffp-contract=off like every user of raster.h.
#include <algorithm>

#include "raster.h"

namespace roft {

constexpr int kSilhouetteThreads = 256;

__global__ __launch_bounds__(kSilhouetteThreads) void pose_silhouette_kernel(SilhouetteArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_rows[2];   // first and last image row anything can be drawn in
    __shared__ int s_behind;    // some vertex is not in front of the near plane: a closed mesh is then drawn whole too
    const int obj = blockIdx.y, tid = threadIdx.x;
    const int t = (int)((sa.frames_packed >> (4 * blockIdx.z)) & 15u);
    const FrameCtrl& c = sa.ctrl[(size_t)t * sa.n_obj + obj];
    if (c.label_type != kMaskFromPose) return;   // (workgroup-uniform)
    const ObjParams& prm = sa.params[obj];
    const RenderPose P = make_pose(c.pose_x, c.pose_q);
    const int W = sa.W, H = sa.H, wpr = sa.wpr;
    const float fx = sa.fx, fy = sa.fy, cx = sa.cx, cy = sa.cy;
    const int nv = prm.n_verts, nt = prm.n_tris;
    const bool cached = nv <= sa.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    uint32_t* s_win = reinterpret_cast<uint32_t*>(smem + (((size_t)sa.vcache_cap * 12 + 15) & ~(size_t)15));
    if (tid == 0) { s_rows[0] = INT32_MAX; s_rows[1] = -1; s_behind = 0; }
    __syncthreads();

    // vertices -> screen, and the rows of everything that can be drawn (the row range raster_projected clips a triangle to is
    // monotone in the coordinates of its vertices, so the range of the vertices in front covers every triangle that is drawn)
    {
        int bj0 = INT32_MAX, bj1 = -1;
        bool behind = false;
        for (int v = tid; v < nv; v += kSilhouetteThreads) {
            float vc[3], sx, sy, z;
#pragma unroll
            for (int q = 0; q < 3; ++q) vc[q] = prm.verts[(size_t)3 * v + q];
            project_vertex(vc, P, fx, fy, cx, cy, sx, sy, z);
            if (cached) { s_v[3 * v] = sx; s_v[3 * v + 1] = sy; s_v[3 * v + 2] = z; }
            if (z > 0.001f) {
                // (a vertex far outside the image clamps to an empty or full range; NaN coordinates fail every comparison of the
                //  rasteriser: nothing of such a triangle is drawn, and fminf / fmaxf drop the NaN here)
                const float lo_j = fminf(fmaxf(ceilf(sy - 0.5f), 0.0f), (float)H), hi_j = fminf(fmaxf(floorf(sy - 0.5f), -1.0f), (float)(H - 1));
                bj0 = min(bj0, (int)lo_j); bj1 = max(bj1, (int)hi_j);
            } else {
                behind = true;
            }
        }
        if (__any(behind) && (tid & 63) == 0) atomicOr(&s_behind, 1);
        for (int off = 32; off > 0; off >>= 1) {
            bj0 = min(bj0, __shfl_xor(bj0, off, 64));
            bj1 = max(bj1, __shfl_xor(bj1, off, 64));
        }
        if ((tid & 63) == 0) { atomicMin(&s_rows[0], bj0); atomicMax(&s_rows[1], bj1); }
    }
    __syncthreads();
    const int box0 = s_rows[0], box1 = s_rows[1];
    const uint8_t* const flips = (prm.tri_flip && !s_behind) ? prm.tri_flip : nullptr;

    // the band's rows, strip by strip
    const int bands = (int)gridDim.x, band = (int)blockIdx.x;
    const int r0 = (int)(((long long)band * H) / bands), r1 = (int)(((long long)(band + 1) * H) / bands) - 1;
    uint32_t* const planes = sa.planes + (size_t)obj * sa.obj_stride + (size_t)(sa.slot0 + t) * 2 * sa.plane_words;
    int count = 0;
    for (int js = r0; js <= r1; js += sa.win_rows) {
        const int je = min(r1, js + sa.win_rows - 1), n_words = (je - js + 1) * wpr;
        for (int i = tid; i < n_words; i += kSilhouetteThreads) s_win[i] = 0u;
        __syncthreads();
        const int j_lo = max(js, box0), j_hi = min(je, box1);
        if (j_lo <= j_hi) {
            ROFT_LDS uint32_t* const win = pin_lds(s_win);
            auto store = [win, js, wpr](int i, int j, float) {
                (void)__hip_atomic_fetch_or(win + ((j - js) * wpr + (i >> 5)), 1u << (i & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            for (int k = tid; k < nt; k += kSilhouetteThreads) {
                const int32_t* tri = prm.tris + (size_t)3 * k;
                const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
                const int cull = flips ? 1 + (int)flips[k] : 0;
                float x0, y0, z0, x1, y1, z1, x2, y2, z2;
                if (cached) {
                    x0 = s_v[3 * v0]; y0 = s_v[3 * v0 + 1]; z0 = s_v[3 * v0 + 2];
                    x1 = s_v[3 * v1]; y1 = s_v[3 * v1 + 1]; z1 = s_v[3 * v1 + 2];
                    x2 = s_v[3 * v2]; y2 = s_v[3 * v2 + 1]; z2 = s_v[3 * v2 + 2];
                } else {
                    project_vertex(prm.verts + (size_t)3 * v0, P, fx, fy, cx, cy, x0, y0, z0);
                    project_vertex(prm.verts + (size_t)3 * v1, P, fx, fy, cx, cy, x1, y1, z1);
                    project_vertex(prm.verts + (size_t)3 * v2, P, fx, fy, cx, cy, x2, y2, z2);
                }
                raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, W, H, j_lo, j_hi, cull, store);
            }
            __syncthreads();
        }
        // flush: the strip's words are consecutive in the planes (wpr words per row, rows js .. je)
        uint32_t* const nz = planes + (size_t)js * wpr;
        uint32_t* const ob = nz + sa.plane_words;
        for (int i = tid; i < n_words; i += kSilhouetteThreads) {
            const uint32_t w = s_win[i];
            nz[i] = w;
            ob[i] = w;
            count += __popc(w);
        }
        __syncthreads();   // the next strip clears the window
    }
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if ((tid & 63) == 0 && count) atomicAdd(&sa.mrec[(size_t)(t + 1) * sa.n_obj + obj].new_count, count);
}

// LDS of a workgroup: the projected vertices of the largest mesh where the cache is on and they fit it, and the bit window of one
// strip -- the rows of a band, at most kSilhouetteWindowWords words.  A small mesh on a small image takes a few KB, so that several
// workgroups share a CU with the chains the launch runs next to.
bool launch_pose_silhouette(SilhouetteArgs sa, int n_frames, int max_verts, int bands, int vertex_cache, hipStream_t s, hipEvent_t start,
                            hipEvent_t stop)
{
    if (sa.wpr <= 0 || sa.wpr > kSilhouetteWindowWords || sa.H <= 0 || n_frames <= 0 || sa.n_obj <= 0) return false;
    if (bands <= 0) bands = (sa.H + 63) / 64;
    bands = std::min(bands, std::min(sa.H, 1024));
    const int band_rows = (sa.H + bands - 1) / bands;   // (the tallest band)
    sa.win_rows = std::max(1, std::min(band_rows, kSilhouetteWindowWords / sa.wpr));
    sa.vcache_cap = (vertex_cache && max_verts <= kSilhouetteCacheVerts) ? std::max(max_verts, 0) : 0;
    const size_t vbytes = ((size_t)sa.vcache_cap * 12 + 15) & ~(size_t)15;
    const size_t lds = vbytes + 4 * (size_t)sa.win_rows * sa.wpr;
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(pose_silhouette_kernel), 160 * 1024 - 4096);
    hipExtLaunchKernelGGL(pose_silhouette_kernel, dim3(bands, sa.n_obj, n_frames), dim3(kSilhouetteThreads), (uint32_t)lds, s, start, stop, 0, sa);
    return true;
}

}  // namespace roft
