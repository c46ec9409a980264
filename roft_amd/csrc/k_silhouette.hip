// k_silhouette.hip -- masks from poses (gfx950): the silhouette of an object's mesh at a delivered pose, drawn straight into the
// bit planes a delivered mask would have been ingested into (include/roft_engine.h, section 3e).
//
// The mask is M(p) = roft_render_depth(mesh, pose_x, pose_q, cam, 1)(p) > 0 ? 255 : 0: the render contract at full resolution
// (raster.h's draw contract), of which only "some triangle covers the pixel with z > 0" is kept -- one bit.  So the store of the
// rasteriser is an LDS atomicOr, the result is an order-free OR, and no band count, strip height or triangle order changes it.
//
// One workgroup = one band of image rows of one (delivering frame, enrolled object) pair; ONE launch covers every pair of a batch
// (grid z: the batch's delivering frames, four bits each in frames_packed; a pair that is not enrolled, or whose mask arrived
// another way, leaves at once).  What the kernel does with raster.h's draw contract: its window holds BITS, wpr words per image
// row, and it uses only the ROWS of the box (project_mesh's kRowsOnly, read as the pass left them: a box nothing widened meets no
// band), drawing over [j_lo, j_hi] = band x box.  Its triangle loop is draw_triangles' spelled out (measured: docs/notebook.md).
// The flush writes EVERY word of BOTH planes of slot slot0 + t, zeros included (the slot holds stale words; a silhouette has no
// pixel of value 1: nz == obj, new_ones stays 0), consecutive threads consecutive words, and the population count goes to
// mrec[t + 1][obj].new_count behind a wave reduction, as label_ingest_kernel does.
// Built with -ffp-contract=off like every user of raster.h.
//
// THE DEPTH GATE (kGate; section 3e, "gated against the depth of the pose's own frame").  With R(p) the rendered depth -- the
// smallest z any covering triangle has at p -- and D = FrameCtrl::gate_depth[p], a covered pixel stays when
//     keep(R, D) = !(D > 0 && D < fl(R - tf)) && !(tb > 0 && D > fl(R + tb)).
// A pair drawn alone keeps NO z: rounding to float is monotone, so fl(min_t z_t - tf) = min_t fl(z_t - tf) and likewise for + tb;
// "D < the smallest bound" holds exactly when it holds for every covering triangle, and "D > fl(R + tb)" exactly when it holds for
// some covering triangle (the smallest z gives the smallest bound).  Hence
//     not occluded = OR_t !(D > 0 && D < fl(z_t - tf)),      behind = OR_t (D > fl(z_t + tb)),
// two more order-free bit windows next to the covered one, and the flush keeps covered & not-occluded & ~behind.  (A NaN or zero D
// fails every comparison: kept.)  The window's rows shrink to a third; the price is one scattered 4-byte load of D per covered
// (triangle, pixel) -- the lanes of a wave walk different triangles -- inside the object's box, which the L2 holds.
// A pair drawn against a z-buffer is gated by the resolve, which holds R(p) in the entry's high word.
// The pair's workgroups add what they saw to its SilhouettePair; the last one (a ticket) adds the pair to gstats -- emptied, pixels
// removed in front, pixels removed behind --, writes gremoved where the caller asked, and leaves the record zeroed.
#include <algorithm>

#include "raster.h"

namespace roft {

constexpr int kSilhouetteThreads = 256;

// The gate's part of a pair's ticket: `had` pixels went into the gate (the plain silhouette's, or the resolved one's); front and
// behind are complete.  Leaves both zeroed.
__device__ __forceinline__ void gate_pair_done(const SilhouetteArgs& sa, SilhouettePair& pr, int had, size_t pair)
{
    const int front = atomicAdd(&pr.front, 0), behind = atomicAdd(&pr.behind, 0);
    if (had > 0 && front + behind == had) atomicAdd(&sa.gstats[0], 1ull);
    if (front) atomicAdd(&sa.gstats[1], (unsigned long long)front);
    if (behind) atomicAdd(&sa.gstats[2], (unsigned long long)behind);
    if (sa.gremoved) { sa.gremoved[2 * pair] = front; sa.gremoved[2 * pair + 1] = behind; }
    pr.front = 0; pr.behind = 0;
}

// kZ: the launch of a batch that has silhouettes to resolve (section 3e, "objects of one scene hide each other").  A pair whose
// FrameCtrl::label names a z-buffer (1 + its index) is DRAWN here and not flushed: every covered pixel sends
// (float bits of z) << 32 | obj through a 64-bit atomicMin to the z-buffer of its (delivering frame, scene) -- positive floats order
// like their bit patterns, the low word is the tie rule "lower id" --, the bit window only counts the plain silhouette's pixels, and
// the pair leaves its row box; pose_resolve_kernel below writes its planes.  Every other pair is drawn and flushed as without kZ.
template <bool kZ, bool kGate>
__global__ __launch_bounds__(kSilhouetteThreads) void pose_silhouette_kernel(SilhouetteArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ MeshBoxShared s_mb;   // (of which the rows are used: the first and last image row anything can be drawn in)
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
    uint32_t* s_win = reinterpret_cast<uint32_t*>(smem + vertex_cache_bytes(sa.vcache_cap));
    box_reset(s_mb);
    __syncthreads();

    // vertices -> screen and the rows of everything that can be drawn (raster.h; rows only: the columns, which nothing here reads,
    // were measured at 1 - 2 % of the launch, docs/notebook.md)
    auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, P, fx, fy, cx, cy, sx, sy, z); };
    project_mesh<kSilhouetteThreads, 1, true>(prm.verts, nv, cached, s_v, W, H, s_mb.box, &s_mb.behind, project);
    __syncthreads();
    const int box0 = s_mb.box[1], box1 = s_mb.box[3];
    const bool to_z = kZ && c.label > 0;   // (workgroup-uniform)
    unsigned long long* const zb = to_z ? sa.zbuf + ((size_t)blockIdx.z * sa.n_zscenes + (c.label - 1)) * ((size_t)W * H) : nullptr;
    const uint8_t* const flips = cull_table(prm.tri_flip, s_mb.behind);

    // the band's rows, strip by strip
    const int bands = (int)gridDim.x, band = (int)blockIdx.x;
    const int r0 = (int)(((long long)band * H) / bands), r1 = (int)(((long long)(band + 1) * H) / bands) - 1;
    uint32_t* const planes = sa.planes + (size_t)obj * sa.obj_stride + (size_t)(sa.slot0 + t) * 2 * sa.plane_words;
    int count = 0;
    // the gate of a pair drawn alone: three windows of win_words words each -- covered | not occluded | behind
    const float* const gd = c.gate_depth;
    const bool gated = kGate && !to_z && gd;   // (workgroup-uniform; no gate image: drawn as without the gate)
    const float tf = sa.gate_tf, tb = sa.gate_tb;
    const int win_words = sa.win_rows * wpr;
    int n_raw = 0, n_front = 0, n_behind = 0;
    for (int js = r0; js <= r1; js += sa.win_rows) {
        const int je = min(r1, js + sa.win_rows - 1), n_words = (je - js + 1) * wpr;
        for (int i = tid; i < n_words; i += kSilhouetteThreads) {
            s_win[i] = 0u;
            if (gated) { s_win[win_words + i] = 0u; s_win[2 * win_words + i] = 0u; }
        }
        __syncthreads();
        const int j_lo = max(js, box0), j_hi = min(je, box1);
        if (j_lo <= j_hi) {
            ROFT_LDS uint32_t* const win = pin_lds(s_win);
            auto store = [=](int i, int j, float z) {   // (win, js, wpr, zb, W, obj; with the gate: gated, gd, tf, tb, win_words)
                const int wi = (j - js) * wpr + (i >> 5);
                const uint32_t bit = 1u << (i & 31);
                (void)__hip_atomic_fetch_or(win + wi, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (kZ && zb)
                    (void)__hip_atomic_fetch_min(zb + ((size_t)j * W + i), ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)obj,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (kGate && gated) {
                    const float D = gd[(size_t)j * W + i];
                    const float lo = z - tf, hi = z + tb;   // (each rounded once)
                    if (!(D > 0.0f && D < lo)) (void)__hip_atomic_fetch_or(win + (win_words + wi), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (tb > 0.0f && D > hi) (void)__hip_atomic_fetch_or(win + (2 * win_words + wi), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            };
            // (raster.h's draw_triangles, kept inline: through the shared loop the launch took 142.0 us for 138.0, docs/notebook.md)
            for (int k = tid; k < nt; k += kSilhouetteThreads) {
                const int32_t* tri = prm.tris + (size_t)3 * k;
                const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
                const int cull = cull_code(flips, k);
                float x0, y0, z0, x1, y1, z1, x2, y2, z2;
                fetch_triangle(s_v, cached, prm.verts, v0, v1, v2, project, x0, y0, z0, x1, y1, z1, x2, y2, z2);
                raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, W, H, j_lo, j_hi, cull, store);
            }
            __syncthreads();
        }
        // flush: the strip's words are consecutive in the planes (wpr words per row, rows js .. je)
        uint32_t* const nz = planes + (size_t)js * wpr;
        uint32_t* const ob = nz + sa.plane_words;
        for (int i = tid; i < n_words; i += kSilhouetteThreads) {
            uint32_t w = s_win[i];
            if (kGate && gated) {
                const uint32_t clear = s_win[win_words + i], behind = s_win[2 * win_words + i];
                n_raw += __popc(w);
                n_front += __popc(w & ~clear);
                n_behind += __popc(w & clear & behind);
                w &= clear & ~behind;
            }
            if (!to_z) { nz[i] = w; ob[i] = w; }
            count += __popc(w);
        }
        __syncthreads();   // the next strip clears the window
    }
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
    if (kGate && gated) {
        for (int off = 32; off > 0; off >>= 1) {
            n_raw += __shfl_xor(n_raw, off, 64);
            n_front += __shfl_xor(n_front, off, 64);
            n_behind += __shfl_xor(n_behind, off, 64);
        }
        SilhouettePair& pr = sa.zpairs[(size_t)blockIdx.z * sa.n_obj + obj];
        if ((tid & 63) == 0) {
            if (count) atomicAdd(&sa.mrec[(size_t)(t + 1) * sa.n_obj + obj].new_count, count);
            if (n_raw) atomicAdd(&pr.raw, n_raw);
            if (n_front) atomicAdd(&pr.front, n_front);
            if (n_behind) atomicAdd(&pr.behind, n_behind);
        }
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            if (atomicAdd(&pr.done, 1) == bands - 1) {
                __threadfence();
                gate_pair_done(sa, pr, atomicAdd(&pr.raw, 0), (size_t)blockIdx.z * sa.n_obj + obj);
                pr.raw = 0; pr.done = 0;
            }
        }
        return;
    }
    if (to_z) {
        // what the resolve needs of the pair: the rows anything was drawn in, and the plain silhouette's pixels (for the statistics)
        SilhouettePair& pr = sa.zpairs[(size_t)blockIdx.z * sa.n_obj + obj];
        if ((tid & 63) == 0 && count) atomicAdd(&pr.raw, count);
        if (band == 0 && tid == 0) { pr.box0 = box0; pr.box1 = box1; }
        return;
    }
    if ((tid & 63) == 0 && count) atomicAdd(&sa.mrec[(size_t)(t + 1) * sa.n_obj + obj].new_count, count);
}

// The resolve: same grid, behind the draw.  For its band and pair, a workgroup reads the z-buffer inside the pair's row box, sets
// the bit where the low word is its object id -- the object is the nearest surface there, the lower id on an exact tie -- and
// writes EVERY word of BOTH planes of slot slot0 + t, zeros included, and the population count to mrec[t + 1][obj].new_count:
// what the flush above does for a plain silhouette.  A wave takes 64 consecutive pixels -- two plane words, W is a multiple of 32
// and a band begins on a row -- as one ballot, four of them per round so that four loads are in flight.  The pair's last workgroup
// (a ticket) adds the pair to the statistics and leaves its record zeroed for the next batch of this parity.
// kGate: the wave reads the gate depth of the same 64 consecutive pixels next to the z-buffer entries, and keep(R, D) -- R the
// entry's high word -- is folded into the ballot; the resolve itself (who owns the pixel) is decided by the renders alone.
template <bool kGate>
__global__ __launch_bounds__(kSilhouetteThreads) void pose_resolve_kernel(SilhouetteArgs sa)
{
    __shared__ int s_count;
    __shared__ int s_gate[2];   // (kGate: pixels removed in front / behind)
    const int obj = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = (int)((sa.frames_packed >> (4 * blockIdx.z)) & 15u);
    const FrameCtrl& c = sa.ctrl[(size_t)t * sa.n_obj + obj];
    if (c.label_type != kMaskFromPose || c.label <= 0) return;   // (workgroup-uniform)
    const int W = sa.W, H = sa.H;
    SilhouettePair& pr = sa.zpairs[(size_t)blockIdx.z * sa.n_obj + obj];
    const unsigned long long* const zb = sa.zbuf + ((size_t)blockIdx.z * sa.n_zscenes + (c.label - 1)) * ((size_t)W * H);
    const int bands = (int)gridDim.x, band = (int)blockIdx.x;
    const int r0 = (int)(((long long)band * H) / bands), r1 = (int)(((long long)(band + 1) * H) / bands) - 1;
    const int p_begin = r0 * W, p_end = (r1 + 1) * W;   // (W * H < 2^24)
    const int box0 = min(pr.box0, H), box1 = min(pr.box1, H - 1);   // (nothing drawn: INT32_MAX, -1)
    const int b_begin = max(p_begin, box0 * W), b_end = min(p_end, (box1 + 1) * W);   // the box's pixels of this band
    uint32_t* const nz = sa.planes + (size_t)obj * sa.obj_stride + (size_t)(sa.slot0 + t) * 2 * sa.plane_words;
    uint32_t* const ob = nz + sa.plane_words;
    if (tid == 0) s_count = 0;
    if constexpr (kGate) { if (tid < 2) s_gate[tid] = 0; }
    __syncthreads();
    int count = 0, n_front = 0, n_behind = 0;
    const float* const gd = kGate ? c.gate_depth : nullptr;
    const float tf = sa.gate_tf, tb = sa.gate_tb;
    constexpr int kRound = 4;
    for (int p0 = p_begin + wave * (64 * kRound); p0 < p_end; p0 += kSilhouetteThreads * kRound) {
        unsigned long long v[kRound];
        float d[kRound];
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            const int p = p0 + 64 * u + lane;
            const bool in_box = p >= b_begin && p < b_end;
            v[u] = in_box ? zb[p] : ~0ull;
            if (kGate) d[u] = (in_box && gd) ? gd[p] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            const int p = p0 + 64 * u + lane;
            const bool own = (uint32_t)v[u] == (uint32_t)obj;   // (all-ones: nobody's)
            unsigned long long mine = __ballot(own), front = 0ull, behind = 0ull;
            if (kGate) {
                const float R = __uint_as_float((uint32_t)(v[u] >> 32)), D = d[u];
                const float lo = R - tf, hi = R + tb;   // (each rounded once)
                const bool f = own && D > 0.0f && D < lo;
                const bool b = own && !f && tb > 0.0f && D > hi;
                front = __ballot(f);
                behind = __ballot(b);
            }
            if ((lane & 31) == 0 && p < p_end) {
                uint32_t w = lane ? (uint32_t)(mine >> 32) : (uint32_t)mine;
                count += __popc(w);   // (the resolved mask's pixels)
                if (kGate) {
                    const uint32_t wf = lane ? (uint32_t)(front >> 32) : (uint32_t)front, wb = lane ? (uint32_t)(behind >> 32) : (uint32_t)behind;
                    n_front += __popc(wf);
                    n_behind += __popc(wb);
                    w &= ~(wf | wb);
                }
                nz[p >> 5] = w;
                ob[p >> 5] = w;
            }
        }
    }
    count += __shfl_xor(count, 32, 64);
    if (lane == 0 && count) atomicAdd(&s_count, count);
    if (kGate) {
        n_front += __shfl_xor(n_front, 32, 64);
        n_behind += __shfl_xor(n_behind, 32, 64);
        if (lane == 0 && n_front) atomicAdd(&s_gate[0], n_front);
        if (lane == 0 && n_behind) atomicAdd(&s_gate[1], n_behind);
    }
    __syncthreads();
    if (tid == 0) {
        const int n = s_count;
        if constexpr (kGate) {
            const int nf = s_gate[0], nb = s_gate[1];
            if (n - nf - nb) atomicAdd(&sa.mrec[(size_t)(t + 1) * sa.n_obj + obj].new_count, n - nf - nb);
            if (n) atomicAdd(&pr.kept, n);
            if (nf) atomicAdd(&pr.front, nf);
            if (nb) atomicAdd(&pr.behind, nb);
        } else if (n) {
            atomicAdd(&sa.mrec[(size_t)(t + 1) * sa.n_obj + obj].new_count, n);
            atomicAdd(&pr.kept, n);
        }
        __threadfence();
        if (atomicAdd(&pr.done, 1) == bands - 1) {
            __threadfence();
            const int raw = atomicAdd(&pr.raw, 0), kept = atomicAdd(&pr.kept, 0);
            if (raw > 0 && kept == 0) atomicAdd(&sa.zstats[0], 1ull);
            if (raw > kept) atomicAdd(&sa.zstats[1], (unsigned long long)(raw - kept));
            if (kGate) gate_pair_done(sa, pr, kept, (size_t)blockIdx.z * sa.n_obj + obj);
            pr.raw = 0; pr.kept = 0; pr.done = 0;
        }
    }
}

// LDS of a workgroup: the projected vertices of the largest mesh where the cache is on and they fit it, and the bit window of one
// strip -- the rows of a band, at most kSilhouetteWindowWords words.  A small mesh on a small image takes a few KB, so that several
// workgroups share a CU with the chains the launch runs next to.
// With a z-buffer (sa.zbuf: the batch has silhouettes to resolve) the stage is the clear of the z-buffers of its delivering frames
// to all-ones, the draw and the resolve: `start` opens the draw, `stop` ends the resolve.
int launch_pose_silhouette(SilhouetteArgs sa, int n_frames, int max_verts, int bands, int vertex_cache, hipStream_t s, hipEvent_t start,
                           hipEvent_t stop)
{
    if (sa.wpr <= 0 || sa.wpr > kSilhouetteWindowWords || sa.H <= 0 || n_frames <= 0 || sa.n_obj <= 0) return 0;
    if (bands <= 0) bands = (sa.H + 63) / 64;
    bands = std::min(bands, std::min(sa.H, 1024));
    const int band_rows = (sa.H + bands - 1) / bands;   // (the tallest band)
    // (the gate: three windows share the words -- the same launches, a third of the rows per strip)
    const int planes = sa.gate ? 3 : 1;
    if (sa.gate && (sa.wpr > kSilhouetteWindowWords / planes || !sa.zpairs || !sa.gstats)) return 0;
    sa.win_rows = std::max(1, std::min(band_rows, kSilhouetteWindowWords / planes / sa.wpr));
    sa.vcache_cap = (vertex_cache && max_verts <= kSilhouetteCacheVerts) ? std::max(max_verts, 0) : 0;
    const size_t vbytes = vertex_cache_bytes(sa.vcache_cap);
    const size_t lds = vbytes + 4 * (size_t)planes * sa.win_rows * sa.wpr;
    const dim3 grid(bands, sa.n_obj, n_frames);
    const auto draw = [&](auto kernel, hipEvent_t ev0, hipEvent_t ev1) {
        (void)set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)kRasterLdsBudget);
        hipExtLaunchKernelGGL(kernel, grid, dim3(kSilhouetteThreads), (uint32_t)lds, s, ev0, ev1, 0, sa);
    };
    if (!sa.zbuf) {
        if (sa.gate) draw(pose_silhouette_kernel<false, true>, start, stop);
        else draw(pose_silhouette_kernel<false, false>, start, stop);
        return 1;
    }
    if (sa.n_zscenes <= 0 || !sa.zpairs || !sa.zstats) return 0;
    (void)hipMemsetAsync(sa.zbuf, 0xFF, sizeof(unsigned long long) * (size_t)n_frames * sa.n_zscenes * sa.W * sa.H, s);
    if (sa.gate) {
        draw(pose_silhouette_kernel<true, true>, start, nullptr);
        hipExtLaunchKernelGGL(pose_resolve_kernel<true>, grid, dim3(kSilhouetteThreads), 0, s, nullptr, stop, 0, sa);
    } else {
        draw(pose_silhouette_kernel<true, false>, start, nullptr);
        hipExtLaunchKernelGGL(pose_resolve_kernel<false>, grid, dim3(kSilhouetteThreads), 0, s, nullptr, stop, 0, sa);
    }
    return 2;
}

}  // namespace roft
