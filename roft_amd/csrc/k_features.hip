// k_features.hip -- the buffered features of the outlier test: the rank-even pixels of an object's mask plane and their depths
// (gfx950).
//
// Reference:
//   ROFTFilter::buffer_outlier_rejection_features   src/roft-lib/src/ROFTFilter.cpp:624-646 (the scan: :556)
//
// The reference copies the whole depth frame and mask when a pose arrives and scans them six frames later (findNonZero, every
// second pixel).  Here the "features" are extracted once into a compact (pixel, depth) list indexed by rank/2, so the likelihood
// (outlier_fused_kernel, k_render.hip) is a dense reduction over ~N_mask/2 samples and the frame itself need not be retained.
// Nothing here is compared bit for bit with a float computation; the file is built with the flags of the others.
#include "plane_rank.h"

namespace roft {

constexpr int kFeatThreads = 1024;

// The reference buffers depth + mask when a pose arrives (ROFTFilter.cpp:313-322, :353) and tests the NEXT pose against
// them; here the buffered sets live in a small ring (FrameCtrl::feat_write / feat_read name the slots), so buffering
// is part of the mask chain of the frame and never waits for the pose chain that reads an older set.
// Feature slot s holds the pixel of row-major rank 2s of the current obj plane (`k += 2` over the
// findNonZero list, ROFTFilter.cpp:556) and its depth.  Plane words are in row-major order, so one block
// scan over the popcounts of contiguous word chunks gives every chunk its starting rank; the expansion of the
// words into (pixel, depth) slots is described at the loop below.
#ifdef ROFT_FEAT_PROFILE
#define FTICK(i) do { __syncthreads(); if (threadIdx.x == 0) { long long _t = wall_clock64(); a.state[obj].dbg[i] = _t - f_t0; f_t0 = _t; } } while (0)
#else
#define FTICK(i) do {} while (0)
#endif

// LDS = false: planes that do not fit the LDS (beyond ~1.1 Mpixel) are read from memory by both passes.
// grid: (n_obj, frames listed in `frames_packed`: four bits per frame index, the batch's frames that buffer features for some object)
template <bool LDS>
__global__ __launch_bounds__(kFeatThreads) void features_kernel(EngineArrays a, unsigned frames_packed)
{
    ROFT_RESIDENT(a, RK_FEATURES);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_wave[16];
    __shared__ int s_chunk[kFeatThreads];
    const int obj = blockIdx.x;
    const FrameCtrl& c = frame_ctrl(a, (int)((frames_packed >> (4 * blockIdx.y)) & 15u), obj);
#ifdef ROFT_FEAT_PROFILE
    long long f_t0 = wall_clock64();
#endif
    int feat_write = c.feat_write, slot_cur = c.slot_cur;
    const float* depth = c.depth_cur;
    asm volatile("" : "+v"(feat_write), "+v"(slot_cur), "+v"(depth));   // all three fetched before the first barrier
    if (feat_write < 0) return;
    const int W = a.cam.W, wpr = a.cam.wpr;
    const uint32_t* gplane = a.planes + plane_offset(a, obj, slot_cur, 1);
    uint32_t* s_stage = reinterpret_cast<uint32_t*>(smem);   // staged with coalesced 16-byte loads
    if (LDS) {
        const size_t n4 = a.plane_words / 4;
        for (size_t i = threadIdx.x; i < n4; i += blockDim.x)
            reinterpret_cast<uint4*>(s_stage)[i] = reinterpret_cast<const uint4*>(gplane)[i];
        for (size_t i = n4 * 4 + threadIdx.x; i < a.plane_words; i += blockDim.x) s_stage[i] = gplane[i];
        __syncthreads();
    }
    const uint32_t* s_plane = LDS ? s_stage : gplane;
    FTICK(0);
    uint32_t* fpix = a.feat_pix + ((size_t)obj * kFeatRing + feat_write) * a.feat_cap;
    float* fdep = a.feat_depth + ((size_t)obj * kFeatRing + feat_write) * a.feat_cap;
    const int n_words = (int)a.plane_words;
    const int per = (n_words + blockDim.x - 1) / blockDim.x;
    const int w0 = min(n_words, (int)threadIdx.x * per), w1 = min(n_words, w0 + per);
    int cnt = 0;
    for (int w = w0; w < w1; ++w) cnt += __popc(s_plane[w]);
    int total;
    s_chunk[threadIdx.x] = block_exclusive_scan(cnt, s_wave, &total);   // starting rank of the thread's chunk
    __syncthreads();
    FTICK(1);
    // Expansion with the words dealt out round-robin -- the dense words of the mask are neighbours, so a contiguous
    // split would leave the whole expansion to a few threads.  A word's starting rank = its chunk's + the popcounts
    // of the chunk's earlier words; the bits whose rank is even are kept (parity alternates along the set bits).
    for (int w = threadIdx.x; w < n_words; w += blockDim.x) {
        uint32_t bits = s_plane[w];
        if (!bits) continue;
        const int chunk = w / per;
        int r0 = s_chunk[chunk];
        for (int v = chunk * per; v < w; ++v) r0 += __popc(s_plane[v]);
        if (r0 & 1) bits &= bits - 1;                 // first set bit has an odd rank: skip it
        int slot = (r0 + 1) >> 1;
        const int row = w / wpr;
        const uint32_t pix0 = ((uint32_t)row << 16) | (uint32_t)((w - row * wpr) * 32);   // (v << 16 | u): no division by W downstream
        while (bits) {
            if (slot < a.feat_cap) fpix[slot] = pix0 + (uint32_t)__builtin_ctz(bits);
            ++slot;
            bits &= bits - 1;                         // the kept bit ...
            bits &= bits - 1;                         // ... and its odd-ranked successor (no-op on 0)
        }
    }
    __syncthreads();  // fpix is written and read by this workgroup only
    FTICK(2);
    // depth gathers, kBatch per thread in flight together (a loop that consumes each index right after loading it
    // pays two memory latencies per element)
    constexpr int kBatch = 16;
    const int n = min((total + 1) / 2, a.feat_cap);
    for (int sb = threadIdx.x; sb < n; sb += kBatch * blockDim.x) {
        uint32_t px[kBatch];
        float d[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int sl = sb + u * (int)blockDim.x;
            px[u] = (sl < n) ? fpix[sl] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) d[u] = depth[(size_t)(px[u] >> 16) * W + (px[u] & 0xFFFFu)];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int sl = sb + u * (int)blockDim.x;
            if (sl < n) fdep[sl] = d[u];
        }
    }
    FTICK(3);
    if (threadIdx.x == 0) a.state[obj].n_feat[feat_write] = n;
}

// feat_frames: bit t = some object buffers features in frame t of the batch (0: every frame -- the operator level).  Only those
// frames get workgroups (round 6: a 1024-thread workgroup with the plane's 38 KB of LDS needs a place on a CU even to find out
// that its frame has nothing to do, and five of a batch's six frames have not).
void launch_features(const EngineArrays& a, hipStream_t s, hipEvent_t stop, unsigned feat_frames)
{
    unsigned packed = 0;
    int n_frames = 0;
    for (int t = 0; t < a.T && t < 8; ++t)
        if (feat_frames == 0 || (feat_frames & (1u << t))) packed |= (unsigned)t << (4 * n_frames++);
    if (n_frames == 0) n_frames = 1;   // (a.T == 0 cannot happen; the launch carries the caller's stop event: never skipped)
    const size_t lds = (a.plane_words * 4 + 15) & ~(size_t)15;
    const size_t lds_cap = 160 * 1024 - 256 - kFeatThreads * sizeof(int) - 128;
    if (lds <= lds_cap) {
        (void)set_max_dynamic_lds(reinterpret_cast<const void*>(features_kernel<true>), (int)lds_cap);
        hipExtLaunchKernelGGL(features_kernel<true>, dim3(a.n_obj, n_frames), dim3(kFeatThreads), (uint32_t)lds, s, nullptr, stop, 0, a, packed);
    } else {
        hipExtLaunchKernelGGL(features_kernel<false>, dim3(a.n_obj, n_frames), dim3(kFeatThreads), 0, s, nullptr, stop, 0, a, packed);
    }
}

}  // namespace roft
