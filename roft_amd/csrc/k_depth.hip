// k_depth.hip -- raw sensor depth on the device (include/roft_engine.h section 3c): a Z16 frame -> the float depth image in metres
// the engine's kernels read.  CONVERT is one float multiply per reading.  ALIGN registers the frame of a depth camera of its own
// to the colour camera: every reading is deprojected at two corners of its pixel, transformed, projected, and written to the colour
// pixels whose centres lie in the half-open footprint, where the NEAREST reading (the smallest raw value: an integer minimum, so
// no order and no run changes a bit) wins.  The stage of the reference's capture tool that did this on the host:
// tools/rs-capture/src/main.cpp:23-67 (rs2::align, then convertTo(CV_32FC1, 0.001)).
//
// All arithmetic is float, in the operation order of the header, compiled without contraction (Makefile: -ffp-contract=off);
// tests/depth_ref.py restates it in numpy and the GPU tests ask for equal bits.
#include <cmath>
#include <string>

#include "device_owned.h"
#include "depth.h"

namespace roft {

using host::fail;

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes behind a 4-byte aligned address

// ---- convert: a streaming pass, eight readings (16 bytes) in, two 16-byte stores out -----------------------------------------
__global__ __launch_bounds__(256) void depth_convert_kernel(DepthJobs jobs, size_t npix, float scale)
{
    const uint16_t* __restrict__ src = jobs.raw[blockIdx.y];
    float* __restrict__ dst = jobs.out[blockIdx.y];
    const size_t n8 = npix / 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const u32x4_a4 v = *reinterpret_cast<const u32x4_a4*>(src + 8 * i);
        float4 a, b;
        a.x = (float)(v.x & 0xffffu) * scale; a.y = (float)(v.x >> 16) * scale;
        a.z = (float)(v.y & 0xffffu) * scale; a.w = (float)(v.y >> 16) * scale;
        b.x = (float)(v.z & 0xffffu) * scale; b.y = (float)(v.z >> 16) * scale;
        b.z = (float)(v.w & 0xffffu) * scale; b.w = (float)(v.w >> 16) * scale;
        reinterpret_cast<float4*>(dst)[2 * i] = a;
        reinterpret_cast<float4*>(dst)[2 * i + 1] = b;
    }
    // the tail (npix % 8 readings), one reading per thread: nothing is read past the image
    const size_t tail = 8 * n8 + threadIdx.x;
    if (blockIdx.x == 0 && tail < npix) dst[tail] = (float)src[tail] * scale;
}

// ---- align, phase 1: every key = "no reading" ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_clear_kernel(DepthJobs jobs, size_t npix)
{
    unsigned* __restrict__ key = reinterpret_cast<unsigned*>(jobs.out[blockIdx.y]);
    const size_t n4 = npix / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        reinterpret_cast<uint4*>(key)[i] = make_uint4(kDepthNoKey, kDepthNoKey, kDepthNoKey, kDepthNoKey);
    const size_t tail = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4 && tail < npix) key[tail] = kDepthNoKey;
}

// ---- align, phase 2: one thread per depth pixel, lanes along x (a wave's atomics land on neighbouring words) ---------------
// blockIdx.x walks the 64 x 4 pixel tiles of the depth image row by row, blockIdx.y the images.
__global__ __launch_bounds__(256) void depth_scatter_kernel(DepthJobs jobs, DepthAlignGeom g, int tiles_x)
{
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * 64 + (int)(threadIdx.x & 63);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * 4 + (int)(threadIdx.x >> 6);
    if (x >= g.Wd || y >= g.Hd) return;
    const unsigned d = jobs.raw[blockIdx.y][(size_t)y * g.Wd + x];
    if (d == 0) return;   // no reading
    const float z = (float)d * g.scale;
    float u[2], v[2];
    for (int c = 0; c < 2; ++c) {
        const float s = c ? 0.5f : -0.5f;
        const float px = (float)x + s, py = (float)y + s;
        const float X = ((px - g.cxd) / g.fxd) * z, Y = ((py - g.cyd) / g.fyd) * z;
        const float P0 = ((g.R[0] * X + g.R[1] * Y) + g.R[2] * z) + g.t[0];
        const float P1 = ((g.R[3] * X + g.R[4] * Y) + g.R[5] * z) + g.t[1];
        const float P2 = ((g.R[6] * X + g.R[7] * Y) + g.R[8] * z) + g.t[2];
        if (!(P2 > 0.0f)) return;   // behind the colour camera
        u[c] = (P0 / P2) * g.fxc + g.cxc;
        v[c] = (P1 / P2) * g.fyc + g.cyc;
    }
    if (!(__builtin_isfinite(u[0]) && __builtin_isfinite(v[0]) && __builtin_isfinite(u[1]) && __builtin_isfinite(v[1]))) return;
    // the colour pixels whose CENTRES lie in [u0, u1) x [v0, v1), clipped to the image -- in float: a footprint far outside the
    // image is an empty range before anything is converted to an integer
    const float x0 = fmaxf(ceilf(u[0]), 0.0f), x1 = fminf(ceilf(u[1]) - 1.0f, (float)(g.Wc - 1));
    const float y0 = fmaxf(ceilf(v[0]), 0.0f), y1 = fminf(ceilf(v[1]) - 1.0f, (float)(g.Hc - 1));
    if (x1 < x0 || y1 < y0) return;
    if (x1 - x0 >= (float)ROFT_DEPTH_ALIGN_MAX_SPAN || y1 - y0 >= (float)ROFT_DEPTH_ALIGN_MAX_SPAN) return;
    // here 0 <= x0 <= x1 <= Wc - 1 and 0 <= y0 <= y1 <= Hc - 1: every key below is inside the image
    const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
    unsigned* key = reinterpret_cast<unsigned*>(jobs.out[blockIdx.y]);
    for (int yy = iy0; yy <= iy1; ++yy)
        for (int xx = ix0; xx <= ix1; ++xx)
            (void)__hip_atomic_fetch_min(key + (size_t)yy * g.Wc + xx, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- align, phase 3: the keys -> metres, in place ----------------------------------------------------------------------------
__device__ __forceinline__ float depth_of_key(unsigned k, float scale) { return k == kDepthNoKey ? 0.0f : (float)k * scale; }

__global__ __launch_bounds__(256) void depth_resolve_kernel(DepthJobs jobs, size_t npix, float scale)
{
    float* out = jobs.out[blockIdx.y];
    const size_t n4 = npix / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 k = reinterpret_cast<const uint4*>(out)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(depth_of_key(k.x, scale), depth_of_key(k.y, scale), depth_of_key(k.z, scale), depth_of_key(k.w, scale));
    }
    const size_t tail = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4 && tail < npix) out[tail] = depth_of_key(reinterpret_cast<const unsigned*>(out)[tail], scale);
}

static unsigned stream_blocks(size_t units) { return (unsigned)std::max<size_t>(1, std::min<size_t>(4096, (units + 255) / 256)); }

void launch_depth_convert(const DepthJobs& jobs, size_t npix, float scale, hipStream_t s)
{
    hipLaunchKernelGGL(depth_convert_kernel, dim3(stream_blocks(npix / 8), (unsigned)jobs.n), dim3(256), 0, s, jobs, npix, scale);
}

void launch_depth_align(const DepthJobs& jobs, const DepthAlignGeom& g, hipStream_t s)
{
    const size_t npix = (size_t)g.Wc * g.Hc;
    const int tiles_x = (g.Wd + 63) / 64, tiles_y = (g.Hd + 3) / 4;   // (Wd * Hd < 2^24: at most 2^22 + 2^18 tiles)
    hipLaunchKernelGGL(depth_clear_kernel, dim3(stream_blocks(npix / 4), (unsigned)jobs.n), dim3(256), 0, s, jobs, npix);
    hipLaunchKernelGGL(depth_scatter_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)jobs.n), dim3(256), 0, s, jobs, g, tiles_x);
    hipLaunchKernelGGL(depth_resolve_kernel, dim3(stream_blocks(npix / 4), (unsigned)jobs.n), dim3(256), 0, s, jobs, npix, g.scale);
}

// ---- host-side checks (before a device is looked for) -------------------------------------------------------------------------
int depth_check_scale(float scale)
{
    if (!std::isfinite(scale) || !(scale > 0.0f)) return fail(ROFT_ERR_INVALID, "the depth scale (metres per unit) must be finite and > 0");
    return ROFT_OK;
}

int depth_check_camera(const roft_camera& cam, const char* which)
{
    const std::string w(which);
    if (cam.width < 1 || cam.height < 1) return fail(ROFT_ERR_INVALID, "the " + w + " camera's width and height must be at least 1");
    if ((size_t)cam.width * (size_t)cam.height >= ((size_t)1 << 24))
        return fail(ROFT_ERR_INVALID, "the " + w + " camera's width * height must be < 2^24");
    if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !(cam.fx > 0.0) || !(cam.fy > 0.0))
        return fail(ROFT_ERR_INVALID, "the " + w + " camera's focal lengths must be finite and > 0");
    if (!std::isfinite(cam.cx) || !std::isfinite(cam.cy)) return fail(ROFT_ERR_INVALID, "the " + w + " camera's principal point must be finite");
    return ROFT_OK;
}

int depth_check_transform(const roft_depth_source& src)
{
    for (float r : src.R) if (!std::isfinite(r)) return fail(ROFT_ERR_INVALID, "the depth source's R must be finite");
    for (float t : src.t) if (!std::isfinite(t)) return fail(ROFT_ERR_INVALID, "the depth source's t must be finite");
    return ROFT_OK;
}

void depth_align_geometry(DepthAlignGeom& g, const roft_depth_source& src, const roft_camera& colour)
{
    g.Wd = src.cam.width; g.Hd = src.cam.height; g.Wc = colour.width; g.Hc = colour.height;
    g.fxd = (float)src.cam.fx; g.fyd = (float)src.cam.fy; g.cxd = (float)src.cam.cx; g.cyd = (float)src.cam.cy;
    g.fxc = (float)colour.fx; g.fyc = (float)colour.fy; g.cxc = (float)colour.cx; g.cyc = (float)colour.cy;
    for (int i = 0; i < 9; ++i) g.R[i] = src.R[i];
    for (int i = 0; i < 3; ++i) g.t[i] = src.t[i];
    g.scale = src.scale;
}

}  // namespace roft

// ---- the stand-alone operators: HOST buffers, device 0 -------------------------------------------------------------------------
namespace {

using namespace roft::host;

// the one job of a round trip (device_owned.h, host_round_trip): the raw frame that went up, the product's place
roft::DepthJobs one_job(const DevBuf<unsigned char>* in, void* out)
{
    roft::DepthJobs jobs{};
    jobs.n = 1; jobs.raw[0] = reinterpret_cast<const uint16_t*>(in[0].p); jobs.out[0] = static_cast<float*>(out);
    return jobs;
}

}  // namespace

extern "C" {

int roft_depth_convert(const uint16_t* raw, int W, int H, float scale, float* out)
{
    if (!raw || !out) return fail(ROFT_ERR_INVALID, "null argument");
    if (W < 1 || H < 1) return fail(ROFT_ERR_INVALID, "width and height must be at least 1");
    if (int rc = roft::depth_check_scale(scale)) return rc;
    TRY(require_device(0, "no HIP device (the depth conversion has no CPU path)"));
    const size_t npix = (size_t)W * H;
    return host_round_trip({{raw, npix * sizeof(uint16_t)}}, out, npix * sizeof(float), [&](const DevBuf<unsigned char>* in, void* d_out) -> int {
        roft::launch_depth_convert(one_job(in, d_out), npix, scale, nullptr);
        return ROFT_OK;
    });
}

int roft_depth_align(const uint16_t* raw, const roft_depth_source* src, const roft_camera* colour, float* out)
{
    if (!raw || !src || !colour || !out) return fail(ROFT_ERR_INVALID, "null argument");
    if (src->type != ROFT_DEPTH_Z16) return fail(ROFT_ERR_INVALID, "the depth source's type must be ROFT_DEPTH_Z16");
    if (int rc = roft::depth_check_scale(src->scale)) return rc;
    if (int rc = roft::depth_check_camera(src->cam, "depth")) return rc;
    if (int rc = roft::depth_check_camera(*colour, "colour")) return rc;
    if (int rc = roft::depth_check_transform(*src)) return rc;
    TRY(require_device(0, "no HIP device (the depth alignment has no CPU path)"));
    roft::DepthAlignGeom g{};
    roft::depth_align_geometry(g, *src, *colour);
    return host_round_trip({{raw, (size_t)g.Wd * g.Hd * sizeof(uint16_t)}}, out, (size_t)g.Wc * g.Hc * sizeof(float),
                           [&](const DevBuf<unsigned char>* in, void* d_out) -> int {
                               roft::launch_depth_align(one_job(in, d_out), g, nullptr);
                               return ROFT_OK;
                           });
}

}  // extern "C"
