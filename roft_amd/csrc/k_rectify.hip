// k_rectify.hip -- lens distortion on the device (include/roft_engine.h section 3g): the sensor's distorted frames -> the images of
// the pinhole camera the engine's kernels read.  One kernel serves a chunk of jobs that share one lens: a thread owns four
// consecutive output pixels of a row (lanes run along x, so a smooth map sends neighbouring lanes to neighbouring source addresses
// and a store is a whole word: 4 B for 8-bit products, 8 B for 16-bit, 16 B for float), evaluates the Brown-Conrady map for them
// ONCE -- recomputed, not stored: ~25 float operations per pixel against 8 bytes of map traffic per pixel and job -- and gathers
// its jobs of the chunk through it (all of them, or its slice of them where the image is small: launch_rectify): NEAREST for depth, masks and label images, BILINEAR for 8-bit images, with the colour-to-gray
// conversion of a camera image fused into the four taps.
//
// All arithmetic is float, in the operation order of the header, compiled without contraction (Makefile: -ffp-contract=off);
// tests/rectify_ref.py restates it in numpy and the GPU tests ask for equal bits.
#include <algorithm>
#include <cmath>
#include <string>

#include "device_owned.h"
#include "rectify.h"

namespace roft {

using host::fail;

// what one output pixel reads: the nearest source pixel (-1: outside, or the map is not finite there) and the four bilinear taps
// (finite false: the output is 0).  Every index is inside the source image: `near` by the contract's float test, the taps by their clamp.
struct RectPixel {
    int near;
    int i00, i01, i10, i11;
    float ax, ay;
    bool finite;
};

__device__ __forceinline__ void rect_map(const RectGeom& g, float x, float y, float yy, float& sx, float& sy)
{
    const float xx = x * x, xy = x * y, r2 = xx + yy;
    const float rad = 1.0f + r2 * (g.k1 + r2 * (g.k2 + r2 * g.k3));
    const float tx = g.two_p1 * xy + g.p2 * (r2 + 2.0f * xx);
    const float ty = g.p1 * (r2 + 2.0f * yy) + g.two_p2 * xy;
    const float xd = x * rad + tx, yd = y * rad + ty;
    sx = xd * g.fxs + g.cxs;
    sy = yd * g.fys + g.cys;
}

__device__ __forceinline__ RectPixel rect_pixel(const RectGeom& g, float sx, float sy)
{
    RectPixel p;
    const float wmax = (float)(g.Ws - 1), hmax = (float)(g.Hs - 1);
    const float jx = floorf(sx + 0.5f), jy = floorf(sy + 0.5f);
    const bool inside = jx >= 0.0f && jx <= wmax && jy >= 0.0f && jy <= hmax;   // (false for anything not finite)
    p.near = inside ? (int)jy * g.Ws + (int)jx : -1;
    p.finite = __builtin_isfinite(sx) && __builtin_isfinite(sy);
    p.i00 = p.i01 = p.i10 = p.i11 = 0;
    p.ax = p.ay = 0.0f;
    if (p.finite) {
        const float x0 = floorf(sx), y0 = floorf(sy);
        p.ax = sx - x0;
        p.ay = sy - y0;
        const int c0 = (int)fminf(fmaxf(x0, 0.0f), wmax), c1 = (int)fminf(fmaxf(x0 + 1.0f, 0.0f), wmax);
        const int r0 = (int)fminf(fmaxf(y0, 0.0f), hmax), r1 = (int)fminf(fmaxf(y0 + 1.0f, 0.0f), hmax);
        p.i00 = r0 * g.Ws + c0; p.i01 = r0 * g.Ws + c1;
        p.i10 = r1 * g.Ws + c0; p.i11 = r1 * g.Ws + c1;
    }
    return p;
}

__device__ __forceinline__ unsigned rect_blend(const RectPixel& p, float p00, float p01, float p10, float p11)
{
    const float top = (1.0f - p.ax) * p00 + p.ax * p01;
    const float bot = (1.0f - p.ax) * p10 + p.ax * p11;
    const float val = (1.0f - p.ay) * top + p.ay * bot;
    return (unsigned)fminf(rintf(val), 255.0f);
}

// OpenCV's 8-bit COLOR_BGR2GRAY of source pixel i (k_opticalflow.hip, of_gray); `rgb`: the first channel is red
__device__ __forceinline__ float rect_gray_tap(const uint8_t* __restrict__ src, int i, bool rgb)
{
    const unsigned c0 = src[3 * i], c1 = src[3 * i + 1], c2 = src[3 * i + 2];
    const unsigned r = rgb ? c0 : c2, b = rgb ? c2 : c0;
    return (float)((r * 4899u + c1 * 9617u + b * 1868u + 8192u) >> 14);
}

// the product pixel of one job: bilinear kinds return the byte, nearest kinds the element's bits
__device__ __forceinline__ unsigned rect_gray8(const uint8_t* __restrict__ s, const RectPixel& p)
{
    return p.finite ? rect_blend(p, (float)s[p.i00], (float)s[p.i01], (float)s[p.i10], (float)s[p.i11]) : 0u;
}
__device__ __forceinline__ unsigned rect_channel(const uint8_t* __restrict__ s, const RectPixel& p, int c)
{
    return p.finite ? rect_blend(p, (float)s[3 * p.i00 + c], (float)s[3 * p.i01 + c], (float)s[3 * p.i10 + c], (float)s[3 * p.i11 + c]) : 0u;
}
__device__ __forceinline__ unsigned rect_gray_of(const uint8_t* __restrict__ s, const RectPixel& p, bool rgb)
{
    return p.finite ? rect_blend(p, rect_gray_tap(s, p.i00, rgb), rect_gray_tap(s, p.i01, rgb), rect_gray_tap(s, p.i10, rgb), rect_gray_tap(s, p.i11, rgb)) : 0u;
}

// Thread q owns pixels 4 (q % quads) .. + 3 of row q / quads (quads = ceil(W / 4)): lanes run along x and on into the next row.
// With W a multiple of 4 every thread's four pixels exist and start on a whole word of every product; otherwise (the stand-alone
// operators at odd sizes) the existing ones are stored one by one.
// blockIdx.y deals the chunk's jobs out, per_thread to a thread: a thread's jobs are gathers that wait for memory one after the other,
// so a launch with few pixels per job spreads its jobs over more workgroups (launch_rectify) and recomputes the map in each.
__global__ __launch_bounds__(256) void rectify_kernel(RectJobs jobs, RectGeom g, int quads, int total, int per_thread)
{
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= total) return;
    const int v = q / quads, u0 = (q - v * quads) * 4;
    const bool words = (g.W & 3) == 0;
    const float y = ((float)v - g.cy) / g.fy, yy = y * y;
    RectPixel px[4];
    bool live[4];
    for (int k = 0; k < 4; ++k) {
        live[k] = u0 + k < g.W;
        float sx, sy;
        rect_map(g, ((float)(u0 + k) - g.cx) / g.fx, y, yy, sx, sy);
        px[k] = rect_pixel(g, sx, sy);
    }
    const size_t o = (size_t)v * g.W + u0;   // the first of the thread's pixels in a product
    const int j0 = (int)blockIdx.y * per_thread, j1 = min(jobs.n, j0 + per_thread);
    for (int j = j0; j < j1; ++j) {
        const int kind = jobs.kind[j];
        if (kind == ROFT_RECTIFY_F32) {
            const float* __restrict__ s = static_cast<const float*>(jobs.src[j]);
            float* d = static_cast<float*>(jobs.dst[j]);
            float r[4];
            for (int k = 0; k < 4; ++k) r[k] = (live[k] && px[k].near >= 0) ? s[px[k].near] : 0.0f;
            if (words) *reinterpret_cast<float4*>(d + o) = make_float4(r[0], r[1], r[2], r[3]);
            else for (int k = 0; k < 4; ++k) if (live[k]) d[o + k] = r[k];
        } else if (kind == ROFT_RECTIFY_U16) {
            const uint16_t* __restrict__ s = static_cast<const uint16_t*>(jobs.src[j]);
            uint16_t* d = static_cast<uint16_t*>(jobs.dst[j]);
            unsigned r[4];
            for (int k = 0; k < 4; ++k) r[k] = (live[k] && px[k].near >= 0) ? s[px[k].near] : 0u;
            if (words) *reinterpret_cast<uint2*>(d + o) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
            else for (int k = 0; k < 4; ++k) if (live[k]) d[o + k] = (uint16_t)r[k];
        } else if (kind == ROFT_RECTIFY_RGB8) {
            const uint8_t* __restrict__ s = static_cast<const uint8_t*>(jobs.src[j]);
            uint8_t* d = static_cast<uint8_t*>(jobs.dst[j]);
            unsigned r[12];
            for (int k = 0; k < 4; ++k)
                for (int c = 0; c < 3; ++c) r[3 * k + c] = live[k] ? rect_channel(s, px[k], c) : 0u;
            if (words) {   // (4 pixels = 12 bytes = three whole words: 3 o is a multiple of 4)
                unsigned* dw = reinterpret_cast<unsigned*>(d + 3 * o);
                for (int w = 0; w < 3; ++w) dw[w] = r[4 * w] | (r[4 * w + 1] << 8) | (r[4 * w + 2] << 16) | (r[4 * w + 3] << 24);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (live[k]) for (int c = 0; c < 3; ++c) d[3 * (o + k) + c] = (uint8_t)r[3 * k + c];
            }
        } else {   // one byte per pixel: ROFT_RECTIFY_GRAY8, ROFT_RECTIFY_U8, the gray of a colour image
            const uint8_t* __restrict__ s = static_cast<const uint8_t*>(jobs.src[j]);
            uint8_t* d = static_cast<uint8_t*>(jobs.dst[j]);
            unsigned r[4];
            for (int k = 0; k < 4; ++k) {
                if (!live[k]) r[k] = 0u;
                else if (kind == ROFT_RECTIFY_U8) r[k] = px[k].near >= 0 ? s[px[k].near] : 0u;
                else if (kind == ROFT_RECTIFY_GRAY8) r[k] = rect_gray8(s, px[k]);
                else r[k] = rect_gray_of(s, px[k], kind == kRectGrayOfRgb8);
            }
            if (words) *reinterpret_cast<unsigned*>(d + o) = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
            else for (int k = 0; k < 4; ++k) if (live[k]) d[o + k] = (uint8_t)r[k];
        }
    }
}

// the map itself (roft_rectify_map): one thread per pixel, (sx, sy) as one 8-byte store
__global__ __launch_bounds__(256) void rectify_map_kernel(RectGeom g, float2* __restrict__ map, int total)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= total) return;
    const int v = i / g.W, u = i - v * g.W;
    const float y = ((float)v - g.cy) / g.fy;
    float sx, sy;
    rect_map(g, ((float)u - g.cx) / g.fx, y, y * y, sx, sy);
    map[i] = make_float2(sx, sy);
}

void launch_rectify(const RectJobs& jobs, const RectGeom& g, hipStream_t s)
{
    const int quads = (g.W + 3) / 4, total = quads * g.H;   // (W * H < 2^24)
    const int blocks = (total + 255) / 256;
    // enough workgroups to fill the device: the jobs are dealt to as many slices as that takes, the rest share a thread's map
    const int slices = std::max(1, std::min(jobs.n, (kRectTargetBlocks + blocks - 1) / blocks));
    const int per_thread = (jobs.n + slices - 1) / slices;
    hipLaunchKernelGGL(rectify_kernel, dim3((unsigned)blocks, (unsigned)((jobs.n + per_thread - 1) / per_thread)), dim3(256), 0, s, jobs, g, quads, total, per_thread);
}

void launch_rectify_map(const RectGeom& g, float* map_out, hipStream_t s)
{
    const int total = g.W * g.H;
    hipLaunchKernelGGL(rectify_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, reinterpret_cast<float2*>(map_out), total);
}

// ---- host-side checks (before a device is looked for) -------------------------------------------------------------------------
int rect_check_camera(const roft_camera& cam, const char* which)
{
    const std::string w(which);
    if (cam.width < 1 || cam.height < 1) return fail(ROFT_ERR_INVALID, "the " + w + " camera's width and height must be at least 1");
    if ((size_t)cam.width * (size_t)cam.height >= ((size_t)1 << 24))
        return fail(ROFT_ERR_INVALID, "the " + w + " camera's width * height must be < 2^24");
    if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !std::isfinite(cam.cx) || !std::isfinite(cam.cy))
        return fail(ROFT_ERR_INVALID, "the " + w + " camera's intrinsics must be finite");
    if (!(cam.fx > 0.0) || !(cam.fy > 0.0)) return fail(ROFT_ERR_INVALID, "the " + w + " camera's focal lengths must be > 0");
    // (the kernel works in float: an intrinsic that is finite as a double only would not be)
    if (!std::isfinite((float)cam.fx) || !std::isfinite((float)cam.fy) || !std::isfinite((float)cam.cx) || !std::isfinite((float)cam.cy) ||
        !((float)cam.fx > 0.0f) || !((float)cam.fy > 0.0f))
        return fail(ROFT_ERR_INVALID, "the " + w + " camera's intrinsics must be finite, and its focal lengths > 0, as floats");
    return ROFT_OK;
}

int rect_check_lens(const roft_lens& lens)
{
    if (int rc = rect_check_camera(lens.cam, "source")) return rc;
    const double k[5] = {lens.k1, lens.k2, lens.p1, lens.p2, lens.k3};
    static const char* const name[5] = {"k1", "k2", "p1", "p2", "k3"};
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(k[i]) || !std::isfinite((float)k[i]))
            return fail(ROFT_ERR_INVALID, std::string("the lens coefficient ") + name[i] + " must be finite (as a float)");
    return ROFT_OK;
}

void rect_geometry(RectGeom& g, const roft_lens& lens, const roft_camera& target)
{
    g.W = target.width; g.H = target.height; g.Ws = lens.cam.width; g.Hs = lens.cam.height;
    g.fx = (float)target.fx; g.fy = (float)target.fy; g.cx = (float)target.cx; g.cy = (float)target.cy;
    g.fxs = (float)lens.cam.fx; g.fys = (float)lens.cam.fy; g.cxs = (float)lens.cam.cx; g.cys = (float)lens.cam.cy;
    g.k1 = (float)lens.k1; g.k2 = (float)lens.k2; g.k3 = (float)lens.k3; g.p1 = (float)lens.p1; g.p2 = (float)lens.p2;
    g.two_p1 = 2.0f * g.p1; g.two_p2 = 2.0f * g.p2;
}

}  // namespace roft

// ---- the stand-alone operators: HOST buffers, device 0 -------------------------------------------------------------------------
using namespace roft::host;

extern "C" {

int roft_default_lens(roft_lens* lens, const roft_camera* target)
{
    if (!lens || !target) return fail(ROFT_ERR_INVALID, "null argument");
    lens->cam = *target;
    lens->k1 = lens->k2 = lens->p1 = lens->p2 = lens->k3 = 0.0;
    return ROFT_OK;
}

int roft_rectify_map(const roft_lens* lens, const roft_camera* target, float* map_out)
{
    if (!lens || !target || !map_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (int rc = roft::rect_check_lens(*lens)) return rc;
    if (int rc = roft::rect_check_camera(*target, "target")) return rc;
    TRY(require_device(0, "no HIP device (the rectification has no CPU path)"));
    roft::RectGeom g{};
    roft::rect_geometry(g, *lens, *target);
    const size_t bytes = (size_t)g.W * g.H * 2 * sizeof(float);
    DevBuf<unsigned char> d_out;
    HIP_TRY(d_out.ensure(bytes));
    roft::launch_rectify_map(g, reinterpret_cast<float*>(d_out.p), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(map_out, d_out.p, bytes, hipMemcpyDeviceToHost));
    return ROFT_OK;
}

int roft_rectify(const void* src, int kind, const roft_lens* lens, const roft_camera* target, void* out)
{
    if (!src || !lens || !target || !out) return fail(ROFT_ERR_INVALID, "null argument");
    if (kind < ROFT_RECTIFY_GRAY8 || kind > ROFT_RECTIFY_F32) return fail(ROFT_ERR_INVALID, "unknown kind: one of ROFT_RECTIFY_GRAY8, _RGB8, _U8, _U16, _F32");
    if (int rc = roft::rect_check_lens(*lens)) return rc;
    if (int rc = roft::rect_check_camera(*target, "target")) return rc;
    TRY(require_device(0, "no HIP device (the rectification has no CPU path)"));
    roft::RectGeom g{};
    roft::rect_geometry(g, *lens, *target);
    return host_round_trip({{src, (size_t)g.Ws * g.Hs * roft::rect_src_pixel_bytes(kind)}}, out, (size_t)g.W * g.H * roft::rect_dst_pixel_bytes(kind),
                           [&](const DevBuf<unsigned char>* in, void* d_out) -> int {
                               roft::RectJobs jobs{};
                               jobs.n = 1; jobs.src[0] = in[0].p; jobs.dst[0] = d_out; jobs.kind[0] = (unsigned char)kind;
                               roft::launch_rectify(jobs, g, nullptr);
                               return ROFT_OK;
                           });
}

}  // extern "C"
