// k_opticalflow.hip -- dense optical-flow PRODUCER: pyramidal Lucas-Kanade on gfx950.
//
// The reference gets its flow frames from NVIDIA's fixed-function optical-flow engine
// (src/roft-lib/src/ImageOpticalFlowNVOF.cpp:100-159, tools/nvof/dumper/src/main.cpp:40-146); MI355X has no such
// unit, so the flow that feeds the filter is computed here.  The contract kept from the reference is the product:
// forward flow of frame k-1 pixels towards frame k as CV_32FC2 at grid 1 (NVOF 2.0 shape) or CV_16SC2 S10.5 at
// grid 4 (NVOF 1.0 shape, ImageOpticalFlowNVOF.cpp:19-80).  The algorithm is specified in oracle/ro_opticalflow.c
// (edge-extended images, central-difference gradients of the previous frame, (2r+1)^2 window, coarse-to-fine with
// nearest-neighbour x2 initialisation) and this file follows it tap for tap.
//
// MI355X mapping: one workgroup = a 32 x 8 pixel tile of one pyramid level of one image pair; the previous image
// tile with an (r + 1)-pixel halo and its gradient tile (Ix, Iy interleaved) are staged in LDS once and serve the G-matrix and the
// residual taps of all 256 pixels; only the pixels of the current image under the warped window (whose position
// depends on the evolving flow) go to the vector cache.  Batched over image pairs in blockIdx.z.
//
// Two stages (opticalflow.h): the pyramid of an IMAGE -- level 0 from the 8-bit image, gray or colour, and the means below it -- is
// built once, by of_convert_kernel / of_down_kernel; the Lucas-Kanade levels of a PAIR read two pyramids by pointer.  In a camera
// stream every image is the `cur` of one pair and the `prev` of the next: its pyramid serves both.
#include <algorithm>

#include "opticalflow.h"
#include "roft_device.h"

namespace roft {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// OpenCV's 8-bit COLOR_BGR2GRAY (fixed point, 14 fractional bits); `type` says which of c0, c2 is red
__device__ __forceinline__ unsigned of_gray(unsigned c0, unsigned c1, unsigned c2, int type)
{
    const unsigned r = type == kOfBgr8 ? c2 : c0, b = type == kOfBgr8 ? c0 : c2;
    return (r * 4899u + c1 * 9617u + b * 1868u + 8192u) >> 14;
}

// level 0 of one image's pyramid: u8 -> float, four pixels per thread.  A colour image is converted on the way (twelve bytes in
// three aligned words): the integer gray value is what a separate conversion pass would have stored as a byte.
__global__ __launch_bounds__(256) void of_convert_kernel(OfGeom a, OfImages im)
{
    const int img = blockIdx.y, type = im.type[img];
    float4* dst = reinterpret_cast<float4*>(im.pyr[img]);
    const int n4 = a.lv[0].w * a.lv[0].h / 4;
    if (type == kOfGray8) {
        const uchar4* src = reinterpret_cast<const uchar4*>(im.src[img]);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
            const uchar4 v = src[i];
            dst[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
        }
    } else {
        const unsigned* src = reinterpret_cast<const unsigned*>(im.src[img]);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
            const unsigned w0 = src[3 * (size_t)i], w1 = src[3 * (size_t)i + 1], w2 = src[3 * (size_t)i + 2];
            dst[i] = make_float4((float)of_gray(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, type),
                                 (float)of_gray(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, type),
                                 (float)of_gray((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, type),
                                 (float)of_gray((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, type));
        }
    }
}

__global__ __launch_bounds__(256) void of_down_kernel(OfGeom a, OfImages im, int l)
{
    float* base = im.pyr[blockIdx.y];
    const float* src = base + a.lv[l - 1].off;
    float* dst = base + a.lv[l].off;
    const int w = a.lv[l].w, h = a.lv[l].h, ws = a.lv[l - 1].w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        const size_t i0 = (size_t)(2 * y) * ws + 2 * x, i1 = i0 + ws;
        dst[i] = 0.25f * (((src[i0] + src[i0 + 1]) + src[i1]) + src[i1 + 1]);
    }
}

// the stand-alone colour conversion: one pixel per thread, any size
__global__ __launch_bounds__(256) void image_to_gray_kernel(const uint8_t* __restrict__ src, int type, size_t npix, uint8_t* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    dst[i] = type == kOfGray8 ? src[i] : (uint8_t)of_gray(src[3 * i], src[3 * i + 1], src[3 * i + 2], type);
}

__device__ __forceinline__ float at_g(const float* I, int w, int h, int x, int y)
{
    return I[(size_t)clampi(y, 0, h - 1) * w + clampi(x, 0, w - 1)];
}

constexpr int kOfTx = 32, kOfTy = 8;

// One pyramid level.  RT = compile-time window radius (1..4), or 0 for the generic runtime-radius version.
// LDS: the previous-image tile with an (r + 1) halo, and from it the gradient tiles Ix, Iy with an r halo, so that a
// tap costs three LDS reads.  The current image is warped with ONE pair of bilinear weights per pixel and iteration
// (the displacement is constant over the window): the (2r+2)^2 pixels under the window are loaded once, combined
// row by row (horizontal pass in registers, vertical pass against the previous row) -- 64 cached loads per iteration
// at r = 3 instead of 4 per tap.
template <int RT>
__global__ __launch_bounds__(kOfTx * kOfTy) void of_lk_kernel(OfGeom a, OfPairs pr, int l)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int r = RT ? RT : a.radius, R = r + 1;
    const int tw = kOfTx + 2 * R, th = kOfTy + 2 * R;      // I0 tile
    const int gw = kOfTx + 2 * r, gh = kOfTy + 2 * r;      // gradient tiles
    float* tile = reinterpret_cast<float*>(smem);
    float2* grad = reinterpret_cast<float2*>(tile + ((tw * th + 1) & ~1));   // (Ix, Iy) interleaved: one 8-byte LDS read per tap
    const int pair = blockIdx.z;
    const int w = a.lv[l].w, h = a.lv[l].h;
    const float* I0 = pr.pyr0[pair] + a.lv[l].off;
    const float* I1 = pr.pyr1[pair] + a.lv[l].off;
    const int x0 = blockIdx.x * kOfTx, y0 = blockIdx.y * kOfTy;
    const int tid = threadIdx.y * kOfTx + threadIdx.x;
    for (int i = tid; i < tw * th; i += kOfTx * kOfTy) {
        const int ty = i / tw, tx = i - ty * tw;
        tile[i] = at_g(I0, w, h, x0 - R + tx, y0 - R + ty);   // edge-extended previous image
    }
    __syncthreads();
    for (int i = tid; i < gw * gh; i += kOfTx * kOfTy) {
        const int ty = i / gw, tx = i - ty * gw;
        const float* t = tile + (ty + 1) * tw + (tx + 1);
        grad[i] = make_float2(0.5f * (t[1] - t[-1]), 0.5f * (t[tw] - t[-tw]));
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= w || y >= h) return;

    float dx = 0.0f, dy = 0.0f;
    if (l < a.levels - 1) {
        const float* c = pr.coarse[pair] + a.flow_off[l + 1] + 2 * ((size_t)(y >> 1) * a.lv[l + 1].w + (x >> 1));
        dx = 2.0f * c[0];
        dy = 2.0f * c[1];
    }
    // window origin inside the tiles: tap (ox, oy) -> gradient tile (threadIdx + r + o), I0 tile (threadIdx + R + o)
    const float2* g0 = grad + threadIdx.y * gw + threadIdx.x;
    const float* t0 = tile + (threadIdx.y + 1) * tw + (threadIdx.x + 1);
    const int n = 2 * r + 1;
    float g11 = 0.0f, g12 = 0.0f, g22 = 0.0f;
    for (int k = 0; k < n; ++k)
        for (int j = 0; j < n; ++j) {
            const float2 g = g0[k * gw + j];
            g11 = fmaf(g.x, g.x, g11); g12 = fmaf(g.x, g.y, g12); g22 = fmaf(g.y, g.y, g22);
        }
    const float det = g11 * g22 - g12 * g12;
    if (det > a.det_min) {
        const float inv = 1.0f / det;
        constexpr int NMAX = RT ? 2 * RT + 1 : 15;
        for (int it = 0; it < a.iterations; ++it) {
            const float xf = (float)x + dx, yf = (float)y + dy;
            const float fx = floorf(xf), fy = floorf(yf);
            const float ax = xf - fx, ay = yf - fy;
            const int qx = (int)fminf(fmaxf(fx, -64.0f), (float)w + 64.0f) - r;
            const int qy = (int)fminf(fmaxf(fy, -64.0f), (float)h + 64.0f) - r;
            float b1 = 0.0f, b2 = 0.0f;
            float hp[NMAX];   // horizontal pass of the previous row
#pragma unroll 1
            for (int k = 0; k <= n; ++k) {
                const float* row = I1 + (size_t)clampi(qy + k, 0, h - 1) * w;
                float hc[NMAX];
                float left = row[clampi(qx, 0, w - 1)];
#pragma unroll
                for (int j = 0; j < NMAX; ++j) {
                    if (j >= n) break;
                    const float right = row[clampi(qx + j + 1, 0, w - 1)];
                    hc[j] = fmaf(ax, right, (1.0f - ax) * left);
                    left = right;
                }
                if (k > 0) {
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) {
                        if (j >= n) break;
                        const int o = (k - 1) * gw + j;
                        const float dt = fmaf(ay, hc[j], (1.0f - ay) * hp[j]) - t0[(k - 1) * tw + j];
                        const float2 g = g0[o];
                        b1 = fmaf(g.x, dt, b1); b2 = fmaf(g.y, dt, b2);
                    }
                }
#pragma unroll
                for (int j = 0; j < NMAX; ++j) hp[j] = hc[j];
            }
            dx -= (g22 * b1 - g12 * b2) * inv;
            dy -= (g11 * b2 - g12 * b1) * inv;
        }
    }
    float* dst = (l == 0) ? pr.field[pair] : pr.coarse[pair] + a.flow_off[l];
    reinterpret_cast<float2*>(dst)[(size_t)y * w + x] = make_float2(dx, dy);
}

// CV_16SC2 grid 4: block-centre sample, S10.5, saturated
__global__ __launch_bounds__(256) void of_quantise_kernel(OfPairs pr, int W, int H)
{
    const int pair = blockIdx.y;
    const int gw = W / 4, gh = H / 4;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gw * gh) return;
    const int gy = i / gw, gx = i - gy * gw;
    const float2 v = reinterpret_cast<const float2*>(pr.field[pair])[(size_t)(4 * gy + 2) * W + (4 * gx + 2)];
    const float qx = fminf(fmaxf(rintf(v.x * 32.0f), -32768.0f), 32767.0f);
    const float qy = fminf(fmaxf(rintf(v.y * 32.0f), -32768.0f), 32767.0f);
    reinterpret_cast<short2*>(pr.out_s16[pair])[i] = make_short2((short)qx, (short)qy);
}

// The forward-backward check of a chunk's pairs (include/roft_engine.h section 3f states it operation by operation; the library is
// built without contraction, so every product and sum below is one rounded operation).  One pixel per thread: the forward vector
// is one coalesced 8-byte load, the four backward taps are 8-byte gathers around the pixel's target (neighbouring pixels have
// neighbouring targets wherever the flow is smooth), and ONLY an invalid pixel is stored -- a valid one keeps its bits because
// nothing writes them.  A pixel whose target is outside the image (or not finite: every comparison fails) reads nothing.
__global__ __launch_bounds__(256) void of_check_kernel(OfCheck ck, int W, int H)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    float2* F = reinterpret_cast<float2*>(ck.fwd[blockIdx.y]);
    const float2* B = reinterpret_cast<const float2*>(ck.bwd[blockIdx.y]);
    const int y = i / W, x = i - y * W;
    const float2 f = F[i];
    const float xf = (float)x + f.x, yf = (float)y + f.y;
    bool valid = xf >= 0.0f && xf <= (float)(W - 1) && yf >= 0.0f && yf <= (float)(H - 1);
    if (valid) {
        const float x0f = floorf(xf), y0f = floorf(yf);
        const float ax = xf - x0f, ay = yf - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float2 b00 = B[(size_t)y0 * W + x0], b01 = B[(size_t)y0 * W + x1];
        const float2 b10 = B[(size_t)y1 * W + x0], b11 = B[(size_t)y1 * W + x1];
        const float sx = 1.0f - ax, sy = 1.0f - ay;
        const float topx = sx * b00.x + ax * b01.x, botx = sx * b10.x + ax * b11.x;
        const float topy = sx * b00.y + ax * b01.y, boty = sx * b10.y + ax * b11.y;
        const float bx = sy * topx + ay * botx, by = sy * topy + ay * boty;
        const float ex = f.x + bx, ey = f.y + by;
        const float e2 = ex * ex + ey * ey;
        const float m2 = (f.x * f.x + f.y * f.y) + (bx * bx + by * by);
        valid = e2 <= ck.tol_rel * m2 + ck.tol_abs;
    }
    if (!valid) reinterpret_cast<uint2*>(F)[i] = make_uint2(0x7FC00000u, 0x7FC00000u);
}

void launch_of_check(const OfGeom& a, const OfCheck& ck, hipStream_t s)
{
    const int W = a.lv[0].w, H = a.lv[0].h;
    hipLaunchKernelGGL(of_check_kernel, dim3((W * H + 255) / 256, ck.n), dim3(256), 0, s, ck, W, H);
}

void launch_of_pyramids(const OfGeom& a, const OfImages& im, hipStream_t s)
{
    const int n4 = a.lv[0].w * a.lv[0].h / 4;
    hipLaunchKernelGGL(of_convert_kernel, dim3(std::min((n4 + 255) / 256, 256), im.n), dim3(256), 0, s, a, im);
    for (int l = 1; l < a.levels; ++l) {
        const int npx = a.lv[l].w * a.lv[l].h;
        hipLaunchKernelGGL(of_down_kernel, dim3(std::min((npx + 255) / 256, 256), im.n), dim3(256), 0, s, a, im, l);
    }
}

void launch_of_pairs(const OfGeom& a, const OfPairs& pr, hipStream_t s)
{
    const int r = a.radius, R = r + 1;
    const size_t lds = ((((size_t)(kOfTx + 2 * R) * (kOfTy + 2 * R) + 1) & ~(size_t)1) + 2 * (size_t)(kOfTx + 2 * r) * (kOfTy + 2 * r)) * sizeof(float);
    for (int l = a.levels - 1; l >= 0; --l) {
        const dim3 grid((a.lv[l].w + kOfTx - 1) / kOfTx, (a.lv[l].h + kOfTy - 1) / kOfTy, pr.n), block(kOfTx, kOfTy);
        switch (r) {
            case 1: hipLaunchKernelGGL(of_lk_kernel<1>, grid, block, lds, s, a, pr, l); break;
            case 2: hipLaunchKernelGGL(of_lk_kernel<2>, grid, block, lds, s, a, pr, l); break;
            case 3: hipLaunchKernelGGL(of_lk_kernel<3>, grid, block, lds, s, a, pr, l); break;
            case 4: hipLaunchKernelGGL(of_lk_kernel<4>, grid, block, lds, s, a, pr, l); break;
            default: hipLaunchKernelGGL(of_lk_kernel<0>, grid, block, lds, s, a, pr, l); break;
        }
    }
    if (pr.out_s16[0]) {
        const int W = a.lv[0].w, H = a.lv[0].h;
        hipLaunchKernelGGL(of_quantise_kernel, dim3(((W / 4) * (H / 4) + 255) / 256, pr.n), dim3(256), 0, s, pr, W, H);
    }
}

void launch_image_to_gray(const uint8_t* src, int type, size_t npix, uint8_t* dst, hipStream_t s)
{
    hipLaunchKernelGGL(image_to_gray_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, src, type, npix, dst);
}

}  // namespace roft
