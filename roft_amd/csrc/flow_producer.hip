// flow_producer.hip -- host side of the optical-flow producer entry points of include/roft_engine.h (section 3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/roft_engine.h"
#include "opticalflow.h"

using namespace roft;

extern "C" const char* roft_last_error_string(void);
namespace roft {
int set_last_error(int code, const std::string& msg);
int of_check_params(int W, int H, const roft_of_params* p);
int of_check_consistency(const roft_of_consistency* c);
}

#define OF_TRY(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return roft::set_last_error(ROFT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct roft_flow_producer {
    int W = 0, H = 0, max_pairs = 0, out_type = 0, device = 0;
    roft_of_params prm{};
    hipStream_t stream = nullptr;
    OfGeom geom{};
    float* pyr = nullptr;               // [2 * max_pairs][pyr_stride]: one pyramid per DISTINCT image of a call
    float* coarse = nullptr;            // [max_pairs][flow_stride]
    float* field = nullptr;             // [max_pairs][H*W*2] level-0 fields when the product is CV_16SC2
    // the forward-backward check (roft_flow_producer_set_consistency): the backward problems' coarse workspace and level-0 fields
    bool check = false;
    roft_of_consistency tol{};
    float* coarse_b = nullptr;          // [max_pairs][flow_stride]
    float* field_b = nullptr;           // [max_pairs][H*W*2]
};

// finite and >= 0 (a NaN fails both comparisons' complement)
int roft::of_check_consistency(const roft_of_consistency* c)
{
    if (!(c->tolerance_abs >= 0.0f && c->tolerance_abs <= 3.402823466e38f && c->tolerance_rel >= 0.0f && c->tolerance_rel <= 3.402823466e38f))
        return roft::set_last_error(ROFT_ERR_INVALID, "flow consistency: tolerance_abs and tolerance_rel must be finite and >= 0");
    return ROFT_OK;
}

// the ranges roft_flow_producer_create accepts (roft_engine_enable_flow asks the same question)
int roft::of_check_params(int W, int H, const roft_of_params* p)
{
    if (p->levels < 1 || p->levels > 6 || p->radius < 1 || p->radius > 7 || p->iterations < 0)
        return roft::set_last_error(ROFT_ERR_INVALID, "levels 1..6, radius 1..7");
    if (W <= 0 || H <= 0 || (W % (4 << (p->levels - 1))) || (H % (1 << (p->levels - 1))) || (W % 4) || (H % 4))
        return roft::set_last_error(ROFT_ERR_INVALID, "width must be a multiple of 4 * 2^(levels-1), height of 2^(levels-1) and of 4");
    return ROFT_OK;
}

extern "C" {

int roft_default_of_params(roft_of_params* p)
{
    if (!p) return roft::set_last_error(ROFT_ERR_INVALID, "null params");
    p->levels = 3;
    p->radius = 3;
    p->iterations = 3;
    p->det_min = 100.0f;
    return ROFT_OK;
}

int roft_flow_producer_create(int W, int H, int max_pairs, const roft_of_params* p, int out_type, int device,
                              roft_flow_producer** out)
{
    if (!p || !out || max_pairs <= 0) return roft::set_last_error(ROFT_ERR_INVALID, "bad argument");
    if (int rc = roft::of_check_params(W, H, p)) return rc;
    if (out_type != ROFT_FLOW_F32C2 && out_type != ROFT_FLOW_S16C2) return roft::set_last_error(ROFT_ERR_INVALID, "bad out_type");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device)
        return roft::set_last_error(ROFT_ERR_DEVICE, "no HIP device (the flow producer has no CPU path)");
    OF_TRY(hipSetDevice(device));
    roft_flow_producer* fp = new roft_flow_producer();
    fp->W = W; fp->H = H; fp->max_pairs = max_pairs; fp->out_type = out_type; fp->device = device; fp->prm = *p;
    OF_TRY(hipStreamCreateWithFlags(&fp->stream, hipStreamNonBlocking));
    OfGeom& a = fp->geom;
    of_geometry(a, W, H, p->levels, p->radius, p->iterations, p->det_min);
    OF_TRY(hipMalloc(reinterpret_cast<void**>(&fp->pyr), sizeof(float) * 2 * a.pyr_stride * max_pairs));
    OF_TRY(hipMalloc(reinterpret_cast<void**>(&fp->coarse), sizeof(float) * a.flow_stride * max_pairs));
    if (out_type == ROFT_FLOW_S16C2) OF_TRY(hipMalloc(reinterpret_cast<void**>(&fp->field), sizeof(float) * 2 * W * H * max_pairs));
    *out = fp;
    return ROFT_OK;
}

int roft_default_of_consistency(roft_of_consistency* c)
{
    if (!c) return roft::set_last_error(ROFT_ERR_INVALID, "null consistency");
    c->tolerance_abs = 0.5f;
    c->tolerance_rel = 0.01f;
    return ROFT_OK;
}

int roft_flow_producer_set_consistency(roft_flow_producer* fp, const roft_of_consistency* c)
{
    if (!fp) return roft::set_last_error(ROFT_ERR_INVALID, "null producer");
    if (!c) { fp->check = false; return ROFT_OK; }   // (the workspace stays: the check may come back)
    if (fp->out_type != ROFT_FLOW_F32C2)
        return roft::set_last_error(ROFT_ERR_INVALID, "flow consistency: CV_16SC2 has no representation of an invalid vector, the check serves the CV_32FC2 product only");
    if (int rc = roft::of_check_consistency(c)) return rc;
    OF_TRY(hipSetDevice(fp->device));
    if (!fp->coarse_b) OF_TRY(hipMalloc(reinterpret_cast<void**>(&fp->coarse_b), sizeof(float) * fp->geom.flow_stride * fp->max_pairs));
    if (!fp->field_b) OF_TRY(hipMalloc(reinterpret_cast<void**>(&fp->field_b), sizeof(float) * 2 * fp->W * fp->H * fp->max_pairs));
    fp->tol = *c;
    fp->check = true;
    return ROFT_OK;
}

int roft_flow_producer_destroy(roft_flow_producer* fp)
{
    if (!fp) return ROFT_OK;
    (void)hipSetDevice(fp->device);
    if (fp->stream) (void)hipStreamSynchronize(fp->stream);
    if (fp->pyr) (void)hipFree(fp->pyr);
    if (fp->coarse) (void)hipFree(fp->coarse);
    if (fp->field) (void)hipFree(fp->field);
    if (fp->coarse_b) (void)hipFree(fp->coarse_b);
    if (fp->field_b) (void)hipFree(fp->field_b);
    if (fp->stream) (void)hipStreamDestroy(fp->stream);
    delete fp;
    return ROFT_OK;
}

int roft_flow_producer_run(roft_flow_producer* fp, const uint8_t* const* prev, const uint8_t* const* cur, void* const* out,
                           int n)
{
    if (!fp || !prev || !cur || !out || n <= 0 || n > fp->max_pairs) return roft::set_last_error(ROFT_ERR_INVALID, "bad argument");
    OF_TRY(hipSetDevice(fp->device));
    for (int i = 0; i < n; ++i)
        if (!prev[i] || !cur[i] || !out[i] || (reinterpret_cast<uintptr_t>(prev[i]) & 3) || (reinterpret_cast<uintptr_t>(cur[i]) & 3) ||
            (reinterpret_cast<uintptr_t>(out[i]) & 7))
            return roft::set_last_error(ROFT_ERR_INVALID, "null or misaligned image / flow pointer (images 4 B, flow 8 B)");
    // one pyramid per distinct image of the call (the frames of a stream are each the `cur` of one pair and the `prev` of the next)
    const OfGeom& g = fp->geom;
    std::vector<const uint8_t*> images;
    auto pyramid_of = [&](const uint8_t* img) -> float* {
        size_t k = std::find(images.begin(), images.end(), img) - images.begin();
        if (k == images.size()) images.push_back(img);
        return fp->pyr + k * g.pyr_stride;
    };
    // with the check a chunk serves kOfCheckChunk pairs: the forward and the backward problem of each (opticalflow.h)
    const int per = fp->check ? kOfCheckChunk : kOfChunk;
    std::vector<OfPairs> chunks((size_t)(n + per - 1) / per, OfPairs{});
    std::vector<OfCheck> checks(fp->check ? chunks.size() : 0, OfCheck{});
    for (int i = 0; i < n; ++i) {
        OfPairs& c = chunks[(size_t)i / per];
        if (fp->check) {
            float* prev_pyr = pyramid_of(prev[i]);
            float* cur_pyr = pyramid_of(cur[i]);
            of_check_put(c, checks[(size_t)i / per], prev_pyr, cur_pyr, static_cast<float*>(out[i]), fp->coarse + (size_t)i * g.flow_stride,
                         fp->coarse_b + (size_t)i * g.flow_stride, fp->field_b + (size_t)i * 2 * fp->W * fp->H);
            continue;
        }
        const int k = c.n++;
        c.pyr0[k] = pyramid_of(prev[i]);
        c.pyr1[k] = pyramid_of(cur[i]);
        c.coarse[k] = fp->coarse + (size_t)i * g.flow_stride;
        c.field[k] = (fp->out_type == ROFT_FLOW_F32C2) ? static_cast<float*>(out[i]) : fp->field + (size_t)i * 2 * fp->W * fp->H;
        c.out_s16[k] = (fp->out_type == ROFT_FLOW_S16C2) ? static_cast<int16_t*>(out[i]) : nullptr;
    }
    for (size_t i0 = 0; i0 < images.size(); i0 += kOfChunk) {
        OfImages im{};
        for (size_t i = i0; i < std::min(images.size(), i0 + kOfChunk); ++i) {
            const int k = im.n++;
            im.type[k] = kOfGray8; im.src[k] = images[i]; im.pyr[k] = fp->pyr + i * g.pyr_stride;
        }
        launch_of_pyramids(g, im, fp->stream);
    }
    for (size_t i = 0; i < chunks.size(); ++i) {
        if (fp->check) of_check_close(chunks[i]);
        launch_of_pairs(g, chunks[i], fp->stream);
        if (fp->check) {
            checks[i].tol_abs = fp->tol.tolerance_abs; checks[i].tol_rel = fp->tol.tolerance_rel;
            launch_of_check(g, checks[i], fp->stream);
        }
    }
    OF_TRY(hipGetLastError());
    return ROFT_OK;
}

int roft_flow_producer_sync(roft_flow_producer* fp)
{
    if (!fp) return roft::set_last_error(ROFT_ERR_INVALID, "null producer");
    OF_TRY(hipSetDevice(fp->device));
    OF_TRY(hipStreamSynchronize(fp->stream));
    return ROFT_OK;
}

void* roft_flow_producer_stream(roft_flow_producer* fp) { return fp ? (void*)fp->stream : nullptr; }

static int optical_flow_host(const uint8_t* prev, const uint8_t* cur, int W, int H, const roft_of_params* p, int out_type,
                             const roft_of_consistency* check, void* flow_out)
{
    if (!prev || !cur || !p || !flow_out) return roft::set_last_error(ROFT_ERR_INVALID, "null argument");
    if (check) {
        // decided before any device is touched
        if (int rc = roft::of_check_params(W, H, p)) return rc;
        if (int rc = roft::of_check_consistency(check)) return rc;
    }
    roft_flow_producer* fp = nullptr;
    if (int rc = roft_flow_producer_create(W, H, 1, p, out_type, 0, &fp)) return rc;
    if (check)
        if (int rc = roft_flow_producer_set_consistency(fp, check)) { roft_flow_producer_destroy(fp); return rc; }
    const size_t npix = (size_t)W * H;
    const size_t obytes = (out_type == ROFT_FLOW_F32C2) ? npix * 8 : (npix / 16) * 4;
    uint8_t *d0 = nullptr, *d1 = nullptr;
    void* dout = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d0), npix);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d1), npix);
    if (e == hipSuccess) e = hipMalloc(&dout, obytes);
    if (e == hipSuccess) e = hipMemcpy(d0, prev, npix, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d1, cur, npix, hipMemcpyHostToDevice);
    int rc = ROFT_OK;
    if (e == hipSuccess) {
        const uint8_t* pp[1] = {d0};
        const uint8_t* cc[1] = {d1};
        void* oo[1] = {dout};
        rc = roft_flow_producer_run(fp, pp, cc, oo, 1);
        if (rc == ROFT_OK) rc = roft_flow_producer_sync(fp);
        if (rc == ROFT_OK) e = hipMemcpy(flow_out, dout, obytes, hipMemcpyDeviceToHost);
    }
    if (d0) (void)hipFree(d0);
    if (d1) (void)hipFree(d1);
    if (dout) (void)hipFree(dout);
    roft_flow_producer_destroy(fp);
    if (e != hipSuccess) return roft::set_last_error(ROFT_ERR_DEVICE, hipGetErrorString(e));
    return rc;
}

int roft_optical_flow(const uint8_t* prev, const uint8_t* cur, int W, int H, const roft_of_params* p, int out_type, void* flow_out)
{
    return optical_flow_host(prev, cur, W, H, p, out_type, nullptr, flow_out);
}

int roft_optical_flow_checked(const uint8_t* prev, const uint8_t* cur, int W, int H, const roft_of_params* p, const roft_of_consistency* c,
                              float* flow_out)
{
    roft_of_consistency tol;
    if (c) tol = *c; else (void)roft_default_of_consistency(&tol);
    return optical_flow_host(prev, cur, W, H, p, ROFT_FLOW_F32C2, &tol, flow_out);
}

int roft_image_to_gray(const void* image, int image_type, int W, int H, uint8_t* gray_out)
{
    if (!image || !gray_out) return roft::set_last_error(ROFT_ERR_INVALID, "null argument");
    if (image_type != ROFT_IMAGE_GRAY8 && image_type != ROFT_IMAGE_BGR8 && image_type != ROFT_IMAGE_RGB8)
        return roft::set_last_error(ROFT_ERR_INVALID, "image_type must be ROFT_IMAGE_GRAY8, ROFT_IMAGE_BGR8 or ROFT_IMAGE_RGB8");
    if (W < 1 || H < 1) return roft::set_last_error(ROFT_ERR_INVALID, "width and height must be at least 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return roft::set_last_error(ROFT_ERR_DEVICE, "no HIP device (the conversion has no CPU path)");
    }
    const size_t npix = (size_t)W * H, ibytes = npix * (image_type == ROFT_IMAGE_GRAY8 ? 1 : 3);
    uint8_t *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_in), ibytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_out), npix);
    if (e == hipSuccess) e = hipMemcpy(d_in, image, ibytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_image_to_gray(d_in, image_type, npix, d_out, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(gray_out, d_out, npix, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return roft::set_last_error(ROFT_ERR_DEVICE, hipGetErrorString(e));
    return ROFT_OK;
}

}  // extern "C"
