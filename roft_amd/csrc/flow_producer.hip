// flow_producer.hip -- host side of the optical-flow producer entry points of include/roft_engine.h (section 3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_owned.h"
#include "opticalflow.h"

using namespace roft;
using namespace roft::host;

namespace roft {
int of_check_params(int W, int H, const roft_of_params* p);
int of_check_consistency(const roft_of_consistency* c);
}

struct roft_flow_producer {
    int W = 0, H = 0, max_pairs = 0, out_type = 0, device = 0;
    roft_of_params prm{};
    hipStream_t stream = nullptr;
    OfGeom geom{};
    DevBuf<float> pyr;                  // [2 * max_pairs][pyr_stride]: one pyramid per DISTINCT image of a call
    DevBuf<float> coarse;               // [max_pairs][flow_stride]
    DevBuf<float> field;                // [max_pairs][H*W*2] level-0 fields when the product is CV_16SC2
    // the forward-backward check (roft_flow_producer_set_consistency): the backward problems' coarse workspace and level-0 fields
    bool check = false;
    roft_of_consistency tol{};
    DevBuf<float> coarse_b;             // [max_pairs][flow_stride]
    DevBuf<float> field_b;              // [max_pairs][H*W*2]
};

namespace {
// a producer under construction, or one a one-shot call made for itself: destroyed on every way out
struct DestroyProducer { void operator()(roft_flow_producer* fp) const { (void)roft_flow_producer_destroy(fp); } };
using ProducerPtr = std::unique_ptr<roft_flow_producer, DestroyProducer>;
}  // namespace

// finite and >= 0 (a NaN fails both comparisons' complement)
int roft::of_check_consistency(const roft_of_consistency* c)
{
    if (!(c->tolerance_abs >= 0.0f && c->tolerance_abs <= 3.402823466e38f && c->tolerance_rel >= 0.0f && c->tolerance_rel <= 3.402823466e38f))
        return fail(ROFT_ERR_INVALID, "flow consistency: tolerance_abs and tolerance_rel must be finite and >= 0");
    return ROFT_OK;
}

// the ranges roft_flow_producer_create accepts (roft_engine_enable_flow asks the same question)
int roft::of_check_params(int W, int H, const roft_of_params* p)
{
    if (p->levels < 1 || p->levels > 6 || p->radius < 1 || p->radius > 7 || p->iterations < 0)
        return fail(ROFT_ERR_INVALID, "levels 1..6, radius 1..7");
    if (W <= 0 || H <= 0 || (W % (4 << (p->levels - 1))) || (H % (1 << (p->levels - 1))) || (W % 4) || (H % 4))
        return fail(ROFT_ERR_INVALID, "width must be a multiple of 4 * 2^(levels-1), height of 2^(levels-1) and of 4");
    return ROFT_OK;
}

extern "C" {

int roft_default_of_params(roft_of_params* p)
{
    if (!p) return fail(ROFT_ERR_INVALID, "null params");
    p->levels = 3;
    p->radius = 3;
    p->iterations = 3;
    p->det_min = 100.0f;
    return ROFT_OK;
}

int roft_flow_producer_create(int W, int H, int max_pairs, const roft_of_params* p, int out_type, int device,
                              roft_flow_producer** out)
{
    if (!p || !out || max_pairs <= 0) return fail(ROFT_ERR_INVALID, "bad argument");
    if (int rc = roft::of_check_params(W, H, p)) return rc;
    if (out_type != ROFT_FLOW_F32C2 && out_type != ROFT_FLOW_S16C2) return fail(ROFT_ERR_INVALID, "bad out_type");
    TRY(require_device(device, "no HIP device (the flow producer has no CPU path)"));
    HIP_TRY(hipSetDevice(device));
    ProducerPtr fp(new roft_flow_producer());
    fp->W = W; fp->H = H; fp->max_pairs = max_pairs; fp->out_type = out_type; fp->device = device; fp->prm = *p;
    HIP_TRY(hipStreamCreateWithFlags(&fp->stream, hipStreamNonBlocking));
    OfGeom& a = fp->geom;
    of_geometry(a, W, H, p->levels, p->radius, p->iterations, p->det_min);
    HIP_TRY(fp->pyr.ensure((size_t)2 * a.pyr_stride * max_pairs));
    HIP_TRY(fp->coarse.ensure((size_t)a.flow_stride * max_pairs));
    if (out_type == ROFT_FLOW_S16C2) HIP_TRY(fp->field.ensure((size_t)2 * W * H * max_pairs));
    *out = fp.release();
    return ROFT_OK;
}

int roft_default_of_consistency(roft_of_consistency* c)
{
    if (!c) return fail(ROFT_ERR_INVALID, "null consistency");
    c->tolerance_abs = 0.5f;
    c->tolerance_rel = 0.01f;
    return ROFT_OK;
}

int roft_flow_producer_set_consistency(roft_flow_producer* fp, const roft_of_consistency* c)
{
    if (!fp) return fail(ROFT_ERR_INVALID, "null producer");
    if (!c) { fp->check = false; return ROFT_OK; }   // (the workspace stays: the check may come back)
    if (fp->out_type != ROFT_FLOW_F32C2)
        return fail(ROFT_ERR_INVALID, "flow consistency: CV_16SC2 has no representation of an invalid vector, the check serves the CV_32FC2 product only");
    if (int rc = roft::of_check_consistency(c)) return rc;
    HIP_TRY(hipSetDevice(fp->device));
    HIP_TRY(fp->coarse_b.ensure((size_t)fp->geom.flow_stride * fp->max_pairs));
    HIP_TRY(fp->field_b.ensure((size_t)2 * fp->W * fp->H * fp->max_pairs));
    fp->tol = *c;
    fp->check = true;
    return ROFT_OK;
}

int roft_flow_producer_destroy(roft_flow_producer* fp)
{
    if (!fp) return ROFT_OK;
    (void)hipSetDevice(fp->device);
    if (fp->stream) (void)hipStreamSynchronize(fp->stream);
    if (fp->stream) (void)hipStreamDestroy(fp->stream);
    delete fp;   // (the device buffers free themselves)
    return ROFT_OK;
}

int roft_flow_producer_run(roft_flow_producer* fp, const uint8_t* const* prev, const uint8_t* const* cur, void* const* out,
                           int n)
{
    if (!fp || !prev || !cur || !out || n <= 0 || n > fp->max_pairs) return fail(ROFT_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(fp->device));
    for (int i = 0; i < n; ++i)
        if (!prev[i] || !cur[i] || !out[i] || (reinterpret_cast<uintptr_t>(prev[i]) & 3) || (reinterpret_cast<uintptr_t>(cur[i]) & 3) ||
            (reinterpret_cast<uintptr_t>(out[i]) & 7))
            return fail(ROFT_ERR_INVALID, "null or misaligned image / flow pointer (images 4 B, flow 8 B)");
    // one pyramid per distinct image of the call (the frames of a stream are each the `cur` of one pair and the `prev` of the next)
    const OfGeom& g = fp->geom;
    std::vector<const uint8_t*> images;
    auto pyramid_of = [&](const uint8_t* img) -> float* {
        size_t k = std::find(images.begin(), images.end(), img) - images.begin();
        if (k == images.size()) images.push_back(img);
        return fp->pyr.p + k * g.pyr_stride;
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
            of_check_put(c, checks[(size_t)i / per], prev_pyr, cur_pyr, static_cast<float*>(out[i]), fp->coarse.p + (size_t)i * g.flow_stride,
                         fp->coarse_b.p + (size_t)i * g.flow_stride, fp->field_b.p + (size_t)i * 2 * fp->W * fp->H);
            continue;
        }
        const int k = c.n++;
        c.pyr0[k] = pyramid_of(prev[i]);
        c.pyr1[k] = pyramid_of(cur[i]);
        c.coarse[k] = fp->coarse.p + (size_t)i * g.flow_stride;
        c.field[k] = (fp->out_type == ROFT_FLOW_F32C2) ? static_cast<float*>(out[i]) : fp->field.p + (size_t)i * 2 * fp->W * fp->H;
        c.out_s16[k] = (fp->out_type == ROFT_FLOW_S16C2) ? static_cast<int16_t*>(out[i]) : nullptr;
    }
    for (size_t i0 = 0; i0 < images.size(); i0 += kOfChunk) {
        OfImages im{};
        for (size_t i = i0; i < std::min(images.size(), i0 + kOfChunk); ++i) {
            const int k = im.n++;
            im.type[k] = kOfGray8; im.src[k] = images[i]; im.pyr[k] = fp->pyr.p + i * g.pyr_stride;
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
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

int roft_flow_producer_sync(roft_flow_producer* fp)
{
    if (!fp) return fail(ROFT_ERR_INVALID, "null producer");
    HIP_TRY(hipSetDevice(fp->device));
    HIP_TRY(hipStreamSynchronize(fp->stream));
    return ROFT_OK;
}

void* roft_flow_producer_stream(roft_flow_producer* fp) { return fp ? (void*)fp->stream : nullptr; }

static int optical_flow_host(const uint8_t* prev, const uint8_t* cur, int W, int H, const roft_of_params* p, int out_type,
                             const roft_of_consistency* check, void* flow_out)
{
    if (!prev || !cur || !p || !flow_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (check) {
        // decided before any device is touched
        if (int rc = roft::of_check_params(W, H, p)) return rc;
        if (int rc = roft::of_check_consistency(check)) return rc;
    }
    roft_flow_producer* made = nullptr;
    TRY(roft_flow_producer_create(W, H, 1, p, out_type, 0, &made));
    const ProducerPtr fp(made);
    if (check) TRY(roft_flow_producer_set_consistency(made, check));
    const size_t npix = (size_t)W * H;
    const size_t obytes = (out_type == ROFT_FLOW_F32C2) ? npix * 8 : (npix / 16) * 4;
    return host_round_trip({{prev, npix}, {cur, npix}}, flow_out, obytes, [&](const DevBuf<unsigned char>* in, void* out) {
        const uint8_t* const pp[1] = {in[0].p};
        const uint8_t* const cc[1] = {in[1].p};
        void* const oo[1] = {out};
        TRY(roft_flow_producer_run(made, pp, cc, oo, 1));
        return roft_flow_producer_sync(made);
    });
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
    if (!image || !gray_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (image_type != ROFT_IMAGE_GRAY8 && image_type != ROFT_IMAGE_BGR8 && image_type != ROFT_IMAGE_RGB8)
        return fail(ROFT_ERR_INVALID, "image_type must be ROFT_IMAGE_GRAY8, ROFT_IMAGE_BGR8 or ROFT_IMAGE_RGB8");
    if (W < 1 || H < 1) return fail(ROFT_ERR_INVALID, "width and height must be at least 1");
    TRY(require_device(0, "no HIP device (the conversion has no CPU path)"));
    const size_t npix = (size_t)W * H, ibytes = npix * (image_type == ROFT_IMAGE_GRAY8 ? 1 : 3);
    return host_round_trip({{image, ibytes}}, gray_out, npix, [&](const DevBuf<unsigned char>* in, void* out) -> int {
        launch_image_to_gray(in[0].p, image_type, npix, static_cast<uint8_t*>(out), nullptr);
        return ROFT_OK;
    });
}

}  // extern "C"
