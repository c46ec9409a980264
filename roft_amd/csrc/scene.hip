// scene.hip -- host side of the scene renderer entry points of include/roft_engine.h (section 3b): argument checks (all of them
// before the device is looked for), the resident handle with its device buffers, and the two launches of k_scene.hip.
#include "engine_internal.h"
#include "raster.h"
#include "scene.h"

struct roft_scene_renderer {
    int W = 0, H = 0, device = 0, max_frames = 0, n_meshes = 0, max_verts = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    hipStream_t stream = nullptr;
    Event ev[3];
    bool timed = false;
    std::vector<DeviceMesh> resident;   // the meshes the table below names
    DevBuf<MeshView> meshes;
    DevBuf<uint64_t> keys;
    DevBuf<ScenePose> pose_table;
    DevBuf<double> poses;
    DevBuf<uint8_t> valid, background, rgb;
    DevBuf<int> mesh_index;
    DevBuf<SceneStyle> styles;
    DevBuf<float> depth;
    DevBuf<int32_t> instance, triangle;
};

namespace {

// tint of instance i without a style: eight colours that stay apart on a gray frame
const float kPalette[8][3] = {{230, 60, 50},  {50, 140, 230}, {60, 190, 80},  {240, 180, 40},
                              {170, 80, 200}, {40, 200, 200}, {240, 120, 170}, {150, 150, 150}};

bool unit_range(float v) { return v >= 0.0f && v <= 1.0f; }   // (false for NaN)

int check_camera(const roft_camera* cam)
{
    if (!cam) return fail(ROFT_ERR_INVALID, "null camera");
    if (cam->width < 1 || cam->height < 1) return fail(ROFT_ERR_INVALID, "width and height must be >= 1");
    if ((long long)cam->width * cam->height >= (1ll << 24)) return fail(ROFT_ERR_INVALID, "width * height must be < 2^24");
    return ROFT_OK;
}

int check_meshes(const roft_mesh* meshes, int n_meshes)
{
    if (n_meshes < 0 || (n_meshes > 0 && !meshes)) return fail(ROFT_ERR_INVALID, "null mesh array");
    for (int k = 0; k < n_meshes; ++k) TRY(check_mesh(meshes[k], "mesh " + std::to_string(k), false, 24));   // (a pixel's key holds 24 bits of triangle index)
    return ROFT_OK;
}

// max_frames < 0: no limit (the one-shot call sizes its renderer by the description)
int check_desc(const roft_scene_desc* d, int n_meshes, int max_frames)
{
    if (!d) return fail(ROFT_ERR_INVALID, "null scene description");
    if (d->n_frames < 0) return fail(ROFT_ERR_INVALID, "n_frames must be >= 0");
    if (d->n_instances < 0 || d->n_instances > ROFT_SCENE_MAX_INSTANCES) return fail(ROFT_ERR_INVALID, "n_instances must be 0 .. 256");
    if (max_frames >= 0 && d->n_frames > max_frames) return fail(ROFT_ERR_INVALID, "n_frames exceeds the renderer's max_frames_per_call");
    if (d->n_frames > 65536) return fail(ROFT_ERR_INVALID, "n_frames exceeds 65536");
    if (d->window_pixels < 0) return fail(ROFT_ERR_INVALID, "window_pixels must be >= 0");
    if (d->n_instances > 0 && !d->mesh_index) return fail(ROFT_ERR_INVALID, "null mesh_index");
    for (int i = 0; i < d->n_instances; ++i)
        if (d->mesh_index[i] < 0 || d->mesh_index[i] >= n_meshes)
            return fail(ROFT_ERR_INVALID, "mesh_index[" + std::to_string(i) + "] = " + std::to_string(d->mesh_index[i]) + " is not one of the renderer's meshes");
    if (d->n_instances > 0 && d->n_frames > 0 && !d->poses) return fail(ROFT_ERR_INVALID, "null poses");
    if (d->background && d->n_frames > 0 && d->background_frames != 1 && d->background_frames != d->n_frames)
        return fail(ROFT_ERR_INVALID, "background_frames must be n_frames or 1");
    if (d->styles)
        for (int i = 0; i < d->n_instances; ++i)
            if (!unit_range(d->styles[i].opacity) || !unit_range(d->styles[i].ambient))
                return fail(ROFT_ERR_INVALID, "style " + std::to_string(i) + ": opacity and ambient must lie in [0, 1]");
    return ROFT_OK;
}

template <class T>
int upload(DevBuf<T>& b, const T* src, size_t n, hipStream_t s)
{
    HIP_TRY(b.ensure(n));
    if (n) HIP_TRY(hipMemcpyAsync(b.p, src, sizeof(T) * n, hipMemcpyHostToDevice, s));
    return ROFT_OK;
}

int render(roft_scene_renderer* r, const roft_scene_desc* d, uint8_t* rgb_out, float* depth_out, int32_t* instance_out, int32_t* triangle_out)
{
    HIP_TRY(hipSetDevice(r->device));
    (void)hipGetLastError();   // a stale error of another library on this thread is not this call's
    const int F = d->n_frames, I = d->n_instances;
    const size_t WH = (size_t)r->W * r->H, total = WH * F;
    const size_t padded = (total + kResolvePixels - 1) / kResolvePixels * kResolvePixels;
    hipStream_t s = r->stream;
    SceneArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = r->W; a.H = r->H; a.n_frames = F; a.n_instances = I;
    a.fx = r->fx; a.fy = r->fy; a.cx = r->cx; a.cy = r->cy;
    a.meshes = r->meshes.p;
    HIP_TRY(r->keys.ensure(padded));
    a.keys = r->keys.p;
    if (I > 0) {
        if (int rc = upload(r->mesh_index, d->mesh_index, (size_t)I, s)) return rc;
        if (int rc = upload(r->poses, d->poses, (size_t)F * I * 7, s)) return rc;
        if (d->valid)
            if (int rc = upload(r->valid, d->valid, (size_t)F * I, s)) return rc;
        std::vector<SceneStyle> styles((size_t)I);
        for (int i = 0; i < I; ++i) {
            SceneStyle& st = styles[(size_t)i];
            if (d->styles) {
                for (int c = 0; c < 3; ++c) st.tint[c] = d->styles[i].tint[c];
                st.opacity = d->styles[i].opacity;
                st.ambient = d->styles[i].ambient;
            } else {
                for (int c = 0; c < 3; ++c) st.tint[c] = kPalette[i % 8][c];
                st.opacity = 0.75f;
                st.ambient = 0.35f;
            }
        }
        if (int rc = upload(r->styles, styles.data(), (size_t)I, s)) return rc;
        HIP_TRY(hipStreamSynchronize(s));   // (styles lives on this stack)
        HIP_TRY(r->pose_table.ensure((size_t)F * I));
        a.mesh_index = r->mesh_index.p;
        a.poses = r->poses.p;
        a.valid = d->valid ? r->valid.p : nullptr;
        a.styles = r->styles.p;
        a.pose_table = r->pose_table.p;
    }
    if (rgb_out) {
        if (d->background) {
            if (int rc = upload(r->background, d->background, WH * 3 * (size_t)d->background_frames, s)) return rc;
            a.background = r->background.p;
            a.background_frames = d->background_frames;
            a.gray_background = d->gray_background ? 1 : 0;
        }
        HIP_TRY(r->rgb.ensure(padded * 3));
        a.rgb = r->rgb.p;
    }
    if (depth_out) { HIP_TRY(r->depth.ensure(padded)); a.depth = r->depth.p; }
    if (instance_out) { HIP_TRY(r->instance.ensure(padded)); a.instance = r->instance.p; }
    if (triangle_out) { HIP_TRY(r->triangle.ensure(padded)); a.triangle = r->triangle.p; }
    const RasterShape sh = scene_window_shape(r->max_verts, WH, d->window_pixels);   // the LDS of a visibility workgroup
    a.vcache_cap = sh.vcache_cap;
    a.win_cap = sh.win_cap;
    // workgroups per instance: enough of them to fill the chip when the call is small
    a.parts = (int)std::max<size_t>(1, std::min<size_t>(32, (size_t)2 * device_cu_count() / std::max<size_t>((size_t)F * I, 1)));
    HIP_TRY(hipEventRecord(r->ev[0], s));
    HIP_TRY(hipMemsetAsync(r->keys.p, 0xFF, padded * sizeof(uint64_t), s));   // kSceneKeyEmpty
    if (I > 0) launch_scene_visibility(a, sh.lds, s);
    HIP_TRY(hipEventRecord(r->ev[1], s));
    launch_scene_resolve(a, s);
    HIP_TRY(hipEventRecord(r->ev[2], s));
    HIP_TRY(hipGetLastError());
    if (rgb_out) HIP_TRY(hipMemcpyAsync(rgb_out, r->rgb.p, total * 3, hipMemcpyDeviceToHost, s));
    if (depth_out) HIP_TRY(hipMemcpyAsync(depth_out, r->depth.p, total * sizeof(float), hipMemcpyDeviceToHost, s));
    if (instance_out) HIP_TRY(hipMemcpyAsync(instance_out, r->instance.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (triangle_out) HIP_TRY(hipMemcpyAsync(triangle_out, r->triangle.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    r->timed = true;
    return ROFT_OK;
}

}  // namespace

extern "C" {

int roft_scene_renderer_create(const roft_camera* cam, const roft_mesh* meshes, int n_meshes, int max_frames_per_call, int device,
                               roft_scene_renderer** out)
{
    if (!out) return fail(ROFT_ERR_INVALID, "null output pointer");
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_meshes(meshes, n_meshes)) return rc;
    if (max_frames_per_call < 1 || max_frames_per_call > 65536) return fail(ROFT_ERR_INVALID, "max_frames_per_call must be 1 .. 65536");
    if (device < 0) return fail(ROFT_ERR_INVALID, "device must be >= 0");
    TRY(require_device(device, "no such HIP device (the scene renderer has no CPU path)"));
    HIP_TRY(hipSetDevice(device));
    (void)hipGetLastError();
    // (destroyed on every way out but the last)
    struct Destroy { void operator()(roft_scene_renderer* p) const { (void)roft_scene_renderer_destroy(p); } };
    std::unique_ptr<roft_scene_renderer, Destroy> r(new roft_scene_renderer());
    r->W = cam->width; r->H = cam->height; r->device = device; r->max_frames = max_frames_per_call; r->n_meshes = n_meshes;
    // the contract's intrinsics at divider 1 (oracle/ro_render.c: (float)(fx / divider))
    r->fx = (float)cam->fx; r->fy = (float)cam->fy; r->cx = (float)cam->cx; r->cy = (float)cam->cy;
    hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = r->ev[k].create();
    if (e != hipSuccess) return fail(ROFT_ERR_DEVICE, std::string("stream creation: ") + hipGetErrorString(e));
    r->resident = std::vector<DeviceMesh>((size_t)n_meshes);
    std::vector<MeshView> table((size_t)n_meshes);
    for (int k = 0; k < n_meshes; ++k) {
        // the caller's triangles as they are (a key's triangle index is the caller's); closed meshes get their flip bits
        TRY(r->resident[k].upload(meshes[k], MeshLayout::kCallersOrder, r->stream));
        table[k] = r->resident[k].view();
        r->max_verts = std::max(r->max_verts, meshes[k].n_verts);
    }
    e = r->meshes.ensure((size_t)n_meshes);
    if (e == hipSuccess && n_meshes) e = hipMemcpy(r->meshes.p, table.data(), sizeof(MeshView) * n_meshes, hipMemcpyHostToDevice);
    const size_t WH = (size_t)r->W * r->H;
    if (e == hipSuccess) e = r->keys.ensure((WH * max_frames_per_call + kResolvePixels - 1) / kResolvePixels * kResolvePixels);
    if (e != hipSuccess) return fail(ROFT_ERR_DEVICE, std::string("mesh upload: ") + hipGetErrorString(e));
    *out = r.release();
    return ROFT_OK;
}

int roft_scene_renderer_destroy(roft_scene_renderer* r)
{
    if (!r) return ROFT_OK;
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;   // (the device buffers and the events free themselves)
    return ROFT_OK;
}

int roft_scene_render(roft_scene_renderer* r, const roft_scene_desc* desc, uint8_t* rgb_out, float* depth_out, int32_t* instance_out,
                      int32_t* triangle_out)
{
    if (!r) return fail(ROFT_ERR_INVALID, "null renderer");
    if (int rc = check_desc(desc, r->n_meshes, r->max_frames)) return rc;
    if (desc->n_frames == 0) return ROFT_OK;
    return render(r, desc, rgb_out, depth_out, instance_out, triangle_out);
}

int roft_render_scene(const roft_camera* cam, const roft_mesh* meshes, int n_meshes, const roft_scene_desc* desc, uint8_t* rgb_out,
                      float* depth_out, int32_t* instance_out, int32_t* triangle_out)
{
    if (int rc = check_camera(cam)) return rc;
    if (int rc = check_meshes(meshes, n_meshes)) return rc;
    if (int rc = check_desc(desc, n_meshes, -1)) return rc;
    if (desc->n_frames == 0) return ROFT_OK;
    roft_scene_renderer* r = nullptr;
    if (int rc = roft_scene_renderer_create(cam, meshes, n_meshes, desc->n_frames, 0, &r)) return rc;
    const int rc = render(r, desc, rgb_out, depth_out, instance_out, triangle_out);
    roft_scene_renderer_destroy(r);
    return rc;
}

int roft_debug_scene_kernel_ms(roft_scene_renderer* r, double ms_out[2])
{
    if (!r || !ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (!r->timed) return fail(ROFT_ERR_STATE, "no roft_scene_render call to report");
    HIP_TRY(hipSetDevice(r->device));
    float v = 0.f, s = 0.f;
    HIP_TRY(hipEventElapsedTime(&v, r->ev[0], r->ev[1]));
    HIP_TRY(hipEventElapsedTime(&s, r->ev[1], r->ev[2]));
    ms_out[0] = v;
    ms_out[1] = s;
    return ROFT_OK;
}

}  // extern "C"
