// op_context.h -- the one context of the operator-level entry points (engine_ops.hip, roft_track_quality in engine_quality.hip,
// roft_pose_hypotheses_score in engine_hypotheses.hip): the
// engine's own kernels on one object and one frame, on device 0.
//
// THE RULE: the context owns device memory, a stream and a mutex.  It never holds configuration.  Every call derives the EngineArrays
// it launches with BY VALUE from that memory (one_object) and edits only its own copy, so when a call returns, by any path, there is
// nothing to put back; and an entry has nothing to reset except what it uploads anyway (begin_object: state, parameters, control
// block).  What the memory is allocated for -- width, height, radius -- is its shape, not a setting: it decides when to reallocate.
#pragma once

#include "engine_internal.h"

namespace roft {
namespace host {

struct OpContext {
    static constexpr int kSlots = 10;
    std::mutex mu;
    hipStream_t stream = nullptr;
    Arrays arr;                          // one object, one frame, with the one-row log.  arr.a is written by Arrays::alloc / ensure_zmerge and nobody else
    int W = 0, H = 0, radius = 0;        // what arr is allocated for (0: nothing yet)
    DevBuf<QualityRaw> quality;          // the record of roft_track_quality
    HypothesesScratch hypotheses;        // the poses and records of roft_pose_hypotheses_score (grow with the call's chunk)
    DeviceMesh mesh;                     // the mesh of the one-mesh calls ...
    std::vector<DeviceMesh> meshes;      // ... and those of the n-mesh silhouette calls (grows, never shrinks)
    PoseErrorScratch pose_errors;
    VsdScratch vsd;
    DevBuf<unsigned char> slot[kSlots];  // scratch, typed where it is handed out: room / upload.  A call numbers its slots as it likes
    ObjState st;                         // host landing block of the state's upload (begin_object) and read-back (read_state)

    // THE entry of an operator, behind its argument checks: takes the lock, refuses without a device, makes device 0 current, drops a
    // stale error of another library on this thread (it is not this call's) and makes sure of the stream
    int enter(std::unique_lock<std::mutex>& lk)
    {
        lk = std::unique_lock<std::mutex>(mu);
        if (roft_device_count() <= 0) return fail(ROFT_ERR_DEVICE, "no HIP device (libroft_hip has no CPU path)");
        HIP_TRY(hipSetDevice(0));
        (void)hipGetLastError();
        if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return ROFT_OK;
    }

    // room for `count` T in slot k / ... filled with `count` T of the host (in stream order; src must live until the next synchronise)
    template <class T>
    int room(int k, size_t count, T** p)
    {
        HIP_TRY(slot[k].ensure(std::max<size_t>(count * sizeof(T), 16)));
        *p = reinterpret_cast<T*>(slot[k].p);
        return ROFT_OK;
    }
    template <class T>
    int upload(int k, const T* src, size_t count, T** p)
    {
        TRY(room(k, count, p));
        if (count) HIP_TRY(hipMemcpyAsync(*p, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
        return ROFT_OK;
    }

    // The arrays of one object and one frame of camera `cam`, fully derived: cam, divider (0: the camera's default), tile size, flow
    // format (null: CV_32FC2 at full resolution), n_obj = T = 1, no mesh, no log.  (Re)allocates only when width, height or radius
    // changed; the z-buffers are sized for divider 1, the merge slabs follow the divider.  The caller sets its extras on *a.
    int one_object(const roft_camera& cam, const roft_flow* flow, int radius_, int divider, EngineArrays* a)
    {
        TRY(check_geometry(cam.width, cam.height));
        DevCamera dc = make_cam(cam);
        DevFlowFmt ff;
        ff.type = flow ? flow->type : ROFT_FLOW_F32C2;
        ff.grid = flow ? std::max(flow->grid, 1) : 1;
        ff.cols = cam.width / ff.grid;
        ff.rows = cam.height / ff.grid;
        ff.scale = flow ? flow->scale : 1.0f;
        if (W != cam.width || H != cam.height || radius != radius_) {
            W = 0;   // (a failed allocation leaves "nothing yet")
            HIP_TRY(arr.zbuf.ensure((size_t)2 * cam.width * cam.height));   // (before alloc, which then keeps it)
            TRY(arr.alloc(1, 1, dc, ff, std::max(radius_, 1)));
            HIP_TRY(arr.log.ensure(1, true));
            HIP_TRY(quality.ensure(1));
            W = cam.width; H = cam.height; radius = radius_;
        }
        if (divider > 0) dc.divider = divider;
        TRY(arr.ensure_zmerge(1, (size_t)(cam.width / dc.divider) * (cam.height / dc.divider)));
        *a = arr.a;
        a->cam = dc;
        a->ffmt = ff;
        a->tile_w = cam.width / dc.divider;
        a->tile_h = cam.height / dc.divider;
        a->n_obj = a->T = 1;
        return ROFT_OK;
    }
    // ... of an operator without an image (the pose filter): the memory at the size it has, the smallest one if there is none yet
    int one_object(EngineArrays* a)
    {
        const roft_camera cam{W ? W : 64, W ? H : 64, 1.0, 1.0, 0.0, 0.0};
        return one_object(cam, nullptr, W ? radius : 35, 0, a);
    }

    // What every launch on the one object starts from: the state in `st`, the parameters (null: none, zeros) and the control block, on
    // the device when this returns (prm and fc may live on the caller's stack)
    int begin_object(const EngineArrays& a, const ObjParams* prm, const FrameCtrl& fc)
    {
        HIP_TRY(hipMemcpyAsync(a.state, &st, sizeof(st), hipMemcpyHostToDevice, stream));
        if (prm) HIP_TRY(hipMemcpyAsync(a.params, prm, sizeof(*prm), hipMemcpyHostToDevice, stream));
        else HIP_TRY(hipMemsetAsync(a.params, 0, sizeof(ObjParams), stream));
        HIP_TRY(hipMemcpyAsync(a.ctrl, &fc, sizeof(fc), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return ROFT_OK;
    }
    // ... and ends with: everything enqueued has run, the state is back in `st`
    int read_state(const EngineArrays& a)
    {
        HIP_TRY(hipMemcpyAsync(&st, a.state, sizeof(st), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
        return ROFT_OK;
    }
};

OpContext& op_context();   // engine_ops.hip (a function-local static: one per process)

}  // namespace host
}  // namespace roft
