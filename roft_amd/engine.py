"""Batched ROFT filtering engine: host-side mirror of ROFT::ROFTFilter for many objects at once.

Thin wrapper over the C ABI (include/roft_engine.h): `ROFTFilterBatch` plays the role the
reference's `ROFTFilter` plays for one object (src/roft-lib/include/ROFT/ROFTFilter.h:38-194) --
construct with the same parameters, feed one frame at a time -- but every object of the batch
advances in the same kernel launches and all filter state stays in HBM.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .ops import mesh_of


def default_config(width, height, flow_type=L.FLOW_F32C2, max_objects=64, device=0, max_batch_frames=1, render_mode=L.RENDER_CONTRACT):
    """render_mode: how the outlier test renders, L.RENDER_CONTRACT (default) or L.RENDER_GL (the reference's GL numerics)."""
    cfg = L.Config()
    L.check(L.lib().roft_default_config(C.byref(cfg), width, height, flow_type))
    cfg.max_objects = max_objects
    cfg.device = device
    cfg.max_batch_frames = max_batch_frames
    cfg.render_mode = render_mode
    return cfg


def default_object():
    o = L.ObjectDesc()
    L.check(L.lib().roft_default_object(C.byref(o)))
    return o


def aligned_batches(first, last, T, period, phase=0):
    """[first, last) in consecutive batches of at most T frames that END with a pose-arrival frame (frames f with
    f % period == phase: the delayed pose source delivers every `period` frames).  Inside the engine a pose arrival hands
    the pose chain from one belief lineage -- one lane -- to the other: with the arrival as the last frame of
    a batch, every batch is one lineage's ordinary steps followed by the other's re-sync replay, the replay of batch b
    overlaps the ordinary steps of batch b + 1 on the other lane, and no launch of a lane carries both.  Measured against
    full batches of 8 cut anywhere (A/B in one box): +4 % at 20 steps, +5 % at 60, +3.5 % at 240."""
    out = []
    k = first
    while k < last:
        end = k + ((phase - k) % period) + 1 if period <= T else k + T
        while period <= T and (end - k) % period == 0 and end + period - k <= T:   # (whole periods, as many as a batch holds)
            end += period
        end = min(end, last, k + T)
        out.append((k, end - k))
        k = end
    return out



def frame_arrays(n):
    return (L.FrameInput * n)(), (L.LabelMask * n)(), (L.FrameImage * n)()


def fill_frame(frames, inputs, labels, images, base=0):
    """One frame -- one dict per object, see ROFTFilterBatch.submit -- into entries base .. base + len(frames) - 1 of the caller's
    L.FrameInput, L.LabelMask and L.FrameImage arrays.  Returns (keep, any_labels, any_images): the numpy arrays the entries point
    into, whether an object takes its mask from a label image, whether one brings a camera image."""
    keep = []
    shared = {}   # one contiguous copy per distinct label / camera image array of the frame: the engine uploads a host pointer once
    any_labels = any_images = False

    def shared_pointer(a):
        v = shared.get(id(a))
        if v is None:
            v = shared[id(a)] = np.ascontiguousarray(a)
            keep.append(v)
        return v

    for i, f in enumerate(frames):
        fi, lm, im = inputs[base + i], labels[base + i], images[base + i]
        img = f.get("image")
        if img is None:
            im.image, im.image_type = None, 0
        elif isinstance(img, int):
            im.image, im.image_type = img, int(f["image_type"])
        else:
            if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
                raise TypeError("a camera image is [H, W] or [H, W, 3] uint8")
            v = shared_pointer(img)
            im.image, im.image_type = v.ctypes.data, int(f.get("image_type", L.IMAGE_GRAY8 if v.ndim == 2 else L.IMAGE_RGB8))
        any_images = any_images or img is not None
        lab = f.get("labels")
        if lab is None:
            lm.labels, lm.label_type, lm.label = None, 0, 0
        elif isinstance(lab, int):
            lm.labels, lm.label_type, lm.label = lab, int(f["label_type"]), int(f["label"])
        else:
            if lab.dtype not in (np.uint8, np.uint16):
                raise TypeError("a label image is uint8 or uint16, not %s" % lab.dtype)
            v = shared_pointer(lab)
            lm.labels, lm.label_type, lm.label = v.ctypes.data, (L.LABEL_U8 if v.dtype == np.uint8 else L.LABEL_U16), int(f["label"])
        any_labels = any_labels or lab is not None
        kind = f.get("mem_kind", L.MEM_HOST)
        fi.mem_kind = kind
        fi.dt = f.get("dt", 0.0)
        fi.stamp = f.get("stamp", 0.0)            # only read with cfg.stamped_masks
        fi.mask_stamp = f.get("mask_stamp", 0.0)
        for key in ("depth", "flow", "mask"):
            v = f.get(key)
            if v is None:
                setattr(fi, key, None)
            elif kind == L.MEM_DEVICE or isinstance(v, int):
                setattr(fi, key, int(v))   # raw address (device pointer, or a host pointer kept alive by the caller)
            else:
                v = np.ascontiguousarray(v)
                keep.append(v)
                setattr(fi, key, v.ctypes.data)
        pose = f.get("pose")
        if pose is not None:
            fi.pose_valid = 1
            fi.pose_x = (C.c_double * 3)(*pose[0])
            fi.pose_q = (C.c_double * 4)(*pose[1])
        else:
            fi.pose_valid = 0
    return keep, any_labels, any_images


class BatchKeep(list):
    """What a batch built by assemble_batch points into, frame by frame; and its L.LabelMask / L.FrameImage arrays (None: no frame
    of the batch uses that form)."""
    labels = images = None


def assemble_batch(frames_list, n_objects):
    """ROFTFilterBatch.build_batch for n_objects objects."""
    T = len(frames_list)
    arr, lab, img = frame_arrays(n_objects * T)
    keep = BatchKeep()
    for t, frames in enumerate(frames_list):
        assert len(frames) == n_objects
        frame_keep, any_labels, any_images = fill_frame(frames, arr, lab, img, t * n_objects)
        keep.append(frame_keep)
        if any_labels:
            keep.labels = lab
        if any_images:
            keep.images = img
    return arr, keep, T


class ROFTFilterBatch:
    def __init__(self, cfg):
        L.require_device()
        self.cfg = cfg
        self._h = C.c_void_p()
        L.check(L.lib().roft_engine_create(C.byref(cfg), C.byref(self._h)))
        self.n_objects = 0
        self._keep = []
        self._inputs = None
        self.W, self.H = cfg.cam.width, cfg.cam.height

    def add_object(self, desc, verts, tris):
        desc.mesh, (verts, tris) = mesh_of(verts, tris)
        oid = C.c_int(-1)
        L.check(L.lib().roft_object_add(self._h, C.byref(desc), C.byref(oid)))
        self.n_objects += 1
        self._inputs, self._labels, self._images = frame_arrays(self.n_objects)
        self._meshes = getattr(self, "_meshes", []) + [(verts, tris)]   # render_log draws them
        return oid.value

    def restart_objects(self, items, keep_mesh=False):
        """A new track in the same slot (roft_objects_restart): items = [(obj_id, desc, verts, tris), ...], all restarted by ONE call,
        which waits for every stepped batch like sync().  From the engine's next frame on each named slot behaves, bit for bit, like
        the object of a new engine added with `desc` and that mesh; the other objects are untouched.  keep_mesh: verts / tris are
        not looked at (None will do) and the slots keep their resident meshes.  Also updates the meshes render_log draws."""
        items = list(items)
        n = len(items)
        ids = (C.c_int * max(n, 1))()
        descs = (L.ObjectDesc * max(n, 1))()
        keep = []
        for i, (oid, desc, verts, tris) in enumerate(items):
            ids[i] = int(oid)
            C.memmove(C.byref(descs[i]), C.byref(desc), C.sizeof(L.ObjectDesc))
            if keep_mesh:
                descs[i].mesh = L.Mesh(None, 0, None, 0)
                keep.append(None)
            else:
                descs[i].mesh, arrays = mesh_of(verts, tris)
                keep.append(arrays)
        L.check(L.lib().roft_objects_restart(self._h, ids, descs, n, L.RESTART_KEEP_MESH if keep_mesh else 0))
        meshes = getattr(self, "_meshes", [])
        for (oid, _, _, _), m in zip(items, keep):
            if m is not None and 0 <= int(oid) < len(meshes):
                meshes[int(oid)] = m

    def set_symmetry(self, obj, elements):
        """The discrete symmetry group of object `obj` (roft_object_set_symmetry): elements [n, 7] rows x y z, q = (w, x, y, z),
        element 0 the identity, n <= L.MAX_SYMMETRIES; None or a single element: none.  From the next submitted frame on, a
        delivered pose is replaced by its equivalent nearest to the belief it corrects.  Waits for every stepped batch like sync()."""
        if elements is None:
            L.check(L.lib().roft_object_set_symmetry(self._h, int(obj), None, 0))
            return
        sym = np.ascontiguousarray(elements, np.float64).reshape(-1, 7)
        L.check(L.lib().roft_object_set_symmetry(self._h, int(obj), sym.ctypes.data, sym.shape[0]))

    def _read_stats(self, call, struct):
        """one roft_engine_get_*_stats call -> the fields of its struct as a dict"""
        st = struct()
        L.check(call(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in struct._fields_}

    def restart_stats(self):
        """calls / objects restarted / meshes replaced by restart_objects since the engine was created."""
        return self._read_stats(L.lib().roft_engine_get_restart_stats, L.EngineRestartStats)

    def submit(self, frames):
        """frames: one dict per object with keys depth, flow, mask, pose (None or (x, q)), dt,
        mem_kind; depth/flow/mask are numpy arrays (HOST) or integer device addresses (DEVICE).
        After enable_raw_depth(): `depth` is the sensor's uint16 frame.
        Instead of `mask`: `labels` (one H x W uint8 / uint16 label image, typically the same array for every object of the
        frame; or an address, then with `label_type` L.LABEL_U8 / L.LABEL_U16) and `label`: the object's mask is the pixels
        EQUAL to that value (roft_frames_submit_labels).
        Instead of `flow`, on an engine with enable_flow(): `image`, the camera image of the frame (numpy [H, W] gray or
        [H, W, 3]; or an address, then with `image_type` L.IMAGE_GRAY8 / IMAGE_BGR8 / IMAGE_RGB8; a 3-channel array is RGB8
        unless `image_type` says BGR8): the engine computes the flow from it and the frame before (roft_frames_submit_images)."""
        assert len(frames) == self.n_objects
        self._keep, any_labels, any_images = fill_frame(frames, self._inputs, self._labels, self._images)
        self._submit(self._inputs, None, self._labels if any_labels else None, self._images if any_images else None)

    def _submit(self, arr, T, labels=None, images=None):
        """T None: one frame through the one-frame entry point (where the frame has neither label nor camera images)."""
        if images is not None:
            L.check(L.lib().roft_frames_submit_images(self._h, arr, labels, images, self.n_objects, T or 1))
        elif labels is not None:
            L.check(L.lib().roft_frames_submit_labels(self._h, arr, labels, self.n_objects, T or 1))
        elif T is None:
            L.check(L.lib().roft_frame_submit(self._h, arr, self.n_objects))
        else:
            L.check(L.lib().roft_frames_submit(self._h, arr, self.n_objects, T))

    def build_inputs(self, frames):
        """Pre-build the ctypes input array of one frame (see submit) for submit_raw."""
        assert len(frames) == self.n_objects
        arr, lab, img = frame_arrays(self.n_objects)
        keep, any_labels, any_images = fill_frame(frames, arr, lab, img)
        if any_labels or any_images:
            raise ValueError("label and camera images go through build_batch / submit_batch_raw(..., labels=..., images=...)")
        return arr, keep

    def submit_raw(self, inputs):
        self._submit(inputs, None)

    def build_batch(self, frames_list):
        """ctypes input array of a batch: frames_list[t] = one dict per object (see submit), t = 0 .. T-1.  The returned `keep`
        holds what the array points into, and the batch's L.LabelMask / L.FrameImage arrays where a frame uses label images /
        brings camera images (see batch_labels, batch_images)."""
        return assemble_batch(frames_list, self.n_objects)

    @staticmethod
    def batch_labels(keep):
        """The L.LabelMask array of a batch built by build_batch, or None when no frame of it uses label images."""
        return getattr(keep, "labels", None)

    @staticmethod
    def batch_images(keep):
        """The L.FrameImage array of a batch built by build_batch, or None when no frame of it brings camera images."""
        return getattr(keep, "images", None)

    def submit_batch(self, frames_list):
        """A batch of consecutive frames (at most cfg.max_batch_frames): roft_frames_submit, roft_frames_submit_labels when a
        frame takes masks from label images, roft_frames_submit_images when one brings camera images."""
        arr, keep, T = self.build_batch(frames_list)
        self._keep = keep
        self._submit(arr, T, keep.labels, keep.images)

    def submit_batch_raw(self, arr, T, labels=None, images=None):
        self._submit(arr, T, labels, images)

    def enable_flow(self, consistency=None, **of_params):
        """Camera images instead of flow frames (frame key `image`): the engine computes the optical flow itself, with the
        parameters of ops.of_params (levels, radius, iterations, det_min).  consistency: None, True or (tolerance_abs,
        tolerance_rel) -- the forward-backward check of ops.optical_flow on every produced flow (CV_32FC2 engines).  Before the
        first frame."""
        from .ops import of_consistency, of_params as make
        p = make(**of_params)
        c = of_consistency(consistency)
        L.check(L.lib().roft_engine_enable_flow(self._h, C.byref(p)))
        if c is not None:
            self.enable_flow_consistency(c)

    def enable_flow_consistency(self, consistency=True):
        """roft_engine_enable_flow_consistency: behind enable_flow, before the first frame.  True: the default tolerances."""
        from .ops import of_consistency
        c = consistency if isinstance(consistency, L.OFConsistency) else of_consistency(consistency)
        L.check(L.lib().roft_engine_enable_flow_consistency(self._h, None if c is None else C.byref(c)))

    def flow_stats(self):
        """images / image_bytes taken in, pyramids built, pairs (flows) produced since the engine was created."""
        return self._read_stats(L.lib().roft_engine_get_flow_stats, L.EngineFlowStats)

    def produced_flow(self, obj):
        """The flow the engine produced for object `obj`'s last stepped frame, in the engine's flow type: float32 [H, W, 2] or
        int16 [H / 4, W / 4, 2].  Syncs; raises when that frame had none."""
        g = self.cfg.flow_grid
        out = np.zeros((self.H // g, self.W // g, 2), np.float32 if self.cfg.flow_type == L.FLOW_F32C2 else np.int16)
        L.check(L.lib().roft_engine_get_flow(self._h, obj, out.ctypes.data))
        return out

    def enable_raw_depth(self, scale=0.001, cam=None, R=None, t=None):
        """The frame key `depth` carries the sensor's 16-bit frame ([H, W] uint16, or an address) from now on, for every object:
        the float depth is made on the device (roft_engine_enable_raw_depth).  cam None: the frames are in the engine's camera;
        otherwise cam is the DEPTH camera and P_colour = R P_depth + t (ops.depth_source).  Before the first frame."""
        from .ops import depth_source
        src = depth_source(scale, cam, R, t)
        if cam is None:
            src.cam.width, src.cam.height = self.W, self.H
        L.check(L.lib().roft_engine_enable_raw_depth(self._h, C.byref(src)))

    def depth(self, obj):
        """The float depth [H, W] the engine made for object `obj`'s last stepped frame (raw-depth engines).  Syncs."""
        out = np.zeros((self.H, self.W), np.float32)
        L.check(L.lib().roft_engine_get_depth(self._h, obj, out.ctypes.data))
        return out

    def depth_stats(self):
        """distinct raw images / their uploaded image_bytes taken in, float products made since the engine was created."""
        return self._read_stats(L.lib().roft_engine_get_depth_stats, L.EngineDepthStats)

    def depth_kernel_ms(self):
        """Device time (ms, HIP events) of the depth kernels of the last submit call."""
        ms = C.c_double(0.0)
        L.check(L.lib().roft_debug_depth_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def enable_rectification(self, dist, cam=None):
        """Lens distortion (roft_engine_enable_rectification, include/roft_engine.h section 3g): from now on every frame image --
        depth, mask, label image, camera image -- is the sensor's DISTORTED one and is resampled into the engine's pinhole camera on
        the device.  dist: (k1, k2, p1, p2, k3) in OpenCV's order, or a lens (ops.lens); cam: the sensor's camera (same size as the
        engine's, its intrinsics may differ; None: the engine's).  Frames then bring no `flow` (hand the `image`).  Before the
        first frame."""
        from .ops import lens
        ln = lens(dist) if hasattr(dist, "k1") else lens(self.cfg.cam if cam is None else cam, dist)   # (a lens: L.Lens, or shaped like one)
        L.check(L.lib().roft_engine_enable_rectification(self._h, C.byref(ln)))

    def rectify_stats(self):
        """distinct sources taken in, products made, bytes (sources read + products written) since the engine was created."""
        return self._read_stats(L.lib().roft_engine_get_rectify_stats, L.EngineRectifyStats)

    def rectify_kernel_ms(self):
        """Device time (ms, HIP events) of the rectification launches of the last submit call."""
        ms = C.c_double(0.0)
        L.check(L.lib().roft_debug_rectify_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def enable_quality(self, every=1, depth_tolerance=0.01):
        """Track quality (roft_engine_enable_quality): from now on every frame with frame % every == 0 leaves one record per object
        -- silhouette overlap and depth residual of its final estimate against its own mask and depth.  After enable_log (whose
        capacity is the quality ring's), before the first frame."""
        prm = L.QualityParams(int(every), float(depth_tolerance))
        L.check(L.lib().roft_engine_enable_quality(self._h, C.byref(prm)))

    def quality(self, first, n):
        """The quality records of frames first .. first + n - 1: a structured array [n, n_objects] (ops.QUALITY_DTYPE; frame == -1:
        no record).  ops.quality_overlap(records) forms the intersection over union.  Syncs."""
        from .ops import QUALITY_DTYPE
        out = np.zeros((n, self.n_objects), QUALITY_DTYPE)
        L.check(L.lib().roft_engine_get_quality(self._h, first, n, out.ctypes.data))
        return out

    def quality_kernel_ms(self):
        """Device time (ms, HIP events on its dispatch) of the last quality launch."""
        ms = C.c_double(0.0)
        L.check(L.lib().roft_debug_quality_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def score_hypotheses(self, obj, poses, depth_tolerance=0.01):
        """The track-quality record of each of n candidate poses [n, 7] (x y z, q = w x y z) of object `obj` against its last
        stepped frame -- the mask mask(obj) returns, that frame's float depth, the slot's resident mesh -- in one launch on the
        resident images (roft_engine_score_hypotheses; include/roft_engine.h, section 3j).  Reads engine state, changes none.
        Returns ops.QUALITY_DTYPE[n]; `frame` is the scored frame.  Syncs."""
        from .ops import QUALITY_DTYPE, hypothesis_poses
        poses = hypothesis_poses(poses)
        out = np.zeros(poses.shape[0], QUALITY_DTYPE)
        L.check(L.lib().roft_engine_score_hypotheses(self._h, obj, poses.ctypes.data, poses.shape[0], float(depth_tolerance),
                                                     out.ctypes.data_as(C.POINTER(L.QualityRecord))))
        return out

    def relocalise(self, obj, x, q, depth_tolerance=0.01, **kw):
        """Where is object `obj` instead?  relocalise.compass_search from the pose (x, q) over score_hypotheses on the last stepped
        frame; **kw: its t_step, r_step, rounds, max_halvings.  Returns (x, q, trace).  What to do with the pose is the caller's --
        restart(...) with it is one option."""
        from .relocalise import compass_search
        return compass_search(lambda poses: self.score_hypotheses(obj, poses, depth_tolerance), x, q, **kw)

    def enable_pose_masks(self, obj_ids=None):
        """Masks from poses (roft_engine_enable_pose_masks): the listed objects (None: every object the engine has at its first
        frame) take the silhouette of a delivered pose as the frame's mask wherever the frame brings neither `mask` nor `labels`
        -- on their first frame, without a pose, the silhouette of the pose they were added with.  After the objects are added,
        before the first frame."""
        ids = np.ascontiguousarray([] if obj_ids is None else obj_ids, np.int32).reshape(-1)
        L.check(L.lib().roft_engine_enable_pose_masks(self._h, ids.ctypes.data_as(C.POINTER(C.c_int)) if len(ids) else None, len(ids)))

    def pose_mask_stats(self):
        """silhouettes drawn / frames that had any since the engine was created."""
        return self._read_stats(L.lib().roft_engine_get_pose_mask_stats, L.EnginePoseMaskStats)

    def enable_pose_mask_occlusion(self, scene_of=None):
        """Enrolled objects of one scene hide each other's silhouettes (roft_engine_enable_pose_mask_occlusion): each keeps the
        pixels where it is the nearest surface.  scene_of: a dict object id -> scene, or a sequence whose entry i is the scene of
        object i; None: every enrolled object shares scene 0.  After enable_pose_masks, before the first frame."""
        if scene_of is None:
            L.check(L.lib().roft_engine_enable_pose_mask_occlusion(self._h, None, None, 0))
            return
        pairs = sorted(scene_of.items()) if isinstance(scene_of, dict) else list(enumerate(scene_of))
        if not pairs:
            raise ValueError("scene_of names no object (None: every enrolled object shares scene 0)")
        ids = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        scenes = np.ascontiguousarray([p[1] for p in pairs], np.int32)
        ip = C.POINTER(C.c_int)
        L.check(L.lib().roft_engine_enable_pose_mask_occlusion(self._h, ids.ctypes.data_as(ip), scenes.ctypes.data_as(ip), len(ids)))

    def enable_pose_mask_depth_gate(self, front_tolerance=0.02, behind_tolerance=0.0):
        """Every silhouette the engine draws is compared with the depth of the image its pose was computed on
        (roft_engine_enable_pose_mask_depth_gate; include/roft_engine.h, section 3e): it loses the pixels where the sensor saw
        something more than front_tolerance metres nearer than the rendered surface, or (behind_tolerance > 0) more than
        behind_tolerance farther.  After enable_pose_masks, before the first frame."""
        gate = L.PoseMaskGate(front_tolerance, behind_tolerance)
        L.check(L.lib().roft_engine_enable_pose_mask_depth_gate(self._h, C.byref(gate)))

    def pose_mask_gate_stats(self):
        """dict(gated, emptied, pixels_front, pixels_behind); waits for the batches stepped so far"""
        return self._read_stats(L.lib().roft_engine_get_pose_mask_gate_stats, L.EnginePoseMaskGateStats)

    def pose_mask_occlusion_stats(self):
        """silhouettes resolved / of those hidden entirely / pixels removed, since the engine was created (waits for the device)."""
        return self._read_stats(L.lib().roft_engine_get_pose_mask_occlusion_stats, L.EnginePoseMaskOcclusionStats)

    def pose_mask_kernel_ms(self):
        """Device time (ms, HIP events on its dispatch) of the last silhouette launch."""
        ms = C.c_double(0.0)
        L.check(L.lib().roft_debug_pose_mask_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def retain_frames(self):
        return L.lib().roft_engine_retain_frames(self._h)

    def stats(self):
        return self._read_stats(L.lib().roft_engine_get_stats, L.EngineStats)

    def batch_trace(self, n=64):
        """The engine's record of its last (at most 64) batches, oldest first: scheduling decisions and host times
        (roft_batch_trace in include/roft_engine.h)."""
        arr = (L.BatchTrace * n)()
        got = C.c_int(0)
        L.check(L.lib().roft_engine_get_batch_trace(self._h, arr, n, C.byref(got)))
        return [{k: getattr(arr[i], k) for k, _ in L.BatchTrace._fields_} for i in range(got.value)]

    def step(self):
        L.check(L.lib().roft_step(self._h))

    def sync(self):
        L.check(L.lib().roft_sync(self._h))

    def state(self, obj):
        pose, P, tw, Pv = np.zeros(13), np.zeros((12, 12)), np.zeros(6), np.zeros((6, 6))
        L.check(L.lib().roft_get_state(self._h, obj, pose.ctypes.data, P.ctypes.data, tw.ctypes.data, Pv.ctypes.data))
        return pose, P, tw, Pv

    def outputs(self):
        outs = (L.ObjectOutput * self.n_objects)()
        L.check(L.lib().roft_get_outputs(self._h, outs, self.n_objects))
        return outs

    def mask(self, obj):
        m = np.zeros((self.H, self.W), np.uint8)
        L.check(L.lib().roft_get_mask(self._h, obj, m.ctypes.data))
        return m

    def enable_log(self, n_frames):
        L.check(L.lib().roft_engine_enable_log(self._h, n_frames))

    def get_log(self, first, n):
        outs = (L.ObjectOutput * (n * self.n_objects))()
        L.check(L.lib().roft_engine_get_log(self._h, first, n, outs))
        pose = np.zeros((n, self.n_objects, 13))
        twist = np.zeros((n, self.n_objects, 6))
        npts = np.zeros((n, self.n_objects), np.int64)
        sel = np.zeros((n, self.n_objects), np.int64)
        for f in range(n):
            for o in range(self.n_objects):
                r = outs[f * self.n_objects + o]
                pose[f, o] = r.pose[:]
                twist[f, o] = r.twist[:]
                npts[f, o] = r.n_flow_points
                sel[f, o] = r.outlier_selected
        return pose, twist, npts, sel

    def get_log_rows(self, first, n):
        """[n, n_objects, 19] float64: pose(13) | twist(6) per object-frame, as the reference logs them."""
        rows = np.zeros((n, self.n_objects, 19))
        L.check(L.lib().roft_engine_get_log_rows(self._h, first, n, rows.ctypes.data))
        return rows

    def score_log(self, kind, obj, first, n, ref, points=None, symmetries=None):
        """ADD ('add') / ADD-S ('adi') of object `obj` over the logged frames first .. first + n - 1 against ref [n, 7] (x y z,
        q wxyz), on the device: the estimates are read from the log in place (roft_engine_score_log).  points [P, 3]; None:
        every vertex of the mesh the object was added with.  Returns ndarray[n] (metres).
        kind 'mssd' (metres) / 'mspd' (pixels, the engine's camera): the symmetry-aware scores under the group `symmetries`
        [n_sym, 7] (None: the identity alone), roft_engine_score_log_sym."""
        from .ops import pose_error_kind, symmetry_elements
        ref = np.ascontiguousarray(ref, np.float64).reshape(-1, 7)
        if ref.shape[0] != n:
            raise ValueError("ref must hold one pose per scored frame")
        out = np.zeros(n)
        pts = None if points is None else np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        if pose_error_kind(kind) in (L.POSE_ERROR_MSSD, L.POSE_ERROR_MSPD):
            sym = symmetry_elements(symmetries)
            L.check(L.lib().roft_engine_score_log_sym(self._h, pose_error_kind(kind), obj, first, n, None if pts is None else pts.ctypes.data,
                                                      0 if pts is None else pts.shape[0], ref.ctypes.data, sym.ctypes.data, sym.shape[0],
                                                      out.ctypes.data))
            return out
        if symmetries is not None:
            raise ValueError("symmetries are read by kind 'mssd' / 'mspd' only")
        L.check(L.lib().roft_engine_score_log(self._h, pose_error_kind(kind), obj, first, n, None if pts is None else pts.ctypes.data,
                                              0 if pts is None else pts.shape[0], ref.ctypes.data, out.ctypes.data))
        return out

    def render_log(self, first_frame, n_frames, background=None, gray_background=True, styles=None, outputs=("rgb",),
                   frames_per_call=16):
        """The logged estimates of frames first_frame .. first_frame + n_frames - 1 drawn over the camera frames: get_log_rows
        followed by ops.render_scene over the engine's own meshes, all objects in one scene (object o is instance o).
        background: [H, W, 3] or [n_frames, H, W, 3] uint8 RGB, or None.  Returns the dict of ops.SceneRenderer.render."""
        from .ops import SceneRenderer
        rows = self.get_log_rows(first_frame, n_frames)
        poses = np.ascontiguousarray(rows[:, :, 6:13])
        bg = None if background is None else np.asarray(background, np.uint8)
        per_frame = bg is not None and bg.ndim == 4 and bg.shape[0] != 1
        renderer = SceneRenderer(self.cfg.cam, getattr(self, "_meshes", []), max_frames_per_call=min(max(n_frames, 1), frames_per_call),
                                 device=self.cfg.device)
        parts = []
        try:
            for k in range(0, n_frames, renderer.max_frames_per_call):
                sl = slice(k, min(n_frames, k + renderer.max_frames_per_call))
                parts.append(renderer.render(np.arange(self.n_objects), poses[sl], background=bg[sl] if per_frame else bg,
                                             gray_background=gray_background, styles=styles, outputs=outputs))
        finally:
            renderer.close()
        return {key: np.concatenate([p[key] for p in parts]) for key in outputs}

    def stream(self):
        return L.lib().roft_engine_stream(self._h)

    def enable_timing(self, level=2):
        """0 off, 1 only the flow measurement kernel, 2 every launch group."""
        L.check(L.lib().roft_engine_enable_timing(self._h, int(level)))

    def timing(self):
        n = C.c_int(0)
        names = C.POINTER(C.c_char_p)()
        ms = C.POINTER(C.c_float)()
        launches = C.POINTER(C.c_int)()
        L.check(L.lib().roft_engine_get_timing(self._h, C.byref(n), C.byref(names), C.byref(ms), C.byref(launches)))
        return {names[i].decode(): (ms[i], launches[i]) for i in range(n.value)}

    def close(self):
        if self._h:
            L.lib().roft_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
