"""Drop-ins for the reference's ``demo.infer_fast`` / ``demo.run_demo`` (reference: demo.py:54-136).

``infer_fast`` keeps the reference signature and return convention (heatmaps HxWx19 f32, pafs HxWx38 f32,
scale, pad); the network and the x``upsample_ratio`` bicubic up-sampling run on the GPU.
``run_demo`` runs the same per-frame pipeline without a GUI and yields the poses; with ``fused=True`` it
uses the single fused C-ABI call (no up-sampled maps are materialised).
"""
import numpy as np

from .modules.keypoints import extract_keypoints, group_keypoints
from .modules.pose import Pose, poses_from_arrays, track_poses


class ImageReader(object):
    """The reference's image provider (demo.py:14-30) for baseline JPEG files: iterating yields one cuda uint8 (H, W, 3) BGR
    frame per file name, read by ``datasets.coco.imread`` (a file outside its scope is a ValueError naming the file; an
    unreadable path an OSError).  ``engine``: an ``Engine`` or a net that has one.  ``entropy``: ``"host"`` (the default) or
    ``"device"``, as ``imread`` takes it."""

    def __init__(self, file_names, engine, entropy="host"):
        self._entropy = entropy
        self.file_names = list(file_names)
        self.max_idx = len(self.file_names)
        self._engine = getattr(engine, "engine", engine)

    def __iter__(self):
        self.idx = 0
        return self

    def __next__(self):
        from .datasets.coco import imread
        if self.idx == self.max_idx:
            raise StopIteration
        img = imread(self.file_names[self.idx], self._engine, self._entropy)
        self.idx += 1
        return img


def _prepare(net, img, net_input_height_size, stride, pad_value, img_mean, img_scale):
    """demo.py:55-64 (resize by height, normalize, pad, to tensor) as one GPU kernel: uint8 frame -> cuda tensor.  The tensor never
    leaves infer_fast / run_demo, so it stays on the engine's stream (no hand-over to torch's current stream)."""
    return net.engine.preprocess_u8(img, net_input_height_size, stride, pad_value, img_mean, img_scale, hand_over=False)


def infer_fast(net, img, net_input_height_size, stride, upsample_ratio, cpu,
               pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1/256):
    x, scale, pad = _prepare(net, img, net_input_height_size, stride, pad_value, img_mean, img_scale)
    stages_output = net(x)                       # numpy in -> numpy out; `cpu` is accepted and ignored
    eng = net.engine
    heatmaps = eng.upsample(stages_output[-2], upsample_ratio)[0]
    pafs = eng.upsample(stages_output[-1], upsample_ratio)[0]
    return heatmaps, pafs, scale, pad


def poses_from_entries(pose_entries, all_keypoints, scale, pad, stride=8, upsample_ratio=4):
    """demo.py:101-114: map key-points back to image coordinates and build Pose objects."""
    num_keypoints = Pose.num_kpts
    all_keypoints = np.array(all_keypoints, dtype=np.float64, copy=True).reshape(-1, 4)
    for kpt_id in range(all_keypoints.shape[0]):
        all_keypoints[kpt_id, 0] = (all_keypoints[kpt_id, 0] * stride / upsample_ratio - pad[1]) / scale
        all_keypoints[kpt_id, 1] = (all_keypoints[kpt_id, 1] * stride / upsample_ratio - pad[0]) / scale
    poses = []
    for entry in pose_entries:
        if len(entry) == 0:
            continue
        kp = np.ones((num_keypoints, 2), dtype=np.int32) * -1
        for kpt_id in range(num_keypoints):
            if entry[kpt_id] != -1.0:
                kp[kpt_id, 0] = int(all_keypoints[int(entry[kpt_id]), 0])
                kp[kpt_id, 1] = int(all_keypoints[int(entry[kpt_id]), 1])
        poses.append(Pose(kp, entry[18]))
    return poses


def _overlay_options(overlay):
    """``overlay=True`` or a dict of ``Engine.set_overlay`` keywords (color, box_color, boxes, n_draw_limbs)."""
    opts = dict(overlay) if isinstance(overlay, dict) else {}
    unknown = set(opts) - {"color", "box_color", "boxes", "n_draw_limbs"}
    if unknown:
        raise ValueError("unknown overlay option(s): %s" % ", ".join(sorted(unknown)))
    return opts


def run_demo(net, image_provider, height_size, cpu, track, smooth, fused=False, draw=False, device_tail=False, sigmas=None,
             pipelined=False, overlay=False):
    """Generator over frames: yields (img, current_poses).  No GUI (cv2.imshow/waitKey are out of scope).
    Pose / tracking are COCO-18 (modules/pose.py), as in the reference: an engine with a custom skeleton raises ValueError,
    unless ``device_tail=True`` and ``sigmas`` (K values, as ``Pose.sigmas`` holds them) are given.

    ``device_tail=True`` (needs ``fused=True``) runs demo.py:101-118 on the GPU behind the grouping kernels: the un-map, the
    int32 pose rows, ``track_poses`` and the 1-Euro smoothing.  The yielded ``Pose`` objects are filled from the returned arrays
    (see ``poses_from_arrays``: their ``.filters`` is None, the filter state lives on the device).  Ids start at
    ``Pose.last_id + 1`` and ``Pose.last_id`` is written back after every frame, so code that mixes both paths sees one
    counter.  The engine's tracking setting is switched on for the run and off again when the generator ends.

    ``pipelined=True`` (needs ``device_tail=True``) drives the same loop through ``Engine.pipeline_submit_u8``: one call per
    frame enqueues upload, pre-processing, network, grouping and tail, and frame k + 1 is submitted before frame k is fetched
    (two alternating slots), so the host work of one frame overlaps the GPU work of the next.  The yielded sequence, the ids
    and ``Pose.last_id`` are those of the serial device-tail run.  The provider is read ONE FRAME AHEAD: when frame k is
    yielded, frame k + 1 has already been taken from it — a provider that hands out the same buffer again and again must
    copy.  ``draw=True`` draws on the frame the poses belong to.  When the generator ends or is closed early, the slot still
    in flight is fetched and tracking is switched off.

    ``overlay=True`` (needs ``fused=True, device_tail=True``; or a dict of ``Engine.set_overlay`` keywords) runs demo.py:119-124
    on the GPU: the generator yields ``(annotated_img, poses)``, where the annotated frame is a NEW array holding the skeletons
    blended 0.6 / 0.4 into the frame and one box per pose; the provider's frame is not modified.  Pipelined, the kernels follow
    the pose tail inside the one-call submit and the frame comes back with the slot's results; serial, ``Engine.draw_poses``
    runs them on the fetched rows.  Both give the same frames.  The kernels read the engine's limb table, so ``overlay=True``
    is allowed under a custom skeleton (with ``sigmas``) where ``draw=True`` is not.  ``draw=True`` keeps its meaning: the host
    ``Pose.draw`` into the provider's frame.  The id label (cv2.putText) is not drawn; the ids are in the poses.  The engine's
    overlay setting is switched off again when the generator ends."""
    K = net.engine.skeleton["num_kpt_types"]
    if overlay and not (fused and device_tail):
        raise ValueError("run_demo(overlay=True) needs fused=True and device_tail=True: the overlay kernels draw the device tail's pose rows")
    ov = _overlay_options(overlay) if overlay else None
    if pipelined and not device_tail:
        raise ValueError("run_demo(pipelined=True) needs device_tail=True (and fused=True): the pipelined loop reads its poses from the device tail")
    if device_tail and not fused:
        raise ValueError("run_demo(device_tail=True) needs fused=True: the pose tail runs behind the fused grouping kernels")
    if K != Pose.num_kpts and (draw or not device_tail or sigmas is None):       # (overlay=True is fine: the kernels read the engine's limb table)
        raise ValueError("run_demo draws and tracks COCO poses of %d key-points; the engine's skeleton has %d key-point types "
                         "(use infer_poses / poses_from_maps for custom skeletons, or device_tail=True with sigmas and draw=False)"
                         % (Pose.num_kpts, K))
    if pipelined:
        return _run_demo_pipelined(net, image_provider, height_size, track, smooth, draw, sigmas, ov)
    if device_tail:
        return _run_demo_device(net, image_provider, height_size, track, smooth, draw, sigmas, ov)
    return _run_demo(net, image_provider, height_size, cpu, track, smooth, fused, draw)


def _run_demo_device(net, image_provider, height_size, track, smooth, draw, sigmas, ov=None):
    net = net.eval()
    eng = net.engine
    stride, upsample_ratio = 8, 4
    if sigmas is None:
        sigmas = Pose.sigmas
    eng.set_tracking(eng.TRACK_LANES if track else eng.TRACK_ROWS, smooth=smooth, sigmas=sigmas)
    try:
        if ov is not None:
            eng.set_overlay(eng.OVERLAY_OFF, **ov)       # the serial loop draws with draw_poses: only the options are set
        if track:
            eng.reset_tracking(0, Pose.last_id + 1)
        for img in image_provider:
            x, scale, pad = _prepare(net, img, height_size, stride, (0, 0, 0), (128, 128, 128), 1 / 256)
            eng.set_unmap(stride, scale, pad)
            eng.infer_poses(x, upsample_ratio, demo=True)
            rows = eng.poses()[0]
            current_poses = poses_from_arrays(rows["keypoints"], rows["confidence"], rows["bbox"], rows["ids"] if track else None)
            if track:
                Pose.last_id = rows["last_id"]
            if draw:
                for pose in current_poses:
                    pose.draw(img)
            if ov is not None:
                yield eng.draw_poses(img, rows["keypoints"], rows["bbox"], device_out=False), current_poses
            else:
                yield img, current_poses
    finally:
        try:
            if ov is not None:
                eng.set_overlay(eng.OVERLAY_OFF)
        finally:
            eng.set_tracking(eng.TRACK_OFF)


def _drain(eng, in_flight, overlay=False):
    """The end of a pipelined loop: every slot still in flight is fetched and tracking (and the overlay) is switched off.  An
    error of such a fetch is not lost: all slots are tried, tracking is switched off, and then the first error is raised."""
    first = None
    while in_flight:
        _, slot = in_flight.pop(0)
        try:
            eng.pipeline_fetch(slot)
        except Exception as e:
            if first is None:
                first = e
    try:
        if overlay:
            eng.set_overlay(eng.OVERLAY_OFF)
    finally:
        try:
            eng.set_tracking(eng.TRACK_OFF)
        finally:
            if first is not None:
                raise first


def _run_demo_pipelined(net, image_provider, height_size, track, smooth, draw, sigmas, ov=None):
    net = net.eval()
    eng = net.engine
    stride, upsample_ratio = 8, 4
    if sigmas is None:
        sigmas = Pose.sigmas
    eng.set_tracking(eng.TRACK_LANES if track else eng.TRACK_ROWS, smooth=smooth, sigmas=sigmas)
    in_flight = []                                   # [(img, slot)], oldest first: at most two

    def finish():
        img, slot = in_flight.pop(0)
        eng.pipeline_fetch(slot)
        rows = eng.poses(slot)[0]
        current_poses = poses_from_arrays(rows["keypoints"], rows["confidence"], rows["bbox"], rows["ids"] if track else None)
        if track:
            Pose.last_id = rows["last_id"]
        if draw:
            for pose in current_poses:
                pose.draw(img)
        if ov is not None:
            return eng.pipeline_overlay(slot)[0], current_poses
        return img, current_poses

    try:
        if ov is not None:
            eng.set_overlay(eng.OVERLAY_HOST, **ov)
        if track:
            eng.reset_tracking(0, Pose.last_id + 1)
        k = 0
        for img in image_provider:
            eng.pipeline_submit_u8(img, k % 2, height_size, stride, upsample_ratio=upsample_ratio, demo=True)
            in_flight.append((img, k % 2))
            k += 1
            if len(in_flight) == 2:
                yield finish()
        while in_flight:
            yield finish()
    finally:
        _drain(eng, in_flight, ov is not None)       # closed early (or an error): no slot stays pending


def run_cameras(net, providers, height_size, track, smooth, sigmas=None, overlay=False):
    """N same-sized camera streams, one batch per step: yields a list of N (img, poses) per step and stops when the first
    provider ends.  Frame f of every batch is lane f of the device tail (``Engine.TRACK_LANES``): each stream is tracked on its
    own, with its own ids, and the results of stream f are those of ``run_demo(..., fused=True, device_tail=True)`` over
    provider f alone — at the same number of frames per network pass: the fp32 network picks its kernels by the batch of a
    pass, so a ``confidence`` (a sum of float32 map values) of a batch-N step may differ from the batch-1 run's in its last
    bits (1e-6 level), while an engine that walks the batch one frame per pass gives the single-stream bits throughout.
    Every lane gives out ids from ``Pose.last_id + 1`` on; ``Pose.last_id`` itself is left alone (the ids
    are per lane, there is no single counter to write back).  Pipelined like ``run_demo(pipelined=True)``: the providers are read
    one step ahead.  The arguments are checked at the call (ValueError), like ``run_demo``'s; a mismatch of frame sizes shows
    at the step that meets it.  ``overlay=True`` (or a dict of ``Engine.set_overlay`` keywords): every yielded ``img`` is the
    annotated frame of that stream (a new array; the providers' frames are untouched), as ``run_demo(overlay=True)`` yields it."""
    net = net.eval()
    eng = net.engine
    stride, upsample_ratio = 8, 4
    K = eng.skeleton["num_kpt_types"]
    if K != Pose.num_kpts and sigmas is None:
        raise ValueError("run_cameras tracks COCO poses of %d key-points; the engine's skeleton has %d key-point types (give sigmas)"
                         % (Pose.num_kpts, K))
    if sigmas is None:
        sigmas = Pose.sigmas
    providers = [iter(p) for p in providers]
    if not providers:
        raise ValueError("run_cameras needs at least one provider")
    ov = _overlay_options(overlay) if overlay else None
    return _run_cameras(eng, providers, height_size, track, smooth, sigmas, stride, upsample_ratio, ov)


def _run_cameras(eng, providers, height_size, track, smooth, sigmas, stride, upsample_ratio, ov=None):
    eng.set_tracking(eng.TRACK_LANES if track else eng.TRACK_ROWS, smooth=smooth, sigmas=sigmas)
    in_flight = []

    def finish():
        imgs, slot = in_flight.pop(0)
        eng.pipeline_fetch(slot)
        if ov is not None:
            imgs = list(eng.pipeline_overlay(slot))
        return [(img, poses_from_arrays(r["keypoints"], r["confidence"], r["bbox"], r["ids"] if track else None))
                for img, r in zip(imgs, eng.poses(slot))]

    try:
        if ov is not None:
            eng.set_overlay(eng.OVERLAY_HOST, **ov)
        if track:
            eng.reset_tracking(-1, Pose.last_id + 1)
        k = 0
        while True:
            imgs = []
            for p in providers:
                try:
                    imgs.append(next(p))
                except StopIteration:
                    break
            if len(imgs) < len(providers):
                break
            shapes = set(np.shape(i) for i in imgs)
            if len(shapes) != 1:
                raise ValueError("run_cameras needs same-sized frames, got %s" % sorted(shapes))
            eng.pipeline_submit_u8(np.stack(imgs), k % 2, height_size, stride, upsample_ratio=upsample_ratio, demo=True)
            in_flight.append((imgs, k % 2))
            k += 1
            if len(in_flight) == 2:
                yield finish()
        while in_flight:
            yield finish()
    finally:
        _drain(eng, in_flight, ov is not None)


def _run_demo(net, image_provider, height_size, cpu, track, smooth, fused, draw):
    net = net.eval()
    stride, upsample_ratio = 8, 4
    previous_poses = []
    for img in image_provider:
        if fused:
            x, scale, pad = _prepare(net, img, height_size, stride, (0, 0, 0), (128, 128, 128), 1 / 256)
            pose_entries, all_keypoints, _ = net.engine.infer_poses(x, upsample_ratio, demo=True)[0]
        else:
            heatmaps, pafs, scale, pad = infer_fast(net, img, height_size, stride, upsample_ratio, cpu)
            total, by_type = 0, []
            for kpt_idx in range(Pose.num_kpts):      # the 19th map is background
                total += extract_keypoints(heatmaps[:, :, kpt_idx], by_type, total, engine=net.engine)
            pose_entries, all_keypoints = group_keypoints(by_type, pafs, demo=True, engine=net.engine)
        current_poses = poses_from_entries(pose_entries, all_keypoints, scale, pad, stride, upsample_ratio)
        if track:
            track_poses(previous_poses, current_poses, smooth=smooth)
            previous_poses = current_poses
        if draw:
            for pose in current_poses:
                pose.draw(img)
        yield img, current_poses
