"""Drop-ins for the reference's ``demo.infer_fast`` / ``demo.run_demo`` (reference: demo.py:54-136).

``infer_fast`` keeps the reference signature and return convention (heatmaps HxWx19 f32, pafs HxWx38 f32,
scale, pad); the network and the x``upsample_ratio`` bicubic up-sampling run on the GPU.
``run_demo`` runs the same per-frame pipeline without a GUI and yields the poses; with ``fused=True`` it
uses the single fused C-ABI call (no up-sampled maps are materialised).
"""
import os

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
    """``overlay=True`` or a dict of ``Engine.set_overlay`` keywords (color, box_color, boxes, n_draw_limbs) and ``device``
    (True: the annotated frame is yielded as a cuda tensor and never copied to the host).  Returns (keywords, device)."""
    opts = dict(overlay) if isinstance(overlay, dict) else {}
    unknown = set(opts) - {"color", "box_color", "boxes", "n_draw_limbs", "device"}
    if unknown:
        raise ValueError("unknown overlay option(s): %s" % ", ".join(sorted(unknown)))
    return opts, bool(opts.pop("device", False))


def run_demo(net, image_provider, height_size, cpu, track, smooth, fused=False, draw=False, device_tail=False, sigmas=None,
             pipelined=False, overlay=False):
    """Generator over frames: yields (img, current_poses).  No GUI (cv2.imshow/waitKey are out of scope): write the frames with
    ``VideoWriter`` / ``datasets.coco.imwrite`` instead, as ``python -m lwpose_amd.demo --output`` does.
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
    is allowed under a custom skeleton (with ``sigmas``) where ``draw=True`` is not.  With ``overlay={"device": True}`` the
    annotated frame is a cuda uint8 (H, W, 3) tensor instead (overlay mode 1: it is never copied to the host; feed it to
    ``VideoWriter`` or ``Engine.encode_jpeg_batch``); the default stays the NumPy array.  ``draw=True`` keeps its meaning: the host
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
            eng.set_overlay(eng.OVERLAY_OFF, **ov[0])    # the serial loop draws with draw_poses: only the options are set
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
                yield eng.draw_poses(img, rows["keypoints"], rows["bbox"], device_out=ov[1]), current_poses
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
            return eng.pipeline_overlay(slot, device=ov[1])[0], current_poses
        return img, current_poses

    try:
        if ov is not None:
            eng.set_overlay(eng.OVERLAY_DEVICE if ov[1] else eng.OVERLAY_HOST, **ov[0])
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
    annotated frame of that stream (a new array; the providers' frames are untouched), as ``run_demo(overlay=True)`` yields it;
    with ``"device": True`` in the dict, a cuda tensor that never crosses to the host."""
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
            imgs = list(eng.pipeline_overlay(slot, device=ov[1]))
        return [(img, poses_from_arrays(r["keypoints"], r["confidence"], r["bbox"], r["ids"] if track else None))
                for img, r in zip(imgs, eng.poses(slot))]

    try:
        if ov is not None:
            eng.set_overlay(eng.OVERLAY_DEVICE if ov[1] else eng.OVERLAY_HOST, **ov[0])
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


# ---------------------------------------------------------------------------------------------- Motion-JPEG in and out
_AVIIF_KEYFRAME, _AVIF_HASINDEX = 0x10, 0x10
_DHT = []


def _standard_dht():
    """Annex K's four DHT segments as a full file carries them, read from the library's own header bytes (no GPU)."""
    if not _DHT:
        from .runtime import Engine
        hd = Engine.debug_jpeg_encode_header(8, 8)
        first = hd.index(b"\xff\xc4")
        last = hd.index(b"\xff\xdd") if b"\xff\xdd" in hd[first:] else hd.index(b"\xff\xda", first)
        _DHT.append(hd[first:last])
    return _DHT[0]


def _jpeg_frame_end(data, pos):
    """The offset behind the EOI of the JPEG file that starts at ``pos``; ValueError for a stream that is none or is cut off.
    The segments in front of the scan are walked by their lengths (a thumbnail's EOI inside an APPn is not the frame's); in
    the scan every FF is followed by 00, RSTn or a fill FF, so the first FF D9 behind SOS is the frame's own."""
    n = len(data)
    if data[pos:pos + 2] != b"\xff\xd8":
        raise ValueError("no SOI marker at byte %d: not a Motion-JPEG stream" % pos)
    at = pos + 2
    while True:
        while at < n and data[at] == 0xFF and at + 1 < n and data[at + 1] == 0xFF:
            at += 1
        if at + 4 > n or data[at] != 0xFF:
            raise ValueError("the JPEG frame at byte %d is cut off or malformed" % pos)
        marker = data[at + 1]
        at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
        if marker == 0xDA:
            break
    end = data.find(b"\xff\xd9", at)
    if end < 0:
        raise ValueError("the JPEG frame at byte %d has no EOI" % pos)
    return end + 2


def _prepare_frame(data, index):
    """A frame as ``decode_jpeg_batch`` takes it: Annex K's tables are spliced in front of SOS where the frame carries no DHT
    segment (common in camera Motion-JPEG); an interlaced ``AVI1`` field is a ValueError.  The decoder's own refusals stay."""
    n, at, has_dht = len(data), 2, False
    if data[:2] != b"\xff\xd8":
        raise ValueError("frame %d: no SOI marker: not a JPEG frame" % index)
    while at + 4 <= n and data[at] == 0xFF:
        if data[at + 1] == 0xFF:
            at += 1
            continue
        marker, size = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        if marker == 0xE0 and data[at + 4:at + 8] == b"AVI1" and size >= 7 and data[at + 8] != 0:
            raise ValueError("frame %d: an interlaced AVI1 field (polarity %d): field pairs are out of scope" % (index, data[at + 8]))
        if marker == 0xC4:
            has_dht = True
        if marker == 0xDA:
            return data if has_dht else data[:at] + _standard_dht() + data[at:]
        at += 2 + size
    return data                                      # no scan header: the decoder names what is wrong


class VideoReader(object):
    """The reference's video provider (demo.py:33-51) for the two containers ``VideoWriter`` writes: iterating yields one cuda
    uint8 (H, W, 3) BGR frame at a time, decoded ``batch`` files at a time by ``Engine.decode_jpeg_batch``.

    ``file_name``: the path of a RIFF AVI whose first video stream is Motion-JPEG, or of a ``.mjpeg`` / ``.mjpg`` file of
    concatenated JPEG frames (told apart by their first bytes); ``bytes`` are taken as the file's content.  In an AVI the first
    ``vids`` stream is read: ``movi`` is walked chunk by chunk, ``LIST rec `` is followed, odd chunk lengths are padded, the chunks
    of other streams and ``JUNK`` are skipped, and a zero-length (dropped) frame repeats the frame before it.  No index is
    needed or read.  A frame without a DHT segment gets Annex K's tables.  As in the reference, the file is opened when the
    iteration starts: an unreadable path is an OSError there; a camera index (an ``int``, or a string of digits), a handler
    other than MJPG, an OpenDML (``AVIX``) file and interlaced ``AVI1`` field pairs are a ValueError that says so.  Other AVI
    players' files beyond these rules are not pinned.  ``engine``: an ``Engine`` or a net that has one; ``entropy`` as
    ``decode_jpeg_batch`` takes it."""

    def __init__(self, file_name, engine, batch=1, entropy="host"):
        if isinstance(file_name, int) or (isinstance(file_name, str) and file_name.strip().lstrip("-").isdigit()):
            raise ValueError("VideoReader reads Motion-JPEG files: a camera index (%r) needs a capture device, which is out of scope" % (file_name,))
        if int(batch) < 1:
            raise ValueError("batch must be at least 1, not %r" % (batch,))
        self.file_name = file_name
        self.batch = int(batch)
        self._engine = getattr(engine, "engine", engine)
        self._entropy = entropy
        self.fps = None

    # -- containers
    def _avi_frames(self, data):
        """[(offset, length)] of the first video stream's chunks in file order; length 0: a dropped frame."""
        n = len(data)

        def chunks(start, end):
            at = start
            while at + 8 <= end:
                fourcc, size = bytes(data[at:at + 4]), int.from_bytes(data[at + 4:at + 8], "little")
                if at + 8 + size > n:
                    raise ValueError("the %r chunk at byte %d runs past the end of the file (truncated)" % (fourcc, at))
                yield fourcc, at + 8, size
                at += 8 + size + (size & 1)

        if data[8:12] == b"AVIX":
            raise ValueError("an OpenDML (AVIX) file is out of scope")
        riff_end = min(n, 8 + int.from_bytes(data[4:8], "little"))
        if data[riff_end + (riff_end & 1):][:4] == b"RIFF" and data[riff_end + (riff_end & 1) + 8:][:4] == b"AVIX":
            raise ValueError("an OpenDML file (a RIFF AVIX chunk follows the first 2 GiB) is out of scope")
        stream, streams, movi = None, 0, None
        for fourcc, at, size in chunks(12, riff_end):
            if fourcc != b"LIST":
                continue
            kind = bytes(data[at:at + 4])
            if kind == b"hdrl":
                for f2, a2, s2 in chunks(at + 4, at + size):
                    if f2 == b"avih" and s2 >= 4:
                        us = int.from_bytes(data[a2:a2 + 4], "little")
                        self.fps = 1e6 / us if us else None
                    if f2 != b"LIST" or bytes(data[a2:a2 + 4]) != b"strl":
                        continue
                    strh = strf = None
                    for f3, a3, s3 in chunks(a2 + 4, a2 + s2):
                        if f3 == b"strh":
                            strh = bytes(data[a3:a3 + s3])
                        elif f3 == b"strf":
                            strf = bytes(data[a3:a3 + s3])
                    if strh is not None and strh[:4] == b"vids" and stream is None:
                        handler = strf[16:20] if strf is not None and len(strf) >= 20 else strh[4:8]
                        if handler.upper() != b"MJPG" and strh[4:8].upper() != b"MJPG":
                            raise ValueError("the video stream's handler is %r: only Motion-JPEG (MJPG) is read" % (handler,))
                        stream = streams
                        if len(strh) >= 28:
                            scale, rate = int.from_bytes(strh[20:24], "little"), int.from_bytes(strh[24:28], "little")
                            if scale and rate:
                                self.fps = rate / scale
                    streams += 1
            elif kind == b"movi":
                movi = (at + 4, at + size)
        if stream is None:
            raise ValueError("the AVI file has no video stream")
        if movi is None:
            raise ValueError("the AVI file has no movi list")
        ids = (b"%02ddc" % stream, b"%02ddb" % stream)
        frames = []

        def walk(start, end):
            for fourcc, at, size in chunks(start, end):
                if fourcc == b"LIST":
                    if bytes(data[at:at + 4]) == b"rec ":
                        walk(at + 4, at + size)
                elif fourcc in ids:
                    frames.append((at, size))
        walk(*movi)
        return frames

    def _mjpeg_frames(self, data):
        frames, at, n = [], 0, len(data)
        while at < n:
            end = _jpeg_frame_end(data, at)
            frames.append((at, end - at))
            at = end
        return frames

    def __iter__(self):
        if isinstance(self.file_name, (bytes, bytearray, memoryview)):
            data = bytes(self.file_name)
        else:
            with open(self.file_name, "rb") as f:
                data = f.read()
        if data[:4] == b"RIFF" and data[8:12] in (b"AVI ", b"AVIX"):
            self._frames = self._avi_frames(data)
        elif data[:2] == b"\xff\xd8":
            self._frames = self._mjpeg_frames(data)
        else:
            raise ValueError("%s is neither a RIFF AVI nor a stream of JPEG frames" % (self._name(),))
        self._data, self._next, self._ready, self._last = data, 0, [], None
        return self

    def _name(self):
        return "<bytes>" if isinstance(self.file_name, (bytes, bytearray, memoryview)) else str(self.file_name)

    def __next__(self):
        if not self._ready:
            if self._next >= len(self._frames):
                raise StopIteration
            take = self._frames[self._next:self._next + self.batch]
            files = [_prepare_frame(self._data[at:at + size], self._next + k) for k, (at, size) in enumerate(take) if size]
            try:
                decoded = iter(self._engine.decode_jpeg_batch(files, entropy=self._entropy) if files else [])
            except ValueError as e:
                raise ValueError("%s, frames %d..%d: %s" % (self._name(), self._next, self._next + len(take) - 1, e)) from None
            for at, size in take:
                if size:
                    self._last = next(decoded)
                if self._last is not None:             # a dropped frame repeats the one before it (none before the first)
                    self._ready.append(self._last)
            self._next += len(take)
            if not self._ready:
                return self.__next__()
        return self._ready.pop(0)


class VideoWriter(object):
    """Annotated frames to a Motion-JPEG file, encoded on the GPU by ``Engine.encode_jpeg_batch`` (a ``cv2.VideoWriter`` with
    fourcc MJPG in its place): only compressed bytes cross to the host.

    ``path`` ending in ``.avi``: a RIFF AVI with one ``vids`` / ``MJPG`` stream (``avih``, ``strh``, a 40-byte BITMAPINFOHEADER
    with biCompression MJPG, ``00dc`` chunks padded to even length in ``LIST movi``, an ``idx1`` of key-frame entries whose
    offsets count from the ``movi`` four-cc); the sizes and frame counts of the headers are patched by ``close()``.  Ending in
    ``.mjpeg`` / ``.mjpg``: the JPEG files back to back.  ``path`` may be a seekable binary file object with ``container``
    ("avi" or "mjpeg") given.  ``write`` takes one (H, W, 3) uint8 BGR frame or a batch (N, H, W, 3) / a list, arrays or cuda
    tensors; all frames of a file have one size (ValueError).  A file never passes ``max_bytes`` (2^31 - 1, the reach of the
    AVI's 32-bit sizes that every player accepts): the ``write`` that would pass it closes the file properly, index and all,
    without that frame, and raises OverflowError; every ``write`` after a close raises ValueError.  Use as a context manager or
    call ``close()``.  What other AVI players make of the file is not pinned: ``VideoReader`` reads it back."""

    max_bytes = 2 ** 31 - 1

    def __init__(self, path, engine, fps=30, quality=75, subsampling="4:2:0", container=None):
        if container is None:
            ext = os.path.splitext(str(path))[1].lower() if isinstance(path, (str, os.PathLike)) else ""
            container = {".avi": "avi", ".mjpeg": "mjpeg", ".mjpg": "mjpeg"}.get(ext)
        if container not in ("avi", "mjpeg"):
            raise ValueError("VideoWriter writes .avi, .mjpeg and .mjpg files (or container='avi' | 'mjpeg'), not %r" % (path,))
        if not fps > 0:
            raise ValueError("fps must be positive, not %r" % (fps,))
        self._engine = getattr(engine, "engine", engine)
        self._engine._jpeg_encode_options(quality, subsampling, 0)          # ValueError now, not at the first frame
        self.container, self.fps, self.quality, self.subsampling = container, fps, quality, subsampling
        self._own = isinstance(path, (str, os.PathLike))
        self._f = open(path, "wb") if self._own else path
        self._base = 0 if self._own else self._f.tell()
        self.frames, self.size = 0, None
        self._index, self._pos, self._largest, self._closed = [], 0, 0, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _rate(self):
        return (int(self.fps), 1) if float(self.fps).is_integer() else (int(round(self.fps * 1000)), 1000)

    def _header(self, width, height):
        """RIFF 'AVI ' up to and including the movi four-cc; the offsets of the fields close() patches."""
        import struct
        rate, scale = self._rate()
        avih = struct.pack("<14I", int(round(1e6 * scale / rate)), 0, 0, _AVIF_HASINDEX, 0, 0, 1, 0, width, height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, 0, 0, 0xFFFFFFFF, 0, 0, 0, width, height)
        strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF\0\0\0\0AVI " + hdrl + b"LIST\0\0\0\0movi"
        self._at = {"riff": 4, "avih": 12 + 12 + 8, "strh": 12 + 12 + 8 + len(avih) + 12 + 8, "movi_size": len(head) - 8, "movi": len(head) - 4}
        return head

    def _put(self, data):
        self._f.write(data)
        self._pos += len(data)

    def _frame_list(self, frames):
        if isinstance(frames, (list, tuple)):
            return list(frames)
        if getattr(frames, "ndim", 0) == 4:
            return [frames[i] for i in range(frames.shape[0])]
        return [frames]

    def write(self, frame_or_batch):
        if self._closed:
            raise ValueError("write to a closed VideoWriter")
        frames = self._frame_list(frame_or_batch)
        for f in frames:
            size = (int(f.shape[0]), int(f.shape[1])) if getattr(f, "ndim", 0) == 3 else None
            if size is None or f.shape[2] != 3:
                raise ValueError("a frame must be (H, W, 3), not %s" % (tuple(getattr(f, "shape", ())),))
            if self.size is None:
                self.size = size
            if size != self.size:
                raise ValueError("all frames of a file have one size: %d x %d, then %d x %d" % (self.size + size))
        for data in self._engine.encode_jpeg_batch(frames, quality=self.quality, subsampling=self.subsampling):
            if self.container == "avi":
                if self.frames == 0:
                    self._put(self._header(self.size[1], self.size[0]))
                need = 8 + len(data) + (len(data) & 1) + 8 + 16 * (self.frames + 1)          # the chunk, then idx1 with one entry more
            else:
                need = len(data)
            if self._pos + need > self.max_bytes:
                self.close()
                raise OverflowError("the file would pass %d bytes: closed with %d frames" % (self.max_bytes, self.frames))
            if self.container == "avi":
                self._index.append((self._pos - self._at["movi"], len(data)))
                self._put(b"00dc" + len(data).to_bytes(4, "little") + data + (b"\0" if len(data) & 1 else b""))
            else:
                self._put(data)
            self._largest = max(self._largest, len(data))
            self.frames += 1

    def close(self):
        if self._closed:
            return
        self._closed = True
        try:
            if self.container == "avi":
                import struct
                if self.frames == 0:
                    self._put(self._header(0, 0))
                movi_end = self._pos
                self._put(b"idx1" + struct.pack("<I", 16 * len(self._index)) +
                          b"".join(b"00dc" + struct.pack("<III", _AVIIF_KEYFRAME, off, size) for off, size in self._index))
                rate, scale = self._rate()
                patches = [(self._at["riff"], self._pos - 8), (self._at["movi_size"], movi_end - self._at["movi"]),
                           (self._at["avih"] + 4, int(self._largest * rate / scale)), (self._at["avih"] + 16, self.frames),
                           (self._at["avih"] + 28, self._largest), (self._at["strh"] + 32, self.frames), (self._at["strh"] + 36, self._largest)]
                for at, value in patches:
                    self._f.seek(self._base + at)
                    self._f.write(struct.pack("<I", value))
                self._f.seek(self._base + self._pos)
        finally:
            if self._own:
                self._f.close()


def main(argv=None):
    """``python -m lwpose_amd.demo``: the reference's demo flags (demo.py:139-166) around the pipelined, device-tail, overlay loop.
    With ``--output`` every annotated frame is written (a Motion-JPEG file for ``--video``, numbered .jpg files in a folder for
    ``--images``) without its pixels crossing to the host; without it one line per frame is printed (index, pose count, ids)."""
    import argparse
    import torch
    from .datasets.coco import imwrite
    from .models.with_mobilenet import PoseEstimationWithMobileNet
    from .modules.load_state import load_state
    parser = argparse.ArgumentParser(prog="python -m lwpose_amd.demo", description="Pose estimation demo without a GUI: annotated frames go to --output.")
    parser.add_argument("--checkpoint-path", type=str, required=True, help="path to the checkpoint")
    parser.add_argument("--height-size", type=int, default=256, help="network input layer height size")
    parser.add_argument("--video", type=str, default="", help="path to a Motion-JPEG .avi / .mjpeg file")
    parser.add_argument("--images", nargs="+", default="", help="path to input image(s) (baseline JPEG)")
    parser.add_argument("--cpu", action="store_true", help="accepted and ignored: the network runs on the GPU")
    parser.add_argument("--track", type=int, default=1, help="track pose id in video")
    parser.add_argument("--smooth", type=int, default=1, help="smooth pose keypoints")
    parser.add_argument("--output", type=str, default="", help="an .avi / .mjpeg file for --video, a folder for --images")
    parser.add_argument("--quality", type=int, default=None, help="JPEG quality of --output, 1..100 (video: 75, images: 95)")
    args = parser.parse_args(argv)
    if args.video == "" and args.images == "":
        raise ValueError("Either --video or --images has to be provided")
    net = PoseEstimationWithMobileNet()
    load_state(net, torch.load(args.checkpoint_path, map_location="cpu"))
    net = net.eval().cuda()
    if args.video != "":
        provider = VideoReader(args.video, net)
    else:
        provider = ImageReader(args.images, net)
        args.track = 0
    overlay = {"device": True} if args.output else False
    frames = run_demo(net, provider, args.height_size, args.cpu, args.track, args.smooth, fused=True, device_tail=True, pipelined=True,
                      overlay=overlay)
    writer = None
    if args.output and args.video == "":
        os.makedirs(args.output, exist_ok=True)
    try:
        for k, (img, poses) in enumerate(frames):
            if args.output and args.video != "":
                if writer is None:                   # the reader has parsed its header by now: the writer repeats the source's frame rate
                    writer = VideoWriter(args.output, net, fps=provider.fps or 30, quality=75 if args.quality is None else args.quality)
                writer.write(img)
            elif args.output:
                imwrite(os.path.join(args.output, "%06d.jpg" % k), img, net, quality=95 if args.quality is None else args.quality)
            else:
                print("%d %d %s" % (k, len(poses), " ".join(str(p.id) for p in poses)), flush=True)
    finally:
        if writer is not None:
            writer.close()
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
