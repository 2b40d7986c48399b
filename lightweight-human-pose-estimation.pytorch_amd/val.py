"""Drop-ins for the reference's ``val`` helpers (reference: val.py:30-147): ``normalize`` / ``pad_width`` (host, for callers
that use them directly), the multi-scale driver ``infer`` (all of it on the GPU), ``convert_to_coco_format``, the
detection loop, and ``evaluate`` with the detections resident on the device.

OpenCV is not a dependency: ``cv2.copyMakeBorder(BORDER_CONSTANT)`` is a constant fill + copy.  The cubic resizes
(uint8 fixed point of demo.py:59, float64 of val.py:89, float32 of val.py:98-107) run on the GPU with OpenCV's published
algorithms — unpinned against cv2 itself, which is absent from the build container.
"""
import math

import numpy as np


def normalize(img, img_mean, img_scale):
    # float32 image minus an integer tuple promotes to float64 under NumPy 2, exactly like the reference
    return (np.array(img, dtype=np.float32) - img_mean) * img_scale


def pad_width(img, stride, pad_value, min_dims):
    """Centre-pad ``img`` to (min_dims rounded up to ``stride``); returns (padded, [top, left, bottom, right]).
    Mutates ``min_dims`` like the reference (val.py:39-41)."""
    h, w, _ = img.shape
    h = min(min_dims[0], h)
    min_dims[0] = math.ceil(min_dims[0] / float(stride)) * stride
    min_dims[1] = math.ceil(max(min_dims[1], w) / float(stride)) * stride
    top = int(math.floor((min_dims[0] - h) / 2.0))
    left = int(math.floor((min_dims[1] - w) / 2.0))
    pad = [top, left, int(min_dims[0] - h - top), int(min_dims[1] - w - left)]
    out = np.empty((img.shape[0] + pad[0] + pad[2], w + pad[1] + pad[3], img.shape[2]), dtype=img.dtype)
    out[...] = np.asarray(pad_value, dtype=img.dtype)[:img.shape[2]]
    out[pad[0]:pad[0] + img.shape[0], pad[1]:pad[1] + w] = img
    return out, pad


def _as_frames(imgs):
    """(N, H, W, 3) frames for the device kernels: uint8 stays uint8; any other dtype is cast to float32, which is what the
    reference's normalize does first (np.array(img, dtype=np.float32), val.py:31)."""
    if getattr(imgs, "is_cuda", False):
        import torch
        a = imgs if imgs.dtype in (torch.uint8, torch.float32) else imgs.to(torch.float32)
    else:
        a = np.ascontiguousarray(imgs)
        if a.dtype != np.uint8:
            a = np.ascontiguousarray(a, dtype=np.float32)
    if len(a.shape) != 4 or a.shape[-1] != 3:
        raise TypeError("frames must be (N, H, W, 3)")
    return a


def infer(net, img, scales, base_height, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1/256):
    """Drop-in for the reference's multi-scale ``val.infer`` (val.py:81-110): returns (avg_heatmaps HxWx19,
    avg_pafs HxWx38) float32 at the original image size.  Everything between the uint8 frame and the averaged maps runs
    on the GPU: normalize + per-scale cubic resize + pad (lwp_preprocess_scaled_u8), the network, the per-scale
    up-sample / crop / resize / average (lwp_multiscale_accumulate)."""
    avg_heatmaps, avg_pafs = infer_batch(net, np.asarray(img)[None], scales, base_height, stride, pad_value, img_mean, img_scale)
    return avg_heatmaps[0].cpu().numpy(), avg_pafs[0].cpu().numpy()


def scaled_inputs(net, imgs, scales, base_height, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1/256):
    """Image side of val.py:84-93 for a batch of same-sized frames (numpy or cuda tensor, N x H x W x 3; uint8, or any other
    dtype through float32 like the reference's normalize), on the device:
    per scale the float32 (N,3,H',W') network input (cuda tensor) and its pad [top, left, bottom, right]."""
    imgs = _as_frames(imgs)
    height = int(imgs.shape[1])
    return [net.engine.preprocess_scaled_u8(imgs, scale * base_height / float(height), base_height, stride, pad_value, img_mean, img_scale)
            for scale in scales]


def accumulate_scales(net, inputs, height, width, stride):
    """Device side of val.py:94-108 for a batch: inputs = [(x (N,3,H',W') cuda tensor, pad), ...] -> averaged maps
    (N,height,width,19) and (N,height,width,38) float32 cuda tensors."""
    import torch
    eng = net.engine
    dev = torch.device("cuda", eng.device_id)
    N = int(inputs[0][0].shape[0])
    avg_heatmaps = torch.empty((N, height, width, eng.NH), dtype=torch.float32, device=dev)   # zero-initialised by the first scale
    avg_pafs = torch.empty((N, height, width, eng.NP), dtype=torch.float32, device=dev)
    for k, (x, pad) in enumerate(inputs):
        stages_output = net(x)
        eng.multiscale_accumulate(avg_heatmaps, stages_output[-2], stride, pad, len(inputs), init=(k == 0))
        eng.multiscale_accumulate(avg_pafs, stages_output[-1], stride, pad, len(inputs), init=(k == 0))
    return avg_heatmaps, avg_pafs


def infer_batch(net, imgs, scales, base_height, stride, pad_value=(0, 0, 0), img_mean=(128, 128, 128), img_scale=1/256):
    """``infer`` (val.py:81-110) for N same-sized uint8 frames at once; returns cuda tensors (N,H,W,19), (N,H,W,38).  A list may
    hold NumPy arrays or cuda tensors (``datasets.coco.imread`` / ``CocoValDataset`` yield those), not a mix."""
    if isinstance(imgs, (list, tuple)) and len(imgs) and all(getattr(a, "is_cuda", False) for a in imgs):
        import torch
        imgs = torch.stack(list(imgs))
    imgs = _as_frames(np.stack(list(imgs)) if isinstance(imgs, (list, tuple)) else imgs)
    inputs = scaled_inputs(net, imgs, scales, base_height, stride, pad_value, img_mean, img_scale)
    return accumulate_scales(net, inputs, int(imgs.shape[1]), int(imgs.shape[2]), stride)


def poses_batch(net, avg_heatmaps, avg_pafs):
    """val.py:129-134 for a batch on the device: extract_keypoints over the engine skeleton's K key-point maps + group_keypoints
    (demo=False rounding) -> per frame (pose_entries (P,E), all_keypoints (n,4), type_counts (K,)); K / E are 18 / 20 unless
    Engine.set_skeleton chose a custom skeleton."""
    return net.engine.poses_from_maps(avg_heatmaps, avg_pafs, 1, demo=False, layout="NHWC")


# ---------------------------------------------------------------------------------------------- label-grounded loss
def stage_losses(net, images, labels, masks=None, stride=8, sigma=7, paf_thickness=1, batch_size=None):
    """The quantity the reference's training minimises (train.py:92-97), measured, not optimised: forward, targets and the
    masked L2 loss of every stage on the GPU in one call.  ``images``: the network input (N, 3, H, W) float32 as
    CocoTrainDataset yields it ((image - 128) / 256, CHW), numpy or torch; ``labels``: one label dict per frame
    (prepare_train_labels.py's format); ``masks``: (N, H, W) float32 or None for all ones.  Returns the 2 * (nref + 1) floats
    [heat0, paf0, heat1, paf1, ...] with batch_size = N unless given.  Works for every engine dtype; no gradients."""
    import torch
    from .datasets.coco import generate_targets
    x = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32)) if isinstance(images, np.ndarray) else images
    eng = net.engine
    x = x.to(torch.device("cuda", eng.device_id))
    outs = net(x)
    t = generate_targets(net, labels, (int(x.shape[2]), int(x.shape[3])), masks, stride, sigma, paf_thickness)
    if tuple(outs[0].shape[2:]) != tuple(t["keypoint_maps"].shape[2:]):
        raise ValueError("the network's maps are %s but the targets %s: the frame size must be a multiple of the stride"
                         % (tuple(outs[0].shape[2:]), tuple(t["keypoint_maps"].shape[2:])))
    return eng.stage_losses(outs, t["keypoint_maps"], t["paf_maps"], t["keypoint_mask"][:, 0], batch_size)


def stage_gradients(net, images, labels, masks=None, stride=8, sigma=7, paf_thickness=1, batch_size=None, loss_scale=1.0, into=None,
                    log_divisor=None):
    """``stage_losses`` plus the gradient of their sum (train.py:99-102, fp32 engines): retaining forward, targets, loss and
    stage backward on the GPU in one call.  Returns (losses, grads, d_features): the 2 * (nref + 1) floats of ``stage_losses``,
    the dict state-dict key -> gradient of every initial_stage.* / refinement_stages.* parameter, and the gradient at the
    cpm output (N, num_channels, h, w).  ``loss_scale`` scales the gradients only (train.py:102's 1 / batches_per_iter);
    ``into``: the flat array of an earlier call to add to.  The backbone is frozen (the cpm too) unless the engine's train scope
    is "cpm" (``grads`` then holds the cpm.* keys as well) or "all" (the model.* keys too), and the BatchNorms stay at their
    running statistics: this is loss.backward() of the reference network in eval() mode.  ``train_step`` adds the optimiser.
    ``log_divisor``: the losses are added to the engine's loss log (``Engine.log_stage_losses``) instead of being fetched,
    and ``losses`` is None."""
    import torch
    from .datasets.coco import generate_targets
    x = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float32)) if isinstance(images, np.ndarray) else images
    eng = net.engine
    x = x.to(torch.device("cuda", eng.device_id)).to(torch.float32).contiguous()
    outs = eng.train_forward(x)
    t = generate_targets(net, labels, (int(x.shape[2]), int(x.shape[3])), masks, stride, sigma, paf_thickness)
    if tuple(outs[0].shape[2:]) != tuple(t["keypoint_maps"].shape[2:]):
        raise ValueError("the network's maps are %s but the targets %s: the frame size must be a multiple of the stride"
                         % (tuple(outs[0].shape[2:]), tuple(t["keypoint_maps"].shape[2:])))
    mask = t["keypoint_mask"][:, 0]
    if log_divisor is None:
        losses = eng.stage_losses(outs, t["keypoint_maps"], t["paf_maps"], mask, batch_size)
    else:
        losses = eng.log_stage_losses(outs, t["keypoint_maps"], t["paf_maps"], mask, batch_size, log_divisor)
    grads, d_features = eng.stage_backward(t["keypoint_maps"], t["paf_maps"], mask, batch_size, loss_scale, into)
    return losses, grads, d_features


def train_step(net, opt, images, labels, masks=None, batches_per_iter=1, stride=8, sigma=7, paf_thickness=1, log=False):
    """One pass of train.py:85-110's loop body for one loader batch, all on the GPU: targets, retaining forward, stage losses,
    stage backward with loss_scale = 1 / batches_per_iter, and, once ``batches_per_iter`` calls have added their gradients,
    ``opt.step`` (an ``optim.StageAdam`` of this net; it is zeroed at the first batch of an iteration, train.py:87-88).
    Returns the batch's stage losses as ``stage_losses`` does.  Only initial_stage.* / refinement_stages.* move, and cpm.* with ``optim.StageAdam(net, scope="cpm")``,
    every parameter with ``scope="all"``.  ``log=True``: the losses, divided by ``batches_per_iter``, are added to the engine's loss
    log on the device (train.py:96-97's total_losses; ``Engine.read_loss_log``); nothing is fetched and the call returns None."""
    if opt.net is not net:
        raise ValueError("opt is not an optimiser of this net")
    batches_per_iter = int(batches_per_iter)
    if batches_per_iter < 1:
        raise ValueError("batches_per_iter must be at least 1")
    if opt.batch_index == 0:
        opt.zero_grad()
    losses, grads, _ = stage_gradients(net, images, labels, masks, stride, sigma, paf_thickness, None, 1.0 / batches_per_iter, opt.accumulated,
                                       float(batches_per_iter) if log else None)
    opt.accumulated = net.engine.flat_of(grads)
    opt.batch_index += 1
    if opt.batch_index >= batches_per_iter:
        opt.step(opt.accumulated)
        opt.batch_index = 0
    return losses


def augmented_train_step(net, opt, samples, augment, batches_per_iter=1, sigma=7, paf_thickness=1, log=False):
    """``train_step`` from RAW samples (image uint8 (H, W, 3), label dict, and a mask float32 (H, W), or ``"segmentations"``,
    the label's crowd RLE dicts, from which the mask is rendered on the device, or neither): ``augment``, a
    ``datasets.transformations.DeviceAugment``, draws the random numbers and moves the labels on the host and renders the
    crops on the GPU; its ``image``, ``kpts`` and ``mask_small`` feed the same targets, retaining forward, losses, backward
    and optimiser step as ``train_step``.  The small mask is the reference's (coco.py:48 on the uint8 mask CropPad leaves,
    rounded to 0 / 1), not the float mean of ``Engine.mask_downsample``.  Returns the batch's stage losses, or with
    ``log=True`` adds them to the engine's loss log as ``train_step`` does and returns None."""
    if opt.net is not net:
        raise ValueError("opt is not an optimiser of this net")
    batches_per_iter = int(batches_per_iter)
    if batches_per_iter < 1:
        raise ValueError("batches_per_iter must be at least 1")
    eng = net.engine
    batch = augment(samples, engine=eng)
    x = batch["image"]
    if opt.batch_index == 0:
        opt.zero_grad()
    outs = eng.train_forward(x)
    kmaps, pmaps = eng.train_targets(batch["kpts"], batch["n_persons"], (int(x.shape[2]), int(x.shape[3])), augment.stride, sigma, paf_thickness)
    if tuple(outs[0].shape[2:]) != tuple(kmaps.shape[2:]):
        raise ValueError("the network's maps are %s but the targets %s: the crop must be a multiple of the network's stride"
                         % (tuple(outs[0].shape[2:]), tuple(kmaps.shape[2:])))
    mask = batch["mask_small"]
    if log:
        losses = eng.log_stage_losses(outs, kmaps, pmaps, mask, None, float(batches_per_iter))
    else:
        losses = eng.stage_losses(outs, kmaps, pmaps, mask, None)
    grads, _ = eng.stage_backward(kmaps, pmaps, mask, None, 1.0 / batches_per_iter, opt.accumulated)
    opt.accumulated = eng.flat_of(grads)
    opt.batch_index += 1
    if opt.batch_index >= batches_per_iter:
        opt.step(opt.accumulated)
        opt.batch_index = 0
    return losses


# ---------------------------------------------------------------------------------------------- COCO results
# slot of each of the 18 network key-points in COCO's 17-key-point order (the neck, index 1, has none)
_COCO_SLOT = (0, None, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3)


def convert_to_coco_format(pose_entries, all_keypoints):
    """Same contract as the reference's val.convert_to_coco_format (val.py:52-78): per pose a flat list of 17 x
    (x + 0.5, y + 0.5, visibility) in COCO order (missing key-points stay 0, 0, 0) and the pose score
    ``entry[18] * max(0, entry[19] - 1)`` (the neck does not count)."""
    coco_keypoints, scores = [], []
    for entry in pose_entries:
        if len(entry) == 0:
            continue
        flat = [0] * (17 * 3)
        for part, slot in enumerate(_COCO_SLOT):
            if slot is None:
                continue
            kpt_id = entry[part]
            if kpt_id != -1:
                cx, cy = all_keypoints[int(kpt_id), 0:2]
                flat[slot * 3:slot * 3 + 3] = [cx + 0.5, cy + 0.5, 1]
        coco_keypoints.append(flat)
        scores.append(entry[-2] * max(0, entry[-1] - 1))
    return coco_keypoints, scores


def coco_detections(net, samples, multiscale=False, base_height=368, stride=8):
    """The detection loop of val.evaluate (val.py:113-147) without the dataset / pycocotools parts: ``samples`` yields
    dicts with 'file_name' ('<image id>.jpg') and 'img' (uint8 HxWx3); returns the list of COCO result dicts."""
    scales = [0.5, 1.0, 1.5, 2.0] if multiscale else [1]
    results = []
    for sample in samples:
        file_name, img = sample['file_name'], sample['img']
        avg_heatmaps, avg_pafs = infer_batch(net, [img], scales, base_height, stride)
        pose_entries, all_keypoints, _ = poses_batch(net, avg_heatmaps, avg_pafs)[0]
        coco_keypoints, scores = convert_to_coco_format(pose_entries, all_keypoints)
        image_id = int(file_name[0:file_name.rfind('.')])
        for keypoints, score in zip(coco_keypoints, scores):
            results.append({'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in keypoints], 'score': float(score)})
    return results


def write_detections(output_name, coco_result):
    import json
    with open(output_name, 'w') as f:
        json.dump(coco_result, f, indent=4)


# ---------------------------------------------------------------------------------------------- COCO evaluation
def _print_summary(stats):
    """COCOeval.summarize()'s ten lines for iouType 'keypoints', in its format."""
    line = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    rows = [(None, 'all'), (.5, 'all'), (.75, 'all'), (None, 'medium'), (None, 'large')]
    for i, stat in enumerate(stats):
        iou, area = rows[i % 5]
        title, kind = ('Average Precision', '(AP)') if i < 5 else ('Average Recall', '(AR)')
        iou_str = '{:0.2f}:{:0.2f}'.format(0.5, 0.95) if iou is None else '{:0.2f}'.format(iou)
        print(line.format(title, kind, iou_str, area, 20, stat))


def evaluate_detections(gt, results, engine=None):
    """``run_coco_eval`` for in-memory data: ``gt`` a COCO ground-truth dict ('images', 'annotations', 'categories'),
    ``results`` the list ``coco_detections`` returns.  OKS, matching and accumulation run on the GPU (``Engine.coco_eval``); the
    ten summarize() numbers are printed and returned.  ValueError: a detection for an image ``gt`` does not list, a
    non-positive annotation id, more than one category."""
    from .runtime import default_engine
    eng = default_engine() if engine is None else engine
    stats = eng.coco_eval(gt, results)["stats"]
    _print_summary(stats)
    return stats


def evaluate(labels, output_name, samples, net, multiscale=False, visualize=False, store=False, base_height=368, stride=8):
    """The reference's val.evaluate (val.py:113-160) with the results resident on the device: per sample ``infer_batch`` and
    ``Engine.coco_add_maps`` are enqueued (the poses go from the grouping's result block into the engine's detection store;
    the host reads nothing in the loop), then ``output_name`` is written from the store's rows, the evaluation runs on the
    store (``Engine.coco_finish``), the reference's lines are printed and the ten stats returned.

    One difference from the reference: the third argument is an iterable of ``{'file_name': '<image id>.jpg', 'img': uint8
    HxWx3}`` samples (NumPy arrays or cuda tensors), not an images folder; ``datasets.coco.CocoValDataset(labels, images_folder,
    engine)`` yields them from a folder of baseline JPEG files.  ``labels``: the ground-truth file's
    path, or the dict itself.  ``output_name`` None: no file is written.  The file holds the list ``coco_detections`` returns
    for the same samples.  ``store=True`` keeps the ground truth and the store on the engine for the next call with the same
    ``labels`` (the same dict object, or the same path; a training run that validates every ``val_after`` iterations);
    otherwise they are released."""
    if isinstance(samples, (str, bytes)):
        raise TypeError("evaluate takes an iterable of {'file_name', 'img'} samples as its third argument, not an images "
                        "folder: datasets.coco.CocoValDataset(labels, images_folder, engine) makes one from a folder")
    if visualize:
        raise NotImplementedError("visualize needs cv2.imshow, which this package does not depend on")
    eng = net.engine
    kept = getattr(eng, "_val_store", None)
    if kept is not None and (kept[0] is labels or (isinstance(labels, str) and kept[0] == labels)):
        packed = kept[1]
        eng.coco_reset()
    else:
        if isinstance(labels, dict):
            gt = labels
        else:
            import json
            with open(labels) as f:
                gt = json.load(f)
        packed = eng.coco_open(gt)
    eng._val_store = None
    try:
        index = {v: i for i, v in enumerate(packed["image_ids"])}
        scales = [0.5, 1.0, 1.5, 2.0] if multiscale else [1]
        order = []
        for sample in samples:
            file_name, img = sample['file_name'], sample['img']
            image_id = int(file_name[0:file_name.rfind('.')])
            if image_id not in index:
                raise ValueError("sample %r: image %d is not in the ground truth" % (file_name, image_id))
            avg_heatmaps, avg_pafs = infer_batch(net, [img], scales, base_height, stride)
            eng.coco_add_maps(avg_heatmaps, avg_pafs, [index[image_id]], 1, demo=False, layout="NHWC")
            order.append(index[image_id])
        if output_name is not None:
            rows = eng.coco_rows()
            first = np.concatenate([[0], np.cumsum(np.bincount(rows["image"], minlength=len(index)))])
            coco_result = []
            for i in order:                            # the file lists the images in sample order, as the reference's loop does
                for r in range(first[i], first[i + 1]):
                    coco_result.append({'image_id': packed["image_ids"][i], 'category_id': 1,
                                        'keypoints': rows["keypoints"][r].reshape(-1).tolist(), 'score': float(rows["score"][r])})
            write_detections(output_name, coco_result)
        print('Running test for {} results.'.format('keypoints'))
        stats = eng.coco_finish()["stats"]
    except BaseException:
        eng.coco_release()
        raise
    if store:
        eng._val_store = (labels, packed)
    else:
        eng.coco_release()
    _print_summary(stats)
    return stats


def run_coco_eval(gt_file_path, dt_file_path):
    """Drop-in for the reference's val.run_coco_eval (val.py:17-27) without pycocotools: COCOeval(gt, loadRes(dt), 'keypoints')
    evaluate() / accumulate() / summarize() over the images of the ground-truth file in ascending id order.  Prints what the
    reference prints and, unlike it, returns the ten stats."""
    import json
    annotation_type = 'keypoints'
    print('Running test for {} results.'.format(annotation_type))
    with open(gt_file_path) as f:
        gt = json.load(f)
    with open(dt_file_path) as f:
        results = json.load(f)
    return evaluate_detections(gt, results)
