"""``train()`` trains the eval()-mode network: the BatchNorms use their running statistics, which never move (there is no
BatchNorm train mode in this package, and ``net.train(True)`` keeps raising and is never called).

Drop-in for the reference's ``train.py`` (train.py:23-131) otherwise, statement for statement where a counterpart exists: the
dataset (``CocoTrainDataset`` + ``DeviceAugment`` with the reference's five transforms and pads), Adam with train.py:41-55's
thirteen parameter groups (``optim.StageAdam``), ``MultiStepLR([100, 200, 260], 0.333)`` stepped at the top of every epoch,
``load_state`` / ``load_from_mobilenet``, the resume from ``optimizer`` / ``scheduler`` / ``iter`` / ``current_epoch`` in the
reference's own checkpoint format (a run started with the reference continues here and the reverse), gradient accumulation over
``batches_per_iter`` loader batches, the ``Iter:`` / ``stage{}_pafs_loss`` / ``stage{}_heatmaps_loss`` lines every ``log_after``
iterations, a checkpoint every ``checkpoint_after`` and ``val.evaluate`` every ``val_after``.

What differs:
  - no ``DataLoader`` and no ``DataParallel``: every epoch is a shuffled permutation of the samples drawn from one
    ``random.Random(seed)``, which also drives the augmentation; the last batch of an epoch may be short; ``num_workers`` is
    accepted and unused (the JPEG decode already shares a batch's files among host threads);
  - total_losses lives on the device (``Engine.log_stage_losses``): a step no longer fetches its losses, and the loop's own
    steady-state wait is the ``Engine.read_loss_log`` every ``log_after`` iterations (plus one at the top of an epoch, which
    resets the log); the uploads of the augmentation plans and of the key-points still wait for the stream;
  - as in the reference the resumed epoch is run from its start and steps the schedule again, a partial iteration at the end of
    an epoch is forgotten, and the position of the random generator is not part of a checkpoint;
  - ``scope`` chooses what moves ("all": every parameter, as in the reference; "cpm" / "stages": less), ``epochs`` replaces the
    literal 280, ``max_iters`` ends the run after that many iterations of this call; ``train()`` returns (net, opt, num_iter).
"""
import argparse
import collections
import os
import random

from .datasets.coco import CocoTrainDataset, CocoValDataset
from .datasets.transformations import ConvertKeypoints, Scale, Rotate, CropPad, Flip, DeviceAugment
from .models.with_mobilenet import PoseEstimationWithMobileNet
from .modules.load_state import load_state, load_from_mobilenet
from .optim import StageAdam, MultiStepLR
from .val import evaluate, augmented_train_step


def load_checkpoint(path):
    """``torch.load`` of a checkpoint the reference or ``train()`` saved: tensors, plain values and the ``collections.Counter``
    of the scheduler's milestones, on the host."""
    import torch
    with torch.serialization.safe_globals([collections.Counter]):
        return torch.load(path, map_location="cpu")


def train(prepared_train_labels, train_images_folder, num_refinement_stages, base_lr, batch_size, batches_per_iter,
          num_workers, checkpoint_path, weights_only, from_mobilenet, checkpoints_folder, log_after,
          val_labels, val_images_folder, val_output_name, checkpoint_after, val_after, *, scope="all", epochs=280, max_iters=None,
          seed=None, device=0, fallback=None, entropy="host", backward_precision=None, grad_scale=None):
    import torch
    net = PoseEstimationWithMobileNet(num_refinement_stages)
    net.cuda(device)

    stride = 8
    sigma = 7
    path_thickness = 1
    rng = random.Random(seed)
    dataset = CocoTrainDataset(prepared_train_labels, train_images_folder, net, fallback, entropy)
    augment = DeviceAugment([ConvertKeypoints(),
                             Scale(),
                             Rotate(pad=(128, 128, 128)),
                             CropPad(pad=(128, 128, 128)),
                             Flip()], stride=stride, rng=rng)

    checkpoint = load_checkpoint(checkpoint_path) if checkpoint_path else None
    if checkpoint is not None:                          # the weights first: the optimiser below binds the engine that holds them
        if from_mobilenet:
            load_from_mobilenet(net, checkpoint)
        else:
            load_state(net, checkpoint)
    optimizer = StageAdam(net, base_lr, weight_decay=5e-4, scope=scope, backward_precision=backward_precision, grad_scale=grad_scale)

    num_iter = 0
    current_epoch = 0
    drop_after_epoch = [100, 200, 260]
    scheduler = MultiStepLR(optimizer, milestones=drop_after_epoch, gamma=0.333)
    if checkpoint is not None and not from_mobilenet and not weights_only:
        optimizer.load_torch_state_dict(checkpoint['optimizer'])
        scheduler.load_state_dict(checkpoint['scheduler'])
        num_iter = checkpoint['iter']
        current_epoch = checkpoint['current_epoch']

    engine = net.engine
    done = 0
    for epochId in range(current_epoch, epochs):
        scheduler.step()
        engine.read_loss_log(reset=True)                # total_losses = [0, 0] * (num_refinement_stages + 1)
        optimizer.zero_grad()                           # batch_per_iter_idx = 0
        order = list(range(len(dataset)))
        rng.shuffle(order)
        for first in range(0, len(order), batch_size):
            samples = dataset.samples(order[first:first + batch_size])
            augmented_train_step(net, optimizer, samples, augment, batches_per_iter, sigma, path_thickness, log=True)
            if optimizer.batch_index != 0:              # the iteration is still collecting batches
                continue
            num_iter += 1
            done += 1

            if num_iter % log_after == 0:
                total_losses, _ = engine.read_loss_log(reset=True)
                print('Iter: {}'.format(num_iter))
                for loss_idx in range(len(total_losses) // 2):
                    print('\n'.join(['stage{}_pafs_loss:     {}', 'stage{}_heatmaps_loss: {}']).format(
                        loss_idx + 1, total_losses[loss_idx * 2 + 1] / log_after,
                        loss_idx + 1, total_losses[loss_idx * 2] / log_after))
            if num_iter % checkpoint_after == 0:
                snapshot_name = '{}/checkpoint_iter_{}.pth'.format(checkpoints_folder, num_iter)
                torch.save({'state_dict': net.state_dict(),
                            'optimizer': optimizer.torch_state_dict(),
                            'scheduler': scheduler.state_dict(),
                            'iter': num_iter,
                            'current_epoch': epochId},
                           snapshot_name)
            if num_iter % val_after == 0:
                print('Validation...')
                evaluate(val_labels, val_output_name, CocoValDataset(val_labels, val_images_folder, net, fallback, entropy), net, store=True)
            if max_iters is not None and done >= max_iters:
                return net, optimizer, num_iter
    return net, optimizer, num_iter


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('--prepared-train-labels', type=str, required=True,
                        help='path to the file with prepared annotations')
    parser.add_argument('--train-images-folder', type=str, required=True, help='path to COCO train images folder')
    parser.add_argument('--num-refinement-stages', type=int, default=1, help='number of refinement stages')
    parser.add_argument('--base-lr', type=float, default=4e-5, help='initial learning rate')
    parser.add_argument('--batch-size', type=int, default=80, help='batch size')
    parser.add_argument('--batches-per-iter', type=int, default=1, help='number of batches to accumulate gradient from')
    parser.add_argument('--num-workers', type=int, default=8, help='number of workers (accepted, unused)')
    parser.add_argument('--checkpoint-path', type=str, required=True, help='path to the checkpoint to continue training from')
    parser.add_argument('--from-mobilenet', action='store_true',
                        help='load weights from mobilenet feature extractor')
    parser.add_argument('--weights-only', action='store_true',
                        help='just initialize layers with pre-trained weights and start training from the beginning')
    parser.add_argument('--experiment-name', type=str, default='default',
                        help='experiment name to create folder for checkpoints')
    parser.add_argument('--log-after', type=int, default=100, help='number of iterations to print train loss')

    parser.add_argument('--val-labels', type=str, required=True, help='path to json with keypoints val labels')
    parser.add_argument('--val-images-folder', type=str, required=True, help='path to COCO val images folder')
    parser.add_argument('--val-output-name', type=str, default='detections.json',
                        help='name of output json file with detected keypoints')
    parser.add_argument('--checkpoint-after', type=int, default=5000,
                        help='number of iterations to save checkpoint')
    parser.add_argument('--val-after', type=int, default=5000,
                        help='number of iterations to run validation')
    # not in the reference
    parser.add_argument('--scope', type=str, default='all', choices=('stages', 'cpm', 'all'), help='which parameters move')
    parser.add_argument('--epochs', type=int, default=280, help='last epoch + 1')
    parser.add_argument('--max-iters', type=int, default=None, help='stop after this many iterations')
    parser.add_argument('--seed', type=int, default=None, help='seed of the shuffle and the augmentation')
    parser.add_argument('--entropy', type=str, default='host', choices=('host', 'device'), help='where JPEG Huffman data is decoded')
    args = parser.parse_args()

    checkpoints_folder = '{}_checkpoints'.format(args.experiment_name)
    if not os.path.exists(checkpoints_folder):
        os.makedirs(checkpoints_folder)

    train(args.prepared_train_labels, args.train_images_folder, args.num_refinement_stages, args.base_lr, args.batch_size,
          args.batches_per_iter, args.num_workers, args.checkpoint_path, args.weights_only, args.from_mobilenet,
          checkpoints_folder, args.log_after, args.val_labels, args.val_images_folder, args.val_output_name,
          args.checkpoint_after, args.val_after, scope=args.scope, epochs=args.epochs, max_iters=args.max_iters, seed=args.seed,
          entropy=args.entropy)
