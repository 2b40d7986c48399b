"""``train.train`` on the GPU (-m gpu): the device-side loss log against the host's own accumulation of the fetched losses, bit for
bit; a logged training step against a fetched one; optimiser checkpoints in torch's format through the engine; and the loop end
to end on a folder of JPEG files, its checkpoints restored.

Bars.  The log adds ``loss / divisor`` in float64, one thread per entry in launch order: the same two IEEE operations Python
performs on the fetched doubles, so the bar is equality.  A logged step launches the same kernels as a fetched one: equality.  An
engine step from a state imported from CPU torch is held to what tests/test_gpu_optim.py holds every step to: 1 float32 ulp of
``optim_cases.adam_ref`` fed the same state."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import optim, synth, val
from lwpose_amd import train as train_mod
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import augment_cases as ac
import backbone_backward_cases as bb
import coco_eval_cases as cc
import crowd_mask_cases as cm
import jpeg_cases as jc
import optim_cases as oc
import train_cases as tc
import train_loop_cases as lc

pytestmark = pytest.mark.gpu
_engines = {}


def loss_engine(nref):
    if nref not in _engines:
        _engines[nref] = Engine(0, nref=nref, num_channels=32)         # the loss calls need no weights
    return _engines[nref]


def loss_inputs(eng, N, hs, ws, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    outs = [torch.randn((N, eng.NP if i % 2 else eng.NH, hs, ws), generator=g, device="cuda") for i in range(2 * (eng.nref + 1))]
    km = torch.rand((N, eng.NH, hs, ws), generator=g, device="cuda")
    pm = torch.randn((N, eng.NP, hs, ws), generator=g, device="cuda")
    mask = (torch.rand((N, hs, ws), generator=g, device="cuda") > 0.25).float()
    return outs, km, pm, mask


# ------------------------------------------------------------------------------------------------ the loss log
def test_the_log_is_zero_at_creation():
    eng = Engine(0, nref=2, num_channels=32)
    assert eng.read_loss_log(reset=False) == ([0.0] * 6, 0)


# S = 4 and S = 18 (two loss launches) at 2 x 5 x 7; 257 positions: the smallest count with a second workgroup; 256 * 1024 + 1
# positions: the smallest count at which stage_loss_blocks is capped and a thread walks a second position
@pytest.mark.parametrize("nref,N,hs,ws", [(1, 2, 5, 7), (8, 2, 5, 7), (1, 1, 1, 257), (1, 1, 5, 52429)])
def test_log_equals_the_host_sum_of_the_fetched_losses(nref, N, hs, ws):
    eng = loss_engine(nref)
    S = 2 * (nref + 1)
    eng.read_loss_log(reset=True)
    acc = [0.0] * S
    for call in range(3):
        outs, km, pm, mask = loss_inputs(eng, N, hs, ws, 100 * nref + call)
        losses = eng.stage_losses(outs, km, pm, mask)
        assert len(losses) == S and all(np.isfinite(v) and v > 0 for v in losses)
        for i in range(S):
            acc[i] += losses[i] / 3.0
        assert eng.log_stage_losses(outs, km, pm, mask, divisor=3) is None
    print("nref %d, %d x %d x %d: log %s" % (nref, N, hs, ws, acc[:4]))
    assert eng.read_loss_log(reset=False) == (acc, 3)
    assert eng.read_loss_log(reset=True) == (acc, 3)                   # reset=False left the sums in place
    assert eng.read_loss_log(reset=True) == ([0.0] * S, 0)
    # batch_size divides the losses as in stage_losses; a divisor of 1 adds the loss itself
    outs, km, pm, mask = loss_inputs(eng, N, hs, ws, 7)
    want = eng.stage_losses(outs, km, pm, mask, batch_size=5)
    eng.log_stage_losses(outs, km, pm, mask, batch_size=5)
    assert eng.read_loss_log() == (want, 1)


@pytest.mark.parametrize("divisor", [0.0, -1.0, float("inf"), float("nan")])
def test_log_refuses_a_divisor_that_is_not_finite_and_positive(divisor):
    eng = loss_engine(1)
    outs, km, pm, mask = loss_inputs(eng, 1, 3, 4, 1)
    eng.read_loss_log(reset=True)
    with pytest.raises(ValueError, match="divisor"):
        eng.log_stage_losses(outs, km, pm, mask, divisor=divisor)
    with pytest.raises(ValueError):
        eng.log_stage_losses(outs[:2], km, pm, mask)                    # the checks of stage_losses
    assert eng.read_loss_log() == ([0.0] * 4, 0)


# ------------------------------------------------------------------------------------------------ logged step = fetched step
def make_net(nref=1, C=128, seed=31):
    sd = synth.make_state_dict(nref, seed=seed, num_channels=C)
    net = PoseEstimationWithMobileNet(num_refinement_stages=nref, num_channels=C)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    return net, sd


def fixed_batches(n, N=2, H=368, W=368, seed=3):
    """n batches of fixed tensors: the network input, labels of two persons a frame and a block mask."""
    rng = np.random.RandomState(seed)
    out = []
    for b in range(n):
        fr = synth.make_frames(N, H, W, seed0=700 + 10 * b)
        x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
        frames = [[np.concatenate([rng.uniform(0, [W, H], (18, 2)), rng.randint(0, 3, (18, 1))], 1) for _ in range(2)] for _ in range(N)]
        mask = np.ones((N, H, W), np.float32)
        mask[:, 40 * b:40 * b + 64, 80:200] = 0
        out.append((x, tc.frames_to_labels(frames, 18), mask))
    return out


def engine_state(net):
    eng = net.engine
    st = eng.adam_state()
    return eng.flat_of(eng.stage_params()).cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), st["step"]


def same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_logged_step_is_the_fetched_step():
    batches = fixed_batches(4)
    fetched, _ = make_net()
    logged, _ = make_net()
    opt_f = optim.StageAdam(fetched, lc.BASE_LR, scope="all")
    opt_l = optim.StageAdam(logged, lc.BASE_LR, scope="all")
    logged.engine.read_loss_log(reset=True)
    acc = [0.0] * 4
    for x, labels, mask in batches:
        losses = val.train_step(fetched, opt_f, x, labels, mask, batches_per_iter=2)
        for i in range(4):
            acc[i] += losses[i] / 2.0
        assert val.train_step(logged, opt_l, x, labels, mask, batches_per_iter=2, log=True) is None
    assert opt_f.steps == opt_l.steps == 2
    a, b = engine_state(fetched), engine_state(logged)
    assert a[3] == 2 and same_state(a, b)
    assert logged.engine.read_loss_log() == (acc, 4)
    assert fetched.engine.read_loss_log() == ([0.0] * 4, 0)            # the fetching form leaves the log alone


# ------------------------------------------------------------------------------------------------ optimiser interop
def random_flat(eng, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(eng.grad_spec()[1]).astype(np.float32) * 0.01).cuda()


def test_exported_state_resumes_in_a_second_engine_bit_for_bit():
    net1, _ = make_net(C=32)
    opt1 = optim.StageAdam(net1, lc.BASE_LR, scope="all")
    assert opt1.torch_state_dict()["state"] == {}
    sched = optim.MultiStepLR(opt1, [1], 0.333)
    sched.step()                                                        # the rate drops: the export must carry it
    opt1.step(random_flat(net1.engine, 1))
    sd = opt1.torch_state_dict()
    order = optim.torch_param_order(lc.state_spec(1, 32))
    assert sorted(sd["state"]) == list(range(151)) and [len(g["params"]) for g in sd["param_groups"]] == [len(g) for g in order]
    assert sd["param_groups"][10]["lr"] == 8 * lc.BASE_LR * 0.333 and sd["param_groups"][10]["initial_lr"] == 8 * lc.BASE_LR
    net2 = PoseEstimationWithMobileNet(num_refinement_stages=1, num_channels=32)
    net2.load_state_dict(net1.state_dict())
    net2.eval().cuda()
    opt2 = optim.StageAdam(net2, 1.0, scope="all")
    opt2.load_torch_state_dict(sd)
    assert opt2.lr == opt1.lr == lc.BASE_LR * 0.333 and opt2.initial_lr == lc.BASE_LR
    assert same_state(engine_state(net1), engine_state(net2))
    g = random_flat(net1.engine, 2)
    opt1.step(g)
    opt2.step(g)
    a, b = engine_state(net1), engine_state(net2)
    assert a[3] == 2 and same_state(a, b)
    ref, _ = lc.torch_adam(1, 32)
    ref.load_state_dict(opt2.torch_state_dict())                        # and torch takes what the engine exports


def test_a_state_made_by_cpu_torch_adam_steps_within_the_adam_bar():
    net, sd = make_net(nref=0, C=32, seed=21)
    ref, params = lc.torch_adam(0, 32, values=sd)
    lc.seeded_steps(ref, params, 2)
    moved = dict(sd)
    moved.update({k: p.detach().clone() for k, p in params.items()})
    net.load_state_dict(moved)
    opt = optim.StageAdam(net, 1.0, scope="all")
    opt.load_torch_state_dict(ref.state_dict())
    eng = net.engine
    spec, total = eng.grad_spec()
    assert sorted(k for k, _, _ in spec) == sorted(params)
    flat_of = lambda name: np.concatenate([ref.state[params[k]][name].numpy().reshape(-1) for k, _, _ in spec])
    p0 = np.concatenate([params[k].detach().numpy().reshape(-1) for k, _, _ in spec])
    m0, v0 = flat_of("exp_avg"), flat_of("exp_avg_sq")
    got0 = engine_state(net)
    assert got0[3] == 2 and opt.lr == lc.BASE_LR
    for a, w in zip(got0[:3], (p0, m0, v0)):
        assert np.array_equal(a.numpy(), w)                             # the import itself is exact
    g = oc.crafted_gradients(spec, 3)
    opt.step(torch.from_numpy(g).cuda())
    lr, decay = bb.flat_groups(spec, lc.BASE_LR)
    want = oc.adam_ref(p0, g, m0, v0, 3, lr, decay)
    got = engine_state(net)
    assert got[3] == 3
    worst = max(int(oc.ulp_distance(a.numpy(), w.astype(np.float32)).max()) for a, w in zip(got[:3], want))
    print("step 3 from torch's state: worst %d ulp" % worst)
    assert worst <= 1


# ------------------------------------------------------------------------------------------------ train() end to end
TRAIN_FILES = ["large_100x75_420", "37x53_422", "37x53_444", "17x17_420", "33x16_422"]
VAL_FILES = {785: "large_100x75_420", 139: "37x53_444"}


def write_folders(tmp_path):
    fix = jc.fixtures()
    images, val_images = tmp_path / "train", tmp_path / "val"
    images.mkdir()
    val_images.mkdir()
    labels = []
    for n, name in enumerate(TRAIN_FILES):
        (images / (name + ".jpg")).write_bytes(fix[name][0])
        h, w = fix[name][1].shape[:2]
        label = ac.synthetic_sample(500 + n, h, w, others=n % 2, scale_provided=0.5, with_mask=False)["label"]      # one or two persons
        grid = np.zeros((h, w), dtype=bool)
        grid[h // 4:h // 2 + 3, w // 3:w // 3 + 6] = True
        label.update(img_paths=name + ".jpg", segmentations=[cm.rle_encode(grid)])
        labels.append(label)
    for i, name in VAL_FILES.items():
        (val_images / ("%012d.jpg" % i)).write_bytes(fix[name][0])
    kp = np.zeros((17, 3))
    kp[:, 0], kp[:, 1], kp[:, 2] = np.linspace(10, 80, 17), np.linspace(5, 60, 17), 2
    gt = cc.dataset(sorted(VAL_FILES), [{"id": 1, "image_id": 785, "category_id": 1, "keypoints": kp.reshape(-1).tolist(), "num_keypoints": 17,
                                        "area": 3000.0, "iscrowd": 0, "bbox": [10.0, 5.0, 70.0, 55.0]}])
    for im in gt["images"]:
        im["file_name"] = "%012d.jpg" % im["id"]
    with open(tmp_path / "val.json", "w") as f:
        json.dump(gt, f)
    return labels, str(images), str(tmp_path / "val.json"), str(val_images)


def run_train(labels, images, val_json, val_images, folder, **kw):
    os.makedirs(folder, exist_ok=True)
    out = io.StringIO()
    args = dict(checkpoint_path=None, weights_only=False, epochs=2, seed=7)
    args.update(kw)
    with contextlib.redirect_stdout(out):
        got = train_mod.train(labels, images, 1, lc.BASE_LR, 2, 1, 0, args.pop("checkpoint_path"), args.pop("weights_only"), False, folder, 1,
                              val_json, val_images, os.path.join(folder, "detections.json"), 2, 3, **args)
    return got, out.getvalue().splitlines()


def test_train_end_to_end_and_its_checkpoint_restored(tmp_path):
    labels, images, val_json, val_images = write_folders(tmp_path)
    full = str(tmp_path / "full")
    (net, opt, num_iter), lines = run_train(labels, images, val_json, val_images, full)
    # 5 samples in batches of 2, 2, 1: three iterations an epoch, six in all
    assert num_iter == 6 and opt.steps == 6 and net.engine.adam_state()["step"] == 6
    assert sorted(f for f in os.listdir(full) if f.endswith(".pth")) == ["checkpoint_iter_%d.pth" % i for i in (2, 4, 6)]
    assert [l for l in lines if l.startswith("Iter: ")] == ["Iter: %d" % i for i in range(1, 7)]
    assert lines.count("Validation...") == 2 and os.path.exists(os.path.join(full, "detections.json"))
    logged = [l for l in lines if re.match(r"stage[12]_(pafs|heatmaps)_loss: ", l)]
    assert len(logged) == 6 * 4
    assert all(np.isfinite(float(l.split()[-1])) and float(l.split()[-1]) > 0 for l in logged)
    for i in (2, 4, 6):
        ck = train_mod.load_checkpoint(os.path.join(full, "checkpoint_iter_%d.pth" % i))
        assert sorted(ck) == ["current_epoch", "iter", "optimizer", "scheduler", "state_dict"]
        assert ck["iter"] == i and ck["current_epoch"] == (i - 1) // 3 and ck["scheduler"]["last_epoch"] == ck["current_epoch"] + 1
        assert list(ck["state_dict"]) == list(net.state_dict()) and sorted(ck["optimizer"]["state"]) == list(range(151))
    # torch's own classes take the optimiser and the schedule of a checkpoint
    ref, _ = lc.torch_adam(1)
    ref.load_state_dict(ck["optimizer"])
    torch.optim.lr_scheduler.MultiStepLR(ref, [100, 200, 260], 0.333).load_state_dict(ck["scheduler"])

    # a run that ends at iteration 2 returns the state its checkpoint_iter_2.pth was saved from
    short = str(tmp_path / "short")
    (net2, opt2, num_iter2), _ = run_train(labels, images, val_json, val_images, short, max_iters=2)
    assert num_iter2 == 2 and os.listdir(short) == ["checkpoint_iter_2.pth"]
    path = os.path.join(short, "checkpoint_iter_2.pth")
    first = train_mod.load_checkpoint(os.path.join(full, "checkpoint_iter_2.pth"))
    again = train_mod.load_checkpoint(path)
    assert all(torch.equal(first["state_dict"][k], again["state_dict"][k]) for k in first["state_dict"])     # seed 7 twice: the same run
    saved = engine_state(net2)
    # restored by train()'s own loading code (no epoch runs), on a fresh net, optimiser and schedule
    (net3, opt3, num_iter3), _ = run_train(labels, images, val_json, val_images, str(tmp_path / "resumed"), checkpoint_path=path, epochs=0)
    assert num_iter3 == 2 and again["iter"] == 2 and again["current_epoch"] == 0
    assert opt3.lr == opt2.lr == lc.BASE_LR and opt3.initial_lr == lc.BASE_LR
    assert saved[3] == 2 and same_state(saved, engine_state(net3))
    sched = optim.MultiStepLR(opt3, [100, 200, 260], 0.333)
    sched.load_state_dict(again["scheduler"])
    assert sched.last_epoch == 1 and sched.state_dict()["_step_count"] == 2
    # one more step on fixed tensors from the restored and from the continuing state
    x, step_labels, mask = fixed_batches(1)[0]
    l2 = val.train_step(net2, opt2, x, step_labels, mask)
    l3 = val.train_step(net3, opt3, x, step_labels, mask)
    assert l2 == l3 and same_state(engine_state(net2), engine_state(net3)) and engine_state(net3)[3] == 3

    # weights only: the weights of the checkpoint, the optimiser at step 0
    (net4, opt4, num_iter4), _ = run_train(labels, images, val_json, val_images, str(tmp_path / "weights"), checkpoint_path=path,
                                           weights_only=True, epochs=0)
    assert num_iter4 == 0 and net4.engine.adam_state()["step"] == 0 and opt4.torch_state_dict()["state"] == {}
    got = net4.state_dict()
    assert all(torch.equal(got[k], again["state_dict"][k]) for k in got)
