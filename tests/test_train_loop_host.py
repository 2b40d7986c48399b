"""Host side of ``train.train`` (no GPU): torch's parameter numbering against the reference-generated fixture, optimiser
checkpoints exchanged with a CPU ``torch.optim.Adam`` built like train.py:41-55's, the refusals of ``load_torch_state_dict``,
``optim.MultiStepLR`` against torch's class bit for bit, ``load_from_mobilenet`` against what the reference printed and took, and
the loop control of ``train.train`` on a fake engine (tests/train_loop_cases.py)."""
import contextlib
import copy
import ctypes
import io
import os
import warnings

import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, optim
from lwpose_amd import train as train_mod
from lwpose_amd.modules.load_state import load_from_mobilenet

import train_loop_cases as lc


# ------------------------------------------------------------------------------------------------ the C entry points' checks
def test_loss_log_entry_points_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.lwp_version() >= 108
    buf = ctypes.create_string_buffer(64)
    adds = ctypes.c_int64()
    sums = (ctypes.c_double * 4)()
    for divisor in (0.0, -2.0, float("inf"), float("nan")):
        assert L.lwp_stage_losses_log(None, None, 4, buf, buf, buf, 1, 6, 5, 1, divisor) == _lib.LWP_ERR_ARG
        assert b"divisor" in L.lwp_last_error(None)
    assert L.lwp_stage_losses_log(None, None, 4, buf, buf, buf, 1, 6, 5, 1, 1.0) == _lib.LWP_ERR_ARG      # outs is null: lwp_stage_losses' checks
    assert L.lwp_loss_log_read(None, sums, ctypes.byref(adds), 1) == _lib.LWP_ERR_ARG


# ------------------------------------------------------------------------------------------------ group order
@pytest.mark.parametrize("nref", [0, 1, 3])
def test_param_order_is_the_reference_optimisers(nref):
    order = optim.torch_param_order(lc.state_spec(nref))
    assert order == lc.param_groups_fixture()[str(nref)]
    assert [(g[2], g[3]) for g in optim.TORCH_GROUPS] == [(m, wd is None) for m, (_, wd) in zip(lc.MULTIPLIERS, lc.REF_GROUP_OPTIONS)]


def test_group_sizes_and_first_indices_of_one_refinement_stage():
    order = optim.torch_param_order(lc.state_spec(1))
    sizes = [len(g) for g in order]
    assert sizes == lc.NREF1_SIZES and sum(sizes) == 151
    assert [sum(sizes[:i]) for i in range(13)] == lc.NREF1_FIRST
    params = [k for k, _ in lc.state_spec(1) if k.endswith((".weight", ".bias"))]
    assert sorted(k for g in order for k in g) == sorted(params)          # every parameter in exactly one group


def test_a_parameter_outside_the_groups_is_refused():
    with pytest.raises(ValueError, match="initial_stage.dw.0.weight"):
        optim.torch_param_order(lc.state_spec(0) + [("initial_stage.dw.0.weight", (8, 1, 3, 3))])


# ------------------------------------------------------------------------------------------------ torch interop
@pytest.fixture(scope="module")
def stepped():
    """The reference's optimiser over the nref-1 network's parameters after two seeded steps, and a schedule on it."""
    opt, params = lc.torch_adam(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.optim.lr_scheduler.MultiStepLR(opt, [100, 200, 260], 0.333)
    lc.seeded_steps(opt, params, 2)
    shapes = {k: tuple(p.shape) for k, p in params.items()}
    return opt, params, shapes, optim.torch_param_order(lc.state_spec(1))


def test_export_round_trips_torchs_state(stepped):
    opt, params, shapes, order = stepped
    sd = opt.state_dict()
    hyper, step, moments, dropped = optim.unpack_torch_state(sd, order, shapes)
    assert step == 2 and dropped == 0 and sorted(moments) == sorted(shapes)
    assert hyper == dict(lr=lc.BASE_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, initial_lr=lc.BASE_LR)
    back = optim.pack_torch_state(order, hyper, step, moments)
    assert lc.states_equal(back, sd)
    assert all(v["step"].dtype == torch.float32 and v["step"].dim() == 0 and float(v["step"]) == 2.0 for v in back["state"].values())
    fresh, _ = lc.torch_adam(1, seed=5)
    fresh.load_state_dict(back)                                          # torch accepts the exported dict
    assert lc.states_equal(fresh.state_dict(), sd)


def test_export_before_a_schedule_and_before_the_first_step():
    opt, params = lc.torch_adam(0)
    order = optim.torch_param_order(lc.state_spec(0))
    sd = opt.state_dict()
    assert sd["state"] == {} and "initial_lr" not in sd["param_groups"][0]
    hyper, step, moments, dropped = optim.unpack_torch_state(sd, order, {k: tuple(p.shape) for k, p in params.items()})
    assert (step, moments, dropped, hyper["initial_lr"]) == (0, {}, 0, None)
    assert lc.states_equal(optim.pack_torch_state(order, hyper, step, moments), sd)


def test_state_outside_the_scope_is_dropped_and_counted(stepped):
    opt, params, shapes, order = stepped
    stages = {k: s for k, s in shapes.items() if k.startswith(("initial_stage.", "refinement_stages."))}
    hyper, step, moments, dropped = optim.unpack_torch_state(opt.state_dict(), order, stages)
    assert sorted(moments) == sorted(stages) and dropped == len(shapes) - len(stages) == 79 and step == 2
    back = optim.pack_torch_state(order, hyper, step, moments)
    assert sorted(back["state"]) == list(range(79, 151))                 # exactly the scope's parameters, at torch's indices


def edit_group(n, **entries):
    def f(sd):
        sd["param_groups"][n].update(entries)
    return f


def edit_state(i, name, value):
    def f(sd):
        sd["state"][i][name] = value
    return f


REFUSALS = {
    "twelve groups": (lambda sd: sd["param_groups"].pop(), "12 parameter groups"),
    "a group's length": (lambda sd: sd["param_groups"][4]["params"].pop(), "group 4"),
    "amsgrad": (edit_group(3, amsgrad=True), "group 3"),
    "maximize": (edit_group(7, maximize=True), "group 7"),
    "betas": (edit_group(5, betas=(0.8, 0.999)), "group 5"),
    "eps": (edit_group(6, eps=1e-6), "group 6"),
    "weight decay differs": (edit_group(9, weight_decay=1e-4), "group 9"),
    "weight decay on a bias group": (edit_group(8, weight_decay=5e-4), "group 8"),
    "lr pattern": (edit_group(10, lr=lc.BASE_LR * 4, initial_lr=lc.BASE_LR * 4), "group 10"),
    "lr not a multiple": (edit_group(3, lr=lc.BASE_LR * 3), "group 3"),
    "moment shape": (edit_state(80, "exp_avg", torch.zeros(3)), "index 80"),
    "steps differ": (edit_state(100, "step", torch.tensor(3.0)), "index 100"),
    "state lacks a parameter": (lambda sd: sd["state"].pop(150), "index 150"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals_name_the_group_or_the_index(stepped, what):
    opt, params, shapes, order = stepped
    sd = copy.deepcopy(opt.state_dict())
    optim.unpack_torch_state(sd, order, shapes)
    edit, names = REFUSALS[what]
    edit(sd)
    with pytest.raises(ValueError, match=names):
        optim.unpack_torch_state(sd, order, shapes)


def test_stage_adam_checkpoints_on_a_fake_engine(capsys):
    """StageAdam's two methods around the host functions: scope "stages" exports 72 entries at torch's indices, torch loads
    them, and a torch checkpoint of the whole network loads with the other 79 entries dropped and counted."""
    net = lc.FakeNet(1, [], C=128)
    opt = optim.StageAdam(net, lc.BASE_LR)
    assert opt.torch_state_dict()["state"] == {}
    opt.step(torch.arange(net.engine.grad_spec()[1], dtype=torch.float32))
    sd = opt.torch_state_dict()
    assert sorted(sd["state"]) == list(range(79, 151)) and "initial_lr" not in sd["param_groups"][0]
    assert [g["lr"] for g in sd["param_groups"]] == [m * lc.BASE_LR for m in lc.MULTIPLIERS]
    ref, params = lc.torch_adam(1)
    ref.load_state_dict(sd)
    lc.seeded_steps(ref, params, 1)                                      # every parameter gets a state now
    other = lc.FakeNet(1, [], C=128)
    opt2 = optim.StageAdam(other, 1.0)
    opt2.load_torch_state_dict(ref.state_dict())
    assert "79 parameters" in capsys.readouterr().out
    assert opt2.lr == lc.BASE_LR and other.engine.t == 2
    want = torch.cat([ref.state[params[k]]["exp_avg"].reshape(-1) for k, _, _ in other.engine.grad_spec()[0]])
    assert torch.equal(other.engine.m, want)


# ------------------------------------------------------------------------------------------------ schedule
class Rate(object):
    def __init__(self, lr=lc.BASE_LR):
        self.lr, self.initial_lr = lr, None


def torch_schedule(milestones, lr=lc.BASE_LR):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p]}] + [{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr * m} for m in lc.MULTIPLIERS[1:]], lr=lr)
    return opt, torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=0.333)


@pytest.mark.parametrize("milestones,epochs", [([100, 200, 260], 280), ([2, 4], 8)])
@pytest.mark.filterwarnings("ignore")
def test_schedule_follows_torchs_bit_for_bit(milestones, epochs):
    topt, tsched = torch_schedule(milestones)
    opt = Rate()
    sched = optim.MultiStepLR(opt, milestones, 0.333)
    seen = set()
    for epoch in range(epochs):
        tsched.step()
        sched.step()
        assert opt.lr == topt.param_groups[0]["lr"], epoch
        assert sched.get_last_lr() == tsched.get_last_lr() == [g["lr"] for g in topt.param_groups]
        assert lc.schedules_equal(sched.state_dict(), tsched.state_dict())
        seen.add(opt.lr)
    assert len(seen) == len(milestones) + 1
    if milestones == [100, 200, 260]:
        assert sorted(seen, reverse=True)[:3] == [4e-5, 1.3320000000000001e-05, 4.435560000000001e-06]


@pytest.mark.parametrize("milestones,saved_at", [([2, 4], 1), ([2, 4], 3), ([100, 200, 260], 99), ([100, 200, 260], 200)])
@pytest.mark.filterwarnings("ignore")
def test_schedule_resumes_like_torchs_and_the_dicts_load_both_ways(milestones, saved_at):
    """The reference's sequence: construct, step at the top of every epoch, save inside epoch ``saved_at``; the resumed run
    constructs, loads (the optimiser's rate from its own checkpoint) and steps again at the top of the resumed epoch."""
    topt, tsched = torch_schedule(milestones)
    opt = Rate()
    sched = optim.MultiStepLR(opt, milestones, 0.333)
    for _ in range(saved_at + 1):
        tsched.step()
        sched.step()
    saved, tsaved = sched.state_dict(), tsched.state_dict()
    assert lc.schedules_equal(saved, tsaved) and saved["last_epoch"] == saved_at + 1
    # each class resumes from the OTHER's dict
    topt2, tsched2 = torch_schedule(milestones)
    topt2.load_state_dict(topt.state_dict())
    tsched2.load_state_dict(saved)
    opt2 = Rate()
    sched2 = optim.MultiStepLR(opt2, milestones, 0.333)
    opt2.lr = topt.param_groups[0]["lr"]
    sched2.load_state_dict(tsaved)
    for epoch in range(saved_at, min(saved_at + 120, 280)):
        tsched2.step()
        sched2.step()
        assert opt2.lr == topt2.param_groups[0]["lr"], epoch
        assert lc.schedules_equal(sched2.state_dict(), tsched2.state_dict())
    with pytest.raises(ValueError, match="last_epoch"):
        sched2.load_state_dict({k: v for k, v in saved.items() if k != "last_epoch"})


# ------------------------------------------------------------------------------------------------ load_from_mobilenet
def test_load_from_mobilenet_prints_and_takes_what_the_reference_did():
    fix = lc.mobilenet_fixture()
    net = lc.DictNet(fix["num_refinement_stages"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        load_from_mobilenet(net, lc.mobilenet_source(fix))
    assert out.getvalue().splitlines() == fix["printed"]
    assert fix["missing"] not in fix["taken"] and fix["wrong_shape"] not in fix["taken"]
    for k, v in net.state.items():
        assert bool((v == (2 if k in fix["taken"] else 1)).all()), k
    assert sum(k.startswith("model.") for k in fix["taken"]) == len(fix["taken"]) - 2


# ------------------------------------------------------------------------------------------------ loop control
def run_fake(monkeypatch, tmp_path, calls, **kw):
    lc.patch_train(monkeypatch, train_mod, 7, calls)
    out = io.StringIO()
    args = dict(checkpoint_path=None, weights_only=False, epochs=4, seed=3)
    args.update(kw)
    with contextlib.redirect_stdout(out):
        net, opt, num_iter = train_mod.train(
            "labels", "images", 1, lc.BASE_LR, 3, 2, 8, args.pop("checkpoint_path"), args.pop("weights_only"), False, str(tmp_path), 1,
            "val.json", "val_images", "detections.json", 2, 3, scope="stages", **args)
    return net, opt, num_iter, out.getvalue().splitlines()


def expected_lines(iteration, steps):
    """The reference's lines for an iteration made of the given train-step numbers (batches_per_iter 2, log_after 1)."""
    total = [sum(lc.fake_loss(s, i) / 2 for s in steps) for i in range(4)]
    lines = ['Iter: {}'.format(iteration)]
    for loss_idx in range(2):
        lines += '\n'.join(['stage{}_pafs_loss:     {}', 'stage{}_heatmaps_loss: {}']).format(
            loss_idx + 1, total[loss_idx * 2 + 1] / 1, loss_idx + 1, total[loss_idx * 2] / 1).split('\n')
    return lines


def test_loop_control_seven_samples_batch_three_two_batches_per_iteration(monkeypatch, tmp_path):
    calls = []
    net, opt, num_iter, lines = run_fake(monkeypatch, tmp_path, calls)
    lr = lc.BASE_LR
    epoch = lambda n: [("read", True, 0 if n == 0 else 1),               # the epoch's reset finds the forgotten third batch's add
                       ("step", 3, 0), ("step", 3, 1), ("adam", lr), ("read", True, 2)]
    want = (epoch(0) + [("step", 1, 0)] + epoch(1) + [("step", 1, 0)]     # iteration 2: checkpoint (no call of the engine's)
            + epoch(2) + [("val", "detections.json"), ("step", 1, 0)] + epoch(3) + [("step", 1, 0)])
    assert calls == want
    assert num_iter == 4 and opt.steps == 4 and net.engine.t == 4 and opt.batch_index == 1
    assert torch.equal(net.engine.m, torch.full_like(net.engine.m, 4.0))   # a forgotten batch never reaches a step
    want_lines = []
    for it in range(1, 5):
        want_lines += expected_lines(it, (3 * it - 2, 3 * it - 1))
        if it == 3:
            want_lines.append('Validation...')
    assert lines == want_lines
    assert sorted(os.listdir(str(tmp_path))) == ["checkpoint_iter_2.pth", "checkpoint_iter_4.pth"]
    ck = train_mod.load_checkpoint(str(tmp_path / "checkpoint_iter_2.pth"))
    assert sorted(ck) == ["current_epoch", "iter", "optimizer", "scheduler", "state_dict"]
    assert ck["iter"] == 2 and ck["current_epoch"] == 1 and ck["scheduler"]["last_epoch"] == 2
    assert sorted(ck["optimizer"]["state"]) == list(range(79, 151)) and float(ck["optimizer"]["state"][79]["step"]) == 2.0


def test_loop_resumes_weights_only_and_stops_at_max_iters(monkeypatch, tmp_path):
    calls = []
    run_fake(monkeypatch, tmp_path, calls)
    path = str(tmp_path / "checkpoint_iter_2.pth")
    later = tmp_path / "later"
    later.mkdir()
    # a resume runs epoch 1 again from its start: the schedule steps to 3, iterations go on from 2
    del calls[:]
    net, opt, num_iter, lines = run_fake(monkeypatch, later, calls, checkpoint_path=path, max_iters=1)
    assert num_iter == 3 and net.engine.t == 3 and opt.steps == 1 and lines[0] == 'Iter: 3' and lines[-1] == 'Validation...'
    assert calls[-1] == ("val", "detections.json") and [c[0] for c in calls].count("step") == 2
    # weights only: the optimiser starts over
    del calls[:]
    net, opt, num_iter, lines = run_fake(monkeypatch, later, calls, checkpoint_path=path, weights_only=True, max_iters=1)
    assert num_iter == 1 and net.engine.t == 1 and lines[0] == 'Iter: 1'
    assert list(net.weights) == ["model.0.0.weight"]
