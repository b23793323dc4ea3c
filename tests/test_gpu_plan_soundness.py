"""What a recorded plan may NOT replay (zs3_amd/plan.py): a replay re-issues the library's launches and nothing else, so a step in
which the tensor library did device work -- a criterion written in torch ops (focal loss, 0.5 * CE, CE + a regulariser), a torch op
in backward only, a learnable scalar on the logits -- has to stay eager.  Every configuration runs once with the plan and once
without it from the same initial state (live dropout, poly schedule, a fresh batch per step): losses, every state_dict entry and
every momentum buffer agree bit for bit, and the counters say which configurations were recorded and which gave up.  The failures
of a recording (a table it cannot move, an exception inside a recorded feature pass) fall back instead of leaving a broken plan."""
import types

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

STEPS = 6
RECORDED = (2, 1, STEPS - 3)     # 2 settling calls, 1 recording, replays
EAGER = (STEPS - 1, 0, 0)        # 2 settling calls, 1 recording attempt that gave up (eager result), plain eager calls


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _deeplab(dev, seed=1):
    from zs3_amd.modeling.deeplab import DeepLab
    torch.manual_seed(seed)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False)
    for name, mod in model.named_modules():
        if name.endswith("bn3"):
            mod.weight.data.fill_(0.1)
    return model.to(dev).train()


class _Scaled(nn.Module):
    """DeepLab with a learnable scalar applied to its logits by the tensor library (forward: mul; backward: mul and a sum)"""

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.t = nn.Parameter(torch.full((), 1.25, device=next(net.parameters()).device))

    def forward(self, x):
        return self.net(x) * self.t

    def get_1x_lr_params(self):
        return list(self.net.get_1x_lr_params())

    def get_10x_lr_params(self):
        return list(self.net.get_10x_lr_params()) + [self.t]


class _DoubleGrad(torch.autograd.Function):
    """a view in forward (nothing for the tensor library to launch), the gradient times 2 by a torch op in backward: work that
    only autograd's device thread does"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * 2.0


class _BackwardOp(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        return _DoubleGrad.apply(self.net(x))

    def get_1x_lr_params(self):
        return self.net.get_1x_lr_params()

    def get_10x_lr_params(self):
        return self.net.get_10x_lr_params()


def _class_weights(dev):
    w = torch.ones(21, device=dev)
    w[[10, 14]] = 100.0
    return w


def _criterion(kind, dev):
    from zs3_amd.utils.loss import SegmentationLosses
    w = _class_weights(dev)
    if kind in ("ce", "ce_finetune", "focal"):
        return SegmentationLosses(weight=w, cuda=True).build_loss(kind)
    if kind == "focal_sum":
        return SegmentationLosses(weight=w, cuda=True, batch_average=False).build_loss("focal")
    ce = SegmentationLosses(weight=w, cuda=True).build_loss("ce")
    if kind == "half_ce":
        return lambda p, t: 0.5 * ce(p, t)          # (autograd hands the CE a gradient of 0.5: not the plan's `_one`)
    if kind == "ce_l2":
        return lambda p, t: ce(p, t) + 1e-3 * (p ** 2).mean()
    raise ValueError(kind)


def _batches(dev, n=STEPS + 1, size=65):
    from zs3_amd.utils.synthetic import make_batch
    return [make_batch(2, size, 21, [10, 14], seed=50 + i, device=dev) for i in range(n)]


def _run(dev, use_plan, crit="ce", wrap=None, opt_cls=None, verify=False):
    from zs3_amd import functional as Fz
    from zs3_amd.optim import SGD
    from zs3_amd.plan import StepPlan
    from zs3_amd.utils.lr_scheduler import LR_Scheduler
    model = _deeplab(dev)
    if wrap == "scaled":
        model = _Scaled(model)
    elif wrap == "backward_op":
        model = _BackwardOp(model)
    groups = [{"params": model.get_1x_lr_params(), "lr": 0.007}, {"params": model.get_10x_lr_params(), "lr": 0.07}]
    opt = (opt_cls or SGD)(groups, momentum=0.9, weight_decay=5e-4, nesterov=False)
    Fz.manual_seed(1234)
    sched = LR_Scheduler("poly", 0.007, 1, STEPS, verbose=False)
    step = StepPlan(model, _criterion(crit, dev), opt, enabled=use_plan)
    bs = _batches(dev)
    losses = []
    for i, b in enumerate(bs[:STEPS]):
        sched(opt, i, 0, 0.0)
        pred, loss = step(b["image"], b["label"])
        assert pred.shape == (2, 21, 65, 65)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    out = types.SimpleNamespace(
        losses=torch.stack(losses).cpu(), state={k: v.detach().clone() for k, v in model.state_dict().items()},
        mom=[opt.state[p]["momentum_buffer"].detach().clone() for g in opt.param_groups for p in g["params"]],
        counts=(step.eager_calls, step.recordings, step.replays), unrecorded=list(step.unrecorded_ops), verified=None)
    if verify and step._plan is not None:
        out.verified = step.verify(bs[STEPS]["image"], bs[STEPS]["label"], poison=True)
    step.close()
    return out


def _assert_same(e, p):
    assert torch.equal(e.losses, p.losses), (e.losses.tolist(), p.losses.tolist())
    assert e.state.keys() == p.state.keys()
    bad = [k for k in e.state if not torch.equal(e.state[k], p.state[k])]
    assert not bad, bad[:8]
    assert len(e.mom) == len(p.mom) and all(torch.equal(a, b) for a, b in zip(e.mom, p.mom))


CASES = [
    ("ce", None, RECORDED),               # control: the 100x class weights, recorded and replayed
    ("ce_finetune", None, RECORDED),
    ("focal", None, EAGER),               # batch_average True
    ("focal_sum", None, EAGER),           # batch_average False
    ("half_ce", None, EAGER),
    ("ce_l2", None, EAGER),
    ("ce", "backward_op", EAGER),         # torch work only on autograd's device thread
    ("ce", "scaled", EAGER),              # a learnable scalar on the logits, in the 10x group
]


@pytest.mark.parametrize("crit,wrap,counts", CASES, ids=[f"{c}-{w}" if w else c for c, w, _ in CASES])
def test_plan_replays_only_steps_made_of_library_launches(dev, crit, wrap, counts):
    e = _run(dev, False, crit, wrap)
    p = _run(dev, True, crit, wrap, verify=counts == RECORDED)
    print(f"\n[{crit} {wrap}] counts {p.counts}, unrecorded ops {p.unrecorded[:8]}\n  losses eager {e.losses.tolist()}\n"
          f"  losses plan  {p.losses.tolist()}")
    _assert_same(e, p)
    assert e.counts == (STEPS, 0, 0) and p.counts == counts, (e.counts, p.counts)
    if counts == RECORDED:
        assert p.unrecorded == [] and p.verified == [], (p.unrecorded, p.verified)
    else:
        assert p.unrecorded, "the recording gave up without naming the tensor-library work it saw"
    if crit.startswith("focal"):
        assert len(set(p.losses.tolist())) == STEPS, p.losses.tolist()        # (a replay would log one loss over and over)
    if wrap == "scaled":
        assert torch.equal(e.state["t"], p.state["t"]) and float(p.state["t"]) != 1.25


def test_base_trainer_with_focal_loss_logs_the_eager_losses(dev, monkeypatch):
    """BaseTrainer.training (base_trainer.py:5-57) with the reference's `--loss-type focal` criterion: six iterations through the
    trainer's own StepPlan log the running loss of the same trainer with the plan switched off, value for value"""
    import zs3_amd.plan
    from zs3_amd import functional as Fz
    from zs3_amd.base_trainer import BaseTrainer
    from zs3_amd.optim import SGD
    from zs3_amd.utils.lr_scheduler import LR_Scheduler

    class Log:
        def __init__(self):
            self.scalars = []

        def add_scalar(self, tag, value, step):
            self.scalars.append((tag, float(value), int(step)))

        def visualize_image(self, *a):
            pass

    bs = _batches(dev, STEPS)
    # (4 single-image batches at the end: skipped by the trainer, they make the loader long enough for its image-dump interval)
    loader = [{"image": b["image"].cpu(), "label": b["label"].cpu()} for b in bs] + \
        [{"image": bs[0]["image"][:1].cpu(), "label": bs[0]["label"][:1].cpu()}] * 4
    runs = []
    for enabled in (False, True):
        monkeypatch.setattr(zs3_amd.plan, "ENABLED", enabled)
        model = _deeplab(dev)
        t = BaseTrainer()
        log = Log()
        t.model, t.criterion, t.train_loader = model, _criterion("focal", dev), loader
        t.optimizer = SGD([{"params": model.get_1x_lr_params(), "lr": 0.007}, {"params": model.get_10x_lr_params(), "lr": 0.07}],
                          momentum=0.9, weight_decay=5e-4, nesterov=False)
        t.scheduler = LR_Scheduler("poly", 0.007, 1, len(loader), verbose=False)
        t.args = types.SimpleNamespace(cuda=True, batch_size=2, dataset="pascal", no_val=False)
        t.best_pred, t.writer, t.summary = 0.0, log, log
        Fz.manual_seed(99)
        t.training(0)
        torch.cuda.synchronize()
        step = t._zs3_step_plan
        runs.append(([v for tag, v, _ in log.scalars if tag == "train/total_loss_iter"],
                     [v for tag, v, _ in log.scalars if tag == "train/total_loss_epoch"],
                     (step.eager_calls, step.recordings, step.replays)))
        step.close()
    (le, re_, ce), (lp, rp, cp) = runs
    print(f"\n[trainer focal] eager {le} {re_}\n[trainer focal] plan  {lp} {rp}")
    assert lp == le and rp == re_ and len(rp) == 1
    assert len(lp) == STEPS and len(set(lp)) == STEPS
    assert ce == (STEPS, 0, 0) and cp == EAGER, (ce, cp)


def test_a_table_the_recording_cannot_move_falls_back_to_eager(dev):
    """_record moves the optimizer's record tables out of the step's pool and points the recorded optimizer launch at the copy:
    a table that is no argument of exactly one recorded optimizer launch gives up -- the recorded call returns its eager result,
    the configuration stays eager, nothing raises"""
    from zs3_amd.optim import SGD

    class StraySGD(SGD):
        def step(self, closure=None):
            out = super().step(closure)
            stray = self.__dict__.get("_stray")
            if stray is None:
                stray = self._stray = torch.empty(16, dtype=torch.int64, device=dev)
            self._zs3_tables.append(stray)         # a device tensor no recorded launch reads
            return out

    e = _run(dev, False, opt_cls=StraySGD)
    p = _run(dev, True, opt_cls=StraySGD)
    _assert_same(e, p)
    assert e.counts == (STEPS, 0, 0) and p.counts == EAGER and p.unrecorded == [], (e.counts, p.counts, p.unrecorded)


def _feature_pass_runs(dev, make_fn, calls):
    """the GMMN step's frozen-backbone feature pass (train-mode BatchNorm, live dropout, no gradients) through a ForwardPlan,
    with the plan and without it: [(outputs or the exception, state_dict, counters, forward plan)]"""
    from zs3_amd import functional as Fz
    from zs3_amd.plan import ForwardPlan
    bs = _batches(dev, calls)
    res = []
    for use_plan in (False, True):
        model = _deeplab(dev)
        Fz.manual_seed(21)
        fp = ForwardPlan(make_fn(model), [model], enabled=use_plan)
        outs = []
        with torch.no_grad():
            for b in bs:
                try:
                    outs.append(fp(b["image"]).clone())
                except RuntimeError as ex:
                    outs.append(ex)
        torch.cuda.synchronize()
        res.append((outs, {k: v.detach().clone() for k, v in model.state_dict().items()},
                    (fp.eager_calls, fp.recordings, fp.replays), fp))
    return res


def _assert_same_passes(e, p):
    assert len(e[0]) == len(p[0])
    for a, b in zip(e[0], p[0]):
        if isinstance(a, Exception):
            assert isinstance(b, Exception) and str(a) == str(b)
        else:
            assert torch.is_tensor(b) and torch.equal(a, b)
    assert not [k for k in e[1] if not torch.equal(e[1][k], p[1][k])]


def test_feature_pass_that_raises_while_recording_leaves_no_plan_behind(dev):
    """an exception inside the recorded call propagates; the plan is closed, the library records nothing, PLAN_RECORDING is off,
    no side-stream operand is held -- and the next calls settle, record and replay like eager calls"""
    from zs3_amd import functional as Fz
    from zs3_amd import ops
    from zs3_amd.plan import LaunchPlan

    def make_fn(model):
        n = [0]

        def fn(im):
            n[0] += 1
            out = ops.nhwc(model.forward_before_class_prediction(im))
            if n[0] == 3:                    # the plan run's recording call: after the pass has run (and been recorded)
                raise RuntimeError("feature pass failed")
            return out
        return fn

    e, p = _feature_pass_runs(dev, make_fn, 8)
    assert isinstance(p[0][2], RuntimeError) and not isinstance(p[0][3], Exception)
    # call 3 raised, calls 4-5 settle again, call 6 records, calls 7-8 replay
    assert e[2] == (8, 0, 0) and p[2] == (4, 1, 2), (e[2], p[2])
    assert not Fz.PLAN_RECORDING and Fz._plan_keep == []
    _assert_same_passes(e, p)
    assert len(p[3]._plans) == 1 and next(iter(p[3]._plans.values()))["plan"] is not None
    probe = LaunchPlan()                     # (a plan left recording would make this -2: another plan is recording)
    probe.begin()
    assert probe.end() == 0
    probe.close()
    for r in (e, p):
        r[3].close()


def test_feature_pass_ending_in_a_torch_op_stays_eager(dev):
    """fn's result is made by the tensor library (`feats * 2.0`): the recording sees the op, gives up, and every call returns
    exactly what the eager pass returns"""
    from zs3_amd import ops

    e, p = _feature_pass_runs(dev, lambda model: (lambda im: ops.nhwc(model.forward_before_class_prediction(im)) * 2.0), STEPS)
    print(f"\n[feature pass * 2] counts {p[2]}, unrecorded ops {p[3].unrecorded_ops}")
    _assert_same_passes(e, p)
    assert e[2] == (STEPS, 0, 0) and p[2] == EAGER, (e[2], p[2])
    assert p[3].unrecorded_ops and all("mul" in op for op in p[3].unrecorded_ops), p[3].unrecorded_ops
    for r in (e, p):
        r[3].close()
