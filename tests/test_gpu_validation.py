"""The device-resident validation step: zs3_val_ce_confusion (csrc/pool_resize.hip: upsample + weighted CE + argmax + confusion +
class pixel counts in one pass over the target pixels) against the two- / three-kernel composition it replaces and the float64
oracle, and zs3_amd.validation.ValidationStep / validate against the scripts' own validation loop written with the older pieces
(`model(image)`, the criterion, `Evaluator.add_batch_logits`, `.item()` per batch)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def ulp32(x):
    """spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def _class_weights(classes, dev):
    w = torch.ones(classes, device=dev)
    w[[10, 14]] = 100.0
    return w


def _labels(g, b, classes, HW):
    gt = torch.randint(0, classes, (b, *HW), generator=g)
    brd = min(8, HW[0] // 8)                      # the 8-pixel border of 255 of the data sets' crops
    gt[:, :brd] = 255
    gt[:, -brd:] = 255
    gt[:, :, :brd] = 255
    gt[:, :, -brd:] = 255
    gt[0, HW[0] // 2:HW[0] // 2 + 5] = 255        # five rows of 255 inside the first image
    return gt


def _scores(g, b, classes, hw, pad, dev):
    """fp32 [b, h, w, C] class scores in NHWC; pad > 0: a channel slice of a wider buffer (pixel stride ld = C + pad)"""
    full = (3.0 * torch.randn(b, *hw, classes + pad, generator=g)).to(dev)
    return full[..., :classes] if pad else full


def _fused(scores, tgt, classes, weight, batch, conf=None, totals=None):
    from zs3_amd import ops
    dev = scores.device
    conf = torch.zeros((classes, classes), dtype=torch.int64, device=dev) if conf is None else conf
    cp = torch.full((scores.shape[0], classes), -7, dtype=torch.int32, device=dev)     # (overwritten, not accumulated)
    totals = torch.zeros(2, dtype=torch.float64, device=dev) if totals is None else totals
    loss_ws = ops.val_ce_confusion(scores, tgt, conf, weight, 255, batch, class_pixels=cp, totals=totals)
    return conf, cp, loss_ws, totals


SHAPES = [(21, (33, 33), (129, 129), 3, 0), (21, (33, 33), (129, 129), 3, 3), (60, (17, 19), (65, 73), 3, 0),
          (60, (17, 19), (65, 73), 3, 4), (21, (40, 40), (40, 40), 3, 0), (21, (40, 40), (40, 40), 3, 3),
          (21, (129, 129), (513, 513), 16, 0), (60, (129, 129), (513, 513), 2, 0)]


@pytest.mark.parametrize("classes,hw,HW,b,pad", SHAPES)
def test_fused_validation_kernel_against_the_composition_and_the_oracle(dev, classes, hw, HW, b, pad):
    """Items 1-4 and 6 of the feature's check list.  Confusion counts equal (integers) those of Evaluator.add_batch_logits and of
    the oracle on argmax of the materialised upsample, two calls give exactly twice; class_pixels equals bincount per image.
    Loss: the yardstick `ref` is the float64 oracle criterion on the materialised fp32 upsample of zs3_bilinear_fwd; e_old is the
    distance of the two-kernel path (Fz.bilinear + cross_entropy_2d), e_new that of the fused launch.  Control on the inputs:
    e_old <= 2e-6 |ref| + 1e-7 (the project's CE tolerance).  Requirement: e_new <= e_old + 2 ulp_fp32(|ref|) -- derived, not
    measured: on the same bilerp values and the per-pixel terms of ce_tile_kernel the two paths differ only in the order of a
    double accumulation over <= 4.2e6 non-negative terms (relative error <= P * 2^-53 ~ 5e-10, far below an fp32 ulp), so the fp32
    results can differ by one rounding of the quotient and one of the 1/B product.  loss_ws[1:3] within 1 fp32 ulp of the
    two-kernel path's.  totals[0] after k calls equals the float64 sum, in call order, of the k fp32 losses.  Two runs from the
    same inputs are bit-identical."""
    import zs3_oracle as zo
    from zs3_amd import functional as Fz, ops
    from zs3_amd.utils.loss import cross_entropy_2d
    from zs3_amd.utils.metrics import Evaluator
    g = torch.Generator().manual_seed(classes + hw[0] + pad)
    scores = _scores(g, b, classes, hw, pad, dev)
    gt = _labels(g, b, classes, HW)
    up = Fz.bilinear(scores, HW) if hw != HW else scores            # [b, H, W, C]: the parent's kernel, materialised
    up_nchw = ops.nchw(up)
    want_conf = zo.confusion_matrix(gt.numpy(), up_nchw.argmax(1).cpu().numpy(), classes)
    want_cp = torch.stack([torch.bincount(gt[i][gt[i] < classes].reshape(-1), minlength=classes) for i in range(b)])
    up64 = up_nchw.cpu().double()
    weights = {"ce": _class_weights(classes, dev), "ce_finetune": None}
    for tgt in (gt.float().to(dev), gt.to(dev)):
        ev = Evaluator(classes)
        ev.add_batch_logits(tgt, ops.nchw(scores))
        assert np.array_equal(ev.confusion_matrix, want_conf)
        for mode, weight in weights.items():
            for batch_average in (True, False):
                batch = b if batch_average else 0
                conf, cp, loss_ws, totals = _fused(scores, tgt, classes, weight, batch)
                first = [t.clone() for t in (conf, cp, loss_ws, totals)]
                assert np.array_equal(conf.cpu().numpy(), want_conf)                        # item 1
                assert torch.equal(cp.cpu().long(), want_cp)                                # item 3
                crit = zo.SegmentationLosses(weight=None if weight is None else weight.cpu().double(),
                                             batch_average=batch_average).build_loss(mode)
                ref = float(crit(up64, gt))
                with torch.no_grad():
                    old = cross_entropy_2d(up_nchw, tgt, weight, 255, batch_average, group=None)
                old_ws = old._base if old._base is not None else None
                e_old, e_new = abs(float(old) - ref), abs(float(loss_ws[0]) - ref)
                print(f"C={classes} {hw}->{HW} b={b} pad={pad} {tgt.dtype} {mode} batch_average={batch_average}: ref={ref:.9g} "
                      f"e_old={e_old:.3g} e_new={e_new:.3g} ulp={ulp32(ref):.3g}")
                assert e_old <= 2e-6 * abs(ref) + 1e-7                                      # control on the inputs
                assert e_new <= e_old + 2 * ulp32(ref)                                      # item 2
                assert old_ws is not None and old_ws.numel() == 3
                for k in (1, 2):
                    assert abs(float(loss_ws[k]) - float(old_ws[k])) <= ulp32(old_ws[k]), (k, float(loss_ws[k]), float(old_ws[k]))
                # a second call into the same counters: exactly twice; totals: the float64 sum of the fp32 losses, in order
                losses = [float(loss_ws[0])]
                for tg2 in (tgt, tgt.flip(0)):
                    _, _, lw2, _ = _fused(scores, tg2, classes, weight, batch, conf=conf, totals=totals)
                    losses.append(float(lw2[0]))
                    if tg2 is tgt:
                        assert np.array_equal(conf.cpu().numpy(), 2 * want_conf)
                acc = 0.0
                for v in losses:
                    acc += v                                                                # (Python floats: float64, call order)
                assert float(totals[0]) == acc and float(totals[1]) == 3.0                  # item 4
                again = _fused(scores, tgt, classes, weight, batch)                         # item 6
                assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_fused_validation_kernel_edges(dev):
    """Items 5 and 7: a batch whose labels are all 255 gives what cross_entropy_2d gives on that input (0 / 0: NaN, which the
    totals then carry as the reference's test_loss would) and leaves the counters untouched; bad arguments return -1 and launch
    nothing (the outputs keep their bytes)."""
    from zs3_amd import functional as Fz, ops
    from zs3_amd._lib import I, P, lib, stream
    from zs3_amd.utils.loss import cross_entropy_2d
    g = torch.Generator().manual_seed(5)
    classes, hw, HW, b = 21, (33, 33), (129, 129), 2
    scores = _scores(g, b, classes, hw, 0, dev)
    tgt = torch.full((b, *HW), 255.0, device=dev)
    conf, cp, loss_ws, totals = _fused(scores, tgt, classes, _class_weights(classes, dev), b)
    with torch.no_grad():
        old = cross_entropy_2d(ops.nchw(Fz.bilinear(scores, HW)), tgt, _class_weights(classes, dev), 255, True, group=None)
    assert torch.isnan(old) and torch.isnan(loss_ws[0]) and float(loss_ws[1]) == 0.0
    assert int(conf.abs().sum()) == 0 and int(cp.abs().sum()) == 0
    assert torch.isnan(totals[0]) and float(totals[1]) == 1.0
    part = ops.val_ws(dev)
    for n, c in ((b, 0), (b, 129), (0, classes)):
        conf = torch.full((classes, classes), 3, dtype=torch.int64, device=dev)
        cp = torch.full((b, classes), -7, dtype=torch.int32, device=dev)
        ws = torch.full((3,), 5.0, device=dev)
        tot = torch.full((2,), 9.0, dtype=torch.float64, device=dev)
        rc = lib().zs3_val_ce_confusion(P(scores), I(classes), I(n), I(hw[0]), I(hw[1]), I(c), P(tgt), I(0), I(HW[0]), I(HW[1]), None,
                                        I(255), I(b), P(conf), P(cp), P(part), P(ws), P(tot), stream())
        torch.cuda.synchronize()
        assert rc == -1
        assert bool((conf == 3).all()) and bool((cp == -7).all()) and bool((ws == 5).all()) and bool((tot == 9).all())
    # C = 128, the largest class count: the block histogram alone fills the default LDS limit; counts against torch
    classes = 128
    scores = _scores(g, 1, classes, (9, 9), 0, dev)
    gt = _labels(g, 1, classes, (33, 33))
    conf, cp, loss_ws, _ = _fused(scores, gt.to(dev), classes, None, 1)
    up = ops.nchw(Fz.bilinear(scores, (33, 33)))
    keep = gt < classes
    want = torch.bincount(gt[keep] * classes + up.argmax(1).cpu()[keep], minlength=classes * classes).view(classes, classes)
    assert torch.equal(conf.cpu(), want) and int(cp.sum()) == int(keep.sum())
    ref = torch.nn.functional.cross_entropy(up.cpu().double(), gt, ignore_index=255)
    assert abs(float(loss_ws[0]) - float(ref)) <= 2e-6 * abs(float(ref)) + 1e-7


# ---------------------------------------------------------------------------------------------------------------- the step
def _tamed(dev, seed=1):
    from zs3_amd.modeling.deeplab import DeepLab
    torch.manual_seed(seed)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False)
    for name, mod in model.named_modules():
        if name.endswith("bn3"):
            mod.weight.data.fill_(0.1)
    return model.to(dev).eval()


class _NoHostSync:
    """nothing inside may wait for the device: torch's own sync debugging (where the build honours it) plus stubs on the calls a
    Python validation loop synchronises through"""

    def __enter__(self):
        self.saved = (torch.Tensor.item, torch.Tensor.cpu, torch.Tensor.tolist, torch.cuda.synchronize)

        def refuse(*a, **k):
            raise AssertionError("host synchronisation inside a replayed validation batch")

        torch.Tensor.item = torch.Tensor.cpu = torch.Tensor.tolist = refuse
        torch.cuda.synchronize = refuse
        self.mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        torch.Tensor.item, torch.Tensor.cpu, torch.Tensor.tolist, torch.cuda.synchronize = self.saved


@pytest.mark.parametrize("size,b,storage", [(65, 2, torch.float32), (65, 2, torch.bfloat16), (513, 16, torch.float32)])
def test_validation_step_replayed_equals_eager_and_the_composition(dev, size, b, storage):
    """Items 8-10: eight batches through ValidationStep(enabled=True) (two settling calls, one recording, five replays, nothing
    unrecorded, no host synchronisation while replaying) and enabled=False: confusion matrix equal, test_loss bit-equal; verify()
    (replay against NaN-poisoned pool memory vs the eager call) finds no mismatch.  The same batches through the older composition
    (model(image), criterion, add_batch_logits, .item() per batch): confusion matrix equal, test_loss within
    sum_b 2 ulp_fp32(|loss_b|) (the margin of the kernel test, batch by batch: both paths' scores come from the same eval
    forward).  A shorter ninth batch runs (eagerly: it settles anew) and is counted; BatchNorm buffers are untouched by
    validation; a model.train() flip is not replayed from the eval-mode plan."""
    from zs3_amd import ops
    from zs3_amd.utils.loss import SegmentationLosses
    from zs3_amd.utils.metrics import Evaluator
    from zs3_amd.utils.synthetic import make_batch
    from zs3_amd.validation import ValidationStep
    ops.set_storage(storage)
    try:
        model = _tamed(dev)
        weight = _class_weights(21, dev)
        batches = [make_batch(b, size, 21, [10, 14], seed=70 + i, device=dev) for i in range(8)]
        buffers0 = {k: v.clone() for k, v in model.named_buffers()}

        def run(enabled):
            ev = Evaluator(21)
            step = ValidationStep(model, ev, weight=weight, enabled=enabled)
            for i, bt in enumerate(batches):
                if enabled and i >= 3:
                    with _NoHostSync():
                        step.step(bt["image"], bt["label"])
                else:
                    step.step(bt["image"], bt["label"])
            return step, ev

        step, ev = run(True)
        assert step.unrecorded_ops == []
        assert (step.eager_calls, step.recordings, step.replays) == (2, 1, 5)
        last_cp = step.class_pixels.clone()
        test_loss, cm = step.test_loss, np.array(ev.confusion_matrix)
        assert step.num_batches == 8 and float(step.last_loss) > 0
        step_e, ev_e = run(False)
        assert (step_e.eager_calls, step_e.recordings, step_e.replays) == (8, 0, 0)
        assert np.array_equal(cm, ev_e.confusion_matrix) and cm.sum() > 0
        assert test_loss == step_e.test_loss and np.isfinite(test_loss)
        assert torch.equal(last_cp, step_e.class_pixels)
        lab = batches[-1]["label"]
        assert torch.equal(last_cp.cpu().long(),
                           torch.stack([torch.bincount(lab[i][lab[i] < 21].long().reshape(-1), minlength=21) for i in range(b)]).cpu())
        assert step.verify(batches[0]["image"], batches[0]["label"]) == []
        assert step.test_loss == test_loss and np.array_equal(ev.confusion_matrix, cm)      # verify() leaves them as they were

        # item 9: the composition a script had to write before
        crit = SegmentationLosses(weight=weight, cuda=True).build_loss("ce")
        ev_p, loss_p, bound = Evaluator(21), 0.0, 0.0
        with torch.no_grad():
            for bt in batches:
                out = model(bt["image"])
                v = crit(out, bt["label"]).item()
                loss_p += v
                bound += 2 * ulp32(v)
                ev_p.add_batch_logits(bt["label"], out)
        print(f"size={size} b={b} {storage}: test_loss fused={test_loss!r} composition={loss_p!r} bound={bound:.3g}")
        assert np.array_equal(cm, ev_p.confusion_matrix)
        assert abs(test_loss - loss_p) <= bound

        # item 10: a short last batch, buffers, a train() flip
        short = make_batch(1, size, 21, [10, 14], seed=99, device=dev)
        step.step(short["image"], short["label"])
        assert (step.eager_calls, step.recordings, step.replays) == (3, 1, 5)    # (verify's calls are not counted; +1 eager)
        assert step.num_batches == 9 and ev.confusion_matrix.sum() == cm.sum() + float((short["label"] < 21).sum())
        for k, v in model.named_buffers():
            assert torch.equal(v, buffers0[k]), k
        step.step(batches[1]["image"], batches[1]["label"])
        assert step.replays == 6                                                 # the full-batch plan is still there
        model.train()
        try:
            step.step(batches[1]["image"], batches[1]["label"])
            assert (step.eager_calls, step.replays) == (4, 6)                    # another fingerprint: settles again
        finally:
            model.eval()
        step.close()
    finally:
        ops.set_storage(torch.float32)


def test_validate_loop_saves_the_batches_with_unseen_classes(dev):
    """Item 11: validate() on a six-batch list loader with classes 10 / 14 present in known batches saves exactly those batches, up
    to the cap, and the evaluator's metric tuples equal the host path fed with argmax of model(image)."""
    from zs3_amd.utils.metrics import Evaluator
    from zs3_amd.utils.synthetic import make_batch
    from zs3_amd.validation import validate
    model = _tamed(dev)
    unseen, seen = [10, 14], [c for c in range(21) if c not in (10, 14)]
    present = {0: (), 1: (10,), 2: (14,), 3: (10, 14), 4: (10,), 5: ()}
    loader = []
    for i in range(6):
        bt = make_batch(2, 65, 21, unseen, seed=30 + i, device="cpu")            # (batch < 4: no unseen class of its own)
        label = bt["label"]
        assert not any(bool((label == u).any()) for u in unseen)
        for j, u in enumerate(present[i]):
            label[1, 20 + 8 * j:24 + 8 * j, 30:40] = float(u)
        loader.append({"image": bt["image"], "label": label})
    ev = Evaluator(21, seen, unseen)
    test_loss, ev_out, saved = validate(model, loader, ev, weight=_class_weights(21, dev), unseen_classes_idx_metric=unseen,
                                        saved_validation_images=2)
    assert ev_out is ev and np.isfinite(test_loss) and test_loss > 0
    for u, want in ((10, [1, 3]), (14, [2, 3])):
        assert len(saved[u]) == len(want)
        for (img, tg, sc), i in zip(saved[u], want):
            assert torch.equal(img, loader[i]["image"]) and torch.equal(tg, loader[i]["label"])
            assert not sc.is_cuda and sc.shape[0] == 2 and sc.shape[-1] == 21
    host = Evaluator(21, seen, unseen)
    with torch.no_grad():
        for s in loader:
            out = model(s["image"].to(dev))
            host.add_batch(s["label"].numpy(), out.argmax(1).cpu().numpy())
    for name in ("Pixel_Accuracy", "Pixel_Accuracy_Class", "Mean_Intersection_over_Union",
                 "Frequency_Weighted_Intersection_over_Union"):
        np.testing.assert_equal(getattr(ev, name)(), getattr(host, name)())
    # nothing to save: no per-batch host read is needed and none of the saved lists fills
    _, _, none = validate(model, loader, Evaluator(21, seen, unseen), unseen_classes_idx_metric=unseen, saved_validation_images=0)
    assert none == {10: [], 14: []}
