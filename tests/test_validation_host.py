"""Host side of the device-resident validation step (zs3_amd/validation.py, zs3_val_ce_confusion): what needs no GPU -- the entry
point's place in the C ABI, the refusal to run on CPU tensors, and `ValidationStep.reduce` in a two-process gloo world."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_entry_point_is_declared_exported_and_wrapped():
    from zs3_amd import build
    sigs = {name: params for _, name, params in build.parse_header()}
    assert "zs3_val_ce_confusion" in sigs and "zs3_val_ws_doubles" in sigs
    params = sigs["zs3_val_ce_confusion"]
    # a launching entry point (the plan's recording wrapper exists for it) on fp32 class scores: no `int io`
    assert params[-1] == ("void*", "stream") and params[-2] != ("int", "io") and ("int", "io") not in params
    assert [n for _, n in params] == ["scores", "ld", "N", "H", "W", "C", "target", "target_is_i64", "Ho", "Wo", "weight",
                                      "ignore_index", "batch", "conf", "class_pixels", "partial_ws", "loss_ws", "totals", "stream"]
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "zs3_val_ce_confusion") and lib.zs3_val_ws_doubles() >= 2
    assert "#define zs3_val_ce_confusion zs3_val_ce_confusion__impl" in open(os.path.join(build.GEN, "plan_rename.h")).read()
    wrappers = open(os.path.join(build.GEN, "plan_wrappers.hip")).read()
    assert 'extern "C" int zs3_val_ce_confusion(' in wrappers and '{"zs3_val_ce_confusion", ' in wrappers
    # argument validation happens before any launch (no GPU here: a launch would fail differently)
    from zs3_amd._lib import lib as bound
    L = bound()
    for n, c in ((1, 0), (1, 129), (0, 21)):
        assert L.zs3_val_ce_confusion(None, c, n, 5, 5, c, None, 0, 9, 9, None, 255, n, None, None, None, None, None, None) == -1


def test_validation_step_has_no_cpu_fallback():
    from zs3_amd._lib import Zs3HipError
    from zs3_amd.modeling.deeplab import DeepLab
    from zs3_amd.utils.metrics import Evaluator
    from zs3_amd.validation import ValidationStep, validate
    torch.manual_seed(0)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False).eval()
    ev = Evaluator(21)
    image, target = torch.randn(1, 3, 33, 33), torch.zeros(1, 33, 33)
    for enabled in (True, False):
        step = ValidationStep(model, ev, enabled=enabled)
        with pytest.raises(Zs3HipError):
            step.step(image, target)
        assert (step.eager_calls, step.recordings, step.replays) == (0, 0, 0)
    with pytest.raises(Zs3HipError):
        validate(model, [(image, target)], ev)
    with pytest.raises(Zs3HipError):
        ev.add_batch_scores(target, torch.randn(1, 9, 9, 21))
    assert ev.confusion_matrix.sum() == 0
    # the wrapper of torch.nn.DataParallel is looked through, like the trainers do
    assert ValidationStep(torch.nn.DataParallel(model), ev).model is model


def _matrices(rank, c=5):
    rs = np.random.RandomState(10 + rank)
    return rs.randint(0, 2 ** 40, size=(c, c)).astype(np.int64), np.array([0.25 + 1.5 * rank + 2.0 ** -30, 3.0 + rank])


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from zs3_amd.utils.metrics import Evaluator
        from zs3_amd.validation import ValidationStep
        cm, tot = _matrices(rank)
        ev = Evaluator(5)
        ev.confusion_matrix = cm
        step = ValidationStep(None, ev)
        step.totals = tot
        step.reduce()
        got = np.asarray(ev.confusion_matrix)
        q.put((rank, got.astype(np.int64).tolist(), bool((got == got.astype(np.int64)).all()), step.totals.tolist(),
               step.test_loss, step.num_batches))
    finally:
        dist.destroy_process_group()


def test_reduce_sums_counters_and_totals_on_gloo():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (cm0, t0), (cm1, t1) = _matrices(0), _matrices(1)
    assert not np.array_equal(cm0, cm1)
    for rank, cm, integral, tot, test_loss, nb in out:
        assert integral and np.array_equal(np.array(cm, dtype=np.int64), cm0 + cm1), rank       # integers: exact
        assert tot == (t0 + t1).tolist() and test_loss == float(t0[0] + t1[0]) and nb == 7, rank


def test_reduce_is_a_no_op_in_a_single_process():
    from zs3_amd.utils.metrics import Evaluator
    from zs3_amd.validation import ValidationStep
    cm, tot = _matrices(0)
    ev = Evaluator(5)
    ev.confusion_matrix = cm
    step = ValidationStep(None, ev)
    step.totals = tot
    step.reduce()
    assert np.array_equal(ev.confusion_matrix, cm.astype(np.float64)) and step.totals.tolist() == tot.tolist()
    step.reset()
    assert step.test_loss == 0.0 and step.num_batches == 0
