"""The validation step on the device: `Trainer.validation` of the reference's scripts (train_pascal.py:115-172,
train_pascal_GMMN.py:313-475, the eval_*.py scripts) without full-resolution logits, without a host synchronisation per batch and
issued from C.

    step = ValidationStep(model, evaluator, weight=class_weights)     # the criterion's arguments, not the criterion
    model.eval(); evaluator.reset(); step.reset()
    for image, target in loader:
        step.step(image, target)            # eval forward -> low-resolution scores -> ONE fused launch: loss, argmax, confusion
    step.reduce()                           # sharded validation: one all-reduce; a no-op with one rank
    test_loss = step.test_loss              # the loop's only synchronisation
    mIoU = evaluator.Mean_Intersection_over_Union()

What a batch does: `model.forward_scores(image)` (the forward of `model(image)` up to, not including, the resize to image size) and
zs3_val_ce_confusion (csrc/pool_resize.hip), which samples the resized scores per target pixel and produces the weighted CE of
SegmentationLosses.CrossEntropyLoss, the device-side `test_loss += loss.item()`, the evaluator's confusion counts and the number
of pixels of every class in every image (`class_pixels`: the scripts' "does this batch contain unseen class k").  The
[B, C, 513, 513] logits -- 354 MB at B = 16, C = 21 -- never exist.

Like the training step (plan.StepPlan) and the GMMN feature pass (plan.ForwardPlan), the forward and the fused launch are RECORDED
and REPLAYED: two eager calls settle a configuration, the third is recorded under a private allocator pool while a dispatch mode
watches for device work of the tensor library (a pass that did some stays eager: `unrecorded_ops`), later calls replay the launches
from C with the two inputs (image, target) rebound by pointer.  The outputs live outside the pool and belong to the step or the
evaluator: the evaluator's device counters (re-pointed if the evaluator replaced them), `loss_ws`, the totals, `class_pixels`.
Another fingerprint -- the short last batch of a loader, a train / eval flip, another storage mode or stream -- settles and records
a plan of its own.  The step runs the model as the caller left it (the scripts call model.eval() themselves) under no_grad."""
import numpy as np
import torch

from . import functional as Fz
from . import ops
from ._lib import require_gpu
from .plan import ENABLED, LaunchPlan, _module_scalars, _TensorLibraryWork, collectives_recordable, poison_pool
from .utils.loss import _device_weight


class ValidationStep:
    """See the module docstring.  `model`: a zs3_amd DeepLab or its DataParallel wrapper; `evaluator`: utils.metrics.Evaluator;
    weight / ignore_index / batch_average: the arguments of SegmentationLosses (mode "ce"; weight=None is "ce_finetune").
    Counters `eager_calls / recordings / replays` as on the other plans."""

    MAX_PLANS = 2     # the loader's full batch and its short last one; each owns a pool the size of one eval forward

    def __init__(self, model, evaluator, weight=None, ignore_index=255, batch_average=True, enabled=None, warmup=2):
        self.model = model.module if hasattr(model, "module") else model
        self.evaluator = evaluator
        self.weight, self.ignore_index, self.batch_average = weight, int(ignore_index), bool(batch_average)
        self.enabled = ENABLED if enabled is None else bool(enabled)
        self.warmup = max(2, int(warmup))
        self.replays = self.recordings = self.eager_calls = 0
        self.unrecorded_ops = []      # the tensor library's device work seen by the last recording (non-empty: it gave up)
        self._plans = {}              # fingerprint -> state dict
        self._host_totals = np.zeros(2)    # [sum of the per-batch losses, number of batches] folded in from the device
        self._dev = None              # device buffers: totals fp64 [2], loss_ws fp32 [3], partial sums
        self._cp = {}                 # batch size -> int32 [B, C]
        self._last_cp = None

    # ------------------------------------------------------------------------------------------------ persistent outputs
    def _buffers(self, device, batch):
        """the outputs that outlive a call, allocated outside every recording: (totals, loss_ws, partial_ws, class_pixels)"""
        if self._dev is None or self._dev[0].device != device:
            self._fold()
            self.close()
            self._dev = (torch.zeros(2, dtype=torch.float64, device=device), torch.zeros(3, dtype=torch.float32, device=device),
                         ops.val_ws(device))
            self._cp = {}
        cp = self._cp.get(batch)
        if cp is None:
            cp = self._cp[batch] = torch.zeros((batch, self.evaluator.num_class), dtype=torch.int32, device=device)
        return self._dev + (cp,)

    def _fold(self):
        """device totals -> host (synchronises)"""
        if self._dev is not None:
            self._host_totals = self._host_totals + self._dev[0].cpu().numpy()
            self._dev[0].zero_()

    @property
    def totals(self):
        """numpy [2]: the sum of the per-batch losses and the number of batches since reset() (one synchronisation)"""
        self._fold()
        return self._host_totals

    @totals.setter
    def totals(self, value):
        self._fold()
        self._host_totals = np.asarray(value, dtype=np.float64).reshape(2).copy()

    @property
    def test_loss(self):
        """the scripts' `test_loss`: sum over the batches of the criterion's value, each rounded to fp32 like `loss.item()`"""
        return float(self.totals[0])

    @property
    def num_batches(self):
        return int(self.totals[1])

    @property
    def last_loss(self):
        """the last batch's loss as a device scalar (a view of loss_ws: reading it synchronises, holding it does not)"""
        return None if self._dev is None else self._dev[1][0]

    @property
    def loss_ws(self):
        """fp32 [3] on the device: {loss, sum w, sum w * nll} of the last batch"""
        return None if self._dev is None else self._dev[1]

    @property
    def class_pixels(self):
        """int32 [B, C] on the device: pixels of class c in image b of the last batch"""
        return self._last_cp

    def reset(self):
        """`test_loss = 0.0` (the evaluator has its own reset())"""
        self._host_totals = np.zeros(2)
        if self._dev is not None:
            self._dev[0].zero_()

    def close(self):
        for st in self._plans.values():
            if st.get("plan") is not None:
                st["plan"].close()
        self._plans = {}

    # ------------------------------------------------------------------------------------------------ one batch
    def _eager(self, image, target, bufs):
        totals, loss_ws, partial, cp = bufs
        scores = self.model.forward_scores(image)
        self.evaluator.add_batch_scores(target, scores, self._weight(image.device), self.ignore_index, self.batch_average,
                                        class_pixels=cp, partial_ws=partial, loss_ws=loss_ws, totals=totals)
        return scores

    def _weight(self, device):
        return None if self.weight is None else _device_weight(self.weight, device)

    def _fingerprint(self, image, target):
        w = self._weight(image.device)
        return (tuple(image.shape), image.dtype, tuple(image.stride()), tuple(target.shape), target.dtype, image.device,
                _module_scalars(self.model), tuple(p.data_ptr() for p in self.model.parameters()),
                None if w is None else w.data_ptr(), self.ignore_index, self.batch_average, self.evaluator.num_class,
                Fz.PLAN_EPOCH[0], ops.PREC_DEFAULT, ops.ACT_DTYPE, ops.FWD_F16, torch.cuda.current_stream(image.device).cuda_stream)

    def _prepare(self, image, target):
        require_gpu(image, target)
        if target.dtype not in (torch.float32, torch.int64):
            target = target.float()          # (outside every plan: the converted tensor is what a replay is pointed at)
        return image, target.contiguous()

    def step(self, image, target):
        """one validation batch; -> the low-resolution scores, fp32 [B, h, w, C] (the plan's own buffer after a replay: valid
        until the next call).  No host synchronisation."""
        image, target = self._prepare(image, target)
        with torch.no_grad():
            bufs = self._buffers(image.device, image.shape[0])
            self._last_cp = bufs[3]
            conf = self.evaluator._device_counters(image.device)
            if not self.enabled or not collectives_recordable():
                self.eager_calls += 1
                return self._eager(image, target, bufs)
            key = self._fingerprint(image, target)
            st = self._plans.get(key)
            if st is None:
                if len(self._plans) >= self.MAX_PLANS:
                    self.close()
                st = self._plans[key] = {"seen": 0, "plan": None, "giveup": False}
            if st["giveup"]:
                self.eager_calls += 1
                return self._eager(image, target, bufs)
            if st["plan"] is not None:
                return self._replay(st, image, target, conf)
            st["seen"] += 1
            if st["seen"] <= self.warmup:
                self.eager_calls += 1
                return self._eager(image, target, bufs)
            return self._record(st, image, target, bufs, conf)

    def _replay(self, st, image, target, conf):
        plan = st["plan"]
        for slot, ptr in (("image", image.data_ptr()), ("target", target.data_ptr()), ("conf", conf.data_ptr())):
            if ptr != st[slot]:
                for op, a in st[slot + "_at"]:
                    plan.set_ptr(op, a, ptr)
                st[slot] = ptr
        for k, old in enumerate(st["seeds"]):          # (a model left in training mode: live dropout, seeds in drawing order)
            new = Fz.next_seed()
            if plan.replace_u64(old, new) < 1:
                raise RuntimeError("ValidationStep: a recorded dropout seed is gone from the plan")
            st["seeds"][k] = new
        plan.replay()
        st["held"] = (image, target, conf)             # what the queued launches read and write stays referenced until the next call
        self.replays += 1
        return st["out"]

    def _record(self, st, image, target, bufs, conf):
        dev = image.device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self._weight(dev)                              # (its upload, if any, happens here -- not inside the recording)
        plan, pool = LaunchPlan(), torch.cuda.MemPool()
        drawn, next_seed = [], Fz.next_seed

        def logged_seed():
            v = next_seed()
            drawn.append(v)
            return v

        work, pool_id = _TensorLibraryWork(), pool.id
        torch.cuda.synchronize(dev)
        Fz.next_seed, Fz.PLAN_RECORDING = logged_seed, True
        torch._C._cuda_beginAllocateToPool(idx, pool_id)
        try:
            plan.begin()
            try:
                with work:
                    out = self._eager(image, target, bufs)
            finally:
                plan.end()
        except BaseException:
            # the pass itself failed: nothing was recorded that anyone will replay; the next calls settle and record again
            plan.close()
            del plan, pool
            torch.cuda.synchronize(dev)
            Fz._plan_keep.clear()
            st["seen"] = 0
            raise
        finally:
            torch._C._cuda_endAllocateToPool(idx, pool_id)
            Fz.next_seed, Fz.PLAN_RECORDING = next_seed, False
        Fz._plan_keep.clear()
        self.unrecorded_ops = work.unrecorded()
        if self.unrecorded_ops:
            plan.close()                   # (the tensor library did device work in the pass: a replay would miss it -- stay eager)
            st["giveup"] = True
            return out
        at = {"image": plan.find_ptr(image.data_ptr()), "target": plan.find_ptr(target.data_ptr()),
              "conf": plan.find_ptr(conf.data_ptr())}
        distinct = len({image.data_ptr(), target.data_ptr(), conf.data_ptr()}) == 3
        if not all(at.values()) or not distinct or len(set(drawn)) != len(drawn) or not plan.find_ptr(out.data_ptr()):
            plan.close()                   # (the pass copied an input, or its result is not what a recorded launch wrote: stay eager)
            st["seen"] = 0
            return out
        st.update(plan=plan, pool=pool, seeds=list(drawn), out=out, held=(image, target, conf),
                  image=image.data_ptr(), target=target.data_ptr(), conf=conf.data_ptr(),
                  image_at=at["image"], target_at=at["target"], conf_at=at["conf"])
        self.recordings += 1
        return out

    # ------------------------------------------------------------------------------------------------ checking a live plan
    def verify(self, image, target, poison=True):
        """Replay the recorded plan of this batch's configuration and run the same batch eagerly, both from the same counters, and
        compare bit for bit: scores, loss_ws, class_pixels, the increments of the confusion counters and of the totals.  `poison`: the
        free memory of the plan's pool is filled with NaN patterns first (plan.poison_pool), so a launch missing from the plan shows
        up.  Leaves evaluator and totals as they were.  Returns the list of mismatching names (empty = identical)."""
        image, target = self._prepare(image, target)
        with torch.no_grad():
            st = self._plans.get(self._fingerprint(image, target))
            if st is None or st["plan"] is None:
                raise RuntimeError("ValidationStep.verify: no recorded plan for this batch (call step() warmup + 1 times first)")
            bufs = self._buffers(image.device, image.shape[0])
            totals, loss_ws, _, cp = bufs
            conf = self.evaluator._device_counters(image.device)
            conf0, totals0 = conf.clone(), totals.clone()
            rng = Fz._rng.getstate() if Fz._rng is not None else None

            def snapshot(scores):
                torch.cuda.synchronize(image.device)
                return {"scores": scores.clone(), "loss_ws": loss_ws.clone(), "class_pixels": cp.clone(),
                        "confusion": conf - conf0, "totals": totals.clone()}

            if poison:
                poison_pool(st["pool"], image.device)
            got = snapshot(self._replay(st, image, target, conf))
            self.replays -= 1
            conf.copy_(conf0)
            totals.copy_(totals0)
            if rng is not None:
                Fz._rng.setstate(rng)
            want = snapshot(self._eager(image, target, bufs))
            conf.copy_(conf0)
            totals.copy_(totals0)
            same = lambda a, b: torch.equal(a, b) or (a.is_floating_point() and torch.equal(a.isnan(), b.isnan())
                                                      and torch.equal(a.nan_to_num(), b.nan_to_num()))
            return [k for k in want if not same(got[k], want[k])]

    # ------------------------------------------------------------------------------------------------ several ranks
    def reduce(self, group=None):
        """End of a SHARDED validation (every rank validated its own part of the set): one SUM all-reduce of the C x C confusion
        counters together with the totals, after which every rank's evaluator holds the data set's confusion matrix.  One collective
        per validation, none per batch; on the gloo backend it runs on host copies.  A no-op without torch.distributed or with one
        rank.  The confusion matrix -- and every metric of the evaluator -- is exact under any sharding (integer counts, carried as
        float64 like the evaluator's own matrix: exact below 2^53 pixels per cell); `test_loss` becomes the sum of every rank's
        own per-batch losses, each normalised over that rank's batch, which is not the loss of the gathered batches."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
            return
        c = self.evaluator.num_class
        buf = torch.from_numpy(np.concatenate([np.asarray(self.evaluator.confusion_matrix, dtype=np.float64).reshape(-1),
                                               self.totals]))
        on_device = "gloo" not in str(dist.get_backend(group)) and self._dev is not None
        if on_device:
            buf = buf.to(self._dev[0].device)
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        buf = buf.cpu().numpy()
        self.evaluator.confusion_matrix = buf[:c * c].reshape(c, c)
        self.totals = buf[c * c:]


def validate(model, loader, evaluator, weight=None, ignore_index=255, batch_average=True, unseen_classes_idx_metric=(),
             saved_validation_images=0, step=None, group=None):
    """The loop of train_pascal_GMMN.py:337-375 on the device step.  `loader` yields the scripts' samples (dicts with "image" and
    "label") or (image, target) pairs; CPU batches are moved to the model's device.  The caller puts the model into eval mode, as
    the scripts do.  -> (test_loss, evaluator, saved): saved[k] is the list of (image, target, scores) CPU batches, at most
    `saved_validation_images` of them, that contain unseen class k -- scores are the low-resolution [B, h, w, C] ones.  Batches are
    chosen from the step's `class_pixels`: one host read per batch, and only while something is still to be saved; otherwise the
    loop synchronises once, at its end.  `step`: a ValidationStep to reuse across epochs (it keeps its recorded plans)."""
    own = step is None
    if own:
        step = ValidationStep(model, evaluator, weight, ignore_index, batch_average)
    device = next(step.model.parameters()).device
    evaluator.reset()
    step.reset()
    classes = [int(k) for k in unseen_classes_idx_metric]
    saved = {k: [] for k in classes}
    for sample in loader:
        image, target = (sample["image"], sample["label"]) if isinstance(sample, dict) else sample[:2]
        image, target = image.to(device), target.to(device)
        scores = step.step(image, target)
        if classes and saved_validation_images > 0 and any(len(saved[k]) < saved_validation_images for k in classes):
            present = step.class_pixels.sum(dim=0).cpu()       # the batch's one host read
            for k in classes:
                if int(present[k]) > 0 and len(saved[k]) < saved_validation_images:
                    saved[k].append((image.cpu(), target.cpu(), scores.cpu()))
    step.reduce(group)
    test_loss = step.test_loss
    if own:
        step.close()
    return test_loss, evaluator, saved
