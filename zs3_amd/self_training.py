"""Pseudo-labels for the self-training stage (ZS5 of the paper) on the device.  The reference's data sets take `weak_label=True`
and then read, for every image that contains unseen classes, a label map from `weak_label_pascal_10_unseen_top_by_image_25.0/`
(dataloaders/datasets/pascal.py:87-98, sbd.py:103-111, context.py:134-142): the model's own prediction on the pixels it was never
given a label for, kept where it is among the most confident 25 % (VOC) or 75 % (Context) of its image.  The reference ships
nothing that writes those maps; this module does.

    step = PseudoLabelStep(model, unseen_classes_idx, top_percent=25.0, group="image")
    model.eval()
    for sample, maps in pseudo_label_loader(model, loader, step=step):      # maps: uint8 [B, H, W] on the host
        ...                                                                 # write them where the data set looks for them
    kept, eligible = step.total_selected, step.total_count                  # int64 [C], the loop's only synchronisation

What a batch does: `model.forward_scores(image)` (low-resolution class scores) and two launches of the library:
zs3_pl_candidates (per unlabelled pixel the best unseen class and its softmax probability, sampled at the pixel's position --
the [B, C, H, W] logits never exist) and zs3_pl_select (an exact top-p % per bucket by radix select).  The selection rule: a
pixel is ELIGIBLE when its label is one of `unlabelled` (default: the unseen classes) or equals `unlabelled_value`, never when
it is ignore_index; eligible pixels are bucketed by (image, predicted class) for group "image_class" or by image for "image";
a bucket of m pixels keeps k = min(m, ceil(m * p / 100)) of them: those with conf >= t, t the k-th largest confidence of the
bucket -- pixels tied with the k-th are all kept.  `labels` is the target where a pixel is not eligible, the predicted class
where it is kept and ignore_index otherwise: it goes into SegmentationLosses as it is."""
import torch

from . import ops
from ._lib import require_gpu


class PseudoLabelStep:
    """See the module docstring.  `model`: a zs3_amd DeepLab or its DataParallel wrapper (run as the caller left it, under
    no_grad); `unseen_classes`: the candidate classes.  Outputs and workspace are allocated once per batch shape and reused: what
    step() returns and `last_stats` are valid until the next call with that shape."""

    def __init__(self, model, unseen_classes, top_percent=25.0, group="image_class", unlabelled=None, unlabelled_value=None,
                 ignore_index=255):
        self.model = model.module if hasattr(model, "module") else model
        self.candidates = sorted({int(c) for c in unseen_classes})
        self.unlabelled = None if unlabelled is None else sorted({int(c) for c in unlabelled})
        self.unlabelled_value = unlabelled_value
        self.top_percent, self.group, self.ignore_index = float(top_percent), group, int(ignore_index)
        if group not in ops.PL_GROUPS:
            raise ValueError(f"PseudoLabelStep: group is one of {sorted(ops.PL_GROUPS)}, not {group!r}")
        if not 0.0 <= self.top_percent <= 100.0:
            raise ValueError("PseudoLabelStep: top_percent in [0, 100] expected")
        if not self.candidates:
            raise ValueError("PseudoLabelStep: no candidate class")
        self.last_stats = None
        self.batches = 0
        self._bufs = {}          # (target shape, target dtype, C, device) -> preallocated outputs + workspace
        self._totals = None      # int64 [2, C] on the device: running sums of count / selected

    def _buffers(self, target, c):
        dev = target.device
        if self._totals is None or self._totals.device != dev or self._totals.shape[1] != c:
            self._totals = torch.zeros((2, c), dtype=torch.int64, device=dev)
        key = (tuple(target.shape), target.dtype, c, dev)
        b = self._bufs.get(key)
        if b is None:
            n, shape = target.shape[0], tuple(target.shape)
            b = self._bufs[key] = dict(labels=torch.empty_like(target), cls_map=torch.empty(shape, dtype=torch.uint8, device=dev),
                                       conf_map=torch.empty(shape, dtype=torch.float32, device=dev),
                                       count=torch.empty((n, c), dtype=torch.int32, device=dev),
                                       selected=torch.empty((n, c), dtype=torch.int32, device=dev),
                                       threshold=torch.empty((n, c), dtype=torch.float32, device=dev), ws=ops.pl_ws(n, c, dev))
        return b

    def label_scores(self, scores, target):
        """the step's tail: labels from class scores fp32 [B, h, w, C] and a float32 / int64 target [B, H, W].  Two library
        calls on preallocated buffers, nothing else: no tensor-library device work, no host synchronisation."""
        b = self._buffers(target, scores.shape[-1])
        labels, self.last_stats = ops.pseudo_label(scores, target, self.candidates, self.top_percent, self.group, self.unlabelled,
                                                   self.unlabelled_value, self.ignore_index, totals=self._totals, **b)
        self.batches += 1
        return labels

    def step(self, image, target):
        """one batch -> labels on the device (dtype and shape of the target; a target that is neither float32 nor int64 is read
        as float32)"""
        require_gpu(image, target)
        if target.dtype not in (torch.float32, torch.int64):
            target = target.float()
        target = target.contiguous()
        with torch.no_grad():
            scores = self.model.forward_scores(image)
            return self.label_scores(scores, target)

    @property
    def total_count(self):
        """int64 [C] on the host: eligible pixels per predicted class over all batches since reset() (synchronises)"""
        return torch.zeros(0, dtype=torch.int64) if self._totals is None else self._totals[0].cpu()

    @property
    def total_selected(self):
        """int64 [C] on the host: kept pixels per class over all batches since reset() (synchronises)"""
        return torch.zeros(0, dtype=torch.int64) if self._totals is None else self._totals[1].cpu()

    @property
    def totals_device(self):
        """int64 [2, C] on the device ({count, selected}); holding it does not synchronise"""
        return self._totals

    def reset(self):
        self.batches = 0
        if self._totals is not None:
            self._totals.zero_()


def pseudo_label_loader(model, loader, step=None, **kw):
    """Generator over `loader` -- the reference's samples (dicts with "image" and "label") or (image, target) pairs; CPU batches
    are moved to the model's device -- yielding (sample, maps) with maps the batch's pseudo-label map as uint8 [B, H, W] on the
    host, what the data sets read back from their weak-label directory.  It runs ONE BATCH BEHIND: the maps of batch i are copied
    into pinned memory asynchronously and handed out after batch i + 1 has been queued, so the copy overlaps the next forward;
    the only wait is on that copy's event.  `step`: a PseudoLabelStep to reuse; otherwise one is made from `kw`
    (unseen_classes=..., top_percent=..., group=...).  The caller puts the model into eval mode."""
    if step is None:
        step = PseudoLabelStep(model, **kw)
    device = next(step.model.parameters()).device
    pinned, pending, k = {}, None, 0
    for sample in loader:
        image, target = (sample["image"], sample["label"]) if isinstance(sample, dict) else sample[:2]
        labels = step.step(image.to(device, non_blocking=True), target.to(device, non_blocking=True))
        slot = (k & 1, tuple(labels.shape))
        host = pinned.get(slot)
        if host is None:
            host = pinned[slot] = torch.empty(tuple(labels.shape), dtype=torch.uint8).pin_memory()
        host.copy_(labels.to(torch.uint8), non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(device))
        if pending is not None:
            prev_sample, prev_host, prev_event = pending
            prev_event.synchronize()
            yield prev_sample, prev_host.clone()
        pending = (sample, host, event)
        k += 1
    if pending is not None:
        prev_sample, prev_host, prev_event = pending
        prev_event.synchronize()
        yield prev_sample, prev_host.clone()
