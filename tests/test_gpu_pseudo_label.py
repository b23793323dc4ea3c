"""Device-resident pseudo-labelling for the self-training stage: zs3_pl_candidates (per unlabelled pixel the best candidate class
and its softmax probability, sampled from low-resolution scores) against zs3_bilinear_fwd and a float64 oracle, zs3_pl_select (exact
top-p % per bucket by radix select) against a sort on the CPU, their composition, and zs3_amd.self_training.PseudoLabelStep /
pseudo_label_loader on a small DeepLab."""
import math
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


# ---------------------------------------------------------------------------------------------------------------- the rule, on the CPU
def keep_count(m, p):
    return min(m, math.ceil(m * p / 100))


def cpu_select(cls_map, conf_map, target, classes, candidates, p, group, ignore_index=255):
    """The selection rule by sorting.  cls_map uint8 / conf_map float32 / target: numpy [N, H, W].  -> labels, selected [N, C],
    threshold [N, C] (float32), and per non-empty bucket with k >= 1 the triple (k, #{conf > t}, #{conf >= t}).  Confidences are
    compared as bit patterns (non-negative floats order like their uint32 bits): no arithmetic can flush a denormal."""
    n = cls_map.shape[0]
    bits = conf_map.view(np.uint32)
    labels = target.copy()
    selected = np.zeros((n, classes), dtype=np.int64)
    thr = np.zeros((n, classes), dtype=np.uint32)
    ranks = []
    for i in range(n):
        elig = cls_map[i] != 255
        labels[i][elig] = ignore_index
        buckets = [(elig, list(candidates))] if group == "image" else [(cls_map[i] == c, [c]) for c in candidates]
        for mask, cols in buckets:
            m = int(mask.sum())
            k = keep_count(m, p)
            if k == 0:
                continue
            t = np.sort(bits[i][mask])[::-1][k - 1]
            keep = mask & (bits[i] >= t)
            labels[i][keep] = cls_map[i][keep].astype(labels.dtype)
            for c in candidates:
                selected[i, c] += int((keep & (cls_map[i] == c)).sum())
            thr[i, cols] = t
            ranks.append((k, int((bits[i][mask] > t).sum()), int((bits[i][mask] >= t).sum())))
    return labels, selected, thr.view(np.float32), ranks


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_selection(out, cls_map, conf_map, target, classes, candidates, p, group):
    """labels / selected / threshold of the device against cpu_select on the same maps, exactly"""
    labels, selected, threshold = out
    want_l, want_s, want_t, ranks = cpu_select(cls_map.cpu().numpy(), conf_map.cpu().numpy(), target.cpu().numpy(), classes,
                                               candidates, p, group)
    for k, above, at_least in ranks:
        assert above < k <= at_least
    assert labels.dtype == target.dtype and np.array_equal(labels.cpu().numpy(), want_l), (p, group)
    assert np.array_equal(selected.cpu().numpy().astype(np.int64), want_s), (p, group)
    assert _same_bits(threshold.cpu().numpy(), want_t), (p, group)
    return ranks


# ---------------------------------------------------------------------------------------------------------------- candidates kernel
def _labels(g, b, classes, HW, extra=None):
    gt = torch.randint(0, classes, (b, *HW), generator=g)
    brd = min(8, HW[0] // 8)                      # the 8-pixel border of 255 of the data sets' crops
    gt[:, :brd] = 255
    gt[:, -brd:] = 255
    gt[:, :, :brd] = 255
    gt[:, :, -brd:] = 255
    gt[0, HW[0] // 2:HW[0] // 2 + 5] = 255        # five rows of 255 inside the first image
    if extra is not None:                         # a block of the extra "unlabelled" value in every image
        gt[:, HW[0] // 4:HW[0] // 2, HW[1] // 4:HW[1] // 2] = extra
    return gt


def _scores(g, b, classes, hw, pad, dev):
    """fp32 [b, h, w, C] class scores in NHWC; pad > 0: a channel slice of a wider buffer (pixel stride ld = C + pad)"""
    full = (3.0 * torch.randn(b, *hw, classes + pad, generator=g)).to(dev)
    return full[..., :classes] if pad else full


CAND = {2: [10, 14], 10: [2, 5, 6, 10, 11, 14, 15, 17, 18, 20], 6: [3, 17, 31, 40, 58, 59]}
# (C, h -> H, B, pad, candidates, unlabelled, unlabelled_value)
SHAPES = [(21, 17, 65, 3, 0, CAND[2], None, None), (60, 33, 129, 2, 0, CAND[6], None, None),
          (21, 129, 513, 2, 0, CAND[10], None, None), (21, 78, 312, 2, 0, CAND[2], None, None),
          (21, 17, 65, 3, 3, CAND[10], None, None),                       # ld > C
          (21, 33, 129, 2, 0, CAND[2], [10, 14, 3], 254),                  # unlabelled_value, and a seen class declared unlabelled
          (21, 40, 40, 2, 0, CAND[10], None, None)]                       # ratio 1


@pytest.mark.parametrize("classes,h,H,b,pad,cand,unl,uv", SHAPES)
def test_candidates_kernel_against_the_resize_kernel_and_the_oracle(dev, classes, h, H, b, pad, cand, unl, uv):
    """cls_map = first argmax over the candidates of ops.bilinear_fwd(scores), exactly, on EVERY eligible pixel; 255 / 0 elsewhere;
    count = bincount of cls_map.  conf_map against the float64 softmax of the float64 resize: absolute error <= 4 x e32 + 1e-7,
    e32 the largest error of the fp32 tensor-library composition (F.interpolate + softmax in fp32) against the same float64 values
    on the same input (computed here; measured 3.7e-7 .. 6.4e-7 on the x4 shapes and 1.4e-5 at 78 -> 312, where fp32 source
    coordinates show; the kernel's own error: 1.4e-7 .. 1.2e-6; the factor 4 covers the other order of the bilinear products).  Argmax against the float64 oracle: equal wherever the oracle's top-2 candidate margin exceeds 1e-3, and those
    exclusions are at most 0.5 % of the eligible pixels."""
    import torch.nn.functional as F
    from zs3_amd import ops
    g = torch.Generator().manual_seed(classes + h + pad + len(cand))
    scores = _scores(g, b, classes, (h, h), pad, dev)
    gt = _labels(g, b, classes, (H, H), uv)
    unl_set = sorted(set(cand if unl is None else unl))
    elig = torch.isin(gt, torch.tensor(unl_set + ([] if uv is None else [uv])))
    assert 0 < int(elig.sum()) < elig.numel()
    up = ops.bilinear_fwd(scores, (H, H)).cpu().numpy()                               # [b, H, H, C]: the values the kernel samples
    want_cls = np.asarray(cand)[np.argmax(up[..., cand], axis=-1)]                    # (numpy: first maximum)
    # float64 oracle and the fp32 composition's own error, on the CPU
    s_nchw = scores.cpu().permute(0, 3, 1, 2).contiguous()
    p64 = F.interpolate(s_nchw.double(), size=(H, H), mode="bilinear", align_corners=True).softmax(1)
    p32 = F.interpolate(s_nchw, size=(H, H), mode="bilinear", align_corners=True).softmax(1)
    e32 = float((p32.double() - p64).abs().max())
    up64 = F.interpolate(s_nchw.double(), size=(H, H), mode="bilinear", align_corners=True)[:, cand]
    top2 = up64.topk(2, dim=1).values if len(cand) > 1 else None
    margin = (top2[:, 0] - top2[:, 1]) if top2 is not None else torch.full(gt.shape, 1.0, dtype=torch.float64)
    cls64 = torch.tensor(cand)[up64.argmax(1)]
    e = elig.numpy()
    for tgt in (gt.float().to(dev), gt.to(dev)):
        cls_map, conf_map, count = ops.pl_candidates(scores, tgt, cand, unlabelled=unl, unlabelled_value=uv)
        cm, cf = cls_map.cpu().numpy(), conf_map.cpu().numpy()
        assert cm.dtype == np.uint8 and cf.dtype == np.float32
        assert np.array_equal(cm[e], want_cls[e])                                     # every eligible pixel, no exclusions
        assert (cm[~e] == 255).all() and (cf[~e] == 0).all()
        want_count = np.stack([np.bincount(cm[i][e[i]], minlength=classes) for i in range(b)])
        assert np.array_equal(count.cpu().numpy(), want_count)
        # conf against float64 at the kernel's own class
        idx = torch.from_numpy(np.where(e, cm, 0).astype(np.int64))
        ref = p64.gather(1, idx[:, None])[:, 0].numpy()
        err = float(np.abs(cf.astype(np.float64) - ref)[e].max())
        clear = (margin.numpy() > 1e-3) & e
        excluded = 1.0 - clear.sum() / e.sum()
        print(f"C={classes} {h}->{H} b={b} pad={pad} cand={len(cand)} {tgt.dtype}: conf err={err:.3g} e32={e32:.3g} "
              f"bound={4 * e32 + 1e-7:.3g} excluded={100 * excluded:.3g} %")
        assert err <= 4 * e32 + 1e-7
        assert np.array_equal(cm[clear], cls64.numpy()[clear])
        assert excluded <= 0.005


# ---------------------------------------------------------------------------------------------------------------- select kernel
def _crafted(kind, g, n, HW, classes, cand):
    """cls_map / conf_map / target (int64) on the CPU.  Image 0: mixed classes; image 1: one bucket spanning nearly the whole image;
    image 2: a one-pixel bucket, a two-pixel bucket, the other buckets empty; image 3: nothing eligible; further images mixed, half
    of their pixels not eligible."""
    H, W = HW
    pick = torch.tensor(cand)[torch.randint(0, len(cand), (n, H, W), generator=g)]
    cls = torch.full((n, H, W), 255, dtype=torch.int64)
    cls[0] = pick[0]
    cls[0, :3] = 255
    cls[1] = cand[-1]
    cls[1, 0, :5] = 255
    cls[2, 7, 9] = cand[0]
    cls[2, 20, 3] = cls[2, 21, 30] = cand[1]
    for i in range(4, n):
        cls[i] = torch.where(torch.rand(H, W, generator=g) < 0.5, pick[i], cls[i])
    if kind == "random":
        conf = torch.rand(n, H, W, generator=g)
    elif kind == "ties8":
        conf = torch.randint(0, 8, (n, H, W), generator=g).float() / 8
    elif kind == "equal":
        conf = torch.full((n, H, W), 0.37)
    elif kind == "tiny":
        vals = torch.from_numpy(np.array([0, 1, 2, 3, 0x7FFFFF, 0x800000, 0x800001, 0x3F800000], dtype=np.uint32).view(np.float32).copy())
        conf = vals[torch.randint(0, len(vals), (n, H, W), generator=g)]              # zeros, denormals, the smallest normals, 1.0
    else:
        raise ValueError(kind)
    conf = torch.where(cls == 255, torch.zeros_like(conf), conf)
    target = torch.randint(0, classes, (n, H, W), generator=g)
    target[:, :2] = 255
    return cls.to(torch.uint8), conf.contiguous(), target


PERCENTS = (0, 12.5, 25, 75, 100)


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("kind", ["random", "ties8", "equal", "tiny"])
def test_select_kernel_equals_a_sort_on_the_cpu(dev, kind, i64):
    """labels, selected and threshold equal, exactly, what sorting every bucket on the CPU gives under the rule (conf >= t, t the
    k-th largest, k = min(m, ceil(m p / 100)); ties at t all kept), for p in {0, 12.5, 25, 75, 100}, both groups, on random
    confidences, confidences quantised to 8 values, all-equal buckets, zeros / denormals, one-pixel and empty buckets and a bucket
    spanning nearly a whole image; #{conf > t} < k <= #{conf >= t} for every non-empty bucket with k >= 1; a second run is
    bit-identical."""
    from zs3_amd import ops
    classes, cand, n, HW = 21, [3, 10, 14, 20], 6, (41, 53)
    g = torch.Generator().manual_seed(len(kind) + 2 * i64)
    cls, conf, target = _crafted(kind, g, n, HW, classes, cand)
    if kind == "tiny":
        assert int(((conf > 0) & (conf < 1e-38)).sum()) > 0                           # denormals survive on the host side
    count = torch.stack([torch.bincount(cls[i][cls[i] != 255].long(), minlength=classes) for i in range(n)]).int()
    tgt = target if i64 else target.float()
    d = [t.to(dev) for t in (cls, conf, count, tgt)]
    assert _same_bits(d[1].cpu().numpy(), conf.numpy())
    buckets = 0
    for group in ("image_class", "image"):
        for p in PERCENTS:
            out = ops.pl_select(d[0], d[1], d[2], d[3], cand, p, group)
            buckets += len(_check_selection(out, d[0], d[1], d[3], classes, cand, p, group))
            again = ops.pl_select(d[0], d[1], d[2], d[3], cand, p, group)
            assert all(torch.equal(x, y) for x, y in zip(out, again)) and _same_bits(out[2].cpu().numpy(), again[2].cpu().numpy())
            if p == 0:
                assert int(out[1].sum()) == 0 and bool((out[0][d[0] != 255] == 255).all())
            if p == 100:
                assert torch.equal(out[1], d[2])                                      # everything eligible is kept
    assert buckets > 20


def test_select_kernel_many_candidates_and_running_totals(dev):
    """C = 128 with every class a candidate (classes beyond 63: the high mask word; more buckets per image than block-private
    histograms fit: the workspace histograms are updated directly) against the CPU rule, and `totals` accumulates count / selected
    over calls."""
    from zs3_amd import ops
    classes, cand, n, HW = 128, list(range(128)), 2, (64, 70)
    g = torch.Generator().manual_seed(11)
    cls = torch.randint(0, classes, (n, *HW), generator=g)
    cls[:, :4] = 255
    conf = torch.rand(n, *HW, generator=g)
    conf = torch.where(cls == 255, torch.zeros_like(conf), conf)
    target = torch.randint(0, classes, (n, *HW), generator=g).float()
    count = torch.stack([torch.bincount(cls[i][cls[i] != 255], minlength=classes) for i in range(n)]).int()
    d = [t.to(dev) for t in (cls.to(torch.uint8), conf, count, target)]
    totals = torch.zeros((2, classes), dtype=torch.int64, device=dev)
    want = torch.zeros((2, classes), dtype=torch.int64)
    for group, p in (("image_class", 25), ("image", 75), ("image_class", 12.5)):
        out = ops.pl_select(d[0], d[1], d[2], d[3], cand, p, group, totals=totals)
        _check_selection(out, d[0], d[1], d[3], classes, cand, p, group)
        want[0] += count.sum(0)
        want[1] += out[1].cpu().sum(0)
    assert torch.equal(totals.cpu(), want) and int(want[1].sum()) > 0
    # a candidate subset reaching into the high mask word
    sub = [5, 63, 64, 100, 127]
    cls_sub = torch.where(torch.isin(cls, torch.tensor(sub)), cls, torch.full_like(cls, 255)).to(torch.uint8)
    cnt_sub = torch.stack([torch.bincount(cls_sub[i][cls_sub[i] != 255].long(), minlength=classes) for i in range(n)]).int()
    out = ops.pl_select(cls_sub.to(dev), d[1], cnt_sub.to(dev), d[3], sub, 25, "image_class")
    _check_selection(out, cls_sub.to(dev), d[1], d[3], classes, sub, 25, "image_class")


# ---------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("classes,h,H,b,cand", [(21, 33, 129, 3, CAND[2]), (60, 33, 129, 2, CAND[6]), (21, 129, 513, 16, CAND[10])])
def test_pseudo_label_is_candidates_then_select(dev, classes, h, H, b, cand):
    """ops.pseudo_label equals pl_select(pl_candidates(...)), and on the kernel's OWN conf_map / cls_map the selection equals the CPU
    rule exactly (arithmetic and selection are checked apart) -- also at B = 16, 513 x 513, C = 21."""
    from zs3_amd import ops
    g = torch.Generator().manual_seed(classes + b)
    scores = _scores(g, b, classes, (h, h), 0, dev)
    gt = _labels(g, b, classes, (H, H))
    for tgt, group, p in ((gt.float().to(dev), "image_class", 25.0), (gt.to(dev), "image", 75.0)):
        labels, stats = ops.pseudo_label(scores, tgt, cand, p, group)
        cls_map, conf_map, count = ops.pl_candidates(scores, tgt, cand)
        out = ops.pl_select(cls_map, conf_map, count, tgt, cand, p, group)
        assert torch.equal(labels, out[0]) and torch.equal(stats["selected"], out[1])
        assert _same_bits(stats["threshold"].cpu().numpy(), out[2].cpu().numpy())
        assert torch.equal(stats["cls_map"], cls_map) and torch.equal(stats["conf_map"], conf_map) and torch.equal(stats["count"], count)
        ranks = _check_selection(out, cls_map, conf_map, tgt, classes, cand, p, group)
        assert len(ranks) >= b and int(out[1].sum()) > 0
        # preallocated outputs and workspace are the ones returned
        pre = dict(labels=torch.empty_like(tgt), selected=torch.empty_like(out[1]), threshold=torch.empty_like(out[2]),
                   ws=ops.pl_ws(b, classes, dev), cls_map=torch.empty_like(cls_map), conf_map=torch.empty_like(conf_map),
                   count=torch.empty_like(count))
        pre["ws"].fill_(-1)                                                           # (the caller does not zero the workspace)
        labels2, stats2 = ops.pseudo_label(scores, tgt, cand, p, group, **pre)
        assert labels2 is pre["labels"] and stats2["selected"] is pre["selected"] and stats2["cls_map"] is pre["cls_map"]
        assert torch.equal(labels2, labels) and torch.equal(stats2["selected"], out[1])


# ---------------------------------------------------------------------------------------------------------------- the step
def _tamed(dev, seed=1):
    from zs3_amd.modeling.deeplab import DeepLab
    torch.manual_seed(seed)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False)
    for name, mod in model.named_modules():
        if name.endswith("bn3"):
            mod.weight.data.fill_(0.1)
    return model.to(dev).eval()


def _batch(seed, b, size, dev, unseen=(10, 14)):
    """an image and a label map in which regions of the unseen classes are to be pseudo-labelled"""
    from zs3_amd.utils.synthetic import make_batch
    bt = make_batch(b, size, 21, list(unseen), seed=seed, device="cpu")
    label = bt["label"]
    for j, u in enumerate(unseen):
        label[:, 12 + 20 * j:28 + 20 * j, 10:50] = float(u)
    return bt["image"].to(dev), label.to(dev)


class _NoHostSync:
    """nothing inside may wait for the device"""

    def __enter__(self):
        self.saved = (torch.Tensor.item, torch.Tensor.cpu, torch.Tensor.tolist, torch.cuda.synchronize)

        def refuse(*a, **k):
            raise AssertionError("host synchronisation inside a pseudo-labelling batch")

        torch.Tensor.item = torch.Tensor.cpu = torch.Tensor.tolist = refuse
        torch.cuda.synchronize = refuse

    def __exit__(self, *exc):
        torch.Tensor.item, torch.Tensor.cpu, torch.Tensor.tolist, torch.cuda.synchronize = self.saved


@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
def test_pseudo_label_step(dev, storage):
    """PseudoLabelStep on a small DeepLab (65 x 65, B = 2): results equal the ops path on model.forward_scores(image); totals
    accumulate over three batches; step() completes with .item / .cpu / synchronize refusing; the tail does no tensor-library
    device work; the labels go into SegmentationLosses as they are and give torch's CE with ignore_index (the project's CE
    tolerance 2e-6 |ref| + 1e-7)."""
    from zs3_amd import ops
    from zs3_amd.plan import _TensorLibraryWork
    from zs3_amd.self_training import PseudoLabelStep
    from zs3_amd.utils.loss import SegmentationLosses
    ops.set_storage(storage)
    try:
        model = _tamed(dev)
        unseen = [10, 14]
        step = PseudoLabelStep(model, unseen, top_percent=25.0, group="image_class")
        batches = [_batch(40 + i, 2, 65, dev) for i in range(3)]
        want_tot = torch.zeros((2, 21), dtype=torch.int64)
        for i, (image, target) in enumerate(batches):
            if i == 2:
                with _NoHostSync():
                    labels = step.step(image, target)
            else:
                labels = step.step(image, target)
            with torch.no_grad():
                scores = model.forward_scores(image)
            want, stats = ops.pseudo_label(scores, target, unseen, 25.0, "image_class")
            assert labels.dtype == target.dtype and torch.equal(labels, want)
            for k in ("cls_map", "conf_map", "count", "selected", "threshold"):
                assert torch.equal(step.last_stats[k], stats[k]), k
            assert int(stats["selected"].sum()) > 0 and int(stats["count"].sum()) == int(torch.isin(target, torch.tensor(unseen, device=dev).float()).sum())
            want_tot[0] += stats["count"].cpu().sum(0)
            want_tot[1] += stats["selected"].cpu().sum(0)
        assert step.batches == 3 and model.training is False
        assert torch.equal(step.total_count, want_tot[0]) and torch.equal(step.total_selected, want_tot[1])
        assert step.totals_device.is_cuda and step.totals_device.dtype == torch.int64
        # the tail under the plan recorder's watch: two library calls and nothing of the tensor library
        image, target = batches[0]
        with torch.no_grad():
            scores = model.forward_scores(image)
            work = _TensorLibraryWork()
            with work:
                labels = step.label_scores(scores, target)
        assert work.unrecorded() == []
        # selected pixels carry an unseen class, the other unlabelled ones 255, the rest is the target
        unl = torch.isin(target, torch.tensor(unseen, device=dev).float())
        assert torch.equal(labels[~unl], target[~unl])
        assert bool(torch.isin(labels[unl], torch.tensor(unseen + [255], device=dev).float()).all())
        # into the criterion with no conversion
        crit = SegmentationLosses(weight=None, cuda=True).build_loss("ce")
        with torch.no_grad():
            out = model(image)
            loss = float(crit(out, labels))
        ref = float(torch.nn.functional.cross_entropy(out.cpu().double(), labels.cpu().long(), ignore_index=255)) / image.shape[0]
        print(f"{storage}: CE on pseudo-labels {loss!r}, torch on the CPU {ref!r}")
        assert abs(loss - ref) <= 2e-6 * abs(ref) + 1e-7
        step.reset()
        assert int(step.total_count.sum()) == 0 and step.batches == 0
        # group "image" with an extra unlabelled value and int64 targets
        step2 = PseudoLabelStep(model, unseen, top_percent=75.0, group="image", unlabelled=[], unlabelled_value=254)
        t64 = target.long()
        t64[:, 30:40, 20:60] = 254
        labels = step2.step(image, t64)
        want, stats = ops.pseudo_label(scores, t64, unseen, 75.0, "image", unlabelled=[], unlabelled_value=254)
        assert labels.dtype == torch.int64 and torch.equal(labels, want)
        assert int(stats["count"].sum()) == int((t64 == 254).sum()) and not bool((labels == 254).any())
    finally:
        ops.set_storage(torch.float32)


def test_pseudo_label_loader_yields_every_batch_once_in_order(dev):
    """pseudo_label_loader over five batches (dict samples, the last one shorter): every batch once, in order, each with the maps
    of its own batch as uint8 on the host."""
    from zs3_amd.self_training import PseudoLabelStep, pseudo_label_loader
    model = _tamed(dev)
    unseen = [10, 14]
    loader = []
    for i in range(5):
        image, label = _batch(60 + i, 2 if i < 4 else 1, 65, "cpu")
        loader.append({"image": image, "label": label, "id": i})
    got = list(pseudo_label_loader(model, loader, unseen_classes=unseen, top_percent=25.0, group="image"))
    assert [s["id"] for s, _ in got] == list(range(5))
    step = PseudoLabelStep(model, unseen, top_percent=25.0, group="image")
    distinct = set()
    for sample, maps in got:
        assert sample is loader[sample["id"]]
        want = step.step(sample["image"].to(dev), sample["label"].to(dev)).cpu()
        assert maps.dtype == torch.uint8 and not maps.is_cuda and maps.shape == sample["label"].shape
        assert torch.equal(maps.float(), want)
        distinct.add(maps.numpy().tobytes())
    assert len(distinct) == 5
    assert list(pseudo_label_loader(model, [], unseen_classes=unseen)) == []
    # a step handed in is used (and keeps its totals); (image, target) pairs work as samples
    pairs = [(s["image"], s["label"]) for s in loader[:2]]
    step.reset()
    out = list(pseudo_label_loader(model, pairs, step=step))
    assert len(out) == 2 and step.batches == 2 and torch.equal(out[1][1], got[1][1])
