"""Timing of the device-resident pseudo-labelling (DESIGN.md "Pseudo-labels on the device").

    python tools/pseudo_label_time.py [--rounds 21] [--inner 10] [--batches 8] [--skip-kernel] [--skip-step]

Part 1, device time of the two-launch tail (zs3_pl_candidates + zs3_pl_select through ops.pseudo_label on preallocated buffers)
at B = 16, 129 -> 513: C = 21 with 2 and with 10 candidate classes, C = 60 with 10, group "image_class" and "image", against
the tensor-library composition on the same device and the same inputs: ops.bilinear_fwd to [B, 513, 513, C], softmax over the
classes, maximum over the candidates, and a Python loop of one kthvalue per bucket (each with the host synchronisation a
data-dependent size costs).  HIP events around `inner` back-to-back repetitions of the tail (one run of the composition: it
synchronises inside), warmed up, median and min..max over `rounds` rounds, the two alternating.  Labels are uniform over the C
classes, so the eligible share of the pixels is (candidates / C); the share of pixels on which the two paths' labels agree is
printed (their softmax arithmetic differs in the last bits, so a pixel at a threshold can fall either way).

Part 2, PseudoLabelStep.step() as a whole (eval forward of a random-init DeepLab + the tail) at B = 16, 513 x 513: host time
inside the calls and wall time per batch up to a final synchronise.  Needs the GPU; prints one JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANDIDATES = {2: [10, 14], 10: [2, 5, 6, 10, 11, 14, 15, 17, 18, 20]}


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def device_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def kernel_part(args, dev):
    from zs3_amd import ops
    for classes, ncand in ((21, 2), (21, 10), (60, 10)):
        cand = CANDIDATES[ncand]
        b, hw, HW, p = 16, (129, 129), (513, 513), 25.0
        g = torch.Generator().manual_seed(classes + ncand)
        scores = (3.0 * torch.randn(b, *hw, classes, generator=g)).to(dev)
        tgt = torch.randint(0, classes, (b, *HW), generator=g).float()
        tgt[:, :8] = tgt[:, -8:] = 255
        tgt[:, :, :8] = tgt[:, :, -8:] = 255
        tgt = tgt.to(dev)
        cand_t = torch.tensor(cand, device=dev)
        up = torch.empty((b, *HW, classes), device=dev)
        pre = dict(labels=torch.empty_like(tgt), cls_map=torch.empty(tgt.shape, dtype=torch.uint8, device=dev),
                   conf_map=torch.empty(tgt.shape, device=dev), count=torch.empty((b, classes), dtype=torch.int32, device=dev),
                   selected=torch.empty((b, classes), dtype=torch.int32, device=dev),
                   threshold=torch.empty((b, classes), device=dev), ws=ops.pl_ws(b, classes, dev))
        for group in ("image_class", "image"):

            def fused():
                return ops.pseudo_label(scores, tgt, cand, p, group, **pre)[0]

            def candidates_only():
                ops.pl_candidates(scores, tgt, cand, cls_map=pre["cls_map"], conf_map=pre["conf_map"], count=pre["count"])

            def composition():
                ops.bilinear_fwd(scores, HW, out=up)
                conf, j = torch.softmax(up, dim=-1)[..., cand].max(dim=-1)
                cls = cand_t[j]
                elig = torch.isin(tgt, cand_t.float())
                labels = torch.where(elig, torch.full_like(tgt, 255.0), tgt)
                for n in range(b):
                    buckets = [elig[n]] if group == "image" else [elig[n] & (cls[n] == c) for c in cand]
                    for mask in buckets:
                        v = conf[n][mask]                              # (a data-dependent size: the host waits here)
                        m = v.numel()
                        k = min(m, math.ceil(m * p / 100))
                        if k == 0:
                            continue
                        t = v.kthvalue(m - k + 1).values
                        keep = mask & (conf[n] >= t)
                        labels[n] = torch.where(keep, cls[n].float(), labels[n])
                return labels

            agree = float((fused() == composition()).float().mean())
            for fn, inner in ((fused, 5), (candidates_only, 5), (composition, 1)):
                device_ms(fn, inner)
            t_f, t_k, t_c = [], [], []
            for r in range(args.rounds):
                order = ((fused, t_f, args.inner), (composition, t_c, 1))
                for fn, out, inner in (order if r % 2 == 0 else order[::-1]):
                    out.append(device_ms(fn, inner))
                t_k.append(device_ms(candidates_only, args.inner))
            mf, mc = statistics.median(t_f), statistics.median(t_c)
            print(json.dumps({"measurement": "two-launch tail vs the tensor-library composition, device ms", "B": b, "C": classes,
                              "candidates": ncand, "group": group, "top_percent": p,
                              "eligible_share": round(float(torch.isin(tgt, cand_t.float()).float().mean()), 3),
                              "fused_ms": summary(t_f), "of_which_candidates_ms": summary(t_k), "composition_ms": summary(t_c),
                              "speedup_of_medians": round(mc / mf, 1), "labels_agree": round(agree, 6),
                              "rounds": args.rounds, "inner": args.inner}), flush=True)


def step_part(args, dev):
    from zs3_amd.modeling.deeplab import DeepLab
    from zs3_amd.self_training import PseudoLabelStep
    from zs3_amd.utils.synthetic import make_batch
    torch.manual_seed(1)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False)
    for name, mod in model.named_modules():
        if name.endswith("bn3"):
            mod.weight.data.fill_(0.1)
    model = model.to(dev).eval()
    batches = [make_batch(16, 513, 21, [10, 14], seed=70 + i, device=dev) for i in range(4)]
    for bt in batches:
        bt["label"][:, 100:300, 60:400] = 10.0          # regions to pseudo-label
        bt["label"][:, 320:450, 100:500] = 14.0
    step = PseudoLabelStep(model, [10, 14], top_percent=25.0, group="image")
    for k in range(4):
        step.step(batches[k]["image"], batches[k]["label"])
    torch.cuda.synchronize()
    host, wall, dev_ms = [], [], []
    for r in range(args.rounds):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for k in range(args.batches):
            step.step(batches[k % 4]["image"], batches[k % 4]["label"])
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append((t1 - t0) * 1e3 / args.batches)
        wall.append((t2 - t0) * 1e3 / args.batches)
        dev_ms.append(a.elapsed_time(b) / args.batches)
    print(json.dumps({"measurement": "PseudoLabelStep.step(), B=16 513x513 eval, ms per batch", "host_ms": summary(host),
                      "wall_ms": summary(wall), "device_ms": summary(dev_ms), "rounds": args.rounds, "batches": args.batches,
                      "kept": int(step.total_selected.sum()), "eligible": int(step.total_count.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pseudo_label_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if not args.skip_kernel:
        kernel_part(args, dev)
    if not args.skip_step:
        step_part(args, dev)


if __name__ == "__main__":
    main()
