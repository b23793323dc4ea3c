"""Timing of the device-resident validation step (DESIGN.md "Validation on the device").

    python tools/val_step_time.py [--rounds 15] [--inner 20] [--batches 10] [--skip-kernel] [--skip-step]

Part 1, device time (HIP events around `inner` back-to-back repetitions, `rounds` rounds, the two candidates alternating inside
every round; median and min..max over the rounds): the fused launch zs3_val_ce_confusion against the three launches it replaces
(zs3_bilinear_fwd 129 -> 513, zs3_ce_fwd on the result, zs3_argmax_confusion on the low-resolution scores) at B = 16, C = 21 and
C = 60.  Bytes are the algorithmic ones, computed from the shapes; the rate is quoted against the 6.3 TB/s the project uses as
the achievable HBM rate.

Part 2, one validation batch end to end (B = 16, 513 x 513, eval mode, random-init DeepLab): the composition a script wrote before
(model(image), criterion, add_batch_logits, loss.item()) against ValidationStep eager and replayed, alternating; per batch the
host time inside the calls and the wall time of `batches` batches up to a final synchronise; peak allocated memory of each.
Needs the GPU; prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.3e12


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
    import ctypes
    from zs3_amd import functional as Fz, ops
    from zs3_amd._lib import I, P, check, lib, stream
    for classes in (21, 60):
        b, hw, HW = 16, (129, 129), (513, 513)
        g = torch.Generator().manual_seed(classes)
        scores = (3.0 * torch.randn(b, *hw, classes, generator=g)).to(dev)
        tgt = torch.randint(0, classes, (b, *HW), generator=g).float()
        tgt[:, :8] = tgt[:, -8:] = 255
        tgt[:, :, :8] = tgt[:, :, -8:] = 255
        tgt = tgt.to(dev)
        weight = torch.ones(classes, device=dev)
        weight[[10, 14]] = 100.0
        conf = torch.zeros((classes, classes), dtype=torch.int64, device=dev)
        cp = torch.zeros((b, classes), dtype=torch.int32, device=dev)
        totals = torch.zeros(2, dtype=torch.float64, device=dev)
        part, loss_ws = ops.val_ws(dev), torch.zeros(3, device=dev)
        up = torch.empty((b, *HW, classes), device=dev)
        part_old = torch.empty(lib().zs3_ce_ws_doubles(), dtype=torch.float64, device=dev)
        pix = b * HW[0] * HW[1]

        def fused():
            ops.val_ce_confusion(scores, tgt, conf, weight, 255, b, class_pixels=cp, partial_ws=part, loss_ws=loss_ws, totals=totals)

        def trio():
            ops.bilinear_fwd(scores, HW, out=up)
            check(lib().zs3_ce_fwd(P(up), I(classes), P(tgt), I(0), P(weight), ctypes.c_long(pix), I(classes), I(255), I(b),
                                   P(part_old), P(loss_ws), stream()), "zs3_ce_fwd")
            check(lib().zs3_argmax_confusion(P(scores), I(classes), I(b), I(hw[0]), I(hw[1]), I(classes), P(tgt), I(0), I(HW[0]),
                                             I(HW[1]), P(conf), stream()), "zs3_argmax_confusion")

        for fn in (fused, trio):
            device_ms(fn, 5)
        t_f, t_t = [], []
        for r in range(args.rounds):
            order = ((fused, t_f), (trio, t_t)) if r % 2 == 0 else ((trio, t_t), (fused, t_f))
            for fn, out in order:
                out.append(device_ms(fn, args.inner))
        low, lab, full = scores.numel() * 4, tgt.numel() * 4, up.numel() * 4
        bytes_fused = low + lab                                  # scores once, labels once
        bytes_trio = (low + full) + (full + lab) + (low + lab)   # upsample writes, the criterion reads, the argmax pass
        mf, mt = statistics.median(t_f), statistics.median(t_t)
        print(json.dumps({"measurement": "fused launch vs the three launches, device ms", "B": b, "C": classes,
                          "fused_ms": summary(t_f), "trio_ms": summary(t_t), "speedup_of_medians": round(mt / mf, 2),
                          "fused_bytes": bytes_fused, "trio_bytes": bytes_trio,
                          "fused_TBps": round(bytes_fused / (mf * 1e-3) / 1e12, 3), "trio_TBps": round(bytes_trio / (mt * 1e-3) / 1e12, 3),
                          "fused_share_of_6.3TBps": round(bytes_fused / (mf * 1e-3) / HBM_RATE, 3),
                          "rounds": args.rounds, "inner": args.inner}), flush=True)


def step_part(args, dev):
    from zs3_amd.modeling.deeplab import DeepLab
    from zs3_amd.utils.loss import SegmentationLosses
    from zs3_amd.utils.metrics import Evaluator
    from zs3_amd.utils.synthetic import make_batch
    from zs3_amd.validation import ValidationStep
    torch.manual_seed(1)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False)
    for name, mod in model.named_modules():
        if name.endswith("bn3"):
            mod.weight.data.fill_(0.1)
    model = model.to(dev).eval()
    weight = torch.ones(21, device=dev)
    weight[[10, 14]] = 100.0
    batches = [make_batch(16, 513, 21, [10, 14], seed=70 + i, device=dev) for i in range(4)]
    crit = SegmentationLosses(weight=weight, cuda=True).build_loss("ce")
    ev_p = Evaluator(21)
    eager = ValidationStep(model, Evaluator(21), weight=weight, enabled=False)
    replay = ValidationStep(model, Evaluator(21), weight=weight, enabled=True)

    def composition(bt):
        with torch.no_grad():
            out = model(bt["image"])
            v = crit(out, bt["label"]).item()
            ev_p.add_batch_logits(bt["label"], out)
        return v

    variants = {"composition": composition, "step_eager": lambda bt: eager.step(bt["image"], bt["label"]),
                "step_replayed": lambda bt: replay.step(bt["image"], bt["label"])}
    for fn in variants.values():
        for k in range(4):
            fn(batches[k % 4])
    torch.cuda.synchronize()
    assert replay.replays >= 1 and replay.unrecorded_ops == [], (replay.replays, replay.unrecorded_ops)
    host = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.rounds):
        for name in names[r % 3:] + names[:r % 3]:
            fn = variants[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.batches):
                fn(batches[k % 4])
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host[name].append((t1 - t0) * 1e3 / args.batches)
            wall[name].append((t2 - t0) * 1e3 / args.batches)
    peak = {}
    for name, fn in variants.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for k in range(3):
            fn(batches[k % 4])
        torch.cuda.synchronize()
        peak[name] = {"peak_allocated_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                      "above_resident_MB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)}
    # the batch's peak sits in the backbone; what the fused launch removes shows in the part AFTER the low-resolution scores exist
    from zs3_amd import ops
    with torch.no_grad():
        scores = model.forward_scores(batches[0]["image"])
        label = batches[0]["label"]
        tail = {}
        for name in ("composition", "fused"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            if name == "composition":
                out = model._logits_to_image(scores, label.shape[1:])
                crit(out, label).item()
                ev_p.add_batch_logits(label, out)
                del out
            else:
                eager.evaluator.add_batch_scores(label, scores, weight)
            torch.cuda.synchronize()
            tail[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    print(json.dumps({"measurement": "peak allocated above the low-resolution scores, loss + confusion part only, MB", **tail}), flush=True)
    for name in names:
        print(json.dumps({"measurement": "one validation batch, B=16 513x513 eval, ms per batch", "variant": name,
                          "host_ms": summary(host[name]), "wall_ms": summary(wall[name]), **peak[name],
                          "rounds": args.rounds, "batches": args.batches}), flush=True)
    # a replay allocates nothing: its activations live in the plan's private pool, which stays reserved between calls
    pools = {tuple(st["pool"].id) for st in replay._plans.values() if st.get("pool") is not None}
    pool_bytes = sum(seg["total_size"] for seg in torch.cuda.memory_snapshot() if tuple(seg.get("segment_pool_id", (0, 0))) in pools)
    print(json.dumps({"replay_pool_reserved_MB": round(pool_bytes / 2 ** 20, 1),
                      "replay_counters": [replay.eager_calls, replay.recordings, replay.replays],
                      "reserved_MB": round(torch.cuda.memory_reserved() / 2 ** 20, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("val_step_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    if not args.skip_kernel:
        kernel_part(args, dev)
    if not args.skip_step:
        step_part(args, dev)


if __name__ == "__main__":
    main()
