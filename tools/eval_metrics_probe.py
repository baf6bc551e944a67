"""Native validation metrics against the stock metrics tail of the reference's evaluation loop (GPU box).

    python tools/eval_metrics_probe.py [--calls 20] [--rounds 5] [--batch 128] [--batches 10] [--sections 1,2] [--out profiles/eval_metrics_probe.txt]

1. The tail alone at 128 x 1000 logits, fp32 and bf16: ``EvalMeter.update`` (lmv_eval_logits + lmv_meter_add, nothing returns to the host) against what
   engine.py:216-231 runs per batch -- F.cross_entropy, timm's topk-based accuracy (topk, transpose, eq, two sums and scalings), a synchronize and three .item().
2. A 10-batch ``validate`` of LeMeViT-Base 224^2, bf16, B = 128 (``lemevit_amd.validate``: one synchronisation at the end) against the same loop with the stock tail.
--sections picks a subset (default: both).
Section 1: windows of --calls calls between device events, --rounds windows per side, the sides alternating; section 2: --rounds passes per side, host wall time around a
final synchronize; median and spread (max - min) reported."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import lemevit_amd

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms


def compare(title, sides, calls, rounds, unit="us", scale=1e3, timer=timed):
    for _, f in sides:
        timer(f, 3 if timer is timed else 1)
    t = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, f in sides:
            t[name].append(timer(f, calls))
    say(title)
    med = {}
    for name, _ in sides:
        v = sorted(x * scale for x in t[name])
        med[name] = v[rounds // 2]
        say(f"  {name:86s} {med[name]:10.3f} {unit}   spread {v[-1] - v[0]:.3f}   {['%.3f' % (x * scale) for x in t[name]]}")
    return med


def timm_accuracy(output, target, topk=(1,)):
    """timm.utils.accuracy"""
    maxk = min(max(topk), output.size(1))
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:min(k, maxk)].reshape(-1).float().sum(0) * 100. / batch_size for k in topk]


class AverageMeter:
    """timm.utils.AverageMeter"""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / self.count


def stock_tail(output, target, meters):
    """engine.py:216-231 on one GPU: loss, accuracy, synchronize, three .item()"""
    loss = F.cross_entropy(output, target)
    acc1, acc5 = timm_accuracy(output, target, topk=(1, 5))
    torch.cuda.synchronize()
    meters[0].update(loss.item(), output.size(0))
    meters[1].update(acc1.item(), output.size(0))
    meters[2].update(acc5.item(), output.size(0))


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--sections", default="1,2")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_metrics_probe.txt"))
    a = ap.parse_args()
    sections = {int(v) for v in a.sections.split(",")}
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    B, N, dev = a.batch, 1000, "cuda"
    y = torch.randint(0, N, (B,), device=dev)
    if 1 in sections:
        for dtype in (torch.float32, torch.bfloat16):
            logits = torch.randn(B, N, device=dev).to(dtype)
            meter = lemevit_amd.EvalMeter(topk=(1, 5))
            meters = [AverageMeter() for _ in range(3)]
            sides = [("(a) EvalMeter.update: lmv_eval_logits + lmv_meter_add, no synchronisation", lambda: meter.update(logits, y)),
                     ("(b) stock: F.cross_entropy + topk-based accuracy + synchronize + three .item()", lambda: stock_tail(logits, y, meters)),
                     ("(c) stock without the synchronize and the .item() calls (device work only)", lambda: (F.cross_entropy(logits, y), timm_accuracy(logits, y, (1, 5))))]
            compare(f"metrics tail, {B} x {N} {str(dtype).replace('torch.', '')} logits, {a.rounds} windows of {a.calls} calls per side, sides alternating (us per call, median; spread; all windows)",
                    sides, a.calls, a.rounds)
            m = meter.compute()
            say(f"  agreement over the accumulated calls: loss {m['loss']:.6f} / {meters[0].avg:.6f}, top1 {m['top1']:.4f} / {meters[1].avg:.4f}, top5 {m['top5']:.4f} / {meters[2].avg:.4f}")
    if 2 in sections:
        model = lemevit_amd.create_model("lemevit_base", num_classes=N).cuda().eval()
        loader = [(torch.randn(B, 3, 224, 224, device=dev), y) for _ in range(a.batches)]
        res = {}

        def native():
            res["native"] = lemevit_amd.validate(model, loader, topk=(1, 5))

        def stock():
            meters = [AverageMeter() for _ in range(3)]
            with torch.no_grad():
                for x, t in loader:
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        out = model(x)
                    stock_tail(out, t, meters)
            res["stock"] = [m.avg for m in meters]
        med = compare(f"lemevit_base 224^2 bf16 B={B}, validate over {a.batches} batches, {a.rounds} passes per side, sides alternating (ms per pass, host wall time; median; spread; all passes)",
                      [("(a) lemevit_amd.validate: EvalMeter, one synchronisation at the end", native), ("(b) the same loop with the stock tail (a synchronize and three .item() per batch)", stock)],
                      1, a.rounds, "ms", 1.0, wall)
        names = list(med)
        say(f"  per batch: {med[names[0]] / a.batches:.3f} ms against {med[names[1]] / a.batches:.3f} ms; the native tail changes the pass by {med[names[0]] - med[names[1]]:+.3f} ms")
        say(f"  agreement: loss {res['native']['loss']:.6f} / {res['stock'][0]:.6f}, top1 {res['native']['top1']:.4f} / {res['stock'][1]:.4f}, top5 {res['native']['top5']:.4f} / {res['stock'][2]:.4f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
