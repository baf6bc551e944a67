"""Native dense-prediction losses and metrics against the same formulas in stock PyTorch (GPU box).

    python tools/dense_loss_probe.py [--calls 20] [--rounds 5] [--out profiles/dense_loss_probe.txt]

Two shapes: the change-detection batch 8 x 2 x 256 x 256 in bf16 (metadata.json: loss_function hybrid) and the segmentation batch 10 x 5 x 512 x 512 in fp32
(num_classes 5, ignore_index 5), uint8 label maps for the native side, int64 for PyTorch (F.cross_entropy takes nothing else).
1. DenseLoss forward + backward against the reference's hybrid_loss restated here (FocalLoss(gamma=0) + dice_loss: view / transpose / contiguous / log_softmax /
   gather / mean, an eye(K)[true] one-hot, permute, softmax and two reductions) and its autograd backward; the forward alone; and the accuracy of both against
   the float64 oracle on the same logits.
2. DenseLoss(ignore_index=) against F.cross_entropy(ignore_index=), forward + backward.
3. SegMeter.update against argmax + bincount(K y + pred) + the copy of the histogram to the host (what a device-side confusion matrix costs in PyTorch; the
   reference copies the whole prediction map instead).
The bytes of a native launch (logits + labels read; + dlogits written in the backward; + the prediction map in the meter) over its time give the rate printed.
Windows of --calls calls between device events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import lemevit_amd
from lemevit_amd import dense

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


def compare(title, sides, calls, rounds):
    for _, f in sides:
        timed(f, 3)
    t = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, f in sides:
            t[name].append(timed(f, calls))
    say(title)
    med = {}
    for name, _ in sides:
        v = sorted(x * 1e3 for x in t[name])
        med[name] = v[rounds // 2]
        say(f"  {name:86s} {med[name]:10.3f} us   spread {v[-1] - v[0]:.3f}   {['%.3f' % (x * 1e3) for x in t[name]]}")
    return med


def torch_focal0(input, target):
    """FocalLoss(gamma=0, alpha=None).forward of the reference, restated"""
    input = input.view(input.size(0), input.size(1), -1).transpose(1, 2)
    input = input.contiguous().view(-1, input.size(2))
    logpt = F.log_softmax(input, dim=-1).gather(1, target.view(-1, 1)).view(-1)
    return (-1 * logpt).mean()


def torch_dice(logits, true, eye, eps=1e-7):
    """dice_loss of the reference, restated (the reference builds eye(K) on the host per call; here it is a device tensor made once)"""
    one_hot = eye[true.squeeze(1)].permute(0, 3, 1, 2).float().type(logits.type())
    probas = F.softmax(logits, dim=1)
    dims = (0,) + tuple(range(2, true.ndimension()))
    inter = torch.sum(probas * one_hot, dims)
    card = torch.sum(probas + one_hot, dims)
    return 1 - (2.0 * inter / (card + eps)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_loss_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_loss_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    dev = "cuda"
    say(f"dense_loss_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    for (B, K, H, W), dtype, ignore in (((8, 2, 256, 256), torch.bfloat16, None), ((10, 5, 512, 512), torch.float32, 5)):
        es = 2 if dtype == torch.bfloat16 else 4
        npix = B * H * W
        x = (torch.randn(B, K, H, W, device=dev) * 3).to(dtype)
        y64 = torch.randint(0, K, (B, 1, H, W), device=dev)
        if ignore is not None:
            y64[torch.rand(B, 1, H, W, device=dev) < 0.2] = ignore
        y8 = y64.to(torch.uint8)
        eye = torch.eye(K, device=dev)
        say(f"--- logits [{B}, {K}, {H}, {W}] {str(dtype).replace('torch.', '')} ({npix * K * es / 1e6:.1f} MB), labels uint8 ({npix / 1e6:.1f} MB) native / int64 ({npix * 8 / 1e6:.1f} MB) PyTorch")
        fwd_bytes, bwd_bytes = npix * (K * es + 1), npix * (2 * K * es + 1)
        if ignore is None:
            # 1. hybrid
            crit = dense.DenseLoss(ce=1.0, dice=1.0, avg="all")
            xn, xt = x.clone().requires_grad_(True), x.clone().requires_grad_(True)

            def native_fb():
                xn.grad = None
                crit(xn, y8).backward()

            def torch_fb():
                xt.grad = None
                (torch_focal0(xt, y64) + torch_dice(xt, y64, eye)).backward()

            with torch.no_grad():
                med = compare("1. hybrid loss (cross-entropy + dice), forward", [("DenseLoss(ce=1, dice=1, avg='all'): lmv_dense_loss_fwd (two launches)", lambda: crit(x, y8)),
                                                                                  ("PyTorch: FocalLoss(gamma=0) + dice_loss restated", lambda: torch_focal0(x, y64) + torch_dice(x, y64, eye))], a.calls, a.rounds)
            n = med["DenseLoss(ce=1, dice=1, avg='all'): lmv_dense_loss_fwd (two launches)"]
            say(f"  native forward: {fwd_bytes / 1e6:.1f} MB in {n:.1f} us = {fwd_bytes / n / 1e6:.2f} TB/s (both launches)")
            med = compare("1. hybrid loss, forward + backward", [("DenseLoss: lmv_dense_loss_fwd + lmv_dense_loss_bwd (three launches)", native_fb),
                                                               ("PyTorch: FocalLoss(gamma=0) + dice_loss restated, autograd", torch_fb)], a.calls, a.rounds)
            n = med["DenseLoss: lmv_dense_loss_fwd + lmv_dense_loss_bwd (three launches)"]
            say(f"  native forward + backward: {(fwd_bytes + bwd_bytes) / 1e6:.1f} MB in {n:.1f} us = {(fwd_bytes + bwd_bytes) / n / 1e6:.2f} TB/s (three launches and autograd's host time)")
            native_fb(); torch_fb()
            ref = dense.reference_dense(x.cpu(), y64.cpu(), ce=1.0, dice=1.0, avg="all")
            rg = torch.from_numpy(ref["dlogits"])
            gmax = float(rg.abs().max())
            say(f"  accuracy against float64: loss error native {abs(float(crit(x, y8)) - ref['loss']):.3e}, PyTorch {abs(float(torch_focal0(x.float(), y64) + torch_dice(x.float(), y64, eye)) - ref['loss']):.3e} (fp32 inputs);"
                f" largest dlogits error native {float((xn.grad.double().cpu() - rg).abs().max()):.3e}, PyTorch {float((xt.grad.double().cpu() - rg).abs().max()):.3e} of {gmax:.3e} (both stored in {str(dtype).replace('torch.', '')})")
        else:
            # 2. cross-entropy with an ignore index
            crit = dense.DenseLoss(ignore_index=ignore)
            xn, xt = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            yt = y64[:, 0]

            def native_fb():
                xn.grad = None
                crit(xn, y8).backward()

            def torch_fb():
                xt.grad = None
                F.cross_entropy(xt, yt, ignore_index=ignore).backward()

            with torch.no_grad():
                med = compare("2. cross-entropy with ignore_index, forward", [("DenseLoss(ignore_index=5): lmv_dense_loss_fwd (two launches)", lambda: crit(x, y8)),
                                                                             ("PyTorch: F.cross_entropy(ignore_index=5)", lambda: F.cross_entropy(x, yt, ignore_index=ignore))], a.calls, a.rounds)
            n = med["DenseLoss(ignore_index=5): lmv_dense_loss_fwd (two launches)"]
            say(f"  native forward: {fwd_bytes / 1e6:.1f} MB in {n:.1f} us = {fwd_bytes / n / 1e6:.2f} TB/s (both launches)")
            med = compare("2. cross-entropy with ignore_index, forward + backward", [("DenseLoss: lmv_dense_loss_fwd + lmv_dense_loss_bwd (three launches)", native_fb),
                                                                                     ("PyTorch: F.cross_entropy(ignore_index=5), autograd", torch_fb)], a.calls, a.rounds)
            n = med["DenseLoss: lmv_dense_loss_fwd + lmv_dense_loss_bwd (three launches)"]
            say(f"  native forward + backward: {(fwd_bytes + bwd_bytes) / 1e6:.1f} MB in {n:.1f} us = {(fwd_bytes + bwd_bytes) / n / 1e6:.2f} TB/s (three launches and autograd's host time)")
            native_fb(); torch_fb()
            ref = dense.reference_dense(x.cpu(), y64.cpu(), ignore_index=ignore)
            rg = torch.from_numpy(ref["dlogits"])
            say(f"  accuracy against float64: loss error native {abs(float(crit(x, y8)) - ref['loss']):.3e}, PyTorch {abs(float(F.cross_entropy(x, yt, ignore_index=ignore)) - ref['loss']):.3e};"
                f" largest dlogits error native {float((xn.grad.double().cpu() - rg).abs().max()):.3e}, PyTorch {float((xt.grad.double().cpu() - rg).abs().max()):.3e} of {float(rg.abs().max()):.3e}")
        # 3. the meter
        meter = dense.SegMeter(K, ignore_index=ignore)
        meter.update(x, y8)
        yflat = y64.reshape(-1)

        def torch_conf():
            pred = x.argmax(1).reshape(-1)
            on = yflat < K if ignore is None else (yflat != ignore)
            return torch.bincount(yflat[on] * K + pred[on], minlength=K * K).cpu()

        with torch.no_grad():
            med = compare("3. confusion matrix of a batch", [("SegMeter.update: lmv_dense_loss_fwd in metrics mode (two launches, no synchronisation)", lambda: meter.update(x, y8)),
                                                            ("PyTorch: argmax + bincount(K y + pred) + the histogram's copy to the host", torch_conf)], a.calls, a.rounds)
        n = med["SegMeter.update: lmv_dense_loss_fwd in metrics mode (two launches, no synchronisation)"]
        say(f"  native: {(fwd_bytes + npix) / 1e6:.1f} MB in {n:.1f} us = {(fwd_bytes + npix) / n / 1e6:.2f} TB/s (both launches)")
        meter.reset()
        meter.update(x, y8)
        assert torch.equal(meter.conf.cpu().reshape(-1), torch_conf()), "the two confusion matrices differ"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
