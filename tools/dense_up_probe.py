"""The dense losses on low-resolution logits (lmv_dense_up_loss_fwd / _bwd: the bilinear upsampling inside the pass) against the two paths that store the
upsampled map (GPU box).

    python tools/dense_up_probe.py [--calls 20] [--rounds 5] [--out profiles/dense_up_probe.txt]

Three shapes: the change-detection head 8 x 2 x 64 x 64 -> 256 x 256 in bf16 with align_corners=True and the hybrid loss (Models.py:221 + hybrid_loss); the
segmentation decode head 10 x 6 x 128 x 128 -> 512 x 512 in fp32, cross-entropy with ignore_index; the 16 x auxiliary head 10 x 6 x 32 x 32 -> 512 x 512.
For each: forward, forward + backward and SegMeter.update of
    fused   DenseLoss(upsample=True) / SegMeter(upsample=True) on the low-resolution logits;
    (a)     F.interpolate followed by the plain DenseLoss / SegMeter -- the best path without these kernels;
    (b)     F.interpolate followed by stock PyTorch (the formulas of tools/dense_loss_probe.py).
with torch.cuda.max_memory_allocated over one forward + backward of each (reset before it; the inputs are allocated already and count in all three).
Windows of --calls calls between device events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from lemevit_amd import dense
from dense_loss_probe import LINES, compare, say, torch_dice, torch_focal0


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_up_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_up_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    dev = "cuda"
    say(f"dense_up_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    shapes = [((8, 2, 64, 64), (256, 256), torch.bfloat16, True, None, "hybrid loss (change detection, 4 x)"),
              ((10, 6, 128, 128), (512, 512), torch.float32, False, 255, "cross-entropy with ignore_index (decode head, 4 x)"),
              ((10, 6, 32, 32), (512, 512), torch.float32, False, 255, "cross-entropy with ignore_index (auxiliary head, 16 x)")]
    for (B, K, h, w), (H, W), dtype, ac, ignore, what in shapes:
        es = 2 if dtype == torch.bfloat16 else 4
        x = (torch.randn(B, K, h, w, device=dev) * 3).to(dtype)
        y64 = torch.randint(0, K, (B, 1, H, W), device=dev)
        if ignore is not None:
            y64[torch.rand(B, 1, H, W, device=dev) < 0.2] = ignore
        y8, yt = y64.to(torch.uint8), y64[:, 0].contiguous()
        eye = torch.eye(K, device=dev)
        kw = dict(ce=1.0, dice=1.0, avg="all") if ignore is None else dict(ignore_index=ignore)
        fused, plain = dense.DenseLoss(upsample=True, align_corners=ac, **kw), dense.DenseLoss(**kw)
        say(f"--- {what}: logits [{B}, {K}, {h}, {w}] {str(dtype).replace('torch.', '')} ({B * K * h * w * es / 1e6:.2f} MB) -> {H} x {W}, align_corners={ac}; "
            f"the upsampled map: {B * K * H * W * es / 1e6:.1f} MB, uint8 labels {B * H * W / 1e6:.1f} MB")

        def up(t):
            return F.interpolate(t, size=(H, W), mode="bilinear", align_corners=ac)

        def stock(z):
            return torch_focal0(z, y64) + torch_dice(z, y64, eye) if ignore is None else F.cross_entropy(z, yt, ignore_index=ignore)

        xs = [x.clone().requires_grad_(True) for _ in range(3)]

        def fb(i, f):
            def run():
                xs[i].grad = None
                f(xs[i]).backward()
            return run
        sides_f = [("fused: DenseLoss(upsample=True) (two launches)", lambda: fused(x, y8)), ("(a) F.interpolate + DenseLoss", lambda: plain(up(x), y8)),
                   ("(b) F.interpolate + stock PyTorch", lambda: stock(up(x)))]
        sides_fb = [("fused: DenseLoss(upsample=True) (three launches)", fb(0, lambda t: fused(t, y8))), ("(a) F.interpolate + DenseLoss, autograd", fb(1, lambda t: plain(up(t), y8))),
                    ("(b) F.interpolate + stock PyTorch, autograd", fb(2, lambda t: stock(up(t))))]
        with torch.no_grad():
            compare("forward", sides_f, a.calls, a.rounds)
        med = compare("forward + backward", sides_fb, a.calls, a.rounds)
        names = [n for n, _ in sides_fb]
        if med[names[0]] > med[names[1]]:
            say(f"  the fused path LOSES to (a) at this shape: {med[names[0]]:.1f} us against {med[names[1]]:.1f} us")
        say("  peak memory of one forward + backward above what was allocated before it: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, (_, f) in zip(("fused", "(a)", "(b)"), sides_fb)))
        ref = dense.reference_dense(x.cpu(), y64.cpu(), upsample=(H, W), align_corners=ac, **kw)
        rg = torch.from_numpy(ref["dlogits"])
        for f in (s[1] for s in sides_fb):
            f()
        say(f"  accuracy against float64: loss error fused {abs(float(fused(x, y8)) - ref['loss']):.3e}, (a) {abs(float(plain(up(x), y8)) - ref['loss']):.3e}, (b) {abs(float(stock(up(x).float())) - ref['loss']):.3e};"
            f" largest dlogits error fused {float((xs[0].grad.double().cpu() - rg).abs().max()):.3e}, (a) {float((xs[1].grad.double().cpu() - rg).abs().max()):.3e},"
            f" (b) {float((xs[2].grad.double().cpu() - rg).abs().max()):.3e} of {float(rg.abs().max()):.3e}")
        # the meter
        mf, mp = dense.SegMeter(K, ignore_index=ignore, upsample=True, align_corners=ac), dense.SegMeter(K, ignore_index=ignore)
        mf.update(x, y8)
        mp.update(up(x), y8)
        yflat = y64.reshape(-1)

        def torch_conf():
            pred = up(x).argmax(1).reshape(-1)
            on = yflat < K if ignore is None else (yflat != ignore)
            return torch.bincount(yflat[on] * K + pred[on], minlength=K * K).cpu()

        with torch.no_grad():
            compare("confusion matrix of a batch", [("fused: SegMeter(upsample=True).update (two launches, no synchronisation)", lambda: mf.update(x, y8)),
                                                   ("(a) F.interpolate + SegMeter.update", lambda: mp.update(up(x), y8)),
                                                   ("(b) F.interpolate + argmax + bincount + the histogram's copy to the host", torch_conf)], a.calls, a.rounds)
            say("  peak memory of one update: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, f in (("fused", lambda: mf.update(x, y8)), ("(a)", lambda: mp.update(up(x), y8)), ("(b)", torch_conf))))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
