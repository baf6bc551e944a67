"""Native mixup / cutmix and soft-target loss against their hand-written PyTorch restatement (GPU box).

    python tools/recipe_probe.py [--calls 20] [--steps 10] [--rounds 5] [--batch 128] [--sections 1,2,3,4] [--out profiles/recipe_probe.txt]

1. The mix launch at LeMeViT-Base's batch, 128 x 3 x 224 x 224: lmv_mix_images fp32 -> bf16 and uint8 -> bf16 (with the PrefetchLoader normalisation fused in)
   against the four-pass form a port of timm's Mixup runs -- x * lam + x.flip(0) * (1 - lam): flip, mul, mul, add -- plus the casts / normalisation it needs to
   hand the model the same tensor.  Mixup records (every pixel is computed); the batch (77 MB fp32) fits the 256 MB Infinity Cache, so these are warm numbers.
2. The loss, forward + backward, at 128 x 1000 bf16 logits: SoftTargetCrossEntropy on a MixedTarget (lmv_soft_ce + one multiply) against mixup_target (two one-hot
   scatters and two blends) + sum(-t * log_softmax(x)).mean() and its autograd backward.  And the accuracy of both against float64 on the same logits.
3. The LeMeViT-Base 224^2, bf16, B = 128 eager train step (FlatAdamW) with the native pair and with the PyTorch pair, two models, the sides alternating.
4. Random erasing in the mix launch, uint8 -> bf16 with the normalisation: lmv_mix_images; lmv_augment_images with an all-empty erase table, with a table drawn at
   probability 0.25 in 'pixel' mode (the reference's setting) and with every image erased; and the stock form, ops.mix_images followed by a per-image normal_() loop
   over the same boxes (what timm's RandomErasing does behind the PrefetchLoader normalisation, without its host draws).
--sections picks a subset (default: all four).
Windows of --calls / --steps between device events in one process, --rounds windows per side, median and spread (max - min) reported."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import lemevit_amd
from lemevit_amd import ops, recipe

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


def compare(title, sides, calls, rounds, unit="us", scale=1e3):
    for _, f in sides:
        timed(f, 3)
    t = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, f in sides:
            t[name].append(timed(f, calls))
    say(title)
    med = {}
    for name, _ in sides:
        v = sorted(x * scale for x in t[name])
        med[name] = v[rounds // 2]
        say(f"  {name:78s} {med[name]:10.3f} {unit}   spread {v[-1] - v[0]:.3f}   {['%.3f' % (x * scale) for x in t[name]]}")
    return med


def torch_target(y, lam, N, s):
    """timm.data.mixup.mixup_target"""
    off = s / N
    on = 1.0 - s + off
    y1 = torch.full((y.shape[0], N), off, device=y.device).scatter_(1, y.view(-1, 1), on)
    y2 = torch.full((y.shape[0], N), off, device=y.device).scatter_(1, y.flip(0).view(-1, 1), on)
    return y1 * lam + y2 * (1.0 - lam)


def torch_soft_ce(x, t):
    return torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--sections", default="1,2,3,4")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "recipe_probe.txt"))
    a = ap.parse_args()
    sections = {int(v) for v in a.sections.split(",")}
    if not torch.cuda.is_available():
        raise SystemExit("recipe_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    B, N, lam = a.batch, 1000, 0.3
    dev = "cuda"
    table = recipe.pack_records(recipe.make_records([(lam, 0, 0, 0, 0, lam)] * B)).to(dev)

    xf = torch.randn(B, 3, 224, 224, device=dev)
    xu = torch.randint(0, 256, (B, 3, 224, 224), device=dev, dtype=torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1) * 255
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1) * 255
    scale, shift = (1.0 / std).reshape(3).contiguous(), (-mean / std).reshape(3).contiguous()
    nel = xf.numel()
    logits = torch.randn(B, N, device=dev).to(torch.bfloat16)
    y = torch.randint(0, N, (B,), device=dev)
    tgt = lemevit_amd.MixedTarget(y, table, 0.1, N)
    crit = lemevit_amd.SoftTargetCrossEntropy()
    if 1 in sections:
        mix_section(a, B, lam, table, xf, xu, mean, std, scale, shift, nel)
    if 2 in sections:
        loss_section(a, B, N, lam, table, logits, y, tgt, crit)
    if 4 in sections:
        erase_section(a, B, table, xu, scale, shift)
    del xu
    if 3 in sections:
        step_section(a, B, N, lam, xf, y, crit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


def mix_section(a, B, lam, table, xf, xu, mean, std, scale, shift, nel):
    # ---- 1. the mix launch
    sides = [("(a) lmv_mix_images fp32 -> bf16 (4 + 2 B / element)", lambda: ops.mix_images(xf, table, torch.bfloat16)),
             ("(b) torch: (x * lam + x.flip(0) * (1 - lam)).to(bf16)", lambda: (xf * lam + xf.flip(0) * (1.0 - lam)).to(torch.bfloat16))]
    med = compare(f"mix {B} x 3 x 224 x 224, fp32 -> bf16, {a.rounds} windows of {a.calls} calls per side, sides alternating (us per call, median; spread; all windows)", sides, a.calls, a.rounds)
    say(f"  (a) {6.0 * nel / 1e6:.1f} MB per call from the shapes -> {6.0 * nel / (med[sides[0][0]] * 1e-6) / 1e12:.2f} TB/s (the batch fits the Infinity Cache: not an HBM figure)")

    def torch_u8():
        x = (xu.float() - mean) / std
        return (x * lam + x.flip(0) * (1.0 - lam)).to(torch.bfloat16)
    sides = [("(a) lmv_mix_images uint8 -> bf16, normalisation fused (1 + 2 B / element)", lambda: ops.mix_images(xu, table, torch.bfloat16, scale, shift)),
             ("(b) torch: ((x.float() - mean) / std), then the four passes, then .to(bf16)", torch_u8)]
    compare(f"mix {B} x 3 x 224 x 224, uint8 -> bf16 with normalisation (us per call)", sides, a.calls, a.rounds)
    d = (ops.mix_images(xu, table, torch.bfloat16, scale, shift).float() - torch_u8().float()).abs().max()
    say(f"  largest difference between the two results: {float(d):.3e} (bf16 outputs)")


def loss_section(a, B, N, lam, table, logits, y, tgt, crit):
    # ---- 2. the loss
    def native_loss():
        leaf = logits.detach().requires_grad_(True)
        crit(leaf, tgt).backward()
        return leaf.grad

    def torch_loss():
        leaf = logits.detach().requires_grad_(True)
        torch_soft_ce(leaf.float(), torch_target(y, lam, N, 0.1)).backward()
        return leaf.grad
    compare(f"soft-target loss forward + backward, {B} x {N} bf16 logits (us per call)",
            [("(a) SoftTargetCrossEntropy(MixedTarget): lmv_soft_ce (2 launches) + 1 multiply", native_loss), ("(b) torch: mixup_target + log_softmax-based loss + autograd", torch_loss)],
            a.calls, a.rounds)
    x32 = logits.float()
    t64 = tgt.dense(torch.float64)
    logp = F.log_softmax(x32.double(), dim=-1)
    ref_loss = float((-(t64 * logp).sum(-1)).mean())
    ref_grad = (logp.exp() - t64) / B
    l_n, _, g_n = ops.soft_ce(x32, labels=y, table=table, smoothing=0.1)
    leaf = x32.clone().requires_grad_(True)
    l_t = torch_soft_ce(leaf, t64.float())
    l_t.backward()
    say(f"  accuracy against float64 on the same fp32 logits: loss error native {abs(float(l_n) - ref_loss):.3e} / torch fp32 {abs(float(l_t) - ref_loss):.3e}; "
        f"largest dlogits error native {float((g_n.double() - ref_grad).abs().max()):.3e} / torch fp32 {float((leaf.grad.double() - ref_grad).abs().max()):.3e}")


def step_section(a, B, N, lam, xf, y, crit):
    # ---- 3. the train step
    models = [lemevit_amd.create_model("lemevit_base", num_classes=N).cuda().train() for _ in range(2)]
    opts = [lemevit_amd.FlatAdamW(m, lr=1e-4, eps=1e-8, weight_decay=0.05) for m in models]
    mix = lemevit_amd.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=N, out_dtype=torch.bfloat16, seed=0)

    def native_step():
        opts[0].zero_grad(set_to_none=True)
        xm, t = mix(xf, y)
        with torch.autocast("cuda", torch.bfloat16):
            crit(models[0](xm), t).backward()
        opts[0].step()

    def torch_step():
        opts[1].zero_grad(set_to_none=True)
        xm = xf * lam + xf.flip(0) * (1.0 - lam)
        t = torch_target(y, lam, N, 0.1)
        with torch.autocast("cuda", torch.bfloat16):
            torch_soft_ce(models[1](xm), t).backward()
        opts[1].step()
    sides = [("(a) Mixup (host draw + upload + lmv_mix_images -> bf16) + SoftTargetCrossEntropy", native_step), ("(b) torch: four-pass mixup + mixup_target + log_softmax-based loss", torch_step)]
    med = compare(f"lemevit_base 224^2 bf16 B={B}, eager train step, {a.rounds} windows of {a.steps} steps per side, sides alternating (ms per step)", sides, a.steps, a.rounds, "ms", 1.0)
    say(f"  the native pair changes the step by {med[sides[0][0]] - med[sides[1][0]]:+.3f} ms")


def erase_section(a, B, table, xu, scale, shift):
    # ---- 4. random erasing in the mix launch
    H = W = 224
    dev = xu.device
    empty = torch.zeros((B, ops.ERASE_RECORD_WORDS), dtype=torch.int32, device=dev)
    re = recipe.RandomErasing(probability=0.25, mode="pixel", seed=0)
    boxes_q, _ = re.draw(B, H, W, dev)
    drawn, drawn_key = re.table.clone(), re.key.clone()
    full = recipe.RandomErasing(probability=1.0, mode="pixel", seed=1)
    boxes_f, _ = full.draw(B, H, W, dev)

    def share(bx):
        return float(sum((r[1] - r[0]) * (r[3] - r[2]) for img in bx for r in img)) / (B * H * W)
    say(f"erase tables: probability 0.25 -> {int((boxes_q[:, 0, 1] > boxes_q[:, 0, 0]).sum())} of {B} images, {100 * share(boxes_q):.2f} % of the pixels; every image -> {100 * share(boxes_f):.2f} % of the pixels")

    def stock(bx):
        def run():
            out = ops.mix_images(xu, table, torch.bfloat16, scale, shift)
            for b in range(B):
                yl, yh, xl, xh = (int(v) for v in bx[b, 0])
                if yh > yl:
                    out[b, :, yl:yh, xl:xh].normal_()
            return out
        return run
    sides = [("(a) lmv_mix_images uint8 -> bf16, normalisation fused", lambda: ops.mix_images(xu, table, torch.bfloat16, scale, shift)),
             ("(b) lmv_augment_images, all-empty erase table", lambda: ops.augment_images(xu, table, empty, drawn_key, "pixel", torch.bfloat16, scale, shift)),
             ("(c) lmv_augment_images, table drawn at probability 0.25, pixel mode", lambda: ops.augment_images(xu, table, drawn, drawn_key, "pixel", torch.bfloat16, scale, shift)),
             ("(d) lmv_augment_images, every image erased, pixel mode", lambda: ops.augment_images(xu, table, full.table, full.key, "pixel", torch.bfloat16, scale, shift)),
             ("(e) stock: ops.mix_images + per-image normal_() over the boxes of (c)", stock(boxes_q)),
             ("(f) stock: ops.mix_images + per-image normal_() over the boxes of (d)", stock(boxes_f))]
    compare(f"mix + normalise + erase {B} x 3 x 224 x 224, uint8 -> bf16, {a.rounds} windows of {a.calls} calls per side, sides alternating (us per call, median; spread; all windows)",
            sides, a.calls, a.rounds)
    out = ops.augment_images(xu, table, drawn, drawn_key, "pixel", torch.bfloat16, scale, shift)
    base = ops.mix_images(xu, table, torch.bfloat16, scale, shift)
    inside = torch.zeros((B, 1, H, W), dtype=torch.bool, device=dev)
    for b in range(B):
        yl, yh, xl, xh = (int(v) for v in boxes_q[b, 0])
        inside[b, 0, yl:yh, xl:xh] = True
    m = inside.expand_as(out)
    z = out[m].double()
    say(f"  (c) outside the boxes equal to (a): {bool(torch.equal(out[~m], base[~m]))}; inside: {z.numel()} samples, mean {float(z.mean()):+.5f}, variance {float(z.var()):.5f} (bf16 values)")


if __name__ == "__main__":
    main()
