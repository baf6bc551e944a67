"""Image gradient of the first stem convolution: the one-launch data gradient against stock PyTorch-ROCm, and what an image that requires grad costs a train step (GPU box).

    python tools/input_grad_probe.py [--batch 128] [--launches 50] [--steps 10]

1. lmv_conv3x3s2_nchw_dx at the headline shape (Base: B x 3 x 224 x 224, Co = 48), bf16 and fp32 operands, fp32 dx: us per launch (device events around --launches launches,
   the two sides alternating after a warm-up), the algorithm's bytes (dy once + dx once) over that time as a share of the 6.3 TB/s the MI355X sustains, and stock
   torch.nn.grad.conv2d_input on the same tensors in the same process as the comparison column.
2. LeMeViT-Base 224^2 bf16 train step (FlatAdamW) with and without requires_grad on the image, alternating.
3. in_chans 3 / 4 / 13: inference forward and train step of lemevit_base(in_chans=..)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import lemevit_amd
from lemevit_amd import ops
from lemevit_amd.optim import FlatAdamW

HBM = 6.3e12


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def kernel(B, n, rounds=4):
    Ho = Wo = 112
    Co = 48
    for dt in (torch.bfloat16, torch.float32):
        dy4 = torch.randn(B, Co, Ho, Wo, device="cuda").to(dt).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Co, 3, 3, 3, device="cuda") * 0.2).to(dt)
        wm = torch.zeros(Co, 32, device="cuda", dtype=dt)
        wm[:, :27] = w.reshape(Co, 27)
        g = dy4.permute(0, 2, 3, 1).reshape(-1, Co)
        img = torch.empty(B, 3, 224, 224, device="cuda")
        ours = lambda: ops.conv3x3s2_nchw_dx(g, wm, like=img)
        stock = lambda: torch.nn.grad.conv2d_input(img.shape, w, dy4, stride=2, padding=1)
        for f in (ours, stock):
            timed(f, 5)
        t = {"ours": [], "stock": []}
        for _ in range(rounds):
            t["ours"].append(timed(ours, n))
            t["stock"].append(timed(stock, n))
        to, ts = sorted(t["ours"])[rounds // 2], sorted(t["stock"])[rounds // 2]
        nbytes = g.numel() * g.element_size() + img.numel() * 4
        err = float((ours().double() - stock().double()).abs().max() / stock().double().abs().max())
        print(f"lmv_conv3x3s2_nchw_dx B={B} 3x224x224 Co=48 {str(dt)[6:]:8s}: {to:7.1f} us  ({nbytes / 1e6:.1f} MB -> {nbytes / to / 1e6:5.2f} TB/s = {100 * nbytes / (to * 1e-6) / HBM:4.1f} % of 6.3 TB/s)   "
              f"stock conv2d_input {ts:7.1f} us   ratio ours / stock {to / ts:.3f}   (max-abs difference {err:.1e}; rounds ours {['%.1f' % v for v in t['ours']]} stock {['%.1f' % v for v in t['stock']]})",
              flush=True)


def model_steps(B, steps, cin=3, both=True):
    m = lemevit_amd.create_model("lemevit_base", num_classes=1000, drop_path_rate=0.1, in_chans=cin).cuda().train()
    opt = FlatAdamW(m, lr=1e-3)
    x = torch.randn(B, cin, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (B,), device="cuda")

    def step(need):
        xi = x.detach().requires_grad_(need)
        opt.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(m(xi), y)
        loss.backward()
        opt.step()

    for need in (False, True):
        for _ in range(3):
            step(need)
    res = {False: [], True: []}
    for _ in range(3):
        for need in ((False, True) if both else (False,)):
            res[need].append(timed(lambda: step(need), steps) / 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items() if v}
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        for _ in range(3):
            m(x)
        fwd = sorted(timed(lambda: m(x), steps) / 1e3 for _ in range(3))[1]
    line = f"lemevit_base(in_chans={cin}) 224^2 bf16 B={B}: inference forward {fwd:7.2f} ms   train step {med[False]:7.2f} ms"
    if both:
        line += f"   with requires_grad on the image {med[True]:7.2f} ms ({med[True] - med[False]:+.2f} ms)"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    kernel(a.batch, a.launches)
    for cin in (3, 4, 13):
        model_steps(a.batch, a.steps, cin, both=True)


if __name__ == "__main__":
    main()
