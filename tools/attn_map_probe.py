"""Attention maps: what lmv_attn_probs costs per launch against stock PyTorch-ROCm, and what LeMeViT.attention_maps adds to a forward pass (GPU box).

    python tools/attn_map_probe.py [--launches 50] [--out profiles/attn_map_probe.txt]

1. lmv_attn_probs, bf16 operands, per-head and head-mean, at the D-block shapes of LeMeViT-Base 224^2, B = 128 (stage 1: 16 x 3136 and 3136 x 16 at C = 96; stage 2:
   16 x 784 and 784 x 16 at C = 192) and of LeMeViT-Tiny's dense stage 1 at 1344 x 800, B = 2 (16 x 67 200 at C = 64): us per launch (device events around --launches
   launches, every shape warmed up, the two sides alternating, median of the rounds), the bytes the launch must move (q and k rows once, the log-sum-exp, P once) and their
   share of the 6.29 TB/s measured copy bandwidth; the stock column is torch.softmax(q_h.float() @ k_h.float().transpose(-1, -2) * scale, -1) (.mean(1) for head-mean) on
   heads re-packed to [B, h, L, 32] beforehand, in the same process.
2. The error of both against the float64 softmax of the same operands (the figures tests/test_attn_map_gpu.py derives its bound from).
3. model.attention_maps(img) with every block and heads="mean" against a plain eval forward forced onto the per-block schedule, LeMeViT-Base 224^2 bf16 B = 128."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lemevit_amd
import lemevit_amd.model as M
from lemevit_amd import ops

HBM = 6.29e12
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
    return a.elapsed_time(b) / n * 1e3          # us


def alternate(ours, stock, n, rounds=4):
    for f in (ours, stock):
        timed(f, 3)
    t = {"ours": [], "stock": []}
    for _ in range(rounds):
        t["ours"].append(timed(ours, n))
        t["stock"].append(timed(stock, n))
    return sorted(t["ours"])[rounds // 2], sorted(t["stock"])[rounds // 2], t


def heads_of(t, off, C):
    B, L, _ = t.shape
    return t[..., off:off + C].reshape(B, L, C // 32, 32).permute(0, 2, 1, 3).contiguous()


def kernel(what, B, Lq, Lk, C, scale, n):
    H = C // 32
    torch.manual_seed(0)
    qp = (torch.randn(B, Lq, 3 * C, device="cuda") * 1.5).to(torch.bfloat16)
    kp = (torch.randn(B, Lk, 3 * C, device="cuda") * 1.5).to(torch.bfloat16)
    q, k, v = (qp, 0), (kp, C), (kp, 2 * C)
    _, lse = ops.attn_fwd(q, k, v, C, scale, want_lse=True)
    qh, kh = heads_of(qp, 0, C), heads_of(kp, C, C)
    ref = torch.softmax(qh.double() @ kh.double().transpose(-1, -2) * scale, -1)
    for mean in (False, True):
        ours = lambda: ops.attn_probs(q, k, lse, C, scale, head_mean=mean)
        if mean:
            stock = lambda: torch.softmax(qh.float() @ kh.float().transpose(-1, -2) * scale, -1).mean(1)
        else:
            stock = lambda: torch.softmax(qh.float() @ kh.float().transpose(-1, -2) * scale, -1)
        to, ts, t = alternate(ours, stock, n)
        nbytes = B * (Lq + Lk) * C * 2 + B * H * Lq * 4 + B * (1 if mean else H) * Lq * Lk * 4
        r = ref.mean(1) if mean else ref
        eo = float((ours().double() - r).abs().max() / r.abs().max())
        es = float((stock().double() - r).abs().max() / r.abs().max())
        say(f"lmv_attn_probs {what:34s} {'head-mean' if mean else 'per-head '}: {to:8.1f} us  ({nbytes / 1e6:7.1f} MB -> {nbytes / to / 1e6:5.2f} TB/s = "
            f"{100 * nbytes / (to * 1e-6) / HBM:4.1f} % of 6.29 TB/s)   stock softmax(q k^T) {ts:8.1f} us   ratio ours / stock {to / ts:.3f}   "
            f"error vs float64: ours {eo:.1e}, torch fp32 {es:.1e}   (rounds ours {['%.1f' % x for x in t['ours']]} stock {['%.1f' % x for x in t['stock']]})")
    del ref


def model_pass(B, n):
    m = lemevit_amd.create_model("lemevit_base", num_classes=1000).cuda().eval()
    x = torch.randn(B, 3, 224, 224, device="cuda")

    def plain_per_block():
        keep = (M._SSTAGE, M._INFER_SIDE, M._INFER_TAIL_PARTS)
        M._SSTAGE, M._INFER_SIDE, M._INFER_TAIL_PARTS = False, False, 1
        try:
            with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
                return m(x)
        finally:
            M._SSTAGE, M._INFER_SIDE, M._INFER_TAIL_PARTS = keep

    def plain():
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
            return m(x)

    def maps():
        with torch.autocast("cuda", torch.bfloat16):
            return m.attention_maps(x)

    for f in (plain, plain_per_block, maps):
        timed(f, 3)
    tm, tp, _ = alternate(maps, plain_per_block, n)
    ts = timed(plain, n)
    _, mp = maps()
    nbytes = sum(t.numel() * 4 for rec in mp.values() for _, t in rec.items())
    say(f"lemevit_base 224^2 bf16 B={B}: attention_maps(img), {len(mp)} blocks, heads='mean' ({nbytes / 1e6:.1f} MB of maps) {tm / 1e3:7.2f} ms   "
        f"plain eval forward on the per-block schedule {tp / 1e3:7.2f} ms (+{(tm - tp) / 1e3:.2f} ms)   shipped eval forward (persistent stage kernels) {ts / 1e3:7.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attn_map_probe.txt"))
    a = ap.parse_args()
    B, n = a.batch, a.launches
    sx = lambda N, C: ops.dca_scales(N, 16, C)
    kernel(f"Base s1 meta<-image 16x3136 C=96 B={B}", B, 16, 3136, 96, sx(3136, 96)[1], n)
    kernel(f"Base s1 image<-meta 3136x16 C=96 B={B}", B, 3136, 16, 96, sx(3136, 96)[0], n)
    kernel(f"Base s2 meta<-image 16x784 C=192 B={B}", B, 16, 784, 192, sx(784, 192)[1], n)
    kernel(f"Base s2 image<-meta 784x16 C=192 B={B}", B, 784, 16, 192, sx(784, 192)[0], n)
    kernel("Tiny dense s1 16x67200 C=64 B=2", 2, 16, 67200, 64, sx(67200, 64)[1], n)
    model_pass(B, max(5, n // 5))
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
