"""Gradient clipping: what a native clipped step costs against torch's clipping in front of an unclipped step, and the rate of the norm launch (GPU box).

    python tools/clip_grad_probe.py [--steps 20] [--rounds 5] [--batch 128] [--out profiles/clip_grad_probe.txt]

LeMeViT-Base 224^2, bf16 autocast, B = 128, eager steps (zero_grad, forward, loss, backward, step), ONE model and ONE FlatAdamW whose clipping attributes are switched between
the sides, the sides alternating, --rounds windows of --steps steps each between device events, median of the windows:
  (a) the unclipped step;
  (b) the native step with clip_grad = 5.0 (lmv_grad_norm + lmv_adamw_flat_clip + the coefficient handed to torch's fused AdamW for the other parameters);
  (c) torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0) in front of the unclipped step -- torch's code, the comparison, not the code under test.
Then the norm launch alone over the gradients of that model: us per call (both stages), bytes read (4 per gradient element), TB/s and the share of the 6.29 TB/s
measured copy bandwidth.  Every timed call follows a 512 MB write to another buffer, so the ~212 MB of gradients come from HBM and not from the 256 MB Infinity
Cache a back-to-back loop would re-read them from; the back-to-back (warm re-read) figure is printed next to it, named as such."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lemevit_amd
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
    return a.elapsed_time(b) / n          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--clip", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "clip_grad_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_grad_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    model = lemevit_amd.create_model("lemevit_base", num_classes=1000).cuda().train()
    opt = lemevit_amd.FlatAdamW(model, lr=1e-4, eps=1e-8, weight_decay=0.05)
    x = torch.randn(a.batch, 3, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (a.batch,), device="cuda")
    loss_fn = torch.nn.CrossEntropyLoss()

    def backward():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.bfloat16):
            loss_fn(model(x), y).backward()

    def plain():
        opt.clip_grad = None
        backward()
        opt.step()

    def native():
        opt.clip_grad = a.clip
        backward()
        opt.step()

    def torch_clip():
        opt.clip_grad = None
        backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), a.clip)
        opt.step()

    sides = [("(a) unclipped step", plain), (f"(b) native clip_grad={a.clip}", native), (f"(c) torch clip_grad_norm_({a.clip}) + unclipped step", torch_clip)]
    for _, f in sides:
        timed(f, 3)
    t = {name: [] for name, _ in sides}
    for _ in range(a.rounds):
        for name, f in sides:
            t[name].append(timed(f, a.steps))
    say(f"lemevit_base 224^2 bf16 B={a.batch}, eager train step, {a.rounds} windows of {a.steps} steps per side, sides alternating (ms per step, median; all windows)")
    med = {}
    for name, _ in sides:
        med[name] = sorted(t[name])[a.rounds // 2]
        say(f"  {name:55s} {med[name]:8.3f} ms   {['%.3f' % v for v in t[name]]}")
    names = [n for n, _ in sides]
    say(f"  native clipping adds {med[names[1]] - med[names[0]]:+.3f} ms to the unclipped step; torch's adds {med[names[2]] - med[names[0]]:+.3f} ms")

    backward()
    segs = [opt._flat_g] + opt._rest_grads()
    n = sum(s.numel() for s in segs)
    stat = torch.zeros(ops.GRAD_STAT_FLOATS, device="cuda")
    call = lambda: ops.grad_norm(segs, a.clip, stat)
    timed(call, 10)
    warm = sorted(timed(call, 200) * 1e3 for _ in range(a.rounds))[a.rounds // 2]
    evict = torch.empty(512 << 20, device="cuda", dtype=torch.uint8)
    cold = []
    for _ in range(50):
        evict.zero_()                      # pushes the gradients out of the Infinity Cache
        cold.append(timed(call, 1) * 1e3)
    us = sorted(cold)[len(cold) // 2]
    ref = float(torch.linalg.vector_norm(torch.cat([s.reshape(-1).double() for s in segs])))
    say(f"lmv_grad_norm over {len(segs)} segments, {n} elements ({4 * n / 1e6:.1f} MB read): {us:.1f} us per call (both stages, launch gaps included, "
        f"median of {len(cold)} single calls each behind a 512 MB write) -> {4 * n / us / 1e6:.2f} TB/s = {100 * 4 * n / (us * 1e-6) / HBM:.1f} % of 6.29 TB/s from HBM; "
        f"200 calls back to back (warm re-read, partly from the Infinity Cache: not an HBM rate) {warm:.1f} us; norm {float(stat[0]):.9g} vs float64 {ref:.9g}")
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
