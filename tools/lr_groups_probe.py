"""Per-group learning rates: what the grouped update costs against the scalar one, on the kernel alone and on a whole train step (GPU box).

    python tools/lr_groups_probe.py [--calls 20] [--steps 10] [--rounds 5] [--batch 128] [--out profiles/lr_groups_probe.txt]

1. The kernels on LeMeViT-Base's flat buffer (the parameters, gradients and moments of a FlatAdamW(layer_decay=0.75): ~64 groups of block parameters):
   (a) lmv_adamw_flat with the per-element decay mask -- 34 B per element (p, m, v read and written, g and the mask read, the bf16 copy written);
   (b) lmv_adamw_flat_groups with one group byte per 8 elements and the table in LDS -- 30.125 B per element.
   Both with the step count on the device and the bf16 copy, the sides alternating, --rounds windows of --calls calls each between device events in one process;
   the buffers (~3 GB) are far larger than the 256 MB Infinity Cache, so back-to-back calls read HBM.  Reported: us per call of every window, the median, the
   spread (max - min of the windows) and the rate the byte counts imply.
2. The LeMeViT-Base 224^2, bf16, B = 128 eager train step with FlatAdamW() and with FlatAdamW(layer_decay=0.75), two models, the sides alternating."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lemevit_amd
from lemevit_amd import ops

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


def report(title, sides, t, unit, scale, rounds):
    say(title)
    med = {}
    for name, _ in sides:
        v = sorted(x * scale for x in t[name])
        med[name] = v[rounds // 2]
        say(f"  {name:62s} {med[name]:10.3f} {unit}   spread {v[-1] - v[0]:.3f}   {['%.3f' % (x * scale) for x in t[name]]}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lr_groups_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lr_groups_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    models = [lemevit_amd.create_model("lemevit_base", num_classes=1000).cuda().train() for _ in range(2)]
    plain = lemevit_amd.FlatAdamW(models[0], lr=1e-4, eps=1e-8, weight_decay=0.05)
    grouped = lemevit_amd.FlatAdamW(models[1], lr=1e-4, eps=1e-8, weight_decay=0.05, layer_decay=0.75)

    # ---- 1. the kernels alone, on the grouped optimizer's buffers (gradients: noise, so that the moments stay finite and ordinary)
    o = grouped
    n = o._flat_p.numel()
    o._flat_g.normal_(0.0, 1e-3)
    mask = (o._hyper[o._group_of_unit.long(), 1] != 0).float().repeat_interleave(ops.ADAMW_UNIT)
    g0 = o.param_groups[0]
    b1, b2 = g0["betas"]
    step = torch.ones((), device="cuda", dtype=torch.int32)

    def scalar():
        ops.adamw_flat(o._flat_p, o._flat_g, o._exp_avg, o._exp_avg_sq, mask, 1e-4, b1, b2, g0["eps"], 0.05, 0, shadow=o._shadow, step_dev=step)

    def table():
        ops.adamw_flat_groups(o._flat_p, o._flat_g, o._exp_avg, o._exp_avg_sq, o._group_of_unit, o._hyper, b1, b2, g0["eps"], 0, shadow=o._shadow, step_dev=step)

    sides = [("(a) lmv_adamw_flat, fp32 decay mask (34 B / element)", scalar), (f"(b) lmv_adamw_flat_groups, {o._hyper.shape[0]} groups (30.125 B / element)", table)]
    for _, f in sides:
        timed(f, 3)
    t = {name: [] for name, _ in sides}
    for _ in range(a.rounds):
        for name, f in sides:
            t[name].append(timed(f, a.calls))
    med = report(f"flat update of lemevit_base, {n} elements, {a.rounds} windows of {a.calls} calls per side, sides alternating (us per call, median; spread = max - min; all windows)",
                 sides, t, "us", 1e3, a.rounds)
    for (name, _), nbytes in zip(sides, (34.0, 30.125)):
        say(f"  {name[:3]} {nbytes * n / 1e9:.3f} GB per call from the shapes -> {nbytes * n / (med[name] * 1e-6) / 1e12:.2f} TB/s")
    del mask
    o.refresh()

    # ---- 2. the train step
    x = torch.randn(a.batch, 3, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (a.batch,), device="cuda")
    loss_fn = torch.nn.CrossEntropyLoss()

    def stepper(model, opt):
        def run():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.bfloat16):
                loss_fn(model(x), y).backward()
            opt.step()
        return run
    sides = [("(a) FlatAdamW()", stepper(models[0], plain)), (f"(b) FlatAdamW(layer_decay=0.75): {len(grouped.param_groups)} groups", stepper(models[1], grouped))]
    for _, f in sides:
        timed(f, 3)
    t = {name: [] for name, _ in sides}
    for _ in range(a.rounds):
        for name, f in sides:
            t[name].append(timed(f, a.steps))
    med = report(f"lemevit_base 224^2 bf16 B={a.batch}, eager train step, {a.rounds} windows of {a.steps} steps per side, sides alternating (ms per step, median; spread; all windows)",
                 sides, t, "ms", 1.0, a.rounds)
    names = [nm for nm, _ in sides]
    say(f"  layer_decay adds {med[names[1]] - med[names[0]]:+.3f} ms to the step")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
