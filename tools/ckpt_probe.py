"""Activation checkpointing: ms per train step and torch.cuda.max_memory_allocated, LeMeViT-Base 224^2, bf16 autocast, FlatAdamW (GPU box).

    python tools/ckpt_probe.py [--batch 128] [--steps 10] [--big B --cap-gib G]

Runs use_checkpoint_stages = [] and = all stages at --batch, then prints the per-image peak of each and the batch that each would fit into the
device's memory at that rate.  --big B runs both again at batch B with the caching allocator of this process capped at G GiB
(torch.cuda.set_per_process_memory_fraction): pick B so that only the checkpointed model fits under the cap.  (The whole device would need
B in the thousands, where some activations pass 2^31 elements -- sizes no test of the library covers.)"""
import argparse
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import lemevit_amd
from lemevit_amd.optim import FlatAdamW


def run(ck, B, steps, warmup=3):
    gc.collect()
    torch.cuda.empty_cache()
    m = lemevit_amd.create_model("lemevit_base", num_classes=1000, drop_path_rate=0.1, use_checkpoint_stages=ck).cuda().train()
    opt = FlatAdamW(m, lr=1e-3)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    y = torch.randint(0, 1000, (B,), device="cuda")
    base = torch.cuda.memory_allocated()

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(m(x), y)
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    peak = torch.cuda.max_memory_allocated()
    del m, opt, x, y
    return ms, peak, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--cap-gib", type=float, default=0.0)
    a = ap.parse_args()
    total = torch.cuda.get_device_properties(0).total_memory
    res = {}
    for name, ck in (("[]", []), ("all", [0, 1, 2, 3, 4])):
        ms, peak, base = run(ck, a.batch, a.steps)
        res[name] = (ms, peak, base)
        per_img = (peak - base) / a.batch
        print(f"Base 224^2 bf16 B={a.batch} use_checkpoint_stages={name:4s}: {ms:7.2f} ms/step  max_memory_allocated {peak / 2**30:6.2f} GiB  "
              f"({per_img / 2**20:6.1f} MiB per image above the {base / 2**30:.2f} GiB of weights and optimizer state -> ~B {int((total - base) / per_img)} "
              f"fits in {total / 2**30:.0f} GiB)", flush=True)
    (m0, p0, _), (m1, p1, _) = res["[]"], res["all"]
    print(f"checkpointing all stages: step time x{m1 / m0:.3f} ({m1 - m0:+.2f} ms), peak x{p1 / p0:.3f} ({(p1 - p0) / 2**30:+.2f} GiB)", flush=True)
    if a.big:
        if a.cap_gib:
            torch.cuda.set_per_process_memory_fraction(min(1.0, a.cap_gib * 2**30 / total))
        for name, ck in (("[]", []), ("all", [0, 1, 2, 3, 4])):
            try:
                ms, peak, _ = run(ck, a.big, max(2, a.steps // 2), warmup=1)
                print(f"Base 224^2 bf16 B={a.big} use_checkpoint_stages={name:4s} (allocator cap {a.cap_gib or total / 2**30:.0f} GiB): {ms:7.2f} ms/step  "
                      f"max_memory_allocated {peak / 2**30:6.2f} GiB", flush=True)
            except torch.cuda.OutOfMemoryError:
                print(f"Base 224^2 bf16 B={a.big} use_checkpoint_stages={name:4s} (allocator cap {a.cap_gib or total / 2**30:.0f} GiB): does not fit", flush=True)
                torch.cuda.synchronize()


if __name__ == "__main__":
    main()
