"""Rotated RoIAlign over the FPN levels (csrc/rroi.hip: one plan launch, one forward launch, one backward launch, no atomics) against the stock-PyTorch
formulation run the way the stock extractor runs its RoI layer: per level behind a ``nonzero`` and an index copy (GPU box).

    python tools/rroi_probe.py [--calls 20] [--rounds 5] [--out profiles/rroi_probe.txt]

The Oriented R-CNN shape: B = 2 crops of 1024 x 1024, C = 256, levels 256^2 / 128^2 / 64^2 / 32^2 (strides 4 .. 32), R = 1024 proposals drawn like DOTA's
(sqrt(w h) log-uniform over 16 .. 800 pixels, aspect 1 .. 6, any angle), out 7 x 7, sample_num 2, extend_factor (1.4, 1.2), fp32 and bf16.  Windows of --calls
calls between device events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported, and
torch.cuda.max_memory_allocated of one call above what was allocated before it (features, RoIs and dY are inputs of both sides).  There is no parent-commit number:
the operator is new.  The backward launch is also timed alone and set against its write floor (every dX element stored once)."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lemevit_amd import ops
from lemevit_amd.detection import RotatedRoIExtractor, rroi_align_torch
from dense_loss_probe import LINES, compare, say
from dense_up_probe import peak_mb


def proposals(R, B, size, dev):
    g = torch.Generator().manual_seed(1)
    u = torch.rand(R, 6, generator=g)
    side = 16.0 * (800.0 / 16.0) ** u[:, 0]
    aspect = 1.0 + 5.0 * u[:, 1] ** 2
    rois = torch.stack([torch.floor(u[:, 2] * B).clamp(max=B - 1), u[:, 3] * size, u[:, 4] * size, side * aspect.sqrt(), side / aspect.sqrt(), (u[:, 5] * 2 - 1) * math.pi], 1)
    return rois.float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rois", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rroi_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rroi_probe: needs an MI355X (no CPU fallback)")
    torch.manual_seed(0)
    dev, B, C, size, strides, R = "cuda", 2, 256, 1024, (4, 8, 16, 32), a.rois
    scales = [1.0 / s for s in strides]
    ext = RotatedRoIExtractor(out_size=7, sample_num=2, featmap_strides=strides, out_channels=C)
    rois = proposals(R, B, size, dev)
    say(f"rroi_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    for dtype in (torch.float32, torch.bfloat16):
        es = 2 if dtype == torch.bfloat16 else 4
        feats = [torch.randn(B, C, size // s, size // s, device=dev).to(dtype).requires_grad_(True) for s in strides]
        dy = torch.randn(R, C, 7, 7, device=dev).to(dtype)
        dx_bytes = sum(f.numel() for f in feats) * es
        plan = ops.rroi_plan(rois, [f.shape[-2:] for f in feats], scales, B, (7, 7), 2, True, None, 56.0, (1.4, 1.2))
        hdr = plan.buf[:R * 32].view(torch.int32).reshape(R, 8).cpu()
        per_level = [int((hdr[:, 0] == l).sum()) for l in range(len(strides))]
        say(f"--- {dtype}: B = {B}, C = {C}, levels {[tuple(f.shape[-2:]) for f in feats]}, R = {R} (per level {per_level}), 7 x 7 x 2 x 2; features = dX {dx_bytes / 1e6:.1f} MB, "
            f"out = dY {dy.numel() * es / 1e6:.1f} MB, plan {plan.buf.numel() / 1e6:.1f} MB")
        out_buf = torch.empty(R, C, 7, 7, device=dev, dtype=dtype)
        dx_buf = [torch.empty_like(f) for f in feats]
        detached = [f.detach() for f in feats]

        def native_fwd():
            with torch.no_grad():
                return ext(detached, rois)

        def stock_fwd():
            with torch.no_grad():
                return rroi_align_torch(detached, rois, (7, 7), scales, 2, True, None, 56.0, (1.4, 1.2))

        def native_fb():
            return torch.autograd.grad(ext(feats, rois), feats, dy)

        def stock_fb():
            return torch.autograd.grad(rroi_align_torch(feats, rois, (7, 7), scales, 2, True, None, 56.0, (1.4, 1.2)), feats, dy)

        sides_f = [("native: plan + forward (two launches, no synchronisation)", native_fwd), ("stock: per level nonzero + gather formulation + index copy", stock_fwd)]
        sides_b = [("native: plan + forward + backward (three launches)", native_fb), ("stock: the same, autograd's index_put backward", stock_fb)]
        compare("plan + forward", sides_f, a.calls, a.rounds)
        say("  peak memory of one call above what was allocated before it: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, (_, f) in zip(("native", "stock"), sides_f)))
        compare("forward + backward", sides_b, a.calls, a.rounds)
        say("  peak memory of one call above what was allocated before it: " + ", ".join(f"{n} {peak_mb(f):.1f} MB" for n, (_, f) in zip(("native", "stock"), sides_b)))
        parts = [("lmv_rroi_plan alone", lambda: ops.rroi_plan(rois, plan.sizes, scales, B, (7, 7), 2, True, None, 56.0, (1.4, 1.2), plan=plan.buf)),
                 ("lmv_rroi_fwd alone", lambda: ops.rroi_align_fwd(detached, plan, out=out_buf)),
                 ("lmv_rroi_bwd alone", lambda: ops.rroi_align_bwd(dy, plan, detached, dx=dx_buf))]
        med = compare("the three launches, each alone (caller-supplied buffers)", parts, a.calls, a.rounds)
        t_bwd = med["lmv_rroi_bwd alone"] * 1e-6
        say(f"  backward against its write floor: {dx_bytes / 1e6:.1f} MB of dX stored once in {t_bwd * 1e6:.1f} us = {dx_bytes / t_bwd / 1e12:.3f} TB/s "
            f"(+ {dy.numel() * es / 1e6:.1f} MB of dY read at least once)")
        o_n, o_s = native_fwd().float(), stock_fwd().float()
        g_n, g_s = native_fb(), stock_fb()
        say(f"  agreement: forward max |native - stock| {float((o_n - o_s).abs().max()):.3e} (max |stock| {float(o_s.abs().max()):.3f}); "
            f"dX max |native - stock| {max(float((p.float() - q.float()).abs().max()) for p, q in zip(g_n, g_s)):.3e}")
        del feats, dy, detached, dx_buf, out_buf, o_n, o_s, g_n, g_s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
