"""Horizontal RoIAlign with the adaptive grid (csrc/roi.hip) and horizontal NMS (csrc/nms.hip) against the stock-PyTorch formulations ``roi_align_torch`` (per-level
``nonzero`` loop, the adaptive grid padded to the batch's largest grid, advanced indexing, autograd's ``index_put`` backward) and ``nms_torch`` (mask copy to the host
and the greedy scan there) (GPU box).

    python tools/roi_probe.py [--calls 10] [--rounds 5] [--out profiles/roi_probe.txt]

Shapes of the Mask R-CNN config: R = 512 (training: the sampled RoIs) and R = 1000 (testing: the proposals), C = 256, the four levels of an 800 x 1344 image (strides
4 / 8 / 16 / 32, B = 2), out_size 7 (box head) and 14 (mask head), sample_num = 0, bf16 channels-last and fp32 NCHW; NMS at N = 1000 / 2000, thr 0.7 (RPN) and thr 0.5
over 15 groups (test).  RoIs are drawn like detector proposals: sqrt(w h) log-uniform in 16 .. 600 pixels, w / h in 1/3 .. 3, clipped to the image.  Windows of --calls calls between device
events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported.  There is no parent-commit number: the operators are
new."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from lemevit_amd import ops
from lemevit_amd.detection import RoIExtractor, nms_torch, roi_align_torch
from dense_loss_probe import LINES, compare, say
from detfill import det_uniform
from gen_roi_golden import make_boxes

IMAGE, STRIDES, B, C = (800, 1344), (4, 8, 16, 32), 2, 256


def proposals(R, dev):
    u = det_uniform(6 * R, 0x9805 + R).reshape(-1, 6) * 0.5 + 0.5
    side, aspect = 16.0 * (600.0 / 16.0) ** u[:, 0], 3.0 ** (2.0 * u[:, 1] - 1.0)          # sqrt(w h) log-uniform in 16 .. 600, w / h log-uniform in 1/3 .. 3
    w, h = side * np.sqrt(aspect), side / np.sqrt(aspect)
    cx, cy = IMAGE[1] * u[:, 2], IMAGE[0] * u[:, 3]
    x1, y1, x2, y2 = np.clip(cx - w / 2, 0, IMAGE[1]), np.clip(cy - h / 2, 0, IMAGE[0]), np.clip(cx + w / 2, 0, IMAGE[1]), np.clip(cy + h / 2, 0, IMAGE[0])
    b = (u[:, 4] * B).astype(np.int64) % B
    return torch.from_numpy(np.stack([b, x1, y1, x2, y2], 1).astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roi_probe: needs an MI355X (no CPU fallback)")
    dev = "cuda"
    torch.manual_seed(0)
    say(f"roi_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    sizes = [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES]
    scales = [1.0 / s for s in STRIDES]
    for dtype, fmt, tag in ((torch.bfloat16, torch.channels_last, "bf16 channels-last"), (torch.float32, torch.contiguous_format, "fp32 NCHW")):
        feats = [torch.randn(B, C, h, w, device=dev).to(dtype).contiguous(memory_format=fmt) for h, w in sizes]
        for R in (512, 1000):
            rois = proposals(R, dev)
            for out_size in (7, 14):
                ext = RoIExtractor(out_size=out_size, sample_num=0, featmap_strides=STRIDES, out_channels=C)
                dy = torch.randn(R, C, out_size, out_size, device=dev).to(dtype)
                xs = [f.clone().requires_grad_(True) for f in feats]
                plan = ops.roi_plan(rois, sizes, scales, B, (out_size, out_size), 0)
                out = torch.empty(R, C, out_size, out_size, device=dev, dtype=dtype)
                dx = [torch.empty_like(f) for f in feats]

                def native():
                    o = ext(xs, rois)
                    return torch.autograd.grad(o, xs, dy)

                def stock():
                    o = roi_align_torch(xs, rois, (out_size, out_size), scales, 0)
                    return torch.autograd.grad(o, xs, dy)

                compare(f"--- RoIAlign forward + backward, {tag}, R = {R}, C = {C}, {out_size} x {out_size}, sample_num = 0, 4 levels of {IMAGE[0]} x {IMAGE[1]}, B = {B}",
                        [("native: RoIExtractor (plan + forward + backward launch)", native), ("stock: roi_align_torch + autograd", stock)], a.calls, a.rounds)
                parts = [("plan launch alone", lambda: ops.roi_plan(rois, sizes, scales, B, (out_size, out_size), 0, plan=plan.buf)),
                         ("forward launch alone", lambda: ops.roi_align_fwd(feats, plan, out=out)),
                         ("backward launch alone", lambda: ops.roi_align_bwd(dy, plan, feats, dx=dx))]
                compare("  the parts of the native call, each alone", parts, a.calls, a.rounds)
                o_n, o_s = ext(feats, rois).float(), roi_align_torch(feats, rois, (out_size, out_size), scales, 0).float()
                say(f"  agreement: max |native - stock| {float((o_n - o_s).abs().max()):.3e} (max |out| {float(o_s.abs().max()):.3f}); plan {plan.buf.numel() / R:.0f} bytes per RoI")
    for title, N, thr, grouped in (("RPN: N = 1000, thr 0.7, one group", 1000, 0.7, False), ("RPN: N = 2000, thr 0.7, one group", 2000, 0.7, False),
                                   ("test: N = 1000, thr 0.5, 15 groups", 1000, 0.5, True), ("test: N = 2000, thr 0.5, 15 groups", 2000, 0.5, True)):
        bx, sc, gr = make_boxes(N, 13, True)
        boxes, scores, groups = torch.from_numpy(bx).float().to(dev), torch.from_numpy(sc).to(dev), torch.from_numpy(gr).to(dev)
        g = groups if grouped else None
        ws = torch.empty(ops.nms_workspace_bytes(N), device=dev, dtype=torch.uint8)
        keep, count = torch.empty(N, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int64)
        order = torch.sort(scores, descending=True, stable=True)[1]

        def native():
            return ops.nms(boxes, scores, thr, g, workspace=ws, keep=keep, count=count)

        def stock():
            return nms_torch(boxes, scores, thr, g)

        compare(f"--- NMS {title}", [("native: sort + mask launch + reduce launch, no host round trip", native),
                                     ("stock: sort + fp32 IoU matrix + mask copy + host greedy scan", stock)], a.calls, a.rounds)
        parts = [("torch.sort(stable=True) alone", lambda: torch.sort(scores, descending=True, stable=True)),
                 ("mask launch alone (phases = 1)", lambda: ops.nms(boxes, scores, thr, g, order=order, workspace=ws, keep=keep, count=count, phases=1)),
                 ("reduce launch alone (phases = 2)", lambda: ops.nms(boxes, scores, thr, g, order=order, workspace=ws, keep=keep, count=count, phases=2))]
        compare("  the parts of the native call, each alone", parts, a.calls, a.rounds)
        k, c = native()
        n = int(c)
        say(f"  kept {n} of {N}; keep lists equal: {k[:n].tolist() == stock().tolist()} (the stock side decides on its own fp32 IoUs: random boxes are not kept clear of the threshold)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
