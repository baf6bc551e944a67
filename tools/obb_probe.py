"""Rotated IoU and rotated NMS (csrc/obb.hip) against the stock-PyTorch formulations ``obb_overlaps_torch`` / ``obb_nms_torch`` -- the latter with its mask copy to
the host and the greedy scan there, which is what the reference's CUDA path pays per image and FPN level (GPU box).

    python tools/obb_probe.py [--calls 20] [--rounds 5] [--out profiles/obb_probe.txt]

Shapes of the Oriented R-CNN configs: overlaps 2 000 proposals x 40 ground truths (the assigners) and 512 x 512; NMS at N = 2 000 with thr 0.8 (the oriented RPN:
nms_pre = 2000) and at N = 2 000 with thr 0.1 over 15 groups (the test config).  Boxes are drawn like the test cases (clusters on a 1024 x 1024 crop, sides 8 ..
300).  Windows of --calls calls between device events in one process, --rounds windows per side, the sides alternating; median and spread (max - min) reported.
There is no parent-commit number: the operators are new.  The mask and the reduce launch of the NMS are also timed alone (``phases``); the reduce launch is one
workgroup walking a serial chain, and its time is reported as measured."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

from lemevit_amd import ops
from lemevit_amd.detection import obb_nms_torch, obb_overlaps_torch
from dense_loss_probe import LINES, compare, say
from gen_obb_golden import make_boxes


def boxes_of(n, seed, dev):
    b, s, g = make_boxes(n, seed, True)
    return torch.from_numpy(b).float().to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obb_probe.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("obb_probe: needs an MI355X (no CPU fallback)")
    dev = "cuda"
    say(f"obb_probe: {torch.cuda.get_device_name(0)}, medians of {a.rounds} windows of {a.calls} calls")
    for N, M in ((2000, 40), (512, 512)):
        b1, b2 = boxes_of(N, 11, dev)[0], boxes_of(M, 12, dev)[0]
        out = torch.empty(N, M, device=dev)
        sides = [("native: lmv_obb_overlaps (one launch, caller-supplied out)", lambda: ops.obb_overlaps(b1, b2, "iou", out=out)),
                 ("stock: obb_overlaps_torch (broadcast fp32 formulation)", lambda: obb_overlaps_torch(b1, b2))]
        compare(f"--- overlaps {N} x {M} (iou)", sides, a.calls, a.rounds)
        say(f"  agreement: max |native - stock| {float((ops.obb_overlaps(b1, b2) - obb_overlaps_torch(b1, b2)).abs().max()):.3e}; "
            f"pairs with IoU > 0: {int((out > 0).sum())} of {N * M}")
    for title, thr, grouped in (("RPN: N = 2000, thr 0.8, one group", 0.8, False), ("test: N = 2000, thr 0.1, 15 groups", 0.1, True)):
        N = 2000
        boxes, scores, groups = boxes_of(N, 13, dev)
        g = groups if grouped else None
        ws = torch.empty(ops.obb_nms_workspace_bytes(N), device=dev, dtype=torch.uint8)
        keep, count = torch.empty(N, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.int64)
        order = torch.sort(scores, descending=True, stable=True)[1]

        def native():
            return ops.obb_nms(boxes, scores, thr, g, workspace=ws, keep=keep, count=count)

        def stock():
            return obb_nms_torch(boxes, scores, thr, g)

        compare(f"--- NMS {title}", [("native: sort + mask launch + reduce launch, no host round trip", native),
                                     ("stock: sort + fp32 IoU matrix + mask copy + host greedy scan", stock)], a.calls, a.rounds)
        parts = [("torch.sort(stable=True) alone", lambda: torch.sort(scores, descending=True, stable=True)),
                 ("mask launch alone (phases = 1)", lambda: ops.obb_nms(boxes, scores, thr, g, order=order, workspace=ws, keep=keep, count=count, phases=1)),
                 ("reduce launch alone (phases = 2)", lambda: ops.obb_nms(boxes, scores, thr, g, order=order, workspace=ws, keep=keep, count=count, phases=2))]
        compare("  the parts of the native call, each alone", parts, a.calls, a.rounds)
        k, c = native()
        n = int(c)
        want = stock()
        say(f"  kept {n} of {N}; keep lists equal: {k[:n].tolist() == want.tolist()} (the stock side decides on its own fp32 IoUs: random boxes are not kept clear of the threshold)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
