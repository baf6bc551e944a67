"""The box coders (csrc/coder.hip) against what a user of the package writes today: upstream's tensor code in stock PyTorch (``midpoint_decode_torch`` ...,
with the ``permute(1, 2, 0).reshape(-1, 6)`` copy of every level's regression map for the map form and the per-image ``nonzero`` gather for the targets) (GPU box).

    python tools/coder_probe.py [--calls 20] [--rounds 5] [--limit 300] [--out profiles/coder_probe.txt]

Shapes of the Oriented R-CNN configs on a 1024 x 1024 crop:
    decode_map        the RPN's proposals of one image: 5 levels (256^2 .. 16^2 positions, 3 anchors each), the 2 000 top-scoring rows of each (768 on the last),
                      MidpointOffsetCoder, stds (1, 1, 1, 1, 0.5, 0.5); the maps are image 0 of a [2, 18, H, W] batch
    decode            the R-CNN head's detections: 512 RoIs x 15 classes, OBB2OBBDeltaXYWHTCoder, stds (0.1, 0.1, 0.2, 0.2, 0.1)
    encode_assigned   the RPN's targets: 8 images x 20 000 anchors x 50 ground truths, gt_inds as an assigner leaves them (about 1 % positive)
Every shape is one GPU step: a child process of its own under a time limit of --limit seconds (a step that fails or runs out ends the probe: nothing more is started),
in which both sides alternate -- windows of --calls calls between device events, --rounds windows per side; median and spread (max - min) reported, with the number
of launches of the native side and of tensor-producing operator calls of the stock side (counted by a dispatch mode: every ATen call whose result is not a view of
an input; each is at least one launch).  There is no parent-commit number: the operators are new.  Whichever side is slower at a shape is reported as measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ["decode_map", "decode", "encode_assigned"]


def count_ops(fn) -> int:
    """ATen calls of fn() whose result owns its memory (not a view of an argument)"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class Counter(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            outs = [o for o in (out if isinstance(out, (tuple, list)) else [out]) if isinstance(o, torch.Tensor)]
            ins = {a.untyped_storage().data_ptr() for a in args if isinstance(a, torch.Tensor)}
            if outs and any(o.untyped_storage().data_ptr() not in ins for o in outs):
                Counter.n += 1
            return out
    with Counter():
        fn()
    return Counter.n


def step(name, calls, rounds):
    import torch
    from dense_loss_probe import compare, say
    import gen_coder_golden as gen
    from lemevit_amd import ops
    from lemevit_amd.detection import (MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder, decode_map_torch, encode_assigned_torch, midpoint_decode_torch, midpoint_encode_torch,
                                       obb2obb_decode_torch)
    dev = "cuda"
    g = torch.Generator().manual_seed(11)
    rpn, rcnn = MidpointOffsetCoder(target_stds=gen.RPN_STDS), OBB2OBBDeltaXYWHTCoder(target_stds=gen.RCNN_STDS)
    if name == "decode_map":
        levels = []
        for stride in (4, 8, 16, 32, 64):
            n = 1024 // stride
            R = n * n * 3
            c = (torch.arange(n, dtype=torch.float32) + 0.5) * stride
            cy, cx = torch.meshgrid(c, c, indexing="ij")
            half = torch.tensor([4.0 * stride * r for r in (0.7, 1.0, 1.4)])
            anchors = torch.stack([cx[..., None] - half, cy[..., None] - half.flip(0), cx[..., None] + half, cy[..., None] + half.flip(0)], -1).reshape(-1, 4).to(dev)
            pred = (torch.randn(2, 18, n, n, generator=g) * 0.3).to(dev)
            index = torch.randperm(R, generator=g)[:min(2000, R)].to(dev)
            levels.append((anchors, pred[0], index, torch.empty(index.shape[0], 5, device=dev)))

        def native():
            return [rpn.decode_map(a, p, i, out=o) for a, p, i, o in levels]

        def stock():
            return [decode_map_torch(midpoint_decode_torch, a, p, i, rpn.means, rpn.stds) for a, p, i, _ in levels]
        title, launches = f"--- decode_map: 5 levels, {sum(l[2].shape[0] for l in levels)} rows of {sum(l[0].shape[0] for l in levels)} anchors", 5
        err = max(float((x - y).abs().max()) for x, y in zip(native(), stock()))
    elif name == "decode":
        N, C = 512, 15
        rois, deltas = (t.to(dev) for t in (gen.obb_decode_case(1000)["proposals"][:N], torch.randn(N, 5 * C, generator=g)))
        out = torch.empty(N, 5 * C, device=dev)

        def native():
            return ops.box_decode("obb2obb", rois, deltas, rcnn.means, rcnn.stds, out=out)

        def stock():
            return obb2obb_decode_torch(rois, deltas, rcnn.means, rcnn.stds)
        title, launches = f"--- decode: {N} RoIs x {C} classes (OBB2OBB)", 1
        err = float((native()[:, :2] - stock()[:, :2]).abs().max())
    else:
        B, N, G = 8, 20000, 50
        gts = torch.stack([torch.from_numpy(gen.canonical_boxes(G, 900 + b)).float() for b in range(B)]).to(dev)
        base = gts[:, torch.arange(N) % G]
        anchors = torch.stack([torch.from_numpy(gen.jitter_anchors(base[b].double().cpu().numpy(), 50 + b)).float() for b in range(B)]).to(dev)
        u = torch.rand(B, N, generator=g)
        inds = torch.where(u < 0.01, (torch.arange(N) % G + 1).expand(B, N), torch.where(u < 0.5, 0, -1)).to(dev)
        counts = torch.full((B,), G, dtype=torch.int32, device=dev)
        t, w = torch.empty(B, N, 6, device=dev), torch.empty(B, N, device=dev)

        def native():
            return rpn.encode_assigned(anchors, gts, inds, counts, targets=t, weights=w)

        def stock():
            return encode_assigned_torch(midpoint_encode_torch, anchors, gts, inds, rpn.means, rpn.stds, counts)
        title, launches = f"--- encode_assigned: {B} images x {N} anchors x {G} ground truths, {int((inds > 0).sum())} positive rows (midpoint)", 1
        err = float((native()[0] - stock()[0]).abs().max())
    sides = [(f"native: csrc/coder.hip, caller-supplied outputs ({launches} launch{'es' if launches > 1 else ''})", native),
             (f"stock PyTorch: upstream's tensor code ({count_ops(stock)} tensor-producing operator calls)", stock)]
    compare(title, sides, calls, rounds)
    say(f"  largest difference between the two sides: {err:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coder_probe.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one shape")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("coder_probe: needs an MI355X (no CPU fallback)")
        step(a.step, a.calls, a.rounds)
        return
    lines = [f"coder_probe: medians of {a.rounds} windows of {a.calls} calls; one process per shape, {a.limit} s each"]
    print(lines[0], flush=True)
    status = 0
    for name in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls), "--rounds", str(a.rounds)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.limit)
            out, code = r.stdout, r.returncode
            if code != 0:
                print(r.stderr, file=sys.stderr, end="", flush=True)
        except subprocess.TimeoutExpired as e:
            out, code = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124
        print(out, end="", flush=True)
        lines += out.rstrip("\n").split("\n")
        if code != 0:
            lines.append(f"  {name}: the step ended with status {code}; nothing more was started")
            print(lines[-1], flush=True)
            status = code
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
