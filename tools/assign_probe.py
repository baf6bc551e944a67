"""Max-IoU assignment without the matrix (csrc/assign.hip) against what a user of the package writes today: the whole [boxes x ground truths] matrix from
``ops.bbox_overlaps`` / ``ops.obb_overlaps`` pushed through upstream's procedure in stock tensor ops (``max_iou_assign_torch``: two ``max``, comparisons, the loop
over the ground truths), image by image (GPU box).

    python tools/assign_probe.py [--calls 20] [--rounds 5] [--limit 300] [--out profiles/assign_probe.txt]

Shapes of the Oriented R-CNN configs on a 1024 x 1024 crop, B = 2 images:
    RPN     261 888 horizontal anchors (3 per position on 256^2 + 128^2 + 64^2 + 32^2 + 16^2 positions) shared by the images, G = 40 / 200 / 1000 ground truths,
            0.7 / 0.3 / 0.3 with low-quality matches (the reference leaves the GPU above gpu_assign_thr = 200 ground truths)
    R-CNN   2 000 + G rotated proposals per image (the ground truths are appended, as upstream's add_gt_as_proposals does), G = 40 / 200, 0.5 / 0.5 / 0.5, no
            low-quality matches
Every shape is one GPU step: a child process of its own under a time limit of --limit seconds (a step that fails or runs out ends the probe: nothing more is started),
in which both sides alternate -- windows of --calls calls between device events, --rounds windows per side; median and spread (max - min) reported, and the peak
allocation of one call above its inputs (``torch.cuda.max_memory_allocated``; the fused side is given its buffers, as a captured call would be).  There is no
parent-commit number: the operator is new.  Whichever side is slower at a shape is reported as measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = [("rpn", 40), ("rpn", 200), ("rpn", 1000), ("rcnn", 40), ("rcnn", 200)]
B = 2


def anchors():
    """the 261 888 anchors of a 1024 x 1024 crop: strides 4 .. 64, scale 8, ratios 0.5 / 1 / 2"""
    import torch
    out = []
    for stride in (4, 8, 16, 32, 64):
        n = 1024 // stride
        c = (torch.arange(n, dtype=torch.float32) + 0.5) * stride
        cy, cx = torch.meshgrid(c, c, indexing="ij")
        for ratio in (0.5, 1.0, 2.0):
            w, h = 8.0 * stride / ratio ** 0.5, 8.0 * stride * ratio ** 0.5
            out.append(torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).reshape(-1, 4))
    return torch.cat(out)


def step(name, G, calls, rounds):
    import torch
    from dense_loss_probe import compare, say
    from gen_assign_golden import hull
    from gen_obb_golden import make_boxes
    from lemevit_amd import ops
    from lemevit_amd.detection import max_iou_assign_torch
    dev = "cuda"
    rot = [make_boxes(G, 21 + b)[0] for b in range(B)]
    if name == "rpn":
        boxes = anchors().to(dev)
        gts = torch.stack([torch.from_numpy(hull(r)).float() for r in rot]).to(dev)
        per_image = [boxes] * B
        cfg, overlaps = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True), ops.bbox_overlaps
    else:
        gts = torch.stack([torch.from_numpy(r).float() for r in rot]).to(dev)
        boxes = torch.stack([torch.cat([torch.from_numpy(make_boxes(2000, 31 + b)[0]).float().to(dev), gts[b]]) for b in range(B)])
        per_image = list(boxes)
        cfg, overlaps = dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False), ops.obb_overlaps
    N = boxes.shape[-2]
    labels = torch.arange(B * G, device=dev).reshape(B, G) % 15
    bufs = dict(gt_inds=torch.empty(B, N, dtype=torch.int64, device=dev), max_overlaps=torch.empty(B, N, device=dev), labels=torch.empty(B, N, dtype=torch.int64, device=dev),
                workspace=torch.empty(ops.max_iou_assign_workspace_bytes(B, G), dtype=torch.uint8, device=dev))

    def fused():
        return ops.max_iou_assign(boxes, gts, gt_labels=labels, **cfg, **bufs)

    def matrix():
        return [max_iou_assign_torch(overlaps(per_image[b], gts[b]), gt_labels=labels[b], **cfg) for b in range(B)]

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    kind = "horizontal anchors, shared" if name == "rpn" else "rotated proposals per image"
    sides = [("fused: lmv_max_iou_assign (B images in one call, caller-supplied buffers)", fused),
             ("matrix: ops overlaps + max_iou_assign_torch (stock tensor ops), image by image", matrix)]
    compare(f"--- {name}: B = {B}, N = {N} {kind}, G = {G}, {cfg['pos_iou_thr']} / {cfg['neg_iou_thr']} / {cfg['min_pos_iou']}, low-quality matches "
            f"{cfg['match_low_quality']}; the fp32 matrix of one image: {N * G * 4 / 1e6:.1f} MB", sides, calls, rounds)
    say(f"  peak allocation of one call above its inputs: fused {peak(fused):.2f} MB (its buffers are the caller's: {sum(t.numel() * t.element_size() for t in bufs.values()) / 1e6:.2f} MB), "
        f"matrix {peak(matrix):.2f} MB")
    gi, mo, lb = fused()
    want = matrix()
    same = all(torch.equal(gi[b], want[b][0]) and torch.equal(mo[b], want[b][1]) and torch.equal(lb[b], want[b][2]) for b in range(B))
    say(f"  results equal bit for bit: {same}; positives {int((gi > 0).sum())}, negatives {int((gi == 0).sum())}, ignored {int((gi < 0).sum())} of {B * N}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_probe.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one shape, e.g. rpn:200")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("assign_probe: needs an MI355X (no CPU fallback)")
        name, G = a.step.split(":")
        step(name, int(G), a.calls, a.rounds)
        return
    lines = [f"assign_probe: medians of {a.rounds} windows of {a.calls} calls; one process per shape, {a.limit} s each"]
    print(lines[0], flush=True)
    status = 0
    for name, G in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{name}:{G}", "--calls", str(a.calls), "--rounds", str(a.rounds)]
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
            lines.append(f"  {name} G = {G}: the step ended with status {code}; nothing more was started")
            print(lines[-1], flush=True)
            status = code
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
