"""The head losses (csrc/headloss.hip) against what a user of the package writes today: the stock-PyTorch formulations ``rpn_head_loss_torch`` /
``bbox_head_loss_torch`` (dense targets from ``encode_assigned_torch``, the permute copies, ``binary_cross_entropy_with_logits`` / ``cross_entropy``, the smooth-L1
element-wise chain, gradients from autograd, host synchronisations) (GPU box).

    python tools/headloss_probe.py [--calls 20] [--rounds 5] [--limit 300] [--out profiles/headloss_probe.txt]

Shapes of the Oriented R-CNN configs:
    rpn_fp32     B = 8, levels 256^2 ... 16^2, A = 3 (261 888 anchors per image), 256 sampled per image (128 positive), fp32 channels-last maps
    rpn_bf16     the same with bf16 channels-last maps; the stock side's time INCLUDES a cast of every map to fp32 (its targets and anchors are fp32)
    rcnn         R = 8 x 512 RoIs, K = 15, class-agnostic regression (C = 1), a quarter positive
Every shape is one GPU step: a child process of its own under a time limit of --limit seconds (a step that fails or runs out ends the probe: nothing more is
started), in which both sides alternate -- windows of --calls calls between device events, --rounds windows per side; median and spread reported for the forward
alone and for forward + backward, with the launches of the native side, the tensor-producing operator calls of the stock side and each side's peak allocation
above the inputs.  There is no parent-commit number: the operators are new.  Whichever side is slower at a shape is reported as measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ["rpn_fp32", "rpn_bf16", "rcnn"]


def step(name, calls, rounds):
    import numpy as np
    import torch
    from coder_probe import count_ops
    from dense_loss_probe import compare, say
    from sampler_probe import peak_above
    from lemevit_amd import ops
    from lemevit_amd.detection import RCNN_TARGET_STDS, RPN_TARGET_STDS, bbox_head_loss, bbox_head_loss_torch, rpn_head_loss, rpn_head_loss_torch
    dev = "cuda"
    rng = np.random.default_rng(0)

    def boxes5(n):          # (cx, cy, w, h, theta)
        return np.stack([rng.uniform(100, 900, n), rng.uniform(100, 900, n), rng.uniform(20, 200, n), rng.uniform(10, 100, n), rng.uniform(-1.5, 1.5, n)], 1).astype(np.float32)

    def clear(ts):
        for t in ts:
            t.grad = None

    if name.startswith("rpn"):
        dt = torch.float32 if name == "rpn_fp32" else torch.bfloat16
        B, A, G, sizes = 8, 3, 40, (256, 128, 64, 32, 16)
        N = sum(s * s * A for s in sizes)
        maps = [torch.randn(B, ch * A, s, s, device=dev).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_() for ch in (1, 6) for s in sizes]
        L = len(sizes)
        ctr, wh = rng.uniform(100, 900, (N, 2)), rng.uniform(16, 256, (N, 2))
        anchors = torch.from_numpy(np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)).to(dev)
        gts = torch.from_numpy(np.stack([boxes5(G) for _ in range(B)])).to(dev)
        inds, mask = np.zeros((B, N), dtype=np.int64), np.zeros((B, N), dtype=np.uint8)
        for b in range(B):
            pick = rng.choice(N, 256, replace=False)
            inds[b, pick[:128]] = rng.integers(1, G + 1, 128)
            mask[b, pick[:128]], mask[b, pick[128:]] = 1, 2
        gt_inds, mask = torch.from_numpy(inds).to(dev), torch.from_numpy(mask).to(dev)
        bufs = dict(stats=torch.empty(2 * L + 3, device=dev), workspace=torch.empty(ops.rpn_loss_workspace_bytes(B, N), dtype=torch.uint8, device=dev))

        def native_fwd():
            with torch.no_grad():
                return rpn_head_loss(maps[:L], maps[L:], anchors, gts, gt_inds, mask, **bufs)

        def native_both():
            clear(maps)
            out = rpn_head_loss(maps[:L], maps[L:], anchors, gts, gt_inds, mask, **bufs)
            (out["loss_rpn_cls"].sum() + out["loss_rpn_bbox"].sum()).backward()
            return out

        def stock_fwd():
            with torch.no_grad():
                return rpn_head_loss_torch([m.float() for m in maps[:L]], [m.float() for m in maps[L:]], anchors, gts, gt_inds, mask, None, (0.0,) * 6, RPN_TARGET_STDS)

        def stock_both():
            clear(maps)
            out = rpn_head_loss_torch([m.float() for m in maps[:L]], [m.float() for m in maps[L:]], anchors, gts, gt_inds, mask, None, (0.0,) * 6, RPN_TARGET_STDS)
            (out["loss_rpn_cls"].sum() + out["loss_rpn_bbox"].sum()).backward()
            return out
        title = f"--- {name}: {B} images x {N} anchors ({L} levels, A = {A}), 256 sampled per image, {str(dt).split('.')[1]} channels-last maps"
        keys, launches = ("loss_rpn_cls", "loss_rpn_bbox"), (2, 3)
    else:
        B, num, K, G = 8, 512, 15, 40
        R = B * num
        z = torch.randn(R, K + 1, device=dev).requires_grad_()
        p = torch.randn(R, 5, device=dev).requires_grad_()
        maps = [z, p]
        gts = torch.from_numpy(np.stack([boxes5(G) for _ in range(B)])).to(dev)
        rois = torch.from_numpy(np.concatenate([np.repeat(np.arange(B), num)[:, None].astype(np.float32), boxes5(R)], 1)).to(dev)
        ind = np.where(np.arange(R) % 4 == 0, rng.integers(1, G + 1, R), 0).astype(np.int64)
        s_gt_inds = torch.from_numpy(ind).to(dev)
        s_labels = torch.from_numpy(np.where(ind > 0, rng.integers(0, K, R), K).astype(np.int64)).to(dev)
        bufs = dict(stats=torch.empty(7, device=dev), workspace=torch.empty(ops.rcnn_loss_workspace_bytes(R), dtype=torch.uint8, device=dev))

        def native_fwd():
            with torch.no_grad():
                return bbox_head_loss(z, p, rois, gts, s_gt_inds, s_labels, **bufs)

        def native_both():
            clear(maps)
            out = bbox_head_loss(z, p, rois, gts, s_gt_inds, s_labels, **bufs)
            (out["loss_cls"] + out["loss_bbox"]).backward()
            return out

        def stock_fwd():
            with torch.no_grad():
                return bbox_head_loss_torch(z, p, rois, gts, s_gt_inds, s_labels, None, (0.0,) * 5, RCNN_TARGET_STDS)

        def stock_both():
            clear(maps)
            out = bbox_head_loss_torch(z, p, rois, gts, s_gt_inds, s_labels, None, (0.0,) * 5, RCNN_TARGET_STDS)
            (out["loss_cls"] + out["loss_bbox"]).backward()
            return out
        title = f"--- rcnn: R = {B} x {num} RoIs, K = {K}, C = 1, {int((ind > 0).sum())} positive"
        keys, launches = ("loss_cls", "loss_bbox"), (2, 3)
    a = native_both()
    g_native = [m.grad.float().clone() for m in maps]
    b = stock_both()
    worst = max(float((x - m.grad.float()).abs().max() / m.grad.float().abs().max().clamp(min=1e-30)) for x, m in zip(g_native, maps))
    say(title)
    say("  losses: " + "; ".join(f"{k} native {a[k].detach().float().sum().item():.6f} stock {b[k].detach().float().sum().item():.6f}" for k in keys) +
        f"; largest gradient difference / largest gradient {worst:.2e}")
    compare("  forward", [(f"native: csrc/headloss.hip, supplied buffers ({launches[0]} launches, no synchronisation)", native_fwd),
                          (f"stock PyTorch ({count_ops(stock_fwd)} tensor-producing operator calls)", stock_fwd)], calls, rounds)
    compare("  forward + backward", [(f"native: one autograd node ({launches[1]} launches + autograd's own for the sum and the upstream gradients; allocates the gradients)", native_both),
                                     ("stock PyTorch, gradients from autograd", stock_both)], calls, rounds)
    say(f"  peak allocation above the inputs, forward: native with stats and workspace supplied {peak_above(native_fwd)} bytes (buffers, allocated once: "
        f"{sum(v.numel() * v.element_size() for v in bufs.values())} bytes), stock {peak_above(stock_fwd)} bytes")
    say(f"  peak allocation above the inputs, forward + backward (the gradients of all inputs, {sum(m.numel() * m.element_size() for m in maps)} bytes, among them): "
        f"native {peak_above(native_both)} bytes, stock {peak_above(stock_both)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headloss_probe.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one shape")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("headloss_probe: needs an MI355X (no CPU fallback)")
        step(a.step, a.calls, a.rounds)
        return
    lines = [f"headloss_probe: medians of {a.rounds} windows of {a.calls} calls; one process per shape, {a.limit} s each"]
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
