"""The RPN head's proposal stage (csrc/proposal.hip, ``rpn_proposals``) against what a user of the package writes today: upstream's ``_get_bboxes_single`` in stock
PyTorch (``rpn_proposals_torch``: per image and level a permute copy, a sigmoid, a full sort, index copies; then ``cat``, the decode, ``obb_nms_torch`` with its
[Ktot, Ktot] fp32 IoU matrix copied to the host, a slice) (GPU box).

    python tools/proposal_probe.py [--calls 20] [--rounds 5] [--stock-calls 20] [--limit 400] [--out profiles/proposal_probe.txt]

Shapes of the Oriented R-CNN configs on a 1024 x 1024 crop: levels 256^2, 128^2, 64^2, 32^2, 16^2 with A = 3 (261 888 anchors per image), nms_pre = max_num = 2000,
nms_thr = 0.8, min_bbox_size = 0 (Ktot = 8 768 slots per image); B = 2 and 8; fp32 and bf16 channels-last maps.  Every shape is one GPU step: a child process of
its own under a time limit of --limit seconds (a step that fails or runs out ends the probe: nothing more is started).  In a step the select launches alone
(``ops.rpn_select``, outputs and workspace supplied) are timed in windows of --calls calls between device events, --rounds windows; then the whole stage, both
sides alternating in that process -- windows of --calls calls of ``rpn_proposals`` with its buffers supplied and of --stock-calls calls of
``rpn_proposals_torch`` (it synchronises per image, and a call takes about half a second at B = 8: a shorter window shortens a step), --rounds windows per side;
median and spread (max - min) reported, with each side's peak allocation above the inputs.  The two sides differ by design where fp32 scores tie (upstream's sort is unstable) and where a NaN logit
occurs; the probe prints the proposals per image of both sides and how many of the stock side's boxes the native side has bit for bit or within 1e-3 pixels.
There is no parent-commit number: the operator is new.  Whichever side is slower at a shape is reported as measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ["2_fp32", "2_bf16", "8_fp32", "8_bf16"]
STRIDES, CROP, NMS_PRE, MAX_NUM, NMS_THR = (4, 8, 16, 32, 64), 1024, 2000, 2000, 0.8


def step(name, calls, rounds, stock_calls):
    import torch
    from dense_loss_probe import compare, say
    from sampler_probe import peak_above
    from lemevit_amd import ops
    from lemevit_amd.detection import AnchorGenerator, MidpointOffsetCoder, RPNProposalBuffers, rpn_proposals, rpn_proposals_torch
    dev = "cuda"
    B, dtype = int(name.split("_")[0]), {"fp32": torch.float32, "bf16": torch.bfloat16}[name.split("_")[1]]
    sizes = [(CROP // s, CROP // s) for s in STRIDES]
    A = 3
    coder = MidpointOffsetCoder(target_stds=(1.0, 1.0, 1.0, 1.0, 0.5, 0.5))
    levels, anchors = AnchorGenerator(strides=STRIDES, ratios=(0.5, 1.0, 2.0), scales=(8,)).grid_anchors(sizes, dev)
    gen = torch.Generator(device=dev).manual_seed(1234 + B)
    scale = torch.tensor([0.01, 0.01, 0.03, 0.03, 0.15, 0.15], device=dev).repeat(A).view(1, 6 * A, 1, 1)
    mean = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.8, 0.8], device=dev).repeat(A).view(1, 6 * A, 1, 1)
    cls = [(2 * torch.randn(B, A, h, w, device=dev, generator=gen)).to(dtype).contiguous(memory_format=torch.channels_last) for h, w in sizes]
    reg = [(torch.randn(B, 6 * A, h, w, device=dev, generator=gen) * scale + mean).to(dtype).contiguous(memory_format=torch.channels_last) for h, w in sizes]
    f = RPNProposalBuffers(sizes, A, B, NMS_PRE, MAX_NUM, dev)

    def select():
        return ops.rpn_select(cls, reg, anchors, coder.means, coder.stds, NMS_PRE, 0.0, index=f.index, groups=f.groups, scores=f.cand_scores, boxes=f.boxes,
                              order=f.order, workspace=f.workspace)

    def native():
        return rpn_proposals(cls, reg, anchors, coder, NMS_PRE, MAX_NUM, NMS_THR, 0, buffers=f)

    def native_alloc():
        return rpn_proposals(cls, reg, anchors, coder, NMS_PRE, MAX_NUM, NMS_THR, 0)

    def stock():
        return rpn_proposals_torch(cls, reg, levels, coder, NMS_PRE, MAX_NUM, NMS_THR, 0)
    title = f"--- B = {B}, {name.split('_')[1]} channels-last maps: {sum(h * w * A for h, w in sizes)} anchors per image, Ktot = {f.Ktot}, nms_pre = max_num = {NMS_PRE}"
    compare(title + ": the select launches alone", [("native: ops.rpn_select, outputs and workspace supplied (3 launches + 1 memset node)", select)], calls, rounds)
    out, ref = native(), stock()
    num = out.num.tolist()
    exact = close = 0
    for b in range(B):
        mine, theirs = out.proposals[b, :num[b]], ref[b][:, :5]
        d = (theirs[:, None, :] - mine[None, :, :]).abs().amax(2)
        exact += int((d.amin(1) == 0).sum())
        close += int((d.amin(1) <= 1e-3).sum())
    # the whole stage: the stock side's window has a length of its own (the module docstring)
    from dense_loss_probe import timed
    timed(native, 3); timed(stock, 1)
    t = {"native": [], "stock": []}
    for _ in range(rounds):
        t["native"].append(timed(native, calls))
        t["stock"].append(timed(stock, stock_calls))
    say(title + ": the whole stage")
    labels = {"native": f"native: rpn_proposals, buffers supplied (a memset and {4 + 2 * B} launches, no synchronisation), windows of {calls} calls",
              "stock": f"stock PyTorch: rpn_proposals_torch ({B} host copies of the suppression mask), windows of {stock_calls} calls"}
    med = {}
    for k in ("native", "stock"):
        v = sorted(x * 1e3 for x in t[k])
        med[k] = v[rounds // 2]
        say(f"  {labels[k]:110s} {med[k]:12.3f} us   spread {v[-1] - v[0]:.3f}   {['%.3f' % (x * 1e3) for x in t[k]]}")
    say(f"  stock / native: {med['stock'] / med['native']:.1f} x")
    say(f"  proposals per image: native {num}, stock {[int(r.shape[0]) for r in ref]}; of the stock side's {sum(int(r.shape[0]) for r in ref)} boxes the native side has "
        f"{exact} bit for bit and {close} within 1e-3")
    bufs = [f.index, f.groups, f.cand_scores, f.boxes, f.order, f.workspace, f.nms_workspace, f.keep, f.count, f.proposals, f.scores, f.num, f.ignore]
    say(f"  peak allocation above the inputs: native with supplied buffers {peak_above(native)} bytes (buffers and workspaces: "
        f"{sum(v.numel() * v.element_size() for v in bufs)} bytes, allocated once; the NMS words: {f.nms_workspace.numel()}), native allocating "
        f"{peak_above(native_alloc)} bytes, stock {peak_above(stock)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stock-calls", type=int, default=20, help="calls per window of the stock side of the whole stage")
    ap.add_argument("--limit", type=int, default=400, help="seconds per GPU step")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_probe.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one shape")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("proposal_probe: needs an MI355X (no CPU fallback)")
        step(a.step, a.calls, a.rounds, a.stock_calls)
        return
    lines = [f"proposal_probe: medians of {a.rounds} windows of {a.calls} calls (the stock side of the whole stage: windows of {a.stock_calls} calls); one process per "
             f"shape, {a.limit} s each"]
    print(lines[0], flush=True)
    status = 0
    for name in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls), "--rounds", str(a.rounds), "--stock-calls", str(a.stock_calls)]
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
