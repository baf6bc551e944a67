"""The samplers (csrc/sampler.hip) against what a user of the package writes today: upstream's per-image tensor code in stock PyTorch (``random_sample_torch``:
``add_gt_``'s ``cat``, two ``nonzero`` -- each a host synchronisation --, ``randperm`` over the candidates of an oversubscribed class, an index copy, ``unique``) (GPU box).

    python tools/sampler_probe.py [--calls 20] [--rounds 5] [--limit 300] [--out profiles/sampler_probe.txt]

Shapes of the Oriented R-CNN configs on a 1024 x 1024 crop, two images:
    rpn          RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False) over 261 888 anchors, about 100 positive, a third ignored
    rcnn_40      OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True) over 2 000 proposals plus Gmax = 40 ground truths (30 and 40 valid)
    rcnn_200     the same with Gmax = 200 (150 and 200 valid)
Every shape is one GPU step: a child process of its own under a time limit of --limit seconds (a step that fails or runs out ends the probe: nothing more is started),
in which both sides alternate -- windows of --calls calls between device events, --rounds windows per side; median and spread (max - min) reported, with the launches
of the native side, the tensor-producing operator calls of the stock side (a dispatch mode counts every ATen call whose result is not a view of an input; each is
at least one launch) and each side's peak allocation above the inputs.  The two sides draw differently: they are compared on the counts and on the class of every
chosen element.  There is no parent-commit number: the operator is new.  Whichever side is slower at a shape is reported as measured."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ["rpn", "rcnn_40", "rcnn_200"]


def peak_above(fn) -> int:
    """bytes the caching allocator holds at the peak of fn() above what was allocated before it"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def step(name, calls, rounds):
    import numpy as np
    import torch
    from coder_probe import count_ops
    from dense_loss_probe import compare, say
    import gen_sampler_cases as gen
    from lemevit_amd import ops
    from lemevit_amd.detection import OBBRandomSampler, RandomSampler, random_sample_torch
    dev = "cuda"
    B = 2
    if name == "rpn":
        N, Gmax, counts = 261888, 0, None
        sampler = RandomSampler(num=256, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False, seed=0)
        g = np.stack([gen.mix(N, 100 + 7 * b, N * 2 // 3, 5 + b, 40) for b in range(B)])
        title = f"--- rpn: {B} images x {N} anchors, {[int((x > 0).sum()) for x in g]} positive, num = 256"
    else:
        N, Gmax = 2000, int(name.split("_")[1])
        counts = [Gmax * 3 // 4, Gmax]
        sampler = OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True, seed=0)
        g = np.stack([np.minimum(gen.mix(N, 300, 1500, 5 + b, counts[b]), counts[b]) for b in range(B)])
        title = f"--- {name}: {B} images x ({Gmax} ground truths, {counts} valid + {N} proposals), 300 positive proposals, num = 512"
    gt_inds = torch.from_numpy(g).to(dev)
    cd = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)
    M = (Gmax if sampler.add_gt_as_proposals else 0) + N
    bufs = dict(inds=torch.empty(B, sampler.num, dtype=torch.int64, device=dev), num_pos=torch.empty(B, dtype=torch.int32, device=dev),
                num_neg=torch.empty(B, dtype=torch.int32, device=dev), mask=torch.empty(B, M, dtype=torch.uint8, device=dev),
                workspace=torch.empty(ops.random_sample_workspace_bytes(B, M), dtype=torch.uint8, device=dev))
    sampler.sample_batched(gt_inds, cd, Gmax)          # (allocates the key)

    def native():
        return sampler.sample_batched(gt_inds, cd, Gmax, **bufs)

    def native_alloc():
        return sampler.sample_batched(gt_inds, cd, Gmax)

    def stock():
        return [random_sample_torch(gt_inds[b], sampler.num, sampler.pos_fraction, sampler.neg_pos_ub, sampler.add_gt_as_proposals, 0 if counts is None else counts[b])
                for b in range(B)]
    s, t = native(), stock()
    ok = True
    for b in range(B):          # counts and class membership (the stock side's element space has only the VALID ground truths in front)
        valid = 0 if counts is None else counts[b]
        off = Gmax if sampler.add_gt_as_proposals else 0
        p, n = int(s.num_pos[b]), int(s.num_neg[b])
        ok &= p == t[b][0].numel() and n == t[b][1].numel()
        mine_pos, mine_neg = s.inds[b, :p], s.inds[b, p:p + n]
        ok &= bool(((mine_pos < valid) | ((mine_pos >= off) & (gt_inds[b][(mine_pos - off).clamp(min=0)] > 0))).all()) and bool((gt_inds[b][mine_neg - off] == 0).all())
        theirs = torch.cat([torch.ones(valid, dtype=torch.int64, device=dev), gt_inds[b]])
        ok &= bool((theirs[t[b][0]] > 0).all()) and bool((theirs[t[b][1]] == 0).all())
    sides = [("native: csrc/sampler.hip, caller-supplied outputs and workspace (2 launches + 1 memset node, no synchronisation)", native),
             (f"stock PyTorch: upstream's per-image tensor code ({count_ops(stock)} tensor-producing operator calls, {2 * B} nonzero synchronisations)", stock)]
    compare(title, sides, calls, rounds)
    say(f"  counts per image (positives, negatives): native {[(int(s.num_pos[b]), int(s.num_neg[b])) for b in range(B)]}, stock {[(x.numel(), y.numel()) for x, y in t]}; "
        f"counts and classes of the chosen agree: {ok}")
    say(f"  peak allocation above the inputs: native with supplied buffers {peak_above(native)} bytes (buffers and workspace: "
        f"{sum(v.numel() * v.element_size() for v in bufs.values())} bytes, allocated once), native allocating {peak_above(native_alloc)} bytes, stock {peak_above(stock)} bytes")
    if not ok:
        raise SystemExit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_probe.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one shape")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sampler_probe: needs an MI355X (no CPU fallback)")
        step(a.step, a.calls, a.rounds)
        return
    lines = [f"sampler_probe: medians of {a.rounds} windows of {a.calls} calls; one process per shape, {a.limit} s each"]
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
