"""What frozen parameters are worth: the data-only block backward (LMV_BLOCK_DATA_ONLY) against another build of the library, e.g. the parent commit, and
the fused dX kernel of the MLP half (lmv_mlp_dx_fused) against the two-launch form (GPU box).

    python tools/frozen_params_probe.py --one                       # this tree: one JSON line per case
    python tools/frozen_params_probe.py --against OTHER_TREE        # this tree and OTHER_TREE (a built checkout) alternately, three repeats each -> profiles/frozen_params_probe.txt

Cases (bf16 autocast, warmed up, every timed window at least --window seconds of steps between device events; peak allocation of one step each):
1. the eval-mode image-gradient step of lemevit_base at 224 x 224, B = 128, model.requires_grad_(False) (saliency / FGSM / PGD);
2. a training step of lemevit_base at 224 x 224, B = 128, with the stem and stages 0 - 2 frozen (partial fine-tuning);
3. a training step of the Tiny dense backbone at 1344 x 800, B = 2, frozen_stages = [0, 1];
4. (this tree only) per width C = 96 / 192 / 384 at Base's row counts for B = 128: lmv_mlp_dx_fused against lmv_linear_fwd(.., LMV_ACT_GELU_GRAD) + the fc1 dX.
Every run is a process of its own (--one), so neither tree sees the other's module state or caches.  The report starts with the run-to-run spread (the OTHER tree's
own spread over its repeats is the comparison margin; for the kernels, the spread of the two-launch form)."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
KERNEL_SHAPES = [(96, 128 * 3136, 128 * 16), (192, 128 * 784, 128 * 16), (384, 128 * 196, 128 * 16)]          # (C, image rows, meta rows) of Base stages 1 - 3 at B = 128


def _timed(torch, step, window):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); step(); b.record(); b.synchronize()
    n = max(3, int(window / max(a.elapsed_time(b) * 1e-3, 1e-5)) + 1)
    times = []
    for _ in range(3):
        a.record()
        for _ in range(n):
            step()
        b.record(); b.synchronize()
        times.append(a.elapsed_time(b) / n)
    return dict(ms=sorted(times)[1], windows_ms=times, steps_per_window=n, peak_mb=peak / 1e6)


def one(tree, window):
    sys.path.insert(0, tree)
    import torch
    import lemevit_amd
    from lemevit_amd import ops
    from lemevit_amd.model import LeMeViTBackbone
    assert os.path.dirname(os.path.dirname(os.path.abspath(lemevit_amd.__file__))) == os.path.abspath(tree)
    dev = "cuda"

    def saliency():
        torch.manual_seed(0)
        m = lemevit_amd.create_model("lemevit_base", num_classes=1000).to(dev).eval().requires_grad_(False)
        x = torch.randn(128, 3, 224, 224, device=dev)
        t = torch.randint(0, 1000, (128,), device=dev)

        def step():
            xi = x.detach().requires_grad_(True)
            with torch.autocast("cuda", torch.bfloat16):
                logits = m(xi)
            logits.float().gather(1, t[:, None]).sum().backward()
        return step

    def finetune():
        torch.manual_seed(0)
        m = lemevit_amd.create_model("lemevit_base", num_classes=1000).to(dev).train()
        m.downsample_layers[0].requires_grad_(False)
        for i in range(3):
            m.stages[i].requires_grad_(False)
        x = torch.randn(128, 3, 224, 224, device=dev)
        t = torch.randint(0, 1000, (128,), device=dev)

        def step():
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(m(x), t)
            loss.backward()
        return step

    def dense():
        torch.manual_seed(0)
        m = LeMeViTBackbone(**TINY, frozen_stages=[0, 1]).to(dev).train()
        x = torch.randn(2, 3, 800, 1344, device=dev)

        def step():
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.bfloat16):
                outs = m(x)
            sum(o.float().mean() for o in outs).backward()
        return step

    for name, make in [("saliency_base_224_b128", saliency), ("finetune_base_224_b128_stem_s012_frozen", finetune), ("dense_tiny_1344x800_b2_s01_frozen", dense)]:
        step = make()
        print(json.dumps(dict(case=name, **_timed(torch, step, window))), flush=True)
        del step
        torch.cuda.empty_cache()

    if not hasattr(ops, "mlp_dx_fused"):
        return
    from lemevit_amd.ops import ACT_GELU_GRAD, Prob
    for C, r0, r1 in KERNEL_SHAPES:
        Hd = 4 * C
        torch.manual_seed(C)
        bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
        fc2_wt, fc1_wt = bf(Hd, C) * Hd ** -0.5, bf(C, Hd) * C ** -0.5
        gs, us = [bf(r0, C), bf(r1, C)], [bf(r0, Hd), bf(r1, Hd)]
        du, dn = [torch.empty_like(u) for u in us], [torch.empty_like(g) for g in gs]

        def two():
            ops.linear_fwd([Prob(g, fc2_wt, o, aux=u) for g, o, u in zip(gs, du, us)], Hd, C, ACT_GELU_GRAD)
            ops.linear_fwd([Prob(d, fc1_wt, o) for d, o in zip(du, dn)], C, Hd)

        def fused():
            ops.mlp_dx_fused(gs, us, fc2_wt, fc1_wt)
        for name, fn in (("two_launch", two), ("fused", fused)):
            print(json.dumps(dict(case=f"mlp_dx_C{C}_rows{r0 + r1}_{name}", **_timed(torch, fn, window / 4))), flush=True)
        del gs, us, du, dn
        torch.cuda.empty_cache()


def against(other, window, out):
    runs = {"this": [], "other": []}
    for r in range(3):
        for side, tree in (("other", other), ("this", ROOT)):
            t0 = time.time()
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--tree", tree, "--window", str(window)], stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"{side} run {r} failed with code {p.returncode}")          # (nothing more is started on the GPU)
            runs[side].append({d["case"]: d for d in map(json.loads, filter(None, p.stdout.splitlines()))})
            print(f"# {side} repeat {r}: {time.time() - t0:.0f} s", flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["frozen_params_probe: this tree against %s, bf16, 3 alternating repeats (each the median of 3 windows of >= %.1f s)" % (os.path.basename(other), window),
             "run-to-run spread (max - min over the repeats), the margin of every comparison below:"]
    shared = [c for c in runs["this"][0] if c in runs["other"][0]]
    for c in shared:
        o = [r[c]["ms"] for r in runs["other"]]; t = [r[c]["ms"] for r in runs["this"]]
        lines.append(f"  {c:42s} other {max(o) - min(o):.3f} ms   this {max(t) - min(t):.3f} ms")
    kern = [c for c in runs["this"][0] if c.startswith("mlp_dx_")]
    for c in kern:
        t = [r[c]["ms"] for r in runs["this"]]
        lines.append(f"  {c:42s} this {max(t) - min(t):.4f} ms")
    lines.append("steps:")
    for c in shared:
        t = [r[c]["ms"] for r in runs["this"]]; o = [r[c]["ms"] for r in runs["other"]]
        tm, om, spread = med(t), med(o), max(o) - min(o)
        verdict = "faster" if tm < om - spread else ("not slower" if tm <= om + spread else "SLOWER")
        a, b = runs["this"][0][c], runs["other"][0][c]
        lines.append(f"  {c:42s} this {tm:8.3f} ms {['%.3f' % v for v in t]}   other {om:8.3f} ms {['%.3f' % v for v in o]}   {100 * (tm / om - 1):+.2f} %  {verdict}"
                     f"   peak {a['peak_mb']:.0f} vs {b['peak_mb']:.0f} MB")
    lines.append("lmv_mlp_dx_fused against the two-launch dX (this tree; mlp_dx_fused = 1 selects the fused kernel only where it wins by more than the spread):")
    for c in kern:
        if not c.endswith("_fused"):
            continue
        two = c[:-len("fused")] + "two_launch"
        f = [r[c]["ms"] for r in runs["this"]]; w = [r[two]["ms"] for r in runs["this"]]
        fm, wm, spread = med(f), med(w), max(max(w) - min(w), max(f) - min(f))
        verdict = "fused faster" if fm < wm - spread else ("within the spread" if fm <= wm + spread else "two-launch faster")
        lines.append(f"  {c[:-6]:34s} fused {fm:7.4f} ms {['%.4f' % v for v in f]}   two-launch {wm:7.4f} ms {['%.4f' % v for v in w]}   {100 * (fm / wm - 1):+.1f} %  {verdict}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--against")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_params_probe.txt"))
    a = ap.parse_args()
    if a.against:
        against(os.path.abspath(a.against), a.window, a.out)
    else:
        one(os.path.abspath(a.tree), a.window)


if __name__ == "__main__":
    main()
