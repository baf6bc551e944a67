"""What training through frozen BatchNorm costs: the paths of LMV_FROZEN_BN against another build of the library, e.g. the parent commit (GPU box).

    python tools/frozen_bn_probe.py --one                       # this tree: one JSON line per configuration
    python tools/frozen_bn_probe.py --against OTHER_TREE        # this tree and OTHER_TREE (a built checkout) alternately, three repeats each -> profiles/frozen_bn_probe.txt

Configurations (bf16 autocast, warmed up, every timed window at least --window seconds of steps between device events):
1. dense train step (forward + backward of LeMeViTBackbone.train(), every norm layer frozen), Base at 1024 x 1024, B = 2;
2. the same for Tiny at 1344 x 800, B = 2;
3. the eval-mode image-gradient step of lemevit_base at 224 x 224, B = 128 (parameters frozen, the image requires grad: saliency / FGSM).
Per configuration also the peak allocation of a step and the number of kernels one step launches (torch.profiler; "n/a" where the profiler is unavailable).
Every run is a process of its own (--one), so neither tree sees the other's module state or caches; the comparison margin is the OTHER tree's own spread over
its repeats."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = dict(depth=[2, 4, 4, 18, 4], embed_dim=[96, 96, 192, 384, 512], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)


def one(tree, window):
    sys.path.insert(0, tree)
    import torch
    import lemevit_amd
    from lemevit_amd.model import LeMeViTBackbone
    assert os.path.dirname(os.path.dirname(os.path.abspath(lemevit_amd.__file__))) == os.path.abspath(tree)
    dev = "cuda"

    def dense(cfg, H, W):
        torch.manual_seed(0)
        m = LeMeViTBackbone(**cfg).to(dev).train()
        x = torch.randn(2, 3, H, W, device=dev)

        def step():
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", torch.bfloat16):
                outs = m(x)
            sum(o.float().mean() for o in outs).backward()
        return step

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
            return xi.grad
        return step

    for name, make in [("dense_base_1024_b2", lambda: dense(BASE, 1024, 1024)), ("dense_tiny_1344x800_b2", lambda: dense(TINY, 800, 1344)), ("saliency_base_224_b128", saliency)]:
        step = make()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); step(); b.record(); b.synchronize()
        n = max(3, int(window / max(a.elapsed_time(b) * 1e-3, 1e-4)) + 1)
        times = []
        for _ in range(3):
            a.record()
            for _ in range(n):
                step()
            b.record(); b.synchronize()
            times.append(a.elapsed_time(b) / n)
        kernels = None
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        except Exception as e:          # noqa: BLE001  (a missing tracer is reported, not fatal)
            kernels = None
            print(f"# profiler unavailable: {type(e).__name__}", file=sys.stderr)
        print(json.dumps(dict(config=name, ms=sorted(times)[1], windows_ms=times, steps_per_window=n, peak_mb=peak / 1e6, kernels=kernels)), flush=True)
        del step
        torch.cuda.empty_cache()


def against(other, window, out):
    runs = {"this": [], "other": []}
    for r in range(3):
        for side, tree in (("other", other), ("this", ROOT)):
            t0 = time.time()
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--tree", tree, "--window", str(window)], stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"{side} run {r} failed with code {p.returncode}")          # (nothing more is started on the GPU)
            runs[side].append({d["config"]: d for d in map(json.loads, filter(None, p.stdout.splitlines()))})
            print(f"# {side} repeat {r}: {time.time() - t0:.0f} s", flush=True)
    lines = ["frozen_bn_probe: this tree (LMV_FROZEN_BN default) against %s, bf16, 3 alternating repeats (each the median of 3 windows of >= %.1f s)" % (other, window)]
    for cfg in runs["this"][0]:
        t = [r[cfg]["ms"] for r in runs["this"]]
        o = [r[cfg]["ms"] for r in runs["other"]]
        tm, om, spread = sorted(t)[1], sorted(o)[1], max(o) - min(o)
        verdict = "not slower" if tm <= om + spread else "SLOWER"
        a, b = runs["this"][0][cfg], runs["other"][0][cfg]
        lines.append(f"{cfg:26s} this {tm:8.3f} ms {['%.3f' % v for v in t]}   other {om:8.3f} ms {['%.3f' % v for v in o]} (spread {spread:.3f})   {100 * (tm / om - 1):+.2f} %  {verdict}"
                     f"   peak {a['peak_mb']:.0f} vs {b['peak_mb']:.0f} MB   kernels per step {a['kernels'] if a['kernels'] is not None else 'n/a'} vs "
                     f"{b['kernels'] if b['kernels'] is not None else 'n/a'}")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_probe.txt"))
    a = ap.parse_args()
    if a.against:
        against(os.path.abspath(a.against), a.window, a.out)
    else:
        one(os.path.abspath(a.tree), a.window)


if __name__ == "__main__":
    main()
