"""Two trees of the Python package on ONE build of the library, bit for bit, on the stem and the stage transitions (GPU box): every output, gradient and BatchNorm
statistic of LeMeViT._run_downsample over both convolution geometries, every operand source and every saved-set variation, plus whole-model train steps.

    python tools/downsample_ab.py TREE_A TREE_B [--timeout 600] [--out profiles/NAME.txt]

TREE_A is the reference side (e.g. ``git archive PARENT lemevit_amd | tar -x -C DIR``), TREE_B the tree under test.  Run order: A, A again, B -- each a FRESH child
process (this process never opens the GPU), one after the other, each under its own time limit; a child that fails ends the run before the next one starts.  Every
child puts its tree first on sys.path, asserts that the package came from there, and loads the SAME library (``LMV_LIB_PATH``, default the build of the tree this file
lives in: the kernel sources of the two trees are meant to be identical).  A child writes one line per case with a digest of the bytes of y, dx, every parameter
gradient (None recorded as such) and every BatchNorm's running statistics and num_batches_tracked afterwards.

A case COUNTS where A's two runs agree with each other; on those B must equal A.  Every bf16 case must count (the bf16 gradients are stated to reproduce from run to
run): one that does not is reported by name and fails the run, as does any differing digest.  fp32 cases outside the counted set are listed.

Cases.  Models: a reduced lemevit_tiny classifier and the reduced LeMeViTBackbone (depth [1, 1, 1, 2, 1]) with in_chans 3, 4, 13 (image form) and 8 (the first
convolution takes the map form), state from detfill.fill_state_dict.  Layers: the stem on 2 x in_chans x 50 x 38 (second convolution: patch-matrix form) and on
64 x in_chans x 20 x 12 (960 rows: implicit form); each transition on 2 x C x 9 x 7 and 64 x C x 9 x 7.  Modes: eval under no_grad (inference fold, one-launch stem),
train() of the classifier (training BatchNorm), train() of the backbone (frozen BatchNorm), the eval classifier with every parameter frozen.  Each with checkpointing
off / on, bf16 autocast / fp32, the input requiring grad or not.  Whole models (bf16, checkpointing off / on): a Tiny-backbone train step at 2 x 3 x 96 x 160 and a
lemevit_tiny train step at 4 x 3 x 96 x 96."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
REDUCED = dict(TINY, depth=[1, 1, 1, 2, 1], drop_path_rate=0.0)
MODES = ("eval_nograd", "train_classifier", "train_backbone", "eval_frozen")
DEV = "cuda:0"


def digest(t):
    import torch
    if t is None:
        return "None"
    t = t.detach().contiguous()
    return hashlib.blake2b((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().tobytes(), digest_size=12).hexdigest()


def child(path, tree):
    sys.path[:0] = [tree, os.path.join(ROOT, "tests", "golden")]
    import torch
    import torch.nn.functional as F
    import lemevit_amd
    import lemevit_amd.model as M
    from detfill import det_tensor, fill_state_dict
    assert os.path.dirname(os.path.dirname(os.path.abspath(lemevit_amd.__file__))) == os.path.abspath(tree), lemevit_amd.__file__

    def build(cls, seed, **kw):
        m = cls(**kw)
        sd = {k: v.to(DEV) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed).items()}
        return m.to(DEV), sd

    def state(mod):
        out = []
        for n, b in mod.named_modules():
            if isinstance(b, torch.nn.BatchNorm2d):
                out += [(f"{n}.running_mean", b.running_mean), (f"{n}.running_var", b.running_var), (f"{n}.num_batches_tracked", b.num_batches_tracked)]
        return out

    def line(f, name, items):
        f.write(name + "\t" + " ".join(f"{k}={digest(v)}" for k, v in items) + "\n")

    def layer_case(f, name, m, sd, seq, mode, shape, bf16, xg):
        m.load_state_dict(sd)
        m.train(mode.startswith("train")).requires_grad_(mode != "eval_frozen")
        m.zero_grad(set_to_none=True)
        x = det_tensor(shape, name + ".x", 5).to(DEV).requires_grad_(xg)
        M.new_training_pass()
        with torch.set_grad_enabled(mode != "eval_nograd"), torch.autocast("cuda", torch.bfloat16, enabled=bf16):
            y = m._run_downsample(seq, x)
        if y.requires_grad:
            y.backward(det_tensor(tuple(y.shape), name + ".dy", 5).to(DEV).to(y.dtype))
        line(f, name, [("y", y), ("dx", x.grad)] + [("d." + n, p.grad) for n, p in seq.named_parameters()] + state(seq))

    def model_case(f, name, m, sd, img, loss):
        m.load_state_dict(sd)
        m.train()
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.bfloat16):
            out = m(img)
            val = loss(out)
        val.backward()
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        line(f, name, [(f"y{i}", o) for i, o in enumerate(outs)] + [("loss", val)] + [("d." + n, p.grad) for n, p in m.named_parameters()] + state(m))

    with open(path, "w") as f:
        for cin in (3, 4, 13, 8):
            models = {"classifier": build(M.LeMeViT, 41, num_classes=10, in_chans=cin, **REDUCED), "backbone": build(M.LeMeViTBackbone, 3, in_chans=cin, **REDUCED)}
            for mode in MODES:
                m, sd = models["backbone" if mode == "train_backbone" else "classifier"]
                layers = [(i, seq) for i, seq in enumerate(m.downsample_layers) if isinstance(seq, torch.nn.Sequential)]
                for i, seq in layers:
                    if i > 0 and cin != 3:
                        continue          # (the transitions do not see in_chans)
                    C = seq[0].in_channels
                    for shape in ([(2, C, 50, 38), (64, C, 20, 12)] if i == 0 else [(2, C, 9, 7), (64, C, 9, 7)]):
                        for ck in (False, True):
                            m.set_grad_checkpointing(ck)
                            for bf16 in (True, False):
                                for xg in (False, True):
                                    name = f"{'bf16' if bf16 else 'fp32'} in_chans={cin} layer{i} {'x'.join(map(str, shape))} {mode} ckpt={int(ck)} xgrad={int(xg)}"
                                    layer_case(f, name, m, sd, seq, mode, shape, bf16, xg)
            del models
        tgt = torch.tensor([1, 7, 3, 3], device=DEV)
        for ck in (False, True):
            m, sd = build(M.LeMeViTBackbone, 3, **TINY)
            m.set_grad_checkpointing(ck)
            model_case(f, f"bf16 model backbone_tiny 2x3x96x160 train ckpt={int(ck)}", m, sd, det_tensor((2, 3, 96, 160), "ab.dense.img", 6).to(DEV),
                       lambda outs: sum((o.float() ** 2).mean() for o in outs))
            m, sd = build(lemevit_amd.create_model, 41, model_name="lemevit_tiny", num_classes=10, drop_path_rate=0.0)
            m.set_grad_checkpointing(ck)
            model_case(f, f"bf16 model lemevit_tiny 4x3x96x96 train ckpt={int(ck)}", m, sd, det_tensor((4, 3, 96, 96), "ab.cls.img", 5).to(DEV),
                       lambda logits: F.cross_entropy(logits, tgt))
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trees", nargs="*")
    ap.add_argument("--child", help="(internal) write the digests of the tree --tree to this file")
    ap.add_argument("--tree")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--out", help="also write the report here")
    a = ap.parse_args()
    if a.child:
        return child(a.child, os.path.abspath(a.tree))
    if len(a.trees) != 2:
        ap.error("two trees expected")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    env = dict(os.environ)
    env.setdefault("LMV_LIB_PATH", os.path.join(ROOT, "lemevit_amd", "csrc", "liblemevit_hip.so"))
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, (side, tree) in enumerate((("A", a.trees[0]), ("A again", a.trees[0]), ("B", a.trees[1]))):
            out = os.path.join(tmp, f"{k}.txt")
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, "--tree", os.path.abspath(tree)], env=env, timeout=a.timeout).returncode
            if rc != 0:
                raise SystemExit(f"downsample_ab: the child of tree {side} ended with status {rc}; nothing more is run")
            runs.append({name: dict(kv.split("=") for kv in rest.split()) for name, rest in (ln.rstrip("\n").split("\t") for ln in open(out))})
    A, A2, B = runs
    counted = [n for n in A if A2.get(n) == A[n]]
    uncounted = [n for n in A if A2.get(n) != A[n]]
    say(f"downsample_ab: {len(A)} cases; A = the first tree (run twice), B = the second; one library for both")
    differ = len(set(A) ^ set(B))
    for n in set(A) ^ set(B):
        say(f"{n}: missing from one tree")
    for n in counted:
        if n in B:
            bad = [k for k in A[n] if A[n][k] != B[n].get(k)] + [k for k in B[n] if k not in A[n]]
            differ += len(bad)
            if bad:
                say(f"{n}: DIFFER: " + ", ".join(bad))
    bad16 = [n for n in uncounted if n.startswith("bf16")]
    for n in uncounted:
        say(f"{n}: A does not reproduce itself ({', '.join(k for k in A[n] if A[n][k] != A2.get(n, {}).get(k))}): " + ("a bf16 case, FAILS the run" if n in bad16 else "fp32, not counted"))
    say(f"cases {len(A)}, counted {len(counted)} (bf16 {sum(n.startswith('bf16') for n in counted)} of {sum(n.startswith('bf16') for n in A)}), "
        f"not counted {len(uncounted)}, differing digests on counted cases: {differ}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if differ == 0 and not bad16 else 1


if __name__ == "__main__":
    sys.exit(main())
