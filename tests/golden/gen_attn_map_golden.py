#!/usr/bin/env python3
"""Golden fixtures for the attention maps, from the REFERENCE implementation (see gen_golden.py: same stand-ins, same deterministic weights and
inputs; the fixtures hold expected outputs only).

The reference routes every attention through torch.nn.functional.scaled_dot_product_attention (models/lemevit.py:203,297,300,402,405,484), which
never returns the probabilities.  For the duration of a run that function is wrapped with the explicit softmax of the reference's own slow path
(:54-63), which records P; an unwrapped run must give the same output to 1e-6, so the wrapper has not changed the model.

    python tests/golden/gen_attn_map_golden.py            # writes attnmap_tiny_96.npz and attnmap_dense_tiny_160x96.npz

Arrays: `mean.<n>` the head-mean map [B, Lq, Lk] of attention call n (call order = forward order; meta["calls"][n] = [block, field, Lq, Lk]),
`heads.<n>` the per-head map [B, h, Lq, Lk] of the calls of meta["per_head_blocks"], `bf16_dev` / `bf16_dev_heads.<n>` the max-abs deviation,
relative to the map's max-abs, of the reference's maps under CPU torch.autocast(bfloat16) from its fp32 maps, and the model outputs."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_tensor, sample  # noqa: E402
from gen_golden import REG, _import_dense_reference, _import_reference, _load, _save  # noqa: E402

FP32_TOL = 1e-5                 # the tolerance the fp32 tests hold the maps to (of each map's max-abs)
PER_HEAD = ["stages.0.0", "stages.1.0", "stages.3.0"]          # one block of each kind
FIELDS = {"C": ["meta_from_image"], "D": ["image_from_meta", "meta_from_image"], "S": ["image_self", "meta_self"], "Sx": ["image_self"]}


def call_names(depth, attn_type, dense=False):
    """[(block name, field)] of the attention calls in forward order."""
    out = []
    for i, (n, t) in enumerate(zip(depth, attn_type)):
        kind = "Sx" if (dense and t == "S") else t
        for j in range(n):
            out += [(f"stages.{i}.{j}", f) for f in FIELDS[kind]]
    return out


def record(fn):
    """fn() with scaled_dot_product_attention wrapped by the recording explicit softmax: (fn's value, [P per call, fp32])."""
    log = []
    real = F.scaled_dot_product_attention

    def recording(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None):
        assert attn_mask is None and dropout_p == 0.0 and not is_causal
        s = scale if scale is not None else q.shape[-1] ** (-0.5)
        attn = (q @ k.transpose(-2, -1)) * s
        attn = attn.softmax(dim=-1)
        log.append(attn.detach().float())
        return attn @ v

    F.scaled_dot_product_attention = recording
    try:
        with torch.no_grad():
            out = fn()
    finally:
        F.scaled_dot_product_attention = real
    return out, log


def rel_dev(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def build(name, model, img, calls, meta, outputs):
    with torch.no_grad():
        plain = model(img)
    out, maps = record(lambda: model(img))
    for a, b in zip(outputs(out), outputs(plain)):
        assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max())), "the recording wrapper changed the model"
    assert len(maps) == len(calls), (len(maps), len(calls))
    with torch.autocast("cpu", torch.bfloat16):
        _, maps16 = record(lambda: model(img))
    arr, dev, worst = {}, [], None
    for n, ((blk, field), p) in enumerate(zip(calls, maps)):
        Lk = p.shape[-1]
        for q in (p, p.mean(1)):          # per head and head-mean: both must tell the right answer from the uniform map
            gap = float((q - 1.0 / Lk).abs().max())
            assert gap >= 100 * FP32_TOL * float(q.abs().max()), (n, blk, field, gap)
            worst = gap if worst is None else min(worst, gap)
        arr[f"mean.{n}"] = p.mean(1).numpy()
        dev.append(rel_dev(maps16[n].mean(1), p.mean(1)))
        if blk in meta["per_head_blocks"]:
            arr[f"heads.{n}"] = p.numpy()
            arr[f"bf16_dev_heads.{n}"] = np.float32(rel_dev(maps16[n], p))
    arr["bf16_dev"] = np.asarray(dev, dtype=np.float32)
    for k, v in arr.items():
        assert np.asarray(v).nbytes <= (1 << 20), (k, "apply detfill.sample to this array")
    arr.update({f"out{i}": (o.numpy() if o.numel() <= 16384 else sample(o.flatten(2).transpose(1, 2), 8192)) for i, o in enumerate(outputs(out))})
    meta = dict(meta, calls=[[b, f, int(p.shape[-2]), int(p.shape[-1])] for (b, f), p in zip(calls, maps)], min_gap_from_uniform=worst)
    print(f"{name}: {len(maps)} calls, smallest max|P - 1/Lk| {worst:.2e}, bf16_dev max {max(dev):.2e}")
    _save(name, meta, arr)


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    ref = _import_reference()
    assert ref.has_torchfunc and not ref.has_flash_attn and not ref.has_xformers

    torch.manual_seed(0)
    m = REG["lemevit_tiny"](num_classes=10)
    _load(m, "", 41)
    m.eval()
    img = det_tensor((2, 3, 96, 96), "train_tiny_96.img", 5)
    build("attnmap_tiny_96", m, img, call_names([1, 2, 2, 8, 2], ["C", "D", "D", "S", "S"]),
          dict(kind="attnmap", variant="lemevit_tiny", res=96, B=2, num_classes=10, seed=41, img="train_tiny_96.img", img_seed=5, per_head_blocks=PER_HEAD),
          lambda o: [o])

    refd = _import_dense_reference()
    tiny = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4],
                attn_type=["C", "D", "D", "S", "S"], queries_len=16)
    torch.manual_seed(0)
    m = refd.LeMeViT(**tiny)
    m.eval()
    _load(m, "", 51)
    img = det_tensor((2, 3, 160, 96), "dense_tiny_160x96.img", 6)
    build("attnmap_dense_tiny_160x96", m, img, call_names(tiny["depth"], tiny["attn_type"], dense=True),
          dict(kind="attnmap_dense", cfg=tiny, H=160, W=96, B=2, seed=51, img="dense_tiny_160x96.img", img_seed=6, per_head_blocks=[]),
          lambda o: list(o))


if __name__ == "__main__":
    main()
