#!/usr/bin/env python3
"""Golden fixtures for the image gradient and for in_chans != 3, from the REFERENCE implementation (see gen_golden.py: same stand-ins,
same deterministic weights and inputs; the fixtures hold expected outputs only).

    python tests/golden/gen_input_grad_golden.py            # writes the five .npz files named below
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_tensor, sample  # noqa: E402
from gen_golden import REG, _import_reference, _load, _save  # noqa: E402

TARGET4 = [1, 7, 3, 3]          # train_tiny_96's targets
FIRST = "downsample_layers.0.0.weight"


def _stats(m):
    return {"stat." + k: v.numpy() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def gen_inputgrad():
    """train_tiny_96's model, image and targets with an image that requires grad: train mode (cross-entropy) and eval mode (sum of the target columns of the logits)."""
    torch.manual_seed(0)
    m = REG["lemevit_tiny"](num_classes=10, drop_path_rate=0.0)
    _load(m, "", 41)
    m.train()
    img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5).requires_grad_(True)
    target = torch.tensor(TARGET4)
    loss = nn.functional.cross_entropy(m(img), target)
    loss.backward()
    _save("inputgrad_tiny_96", dict(kind="inputgrad", variant="lemevit_tiny", res=96, B=4, num_classes=10, seed=41, in_chans=3, target=TARGET4, img="train_tiny_96.img", img_seed=5),
          {"dimg": img.grad.numpy(), "loss": np.float32(loss.item()), "grad." + FIRST: dict(m.named_parameters())[FIRST].grad.numpy()})

    m = REG["lemevit_tiny"](num_classes=10, drop_path_rate=0.0)
    _load(m, "", 41)
    m.eval()
    img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5).requires_grad_(True)
    logits = m(img)
    logits[:, target].sum().backward()
    _save("inputgrad_tiny_96_eval", dict(kind="inputgrad_eval", variant="lemevit_tiny", res=96, B=4, num_classes=10, seed=41, in_chans=3, target=TARGET4, img="train_tiny_96.img",
                                         img_seed=5, objective="logits[:, target].sum()"),
          dict(logits=logits.detach().numpy(), dimg=img.grad.numpy()))


def gen_in_chans():
    for name, cin in [("train_tiny_c4_96", 4), ("train_tiny_c13_96", 13)]:
        torch.manual_seed(0)
        m = REG["lemevit_tiny"](num_classes=10, in_chans=cin, drop_path_rate=0.0)
        _load(m, "", 41)
        m.train()
        img = det_tensor((2, cin, 96, 96), name + ".img", 5).requires_grad_(True)
        target = torch.tensor([1, 7])
        logits = m(img)
        loss = nn.functional.cross_entropy(logits, target)
        loss.backward()
        names = [k for k, _ in m.named_parameters()]
        full = img.grad.numel() * 4 <= 500_000
        arr = {"logits": logits.detach().numpy(), "loss": np.float32(loss.item()),
               "grad_norms": np.asarray([float(p.grad.norm()) if p.grad is not None else 0.0 for _, p in m.named_parameters()], dtype=np.float32),
               "grad." + FIRST: dict(m.named_parameters())[FIRST].grad.numpy(), "dimg": img.grad.numpy() if full else sample(img.grad, 16384)}
        arr.update(_stats(m))
        _save(name, dict(kind="train", variant="lemevit_tiny", res=96, B=2, num_classes=10, seed=41, in_chans=cin, drop_path_rate=0.0, target=[1, 7], param_names=names,
                         dimg_sampled=0 if full else 16384), arr)

    name = "model_tiny_c1_224"
    torch.manual_seed(0)
    m = REG["lemevit_tiny"](num_classes=1000, in_chans=1).eval()
    _load(m, "", 31)
    img = det_tensor((1, 1, 224, 224), name + ".img", 4)
    with torch.no_grad():
        logits = m(img)
    _save(name, dict(kind="model", variant="lemevit_tiny", res=224, B=1, num_classes=1000, seed=31, in_chans=1), dict(logits=logits.numpy()))


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    ref = _import_reference()
    assert ref.has_torchfunc and not ref.has_flash_attn and not ref.has_xformers
    gen_inputgrad()
    gen_in_chans()


if __name__ == "__main__":
    main()
