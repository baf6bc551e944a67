#!/usr/bin/env python3
"""Golden fixture for training through frozen BatchNorm, from the REFERENCE implementation (see gen_golden.py: same stand-ins, same deterministic
weights and inputs; the fixture holds expected outputs only).

    python tests/golden/gen_frozen_bn_golden.py            # writes frozenbn_tiny_96.npz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_tensor  # noqa: E402
from gen_golden import REG, _import_reference, _load, _save  # noqa: E402

TARGET4 = [1, 7, 3, 3]          # train_tiny_96's targets
FIRST = "downsample_layers.0.0.weight"


def gen_frozen_bn():
    """train_tiny_96's model, image and targets in EVAL mode (every BatchNorm on its running statistics) under autograd: cross-entropy, the gradient of every
    BatchNorm weight / bias and of the first stem convolution's weight, the gradient norm of every parameter."""
    torch.manual_seed(0)
    m = REG["lemevit_tiny"](num_classes=10, drop_path_rate=0.0)
    _load(m, "", 41)
    m.eval()
    img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5)
    logits = m(img)
    loss = nn.functional.cross_entropy(logits, torch.tensor(TARGET4))
    loss.backward()
    bn = [k for name, mod in m.named_modules() if isinstance(mod, nn.BatchNorm2d) for k in (name + ".weight", name + ".bias")]
    params = dict(m.named_parameters())
    names = list(params)
    arr = {"logits": logits.detach().numpy(), "loss": np.float32(loss.item()),
           "grad_norms": np.asarray([float(p.grad.norm()) if p.grad is not None else 0.0 for p in params.values()], dtype=np.float32)}
    for k in bn + [FIRST]:
        arr["grad." + k] = params[k].grad.numpy()
    _save("frozenbn_tiny_96", dict(kind="frozen_bn", variant="lemevit_tiny", res=96, B=4, num_classes=10, seed=41, in_chans=3, target=TARGET4, img="train_tiny_96.img", img_seed=5,
                                   drop_path_rate=0.0, mode="eval", bn_params=bn, param_names=names), arr)


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    ref = _import_reference()
    assert ref.has_torchfunc and not ref.has_flash_attn and not ref.has_xformers
    gen_frozen_bn()


if __name__ == "__main__":
    main()
