#!/usr/bin/env python3
"""Golden fixture for the dense-prediction losses, from the REFERENCE implementation: change_detection/utils/metrics.py is loaded by path, unmodified (it imports
only torch); nothing of it is copied.  The fixture holds expected outputs only -- the reference's ``FocalLoss`` (gamma = 0, and gamma = 2 with ``alpha``),
``dice_loss`` and ``jaccard_loss`` and their autograd gradients with respect to the logits, in float64 and float32 -- the logits and label maps are regenerated
from ``detfill.py`` by ``dense_case`` (which the tests import).

    python tests/golden/gen_dense_loss_golden.py            # writes dense_loss.npz
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detfill import det_tensor, det_uniform  # noqa: E402

REF = "/root/reference/change_detection/utils/metrics.py"
SHAPES = [(2, 2, 6, 10), (1, 3, 5, 7), (2, 5, 4, 4)]
ALPHA = {2: [0.25, 0.75], 3: [0.2, 0.3, 0.5], 5: [0.1, 0.15, 0.2, 0.25, 0.3]}
GAMMA = 2


def case_name(shape) -> str:
    return "x".join(str(s) for s in shape)


def dense_case(shape):
    """(logits float64 [B, K, H, W] with values exactly representable in float32, labels int64 [B, 1, H, W] in [0, K)) of a case"""
    B, K, H, W = shape
    name = case_name(shape)
    logits = det_tensor(shape, "dense_loss." + name, 7, 4.0, 0.0, torch.float64)          # (a power of two: the values stay float32 numbers)
    u = det_uniform(B * H * W, 0x5EED + K * 131 + H * W)
    labels = torch.from_numpy(np.minimum(((u + 1.0) * 0.5 * K).astype(np.int64), K - 1)).reshape(B, 1, H, W)
    return logits, labels


def _reference():
    spec = importlib.util.spec_from_file_location("cd_reference_metrics", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = _reference()
    arrays, cases = {}, []
    for shape in SHAPES:
        K = shape[1]
        logits64, labels = dense_case(shape)
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            fns = {"focal0": lambda x: ref.FocalLoss(gamma=0, alpha=None)(x, labels),
                   "focal2": lambda x: ref.FocalLoss(gamma=GAMMA, alpha=list(ALPHA[K]))(x, labels),
                   "dice": lambda x: ref.dice_loss(x, labels),
                   "jaccard": lambda x: ref.jaccard_loss(x, labels)}
            for fname, fn in fns.items():
                x = logits64.to(dt).clone().requires_grad_(True)
                loss = fn(x)
                loss.backward()
                key = f"{case_name(shape)}.{tag}.{fname}"
                arrays[key] = loss.detach().numpy()
                arrays[key + ".grad"] = x.grad.numpy()
        cases.append(dict(shape=list(shape), alpha=ALPHA[K]))
    meta = dict(kind="dense_loss", source="change_detection/utils/metrics.py", cases=cases, gamma=GAMMA, eps=1e-7, losses=["focal0", "focal2", "dice", "jaccard"])
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "dense_loss.npz")
    np.savez_compressed(path, **arrays)
    print(f"dense_loss {os.path.getsize(path) / 1024:8.1f} KiB")


if __name__ == "__main__":
    main()
