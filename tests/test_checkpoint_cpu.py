"""Activation checkpointing: the interface (use_checkpoint_stages, timm's set_grad_checkpointing).  No GPU needed: the flags live on the host
modules; tests/test_checkpoint_gpu.py checks what they do."""
import pytest

import lemevit_amd as L
from lemevit_amd.model import LeMeViTBackbone

TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)


def _block_flags(m):
    return [[blk.grad_checkpointing for blk in stage] for stage in m.stages]


def test_default_is_off():
    m = L.create_model("lemevit_tiny", num_classes=10)
    assert m.use_checkpoint_stages == [] and not m.grad_checkpointing
    assert not any(f for st in _block_flags(m) for f in st)


def test_create_model_records_stages():
    m = L.create_model("lemevit_tiny", num_classes=10, use_checkpoint_stages=[1, 3])
    assert m.use_checkpoint_stages == [1, 3]
    assert m.grad_checkpointing                     # a non-empty list also checkpoints the stem and every transition
    assert _block_flags(m) == [[i in (1, 3)] * d for i, d in enumerate([1, 2, 2, 8, 2])]
    # the option is host state only: the state_dict keys are those of the unchecked model (checkpoints load either way)
    assert list(m.state_dict()) == list(L.create_model("lemevit_tiny", num_classes=10).state_dict())


def test_set_grad_checkpointing_toggles():
    m = L.create_model("lemevit_tiny", num_classes=10)
    m.set_grad_checkpointing()
    assert m.use_checkpoint_stages == [0, 1, 2, 3, 4] and m.grad_checkpointing
    assert all(f for st in _block_flags(m) for f in st)
    m.set_grad_checkpointing(False)
    assert m.use_checkpoint_stages == [] and not m.grad_checkpointing
    assert not any(f for st in _block_flags(m) for f in st)
    m.set_grad_checkpointing(True)
    assert all(f for st in _block_flags(m) for f in st)


@pytest.mark.parametrize("bad", [[5], [0, 7], [-1]])
def test_out_of_range_stage_raises(bad):
    with pytest.raises(ValueError, match="use_checkpoint_stages"):
        L.create_model("lemevit_tiny", num_classes=10, use_checkpoint_stages=bad)
    with pytest.raises(ValueError, match="use_checkpoint_stages"):
        L.LeMeViT(**TINY, use_checkpoint_stages=bad)
    with pytest.raises(ValueError, match="use_checkpoint_stages"):
        LeMeViTBackbone(**TINY, use_checkpoint_stages=bad)


def test_integer_like_indices_accepted():
    import numpy as np
    import torch
    m = L.create_model("lemevit_tiny", num_classes=10, use_checkpoint_stages=[np.int64(1), torch.tensor(3)])
    assert m.use_checkpoint_stages == [1, 3] and all(type(i) is int for i in m.use_checkpoint_stages)
    for bad in ([1.0], [True], ["1"]):
        with pytest.raises(ValueError, match="use_checkpoint_stages"):
            L.create_model("lemevit_tiny", num_classes=10, use_checkpoint_stages=bad)


def test_backbone_honours_the_option():
    b = LeMeViTBackbone(**TINY, use_checkpoint_stages=[0, 1, 2, 3, 4])
    assert b.use_checkpoint_stages == [0, 1, 2, 3, 4] and b.grad_checkpointing
    assert all(f for st in _block_flags(b) for f in st)
    b.set_grad_checkpointing(False)
    assert not b.grad_checkpointing and not any(f for st in _block_flags(b) for f in st)
