"""Host side of the per-group / scheduled learning rates (lmv_adamw_flat_groups, include/lemevit_hip.h; optim.layer_ids; FlatAdamW(layer_decay= / lr_scale= /
device_lr=)) without a GPU: the argument checks run before any launch, the layer ids are pure host code, and the constructor validates before it touches a device."""
import ctypes
import os

import pytest
import torch

ERR_SHAPE = -1
FAKE = 1 << 20          # a 16-byte aligned address that is never dereferenced: every call below is refused before a launch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refused(rc, word):
    from lemevit_amd._lib import lib
    msg = lib.lmv_last_error()
    assert rc == ERR_SHAPE and word in msg, (rc, msg)


def _call(param=FAKE, grad=FAKE, m=FAKE, v=FAKE, shadow=None, n=16, units=FAKE, groups=FAKE, ngroups=3, step=1, step_dev=None, stat=None, clip=0.0):
    from lemevit_amd._lib import lib
    return lib.lmv_adamw_flat_groups(param, grad, m, v, shadow, n, units, groups, ngroups, 0.9, 0.999, 1e-8, step, step_dev, stat, clip, None)


def test_adamw_flat_groups_rejects_bad_arguments_before_any_launch():
    from lemevit_amd import _lib
    _refused(_call(n=12), b"multiple of 8")
    _refused(_call(n=4), b"multiple of 8")
    _refused(_call(ngroups=0), b"ngroups")
    _refused(_call(ngroups=257), b"ngroups")
    _refused(_call(ngroups=-1), b"ngroups")
    for name in ("param", "grad", "m", "v", "units", "groups"):
        _refused(_call(**{name: None}), b"null or misaligned")
    for name in ("param", "grad", "m", "v"):
        _refused(_call(**{name: FAKE + 8}), b"null or misaligned")          # the fp32 buffers: 16 bytes
    _refused(_call(groups=FAKE + 4), b"null or misaligned")                 # the table: 8 bytes
    _refused(_call(shadow=FAKE + 4), b"null or misaligned")
    _refused(_call(stat=FAKE + 2), b"null or misaligned")
    _refused(_call(step=0), b"step")
    _refused(_call(step=-3), b"step")
    _refused(_call(clip=-1.0), b"clip_value")
    _refused(_call(clip=float("nan")), b"clip_value")
    assert _call(n=0) == 0                                                   # nothing to do is not an error, as for lmv_adamw_flat
    assert ctypes.sizeof(_lib.AdamWGroup) == 8
    hdr = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    assert "#define LMV_ADAMW_UNIT 8\n" in hdr and "#define LMV_ADAMW_MAX_GROUPS 256\n" in hdr
    assert (_lib.ADAMW_UNIT, _lib.ADAMW_MAX_GROUPS) == (8, 256)
    from lemevit_amd import optim
    assert optim._ALIGN == _lib.ADAMW_UNIT, "FlatAdamW aligns every slice to one group byte's worth of elements"


def _build(kind):
    import lemevit_amd
    if kind == "backbone":
        cfg = dict(depth=[1, 2, 1, 2, 1], embed_dim=[64, 64, 128, 192, 320], head_dim=32, attn_type=["C", "D", "D", "S", "S"], queries_len=16)
        return lemevit_amd.LeMeViTBackbone(**cfg), 7
    return lemevit_amd.create_model(kind, num_classes=10), {"lemevit_tiny": 15, "lemevit_base": 32}[kind]


@pytest.mark.parametrize("kind", ["lemevit_tiny", "lemevit_base", "backbone"])
def test_layer_ids(kind):
    from lemevit_amd import optim
    from lemevit_amd.model import LeMeBlock
    model, L = _build(kind)
    assert sum(isinstance(m, LeMeBlock) for m in model.modules()) == L
    ids = optim.layer_ids(model)
    names = [n for n, _ in model.named_parameters()]
    assert set(ids) == set(names) and all(isinstance(i, int) and 0 <= i <= L + 1 for i in ids.values())
    assert set(ids.values()) == set(range(L + 2))                          # ids 0 .. L + 1, every one of them used
    # the k-th block in forward order has id k + 1: ids do not decrease along a stage's blocks, nor from one stage to the next
    block_of = {}
    for n in names:
        if n.startswith("stages."):
            s, k = n.split(".")[1:3]
            block_of.setdefault((int(s), int(k)), set()).add(ids[n])
    assert all(len(v) == 1 for v in block_of.values()), "one id per block"
    order = [next(iter(block_of[key])) for key in sorted(block_of)]
    assert order == list(range(1, L + 1))
    for n in names:
        if n.startswith(("head.", "norm.", "norm_c.", "extra_norms.")):
            assert ids[n] == L + 1, n
        if n == "meta_tokens" or n.startswith(("downsample_layers.0.", "meta_token_downsample.0.")):
            assert ids[n] == 0, n
    if kind != "backbone":
        assert any(n.startswith("head.") for n in names) and any(n.startswith("norm_c.") for n in names)
    else:
        assert any(n.startswith("extra_norms.") for n in names) and not any(n.startswith("head.") for n in names)
    for s in range(1, 5):
        first = next(iter(block_of[(s, 0)]))
        for pre in (f"downsample_layers.{s}.", f"meta_token_downsample.{s}."):
            assert all(ids[n] == first for n in names if n.startswith(pre)), pre
    assert any(n.startswith("downsample_layers.2.") for n in names) and ids["downsample_layers.2.0.weight"] == ids["stages.2.0.norm1.weight"]
    # the scale timm's rule gives: decay ** (L + 1 - id) -- 1 for the head, the smallest for the stem
    decay = 0.75
    scales = {n: decay ** (L + 1 - i) for n, i in ids.items()}
    assert scales["meta_tokens"] == decay ** (L + 1) == min(scales.values())
    assert max(scales.values()) == 1.0 and all(scales[n] == 1.0 for n in names if n.startswith("norm."))
    assert scales["stages.0.0.norm1.weight"] == decay ** L


def test_layer_ids_with_a_wrapper_prefix_and_unknown_names():
    from lemevit_amd import optim
    model, L = _build("lemevit_tiny")
    wrapped = torch.nn.Sequential()
    wrapped.add_module("module", model)
    wrapped.add_module("extra", torch.nn.Linear(2, 2))
    ids = optim.layer_ids(wrapped)
    bare = optim.layer_ids(model)
    assert all(ids["module." + n] == i for n, i in bare.items())
    assert ids["extra.weight"] == L + 1


def test_constructor_validates_before_anything_needs_a_gpu():
    import lemevit_amd
    m = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        lemevit_amd.FlatAdamW(m, layer_decay=0.75, lr_scale=lambda n, p: 1.0)
    for bad in (0, 0.0, 1.5, -0.5, float("nan")):
        with pytest.raises(ValueError, match="layer_decay"):
            lemevit_amd.FlatAdamW(m, layer_decay=bad)
    # valid options pass the validation and reach the same refusal as without them: no LeMeBlock parameters on a GPU
    for kw in (dict(layer_decay=1.0), dict(lr_scale=lambda n, p: 2.0), dict(device_lr=True)):
        with pytest.raises(ValueError, match="no fp32 LeMeBlock parameters"):
            lemevit_amd.FlatAdamW(m, **kw)


def test_ops_adamw_flat_groups_refuses_cpu_tensors_and_wrong_dtypes():
    from lemevit_amd import ops
    t = torch.zeros(16)
    units = torch.zeros(2, dtype=torch.uint8)
    groups = torch.zeros(3, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.adamw_flat_groups(t, t, t, t, units, groups, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="group_of_unit"):
        ops.adamw_flat_groups(t, t, t, t, units.to(torch.int32), groups, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="group_of_unit"):
        ops.adamw_flat_groups(t, t, t, t, torch.zeros(3, dtype=torch.uint8), groups, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="groups"):
        ops.adamw_flat_groups(t, t, t, t, units, groups.double(), 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="groups"):
        ops.adamw_flat_groups(t, t, t, t, units, torch.zeros(6), 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="groups"):
        ops.adamw_flat_groups(t, t, t, t, units, torch.zeros(257, 2), 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.adamw_flat_groups(t.double(), t, t, t, units, groups, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="length"):
        ops.adamw_flat_groups(t, t[:8], t, t, units, groups, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(TypeError, match="shadow"):
        ops.adamw_flat_groups(t, t, t, t, units, groups, 0.9, 0.999, 1e-8, 1, shadow=torch.zeros(16))
    with pytest.raises(TypeError, match="step_dev"):
        ops.adamw_flat_groups(t, t, t, t, units, groups, 0.9, 0.999, 1e-8, 0, step_dev=torch.zeros((), dtype=torch.int64))
    with pytest.raises(TypeError, match="stat"):
        ops.adamw_flat_groups(t, t, t, t, units, groups, 0.9, 0.999, 1e-8, 1, stat=torch.zeros(4))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.adamw_flat_groups(t[:12], t[:12], t[:12], t[:12], units[:1], groups, 0.9, 0.999, 1e-8, 1)


def test_graphed_step_takes_before_replay():
    import inspect
    from lemevit_amd.graph import GraphedStep, try_graphed
    assert inspect.signature(GraphedStep.__init__).parameters["before_replay"].default is None
    assert inspect.signature(try_graphed).parameters["before_replay"].default is None
