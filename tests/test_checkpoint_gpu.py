"""Activation checkpointing (use_checkpoint_stages / set_grad_checkpointing) on the MI355X.

The promise: a checkpointed train step is bit-identical to the same step without checkpointing -- loss, every gradient, the BatchNorm running
statistics and the parameters after FlatAdamW steps (bf16 autocast; fp32 wherever the unchecked fp32 step reproduces itself, see
test_checkpointed_step_is_bit_identical) -- while the saved set between forward and backward shrinks by the block arenas of the checkpointed stages.  The memory test is also the proof that the recompute path ran in the bit-identity tests (same
configurations)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict
from test_model_gpu import DEV

import lemevit_amd.model as M
from lemevit_amd import _lib, ops
from lemevit_amd.model import LeMeViT, LeMeViTBackbone
from lemevit_amd.optim import FlatAdamW

TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
BASE2 = dict(TINY, depth=[2, 2, 2, 2, 2], embed_dim=[96, 96, 192, 384, 512])        # LeMeViT-Base widths, two blocks per stage
# (config, batch): Tiny at B = 64 runs the training forward as image ranges (model.TRAIN_PARTS_MIN_BATCH); so does Base2 at B = 32
MODELS = {"tiny-b64": (TINY, 64), "base2-b32": (BASE2, 32)}
LISTS = {"none": [], "1,3": [1, 3], "all": [0, 1, 2, 3, 4]}
LR = 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# lmv_batchnorm_apply_fwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("gelu", [False, True], ids=["id", "gelu"])
@pytest.mark.parametrize("C", [48, 96, 192])
@pytest.mark.parametrize("rows", [1155, 50177])
def test_batchnorm_apply_matches_train_forward(dtype, gelu, C, rows):
    """The apply entry point, from the statistics lmv_batchnorm_train_fwd returned, writes that call's y bit for bit (row counts that are not
    multiples of the workgroup's row tile) and leaves the running statistics alone."""
    x = (det_tensor((rows, C), f"ckpt.bn.{rows}.{C}", 11) * 3.0 + 0.5).to(DEV, dtype)
    g = (1.0 + 0.2 * det_tensor((C,), f"ckpt.bn.g.{C}", 11)).to(DEV)
    b = (0.1 * det_tensor((C,), f"ckpt.bn.b.{C}", 11)).to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, stats = ops.batchnorm_train_fwd(x, g, b, rm, rv, 0.1, 1e-5, gelu)
    rm0, rv0 = rm.clone(), rv.clone()
    assert not torch.equal(rm0, torch.zeros_like(rm0))          # (the training forward did move them)
    ya = ops.batchnorm_apply_fwd(x, g, b, stats, gelu)
    torch.cuda.synchronize()
    assert ya.dtype == dtype and ya.shape == y.shape
    assert torch.equal(ya, y)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bit-identity of a train step
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _model(cfg, ck, seed=5):
    m = LeMeViT(**cfg, num_classes=10, drop_path_rate=0.1, use_checkpoint_stages=ck)
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m.to(DEV).train()


def _bn_state(m):
    return {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


def _step(m, img, tgt, bf16, seed):
    torch.manual_seed(seed)                         # the DropPath draw of the pass
    with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
        loss = F.cross_entropy(m(img), tgt)
    loss.backward()
    return loss.detach()


def _run(cfg, B, ck, bf16):
    m = _model(cfg, ck)
    img = det_tensor((B, 3, 224, 224), f"ckpt.img.{B}", 12).to(DEV)
    tgt = torch.arange(B, device=DEV) % 10
    loss = _step(m, img, tgt, bf16, 100)
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    bn = _bn_state(m)
    m.zero_grad(set_to_none=True)
    # in-place flat gradients of the block parameters, deferred side-stream joins.  fp32: eps = 1 (see test_checkpointed_step_is_bit_identical)
    opt = FlatAdamW(m, lr=LR, eps=1e-8 if bf16 else 1.0)
    for s in range(2):
        opt.zero_grad()
        _step(m, img, tgt, bf16, 200 + s)
        opt.step()
    torch.cuda.synchronize()
    params = {n: p.detach().clone() for n, p in m.named_parameters()}
    return loss, grads, bn, params, _bn_state(m)


def _same(a, b, spread=None, ulps=0):
    """Names whose tensors differ.  spread (fp32): a second unchecked run.  Where that run is bit-equal to the first, the checkpointed run must be
    too, up to `ulps` units in the last place of the tensor's scale; where it is not, the checkpointed run may differ by 8 x as much, plus those
    `ulps` -- but no more."""
    bad = []
    for n, t in a.items():
        if torch.equal(t, b[n]):
            continue
        if spread is not None:
            r = b[n].float()
            slack = ulps * torch.finfo(torch.float32).eps * float(r.abs().max())
            if float((t.float() - r).abs().max()) <= 8 * float((spread[n].float() - r).abs().max()) + slack:
                continue
        bad.append(n)
    return bad


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("model", list(MODELS))
def test_checkpointed_step_is_bit_identical(model, bf16):
    """bf16 autocast: everything torch.equal.  fp32: the loss and the first step's BatchNorm state torch.equal; a gradient torch.equal wherever two
    unchecked fp32 steps are bit-equal to each other, and within 8 x their difference where they are not.  (The unchecked fp32 step is not
    bit-reproducible from run to run in stages 0 - 2 -- the fp32 attention backward accumulates with atomics: gradients there move at ~1e-6
    relative, and the biases of the convolutions in front of a training-mode BatchNorm, whose exact gradient is 0, are rounding noise.  With
    AdamW's eps = 1e-8 those noise-level gradients become updates of +-lr, so the fp32 optimizer steps run with eps = 1, where an update is
    ~lr * g and the noise stays at rounding level: parameters and BatchNorm statistics after the steps then follow the same rule, plus 8 / 64
    units in the last place for values that crossed a rounding boundary in one run and not in the other.)"""
    cfg, B = MODELS[model]
    ref = _run(cfg, B, [], bf16)
    spread = None if bf16 else _run(cfg, B, [], bf16)
    if spread is not None:
        assert torch.equal(spread[0], ref[0]) and not _same(spread[2], ref[2])
    for name, ck in LISTS.items():
        if not ck:
            continue
        loss, grads, bn, params, bn2 = _run(cfg, B, ck, bf16)
        assert torch.equal(loss, ref[0]), f"{name}: loss {float(loss)} vs {float(ref[0])}"
        bad = _same(bn, ref[2])
        assert not bad, f"{name}: BatchNorm state differs after one step: {bad[:8]}"
        bad = _same(grads, ref[1], None if spread is None else spread[1])
        assert not bad, f"{name}: gradients differ: {bad[:8]}"
        bad = _same(params, ref[3], None if spread is None else spread[3], ulps=8)
        assert not bad, f"{name}: parameters differ after two FlatAdamW steps: {bad[:8]}"
        bad = _same(bn2, ref[4], None if spread is None else spread[4], ulps=64)
        assert not bad, f"{name}: BatchNorm state differs after three steps: {bad[:8]}"
    assert all(int(v) == 3 for k, v in ref[4].items() if "num_batches" in k)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# memory
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _arena_bytes(m, B, dtype):
    """lmv_block_arena_bytes of every block of a 224^2 pass (the library's own sizes)."""
    out, H = [], 56
    for i, stage in enumerate(m.stages):
        if i > 0 and m.attn_type[i - 1] != "C":
            H = (H + 1) // 2
        for blk in stage:
            d = _lib.BlockDesc()
            d.kind, d.dtype = {"S": 0, "D": 1, "C": 2}[blk.kind], ops.dtype_code(torch.empty(0, dtype=dtype))
            d.B, d.H, d.W, d.M, d.C, d.hidden, d.eps = B, H, H, 16, m.embed_dim[i], blk.mlp[0].out_features, 1e-6
            n = int(_lib.lib.lmv_block_arena_bytes(d))
            assert n > 0
            out.append(n)
    return out


def _measure(m, img, tgt):
    """(bytes allocated between the end of the forward and the start of the backward, peak during the backward), after one warm-up step."""
    for it in range(2):
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.manual_seed(7)
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(m(img), tgt)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del loss
    return held, peak


@pytest.mark.parametrize("model", list(MODELS))
def test_checkpointing_frees_the_block_arenas(model):
    cfg, B = MODELS[model]
    img = det_tensor((B, 3, 224, 224), f"ckpt.img.{B}", 12).to(DEV)
    tgt = torch.arange(B, device=DEV) % 10
    m = _model(cfg, [])
    held0, peak0 = _measure(m, img, tgt)
    sizes = _arena_bytes(m, B, torch.bfloat16)
    del m
    m = _model(cfg, [0, 1, 2, 3, 4])
    held1, peak1 = _measure(m, img, tgt)
    bound = 0.9 * (sum(sizes) - max(sizes))          # the reused forward arena keeps the largest one
    print(f"{model}: held {held0 / 2**20:.0f} -> {held1 / 2**20:.0f} MiB (saved {(held0 - held1) / 2**20:.0f}, bound {bound / 2**20:.0f}), "
          f"backward peak {peak0 / 2**20:.0f} -> {peak1 / 2**20:.0f} MiB")
    assert held0 - held1 >= bound
    assert peak1 < peak0


def _downsample_saved_bytes(m, B, es):
    """What the unchecked stem and transitions keep for the backward pass at 224^2, at the least (implicit-GEMM convolutions): the stem's patch
    matrix [B * 112^2, 32], its first BatchNorm's input and GELU output [B * 112^2, C0 / 2], its second BatchNorm's input [B * 56^2, C0] and
    each transition's BatchNorm input [B * H_i^2, C_i]."""
    n = B * 112 * 112 * (32 + 2 * (m.embed_dim[0] // 2)) + B * 56 * 56 * m.embed_dim[0]
    H = 56
    for i in range(1, m.num_stages):
        if m.attn_type[i - 1] != "C":
            H = (H + 1) // 2
            n += B * H * H * m.embed_dim[i]
    return n * es


class _Counters:
    """Calls of the checkpointed-downsample recompute and of lmv_batchnorm_apply_fwd (through ops) during a test."""

    def __init__(self, monkeypatch):
        self.recompute = self.apply = 0
        mods, apply = M._downsample_mods, ops.batchnorm_apply_fwd

        def mods_counted(mods_, x, cd, fold, ck=None):
            if ck is not None and ck["recompute"]:
                self.recompute += 1
            return mods(mods_, x, cd, fold, ck)

        def apply_counted(*a, **k):
            self.apply += 1
            return apply(*a, **k)

        monkeypatch.setattr(M, "_downsample_mods", mods_counted)
        monkeypatch.setattr(ops, "batchnorm_apply_fwd", apply_counted)


@pytest.mark.parametrize("ck", [[], [1, 3], [0, 1, 2, 3, 4]], ids=["none", "1,3", "all"])
def test_downsample_recomputed_in_backward(ck, monkeypatch):
    """A non-empty list checkpoints the stem and the three transitions: one recompute each in the backward pass, every training-mode BatchNorm
    rebuilt from its saved statistics with lmv_batchnorm_apply_fwd -- and the running statistics move once per step, in the forward pass."""
    cnt = _Counters(monkeypatch)
    m = _model(TINY, ck)
    bns = [mod for seq in m.downsample_layers for mod in seq.modules() if isinstance(mod, torch.nn.BatchNorm2d)]
    assert len(bns) == 5
    nbt0 = [int(b.num_batches_tracked) for b in bns]
    img = det_tensor((64, 3, 224, 224), "ckpt.img.64", 12).to(DEV)
    tgt = torch.arange(64, device=DEV) % 10
    with torch.autocast("cuda", torch.bfloat16):
        loss = F.cross_entropy(m(img), tgt)
    assert cnt.recompute == 0 and cnt.apply == 0
    loss.backward()
    torch.cuda.synchronize()
    assert (cnt.recompute, cnt.apply) == ((4, 5) if ck else (0, 0))
    assert [int(b.num_batches_tracked) - n for b, n in zip(bns, nbt0)] == [1] * 5


@pytest.mark.parametrize("model", list(MODELS))
def test_checkpointing_frees_the_downsample_saved_set(model):
    """The stem and the transitions on their own: ONE model (no operand copies of another model's parameters in either measurement), blocks
    checkpointed in both runs, the downsample layers in the second."""
    cfg, B = MODELS[model]
    img = det_tensor((B, 3, 224, 224), f"ckpt.img.{B}", 12).to(DEV)
    tgt = torch.arange(B, device=DEV) % 10
    m = _model(cfg, [0, 1, 2, 3, 4])
    m.grad_checkpointing = False                     # (the model-level switch of the stem and the transitions)
    held0, _ = _measure(m, img, tgt)
    bound = 0.9 * _downsample_saved_bytes(m, B, 2)
    m.grad_checkpointing = True
    held1, _ = _measure(m, img, tgt)
    print(f"{model}: stem + transitions checkpointed: held {held0 / 2**20:.0f} -> {held1 / 2**20:.0f} MiB (saved {(held0 - held1) / 2**20:.0f}, "
          f"bound {bound / 2**20:.0f})")
    assert held0 - held1 >= bound


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dense backbone at a detection size
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _backbone_run(ck, frozen=(-1,), cnt=None):
    m = LeMeViTBackbone(**TINY, use_checkpoint_stages=ck, frozen_stages=list(frozen))
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 3))
    m = m.to(DEV).train()
    img = det_tensor((2, 3, 800, 1344), "ckpt.dense.img", 6).to(DEV)
    with torch.autocast("cuda", torch.bfloat16):
        outs = m(img)
    gs = [det_tensor(tuple(o.shape), f"ckpt.dense.g{i}", 6).to(DEV, o.dtype) for i, o in enumerate(outs)]
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    r0 = None if cnt is None else cnt.recompute
    sum((o.float() * g.float()).sum() for o, g in zip(outs, gs)).backward()
    torch.cuda.synchronize()
    if cnt is not None:          # stem + three transitions recomputed; their BatchNorms are in eval mode: no apply-from-statistics
        assert (cnt.recompute - r0, cnt.apply) == ((4, 0) if ck else (0, 0))
    return [o.detach().clone() for o in outs], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, held


@pytest.mark.parametrize("frozen", [(-1,), (0,)], ids=["all-trained", "frozen0"])
def test_dense_backbone_checkpointed_bit_identical(frozen, monkeypatch):
    """LeMeViTBackbone at 1344 x 800, B = 2, bf16, train mode (its BatchNorms stay in eval mode: the recompute repeats their eval call)."""
    cnt = _Counters(monkeypatch)
    o0, g0, h0 = _backbone_run([], frozen, cnt)
    o1, g1, h1 = _backbone_run([0, 1, 2, 3, 4], frozen, cnt)
    assert len(o0) == 4 and all(torch.equal(a, b) for a, b in zip(o0, o1))
    assert set(g0) == set(g1) and g0
    bad = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not bad, f"gradients differ: {bad[:8]}"
    if frozen == (0,):
        assert not any(n.startswith("stages.0.") for n in g1)
    print(f"dense 1344x800 B=2 frozen={frozen}: held {h0 / 2**20:.0f} -> {h1 / 2**20:.0f} MiB")
    assert h1 < h0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inference is untouched
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_eval_forward_unchanged(bf16):
    """An eval forward without autograd of a checkpointed model (the persistent stage kernels in bf16) gives the unchecked model's logits."""
    img = det_tensor((8, 3, 224, 224), "ckpt.eval.img", 13).to(DEV)
    outs = []
    for ck in ([], [0, 1, 2, 3, 4]):
        m = _model(TINY, ck).eval()
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16, enabled=bf16):
            outs.append(m(img).clone())
    assert torch.equal(outs[0], outs[1])
