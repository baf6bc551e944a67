"""Derived operands (model.derived) through the model on a real MI355X: they follow re-homed parameters, assign=True loads and
optimizers, go with their model, and stay put across steady-state passes.  tests/test_derived_cpu.py checks the rule itself."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict

DEV = "cuda:0"


def _model(seed, sd=None):
    import lemevit_amd
    m = lemevit_amd.create_model("lemevit_tiny", num_classes=10)
    if sd is None:
        sd = fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict(sd)
    return m.to(DEV)


def _eval(m, img):
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        y = m(img).float()
    torch.cuda.synchronize()
    return y


def _fresh_eval(m, img):
    """The logits of a new instance loaded with m's current values (every derived operand built from scratch)."""
    f = _model(0, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    y = _eval(f, img)
    assert torch.equal(_eval(f, img), y)
    return y


def test_rehomed_parameters_are_followed():
    """p.data = t swaps a parameter's storage without bumping its version; a no-grad eval pass does not start a training pass.  The next eval
    pass must still read the new values: the persistent stage's pack, the per-block LayerNorm folds, the meta-token MLP's bf16 weights and its
    cached output, the stem, the conv + BatchNorm folds and the classifier tail."""
    import lemevit_amd.model as M
    m = _model(7)
    img = det_tensor((2, 3, 224, 224), "rehome.img", 3).to(DEV)
    y0 = _eval(m, img)
    assert torch.equal(_eval(m, img), y0)
    assert (id(m.stages[3]), ("stage", "S")) in M._derived, "stage 3 did not run as a persistent launch"
    targets = [("stage-3 block matrix", m.stages[3][0].attn.qkv.weight), ("stage-4 block LayerNorm", m.stages[4][0].norm1.weight),
               ("meta-token MLP", m.meta_token_downsample[0][0].weight), ("stem conv", m.downsample_layers[0][0].weight),
               ("BatchNorm running_var", m.downsample_layers[2][1].running_var), ("head", m.head.weight)]
    for what, p in targets:
        p.data = (p.detach() * 1.25).clone()
        y = _eval(m, img)
        assert not torch.equal(y, y0), what
        ref = _fresh_eval(m, img)
        assert torch.equal(y, ref), f"{what}: stale operand, {float((y - ref).abs().max()):.3e} off a fresh instance"
        y0 = y


def test_assign_load_is_followed():
    """load_state_dict(sd, assign=True) on a model that has run replaces its Parameters: eval reads the new ones, and a training step sends the block
    gradients to them."""
    m = _model(7)
    img = det_tensor((2, 3, 224, 224), "assign.img", 3).to(DEV)
    _eval(m, img)
    sd2 = {k: v.to(DEV) for k, v in fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 8).items()}
    m.load_state_dict(sd2, assign=True)
    y = _eval(m, img)
    assert torch.equal(y, _fresh_eval(m, img))
    m.train()
    with torch.autocast("cuda", torch.bfloat16):
        m(img).float().square().mean().backward()
    torch.cuda.synchronize()
    missing = [n for n, p in m.named_parameters() if n.startswith("stages.") and p.grad is None]
    assert not missing, f"block parameters without a gradient after the load: {missing[:4]} ({len(missing)})"


def test_derived_operands_go_with_the_model():
    import lemevit_amd.model as M
    gc.collect()
    before = len(M._derived)
    m = _model(7)
    img = det_tensor((2, 3, 224, 224), "life.img", 3).to(DEV)
    _eval(m, img)
    m.train()
    with torch.autocast("cuda", torch.bfloat16):
        m(img).float().square().mean().backward()
    _eval(m, img)
    torch.cuda.synchronize()
    assert len(M._derived) > before
    del m
    gc.collect()
    assert len(M._derived) == before


def test_steady_state_eval_fills_nothing():
    import lemevit_amd.model as M
    m = _model(7)
    img = det_tensor((2, 3, 224, 224), "steady.img", 3).to(DEV)
    _eval(m, img)
    f = M.cache_fills()
    _eval(m, img)
    assert M.cache_fills() == f


def test_model_ema_follows_flat_adamw_built_after_first_update():
    """FlatAdamW re-homes every block parameter onto its flat buffer (p.data = view); an EMA that has already run must follow."""
    import lemevit_amd as lib
    torch.manual_seed(0)
    m = _model(11).train()
    decay = 0.9
    ema = lib.ModelEma(m, decay=decay)
    ref = {k: v.detach().clone().double() for k, v in m.state_dict().items() if v.dtype.is_floating_point}

    def advance():
        ema.update(m)
        for k, v in m.state_dict().items():
            if v.dtype.is_floating_point:
                ref[k] = decay * ref[k] + (1 - decay) * v.detach().double()

    advance()
    opt = lib.FlatAdamW(m, lr=1e-2, weight_decay=0.05)
    img = det_tensor((4, 3, 96, 96), "ema.img", 2).to(DEV)
    tgt = torch.tensor([1, 2, 3, 4], device=DEV)
    for _ in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", torch.bfloat16):
            torch.nn.functional.cross_entropy(m(img), tgt).backward()
        opt.step()
        advance()
    torch.cuda.synchronize()
    got = ema.module.state_dict()
    for k, r in ref.items():
        err = float((got[k].double() - r).abs().max())
        assert err <= 1e-6 * max(float(r.abs().max()), 1e-30), f"ema {k}: {err:.3e}"
