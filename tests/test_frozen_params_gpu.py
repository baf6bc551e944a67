"""Frozen parameters on the MI355X: a LeMeBlock none of whose parameters requires grad runs DATA-ONLY (LMV_BLOCK_DATA_ONLY) -- reduced saved set, no
weight-gradient launch, no reduce, nothing on the side stream -- and, where selected, the fused dX kernel of the MLP half (lmv_mlp_dx_fused).

Freezing changes no gradient that remains (tests/test_frozen_params_cpu.py pins that to the reference on the oracle), so the yardsticks are the existing
goldens at the tolerances of the tests that already use them: blockgrad_* (tests/test_model_gpu.py: outputs 1e-5, dx / dc 2e-5), the float64 oracle in bf16
(test_block_backward_bf16_vs_oracle: 2e-2 / 3e-2), train_tiny_96 (test_train_step_fp32), inputgrad_tiny_96_eval (tests/test_input_grad_gpu.py: 2e-5 / 2e-4)
and dense_tiny_160x96 (1e-5).  The tolerance of the fused kernel alone is derived inside its test from the error of the existing two-launch form."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict, sample
from oracle import lemevit_oracle as O

DEV = "cuda:0"


def L():
    import lemevit_amd
    return lemevit_amd


def Mod():
    import lemevit_amd.model as M
    return M


def ops():
    from lemevit_amd import ops as o
    return o


def close(out, ref, tol, what):
    out = np.asarray(out.detach().float().cpu().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), what
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max()
    print(f"{what}: max-abs err {err / mx:.2e} of max-abs")
    assert err <= tol * mx, f"{what}: max-abs err {err:.3e} > {tol:.0e} * {mx:.3e}"
    return err / mx


def load(module, prefix, seed):
    spec = {prefix + k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = fill_state_dict(spec, seed)
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items()})
    return module.to(DEV)


def _block(t, C, h, dense=False, mlp_ratio=4):
    return L().LeMeBlock(dim=C, attn_drop=0.0, proj_drop=0.0, drop_path=0.0, attn_type=t, num_heads=h, mlp_ratio=mlp_ratio, **(dict(dense=True) if dense else {}))


def _model(variant, num_classes, seed, **kw):
    m = L().create_model(variant, num_classes=num_classes, **kw)
    spec = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(fill_state_dict(spec, seed))
    return m.to(DEV)


@pytest.fixture
def cfg():
    """lmv_config_set for the test, restored afterwards."""
    from lemevit_amd import _lib
    saved = {}

    def set_(key, value):
        saved.setdefault(key, _lib.config_get(key))
        _lib.config_set(key, value)
    yield set_
    for k, v in saved.items():
        _lib.config_set(k, v)


class _Kinds:
    """The launch kinds the library's timing probe saw (lmv_debug_launch_timing): kind 12 is lmv_mlp_dx_fused."""

    def __enter__(self):
        from lemevit_amd import _lib
        self.lib, self.cap = _lib.lib, 4096
        _lib.check(self.lib.lmv_debug_launch_timing(self.cap), "lmv_debug_launch_timing")
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        ms = (ctypes.c_float * self.cap)(); fl = (ctypes.c_double * self.cap)(); by = (ctypes.c_double * self.cap)(); kd = (ctypes.c_int * self.cap)()
        n = self.lib.lmv_debug_launch_timing_read(ms, fl, by, kd, self.cap)
        self.kinds = [kd[i] for i in range(n)]
        self.lib.lmv_debug_launch_timing(0)
        return False


# ------------------------------------------------------------------------------------------------
# (1) fp32 block kinds against the reference goldens
@pytest.mark.parametrize("name", ["blockgrad_D", "blockgrad_S", "blockgrad_C", "blockgrad_Sx"])
def test_frozen_block_backward_fp32(golden, name):
    meta, g = golden(name)
    dense = name == "blockgrad_Sx"
    t, C, h, H, W, B = ("S" if dense else meta["type"]), meta["C"], meta["h"], meta["H"], meta["W"], meta["B"]
    m = load(_block(t, C, h, dense), "blk.", meta["seed"]).eval().requires_grad_(False)
    x = det_tensor((B, C, H, W), name + ".x", 3).to(DEV).requires_grad_(True); c = det_tensor((B, 16, C), name + ".c", 3).to(DEV).requires_grad_(True)
    gx = det_tensor((B, C, H, W), name + ".gx", 3).to(DEV); gc = det_tensor((B, 16, C), name + ".gc", 3).to(DEV)
    before = ops().wgrad_launches()
    xo, co = m(x, c)
    ((xo * gx).sum() + (co * gc).sum()).backward()
    torch.cuda.synchronize()
    assert ops().wgrad_launches() == before
    close(xo, g["x_out"], 1e-5, "x_out")
    if dense:
        assert torch.equal(co.detach(), c.detach()) and torch.equal(c.grad, gc)
    else:
        close(co, g["c_out"], 1e-5, "c_out"); close(c.grad, g["dc"], 2e-5, "dc")
    close(x.grad, g["dx"], 2e-5, "dx")
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------
# (2) bf16 against the float64 oracle
def _bf16_vs_oracle(t, C, h, Hs, B=3, mlp_ratio=4):
    m = load(_block(t, C, h, mlp_ratio=mlp_ratio), "blk.", 5).eval().requires_grad_(False)
    sd = {"blk." + k: v.detach().to(torch.bfloat16).double().cpu() if ("attn." in k or "mlp." in k) and k.endswith("weight") else v.detach().double().cpu()
          for k, v in m.state_dict().items()}
    xb = det_tensor((B, C, Hs, Hs), "x", 9).to(torch.bfloat16); cb = det_tensor((B, 16, C), "c", 9).to(torch.bfloat16)
    gx = det_tensor((B, C, Hs, Hs), "gx", 9).to(torch.bfloat16); gc = det_tensor((B, 16, C), "gc", 9).to(torch.bfloat16)
    x = xb.to(DEV).requires_grad_(True); c = cb.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        xo, co = m(x, c)
    ((xo.float() * gx.to(DEV).float()).sum() + (co.float() * gc.to(DEV).float()).sum()).backward()
    torch.cuda.synchronize()
    xr = xb.double().requires_grad_(True); cr = cb.double().requires_grad_(True)
    xt, _, _ = O.to_tokens(xr)
    xo_r, co_r = O.leme_block(sd, "blk.", t, xt, cr, Hs, Hs, h)
    xo_r = O.to_nchw(xo_r, Hs, Hs)
    ((xo_r * gx.double()).sum() + (co_r * gc.double()).sum()).backward()
    tag = f"{t} C={C}"
    close(xo, xo_r.detach().numpy(), 2e-2, tag + " x_out"); close(co, co_r.detach().numpy(), 2e-2, tag + " c_out")
    close(x.grad, xr.grad.numpy(), 3e-2, tag + " dx"); close(c.grad, cr.grad.numpy(), 3e-2, tag + " dc")
    assert all(p.grad is None for p in m.parameters())


def test_frozen_block_backward_bf16_vs_oracle():
    """The four blocks of tests/test_model_gpu.py::test_block_backward_bf16_vs_oracle with frozen parameters, in the shipped configuration."""
    for t, C, h, Hs in [("D", 96, 3, 14), ("S", 192, 6, 7), ("C", 64, 2, 14), ("D2", 96, 3, 14)]:
        _bf16_vs_oracle(t, C, h, Hs)


@pytest.mark.parametrize("t,C,h,Hs", [("D", 96, 3, 14), ("S", 192, 6, 7), ("S", 384, 12, 14), ("C", 64, 2, 14)])
def test_frozen_block_backward_bf16_fused_dx_vs_oracle(cfg, t, C, h, Hs):
    """... and with the fused dX kernel of the MLP half forced (mlp_dx_fused = 2), one shape per supported model width; the timing probe confirms the
    kernel was taken (launch kind 12)."""
    cfg("mlp_dx_fused", 2)
    with _Kinds() as k:
        _bf16_vs_oracle(t, C, h, Hs)
    assert k.kinds.count(12) == 1, k.kinds
    cfg("mlp_dx_fused", 0)
    with _Kinds() as k:
        _bf16_vs_oracle(t, C, h, Hs)
    assert 12 not in k.kinds


def test_frozen_block_backward_bf16_fused_dx_ratio3_vs_oracle(cfg):
    """... and at MLP ratio 3 (lemevit_small_v2's stage 2: D, C = 128, hidden 384): the fused dX kernel walks three 128-wide hidden chunks instead of four, reached from
    a block as _frozen_wts sets it up."""
    cfg("mlp_dx_fused", 2)
    with _Kinds() as k:
        _bf16_vs_oracle("D", 128, 4, 12, mlp_ratio=3)
    assert k.kinds.count(12) == 1, k.kinds
    cfg("mlp_dx_fused", 0)
    with _Kinds() as k:
        _bf16_vs_oracle("D", 128, 4, 12, mlp_ratio=3)
    assert 12 not in k.kinds


# ------------------------------------------------------------------------------------------------
# (3) no weight-gradient work
def _run_tokens(kind, C, h, Hs, B, dtype, frozen, ckpt=False, seed=11, dense=False):
    from lemevit_amd.blocks import PARAM_NAMES
    M = Mod()
    blk = load(_block("S" if kind == "Sx" else kind, C, h, dense=kind == "Sx"), "blk.", seed)
    if frozen:
        blk.requires_grad_(False)
    allp = dict(blk.named_parameters())
    params = {n: allp[n] for n in PARAM_NAMES[kind]}
    N = Hs * Hs
    x = det_tensor((B, N, C), "x", 6).to(DEV, dtype).requires_grad_(True); c = det_tensor((B, 16, C), "c", 6).to(DEV, dtype).requires_grad_(True)
    gx = det_tensor((B, N, C), "gx", 6).to(DEV, dtype); gc = det_tensor((B, 16, C), "gc", 6).to(DEV, dtype)
    masks = (None,) * (2 if kind == "C" else 4)
    xo, co = M.run_block(kind, x, c, Hs, Hs, params, masks, ckpt=ckpt)
    before = ops().wgrad_launches()
    ((xo.float() * gx.float()).sum() + (co.float() * gc.float()).sum()).backward()
    torch.cuda.synchronize()
    moved = ops().wgrad_launches() - before
    return dict(xo=xo.detach(), co=co.detach(), dx=x.grad, dc=c.grad, moved=moved, grads=[p.grad for p in params.values()])


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("kind,C,h,Hs", [("D", 96, 3, 14), ("S", 192, 6, 7), ("C", 64, 2, 14)])
def test_no_weight_gradient_launches(kind, C, h, Hs, ckpt):
    for dtype in (torch.float32, torch.bfloat16):
        r = _run_tokens(kind, C, h, Hs, 3, dtype, frozen=True, ckpt=ckpt)
        assert r["moved"] == 0, f"{kind} {dtype}: {r['moved']} weight-gradient launches / reduces / forks for a frozen block"
        assert all(g is None for g in r["grads"])
        t = _run_tokens(kind, C, h, Hs, 3, dtype, frozen=False, ckpt=ckpt)
        assert t["moved"] >= 5, (kind, t["moved"])
        assert all(g is not None for g in t["grads"])
        if dtype == torch.bfloat16:          # (the mode whose kernels reproduce bit for bit from run to run)
            assert torch.equal(r["xo"], t["xo"]) and torch.equal(r["co"], t["co"])


@pytest.mark.parametrize("kind,C,h,Hs", [("D", 96, 3, 14), ("S", 192, 6, 7), ("C", 64, 2, 14), ("D2", 96, 3, 14), ("Sx", 192, 6, 7)])
def test_python_schedule_makes_no_weight_gradient_call(monkeypatch, kind, C, h, Hs):
    """The per-launch Python schedules (LMV_BLOCK_NATIVE=0; "D2" and "Sx" always): no ops.linear_dw / ops.dwconv_bwd_weight call for a frozen block."""
    M = Mod()
    monkeypatch.setattr(M, "_NATIVE", False)
    calls = []
    lin, dwc = ops().linear_dw, ops().dwconv_bwd_weight
    monkeypatch.setattr(ops(), "linear_dw", lambda *a, **k: (calls.append("linear_dw"), lin(*a, **k))[1])
    monkeypatch.setattr(ops(), "dwconv_bwd_weight", lambda *a, **k: (calls.append("dwconv"), dwc(*a, **k))[1])
    res = {}
    for frozen in (True, False):
        calls.clear()
        res[frozen] = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=frozen)
        if frozen:
            assert not calls, calls
            assert all(g is None for g in res[frozen]["grads"])
        else:
            assert "linear_dw" in calls and "dwconv" in calls
    # the same dX launches on both sides: the pruning is bit-exact
    assert torch.equal(res[True]["dx"], res[False]["dx"]) and torch.equal(res[True]["dc"], res[False]["dc"])


# ------------------------------------------------------------------------------------------------
# (4) bit identity of the pruning
@pytest.mark.parametrize("kind,C,h,Hs", [("D", 96, 3, 14), ("S", 192, 6, 7), ("S", 384, 12, 14), ("C", 64, 2, 14)])
def test_data_only_is_bit_identical_to_the_full_backward(monkeypatch, cfg, kind, C, h, Hs):
    M = Mod()
    cfg("mlp_dx_fused", 0)
    monkeypatch.setattr(M, "_FROZEN_WTS", False)          # no transposed copies: both runs select the dX kernels of a plain trainable block
    a = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=True)
    b = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=False)
    assert a["moved"] == 0 and b["moved"] > 0
    for k in ("xo", "co", "dx", "dc"):
        assert torch.equal(a[k], b[k]), f"{kind} {k}: data-only and full backward differ by {float((a[k].float() - b[k].float()).abs().max()):.3e}"
    # the full backward forced for the frozen block (the comparison side of the model-level tests) is the same thing again
    monkeypatch.setattr(M, "_FROZEN_DATA_ONLY", False)
    f = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=True)
    assert f["moved"] > 0 and all(g is None for g in f["grads"])
    assert torch.equal(a["dx"], f["dx"]) and torch.equal(a["dc"], f["dc"])
    # the fused kernel: deterministic
    monkeypatch.setattr(M, "_FROZEN_DATA_ONLY", True)
    monkeypatch.setattr(M, "_FROZEN_WTS", True)
    cfg("mlp_dx_fused", 2)
    u = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=True)
    v = _run_tokens(kind, C, h, Hs, 3, torch.bfloat16, frozen=True)
    assert torch.equal(u["dx"], v["dx"]) and torch.equal(u["dc"], v["dc"])


# ------------------------------------------------------------------------------------------------
# (5) the fused kernel alone
def _gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


# (C, hidden, row counts of the one or two problems): hidden = 4 C at every width the kernel admits, then the 3 C of lemevit_small_v2 (three / six 128-wide chunks) and 2 C
MLP_DX_CASES = [(64, 256, (1000, 37)), (96, 384, (777,)), (96, 384, (3136 * 2 + 5, 32)), (192, 768, (1571, 48)), (384, 1536, (1029, 130)), (384, 1536, (64,)),
                (128, 512, (1029, 130)), (256, 1024, (1029, 130)), (320, 1280, (1029, 130)), (128, 384, (1029, 130)), (256, 768, (64,)), (256, 768, (1029, 130)),
                (192, 384, (64,)), (128, 384, (64,))]


@pytest.mark.parametrize("tm", [0, 128])
@pytest.mark.parametrize("C,Hd,rows", MLP_DX_CASES, ids=[f"{C}-rows{i}" if i < 6 else f"{C}-{Hd}-rows{i}" for i, (C, Hd, _) in enumerate(MLP_DX_CASES)])
def test_mlp_dx_fused_kernel(cfg, C, Hd, rows, tm):
    """lmv_mlp_dx_fused against float64 math on the bf16-rounded operands.  The tolerance is not invented: the existing two-launch form
    (lmv_linear_fwd(.., LMV_ACT_GELU_GRAD) on fc2_wt, then the forward-form dX on fc1_wt) runs on the same inputs, its max-abs error against the float64
    result is measured, and the fused kernel is allowed 1.5 x that -- it rounds du at the same point and differs only in summation order."""
    if tm == 128 and C > 192:
        pytest.skip("C > 192 has the 128-row form only: covered by tm = 0")
    from lemevit_amd.ops import Prob, ACT_GELU_GRAD
    cfg("mlp_tm", tm)
    gen = torch.Generator().manual_seed(1000 + C + len(rows))
    bf = lambda t: t.to(torch.bfloat16)
    w2 = bf(torch.randn(C, Hd, generator=gen) * Hd ** -0.5)          # mlp.3.weight [C, hidden]
    w1 = bf(torch.randn(Hd, C, generator=gen) * C ** -0.5)           # mlp.0.weight [hidden, C]
    gs = [bf(torch.randn(r, C, generator=gen)) for r in rows]
    us = [bf(torch.randn(r, Hd, generator=gen) * 1.5) for r in rows]
    fc2_wt, fc1_wt = w2.t().contiguous().to(DEV), w1.t().contiguous().to(DEV)      # [hidden, C], [C, hidden]
    gd, ud = [g.to(DEV) for g in gs], [u.to(DEV) for u in us]
    assert ops().mlp_dx_fused_supported(C, Hd, torch.bfloat16)
    with _Kinds() as k:
        fused = ops().mlp_dx_fused(gd, ud, fc2_wt, fc1_wt)
    assert k.kinds == [12]
    du = [torch.empty_like(u) for u in ud]
    ops().linear_fwd([Prob(g, fc2_wt, o, aux=u) for g, o, u in zip(gd, du, ud)], Hd, C, ACT_GELU_GRAD)
    two = [torch.empty_like(g) for g in gd]
    ops().linear_fwd([Prob(d, fc1_wt, o) for d, o in zip(du, two)], C, Hd)
    torch.cuda.synchronize()
    for i, (g, u) in enumerate(zip(gs, us)):
        ref = ((g.double() @ w2.double()) * _gelu_grad64(u.double())) @ w1.double()
        mx = float(ref.abs().max())
        e2 = float((two[i].double().cpu() - ref).abs().max())
        ef = float((fused[i].double().cpu() - ref).abs().max())
        print(f"mlp_dx_fused C={C} hidden={Hd} rows={rows[i]} tm={tm}: two-launch err {e2:.3e}, fused err {ef:.3e} (max-abs {mx:.3e})")
        assert torch.isfinite(fused[i]).all()
        assert ef <= 1.5 * e2, f"C={C} hidden={Hd} rows={rows[i]}: fused {ef:.3e} > 1.5 x two-launch {e2:.3e}"
    again = ops().mlp_dx_fused(gd, ud, fc2_wt, fc1_wt)
    assert all(torch.equal(a, b) for a, b in zip(fused, again))


# ------------------------------------------------------------------------------------------------
# (6) model level, fp32
FROZEN = ("stages.0.", "stages.1.")


def test_train_step_fp32_with_frozen_stages(golden):
    meta, g = golden("train_tiny_96")
    m = _model(meta["variant"], meta["num_classes"], meta["seed"], drop_path_rate=meta["drop_path_rate"]).train()
    m.stages[0].requires_grad_(False); m.stages[1].requires_grad_(False)
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), "train_tiny_96.img", 5).to(DEV)
    logits = m(img)
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor(meta["target"], device=DEV))
    loss.backward()
    close(logits, g["logits"], 2e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) < 2e-5
    params = dict(m.named_parameters())
    nfrozen = 0
    for i, k in enumerate(meta["param_names"]):
        if k.startswith(FROZEN):
            assert params[k].grad is None, k
            nfrozen += 1
            continue
        gn = float(params[k].grad.norm()) if params[k].grad is not None else 0.0
        assert abs(gn - g["grad_norms"][i]) <= 1e-3 * max(1.0, abs(g["grad_norms"][i])), (k, gn, g["grad_norms"][i])
    assert nfrozen > 30
    for k in g:
        if k.startswith("grad.") and k != "grad_norms" and not k[5:].startswith(FROZEN):
            close(params[k[5:]].grad, g[k], 2e-4, k)
        if k.startswith("stat."):
            close(m.state_dict()[k[5:]], g[k], 1e-5, k)


def test_image_gradient_fp32_eval_all_frozen(golden):
    meta, g = golden("inputgrad_tiny_96_eval")
    m = _model("lemevit_tiny", 10, meta["seed"], drop_path_rate=0.0).eval().requires_grad_(False)
    img = det_tensor((4, 3, 96, 96), meta["img"], meta["img_seed"]).to(DEV).requires_grad_(True)
    before = ops().wgrad_launches()
    logits = m(img)
    logits[:, torch.tensor(meta["target"], device=DEV)].sum().backward()
    torch.cuda.synchronize()
    assert ops().wgrad_launches() == before
    close(logits, g["logits"], 2e-5, "logits")
    close(img.grad, g["dimg"], 2e-4, "img.grad")
    assert all(p.grad is None for p in m.parameters())


def test_dense_backbone_frozen_stages(golden):
    from lemevit_amd.model import LeMeViTBackbone
    meta, g = golden("dense_tiny_160x96")
    m = LeMeViTBackbone(**meta["cfg"], frozen_stages=[0, 1])
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, meta["seed"]))
    m = m.to(DEV).train()
    img = det_tensor((meta["B"], 3, meta["H"], meta["W"]), "dense_tiny_160x96.img", 6).to(DEV)
    outs = m(img)
    for i, o in enumerate(outs):
        close(sample(o.flatten(2).transpose(1, 2).contiguous(), 8192), g[f"out{i}"], 1e-5, f"out{i}")
    sum(o.square().mean() for o in outs).backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k.startswith(FROZEN):
            assert p.grad is None, k
    assert any(p.grad is not None for k, p in m.named_parameters() if k.startswith("stages.2."))
    assert any(p.grad is not None for k, p in m.named_parameters() if k.startswith("downsample_layers.0."))


# ------------------------------------------------------------------------------------------------
# (7) composition
def _tiny_step(frozen_stages, ckpt_stages=(), B=4, res=96, with_opt=False, seed=41):
    Lm = L()
    torch.manual_seed(0)
    m = _model("lemevit_tiny", 10, seed, drop_path_rate=0.0, **(dict(use_checkpoint_stages=list(ckpt_stages)) if ckpt_stages else {})).train()
    for i in frozen_stages:
        m.stages[i].requires_grad_(False)
    opt = Lm.FlatAdamW(m, lr=1e-3, weight_decay=0.05) if with_opt else None
    img = det_tensor((B, 3, res, res), "frozen.step.img", 5).to(DEV).requires_grad_(True)
    y = torch.tensor([1, 7, 3, 3][:B], device=DEV)
    if opt is not None:
        opt.zero_grad()
    with torch.autocast("cuda", torch.bfloat16):
        loss = torch.nn.functional.cross_entropy(m(img), y)
    loss.backward()
    torch.cuda.synchronize()
    return m, opt, img, loss


def test_checkpointed_frozen_is_bit_identical_to_unchecked_frozen():
    m0, _, i0, l0 = _tiny_step([0, 1, 2])
    m1, _, i1, l1 = _tiny_step([0, 1, 2], ckpt_stages=(0, 1, 2, 3))
    assert torch.equal(l0, l1) and torch.equal(i0.grad, i1.grad)
    for (k, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), k
    assert all(p.grad is None for k, p in m1.named_parameters() if k.startswith(("stages.0.", "stages.1.", "stages.2.")))


def test_flat_adamw_over_frozen_stages(monkeypatch, cfg):
    """FlatAdamW builds its flat buffers over the trainable block parameters only.  After one step the frozen parameters are bitwise unchanged and the
    trainable ones equal, bit for bit, the same step with the frozen blocks forced onto the full backward -- with the switches set so that both runs select
    the same dX kernels (no transposed copies for the frozen blocks, fused dX off), as in test_data_only_is_bit_identical_to_the_full_backward."""
    M = Mod()
    cfg("mlp_dx_fused", 0)
    monkeypatch.setattr(M, "_FROZEN_WTS", False)
    res = {}
    for data_only in (True, False):
        monkeypatch.setattr(M, "_FROZEN_DATA_ONLY", data_only)
        before = ops().wgrad_launches()
        m, opt, img, loss = _tiny_step([0, 1], with_opt=True)
        frozen0 = {k: p.detach().clone() for k, p in m.named_parameters() if k.startswith(FROZEN)}
        flat_names = [n for n, _, _, _ in opt._slices]
        assert flat_names and not any(n.startswith(FROZEN) for n in flat_names)
        opt.step()
        torch.cuda.synchronize()
        for k, p in m.named_parameters():
            if k.startswith(FROZEN):
                assert torch.equal(p.detach(), frozen0[k]) and p.grad is None, k
        res[data_only] = ({k: p.detach().clone() for k, p in m.named_parameters()}, img.grad.clone(), loss.detach().clone(), ops().wgrad_launches() - before)
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][1], res[False][1])
    for k in res[True][0]:
        assert torch.equal(res[True][0][k], res[False][0][k]), k
    assert res[True][3] < res[False][3]


def test_flat_grad_sync_single_rank_with_frozen_stages():
    """FlatGradSync at world size 1 over a model with frozen stages: the chunk plan covers trainable blocks only, every chunk is released by a block that
    does report, finish() returns, and the step equals the twin's without the exchange."""
    import os
    import torch.distributed as dist
    from lemevit_amd.dist import attach_flat_grad_sync
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29543")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        Lm = L()
        torch.manual_seed(0)
        m1 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
        m2 = Lm.create_model("lemevit_tiny", num_classes=10).to(DEV).train()
        m2.load_state_dict(m1.state_dict())
        for m in (m1, m2):
            m.stages[0].requires_grad_(False); m.stages[1].requires_grad_(False)
        o1 = Lm.FlatAdamW(m1, lr=1e-3, weight_decay=0.05); o2 = Lm.FlatAdamW(m2, lr=1e-3, weight_decay=0.05)
        sync = attach_flat_grad_sync(m2, o2, nchunks=3, force=True)
        assert sync.active and sync.bounds[0][0] == 0 and sync.bounds[-1][1] == o2._flat_g.numel()
        assert not any(hasattr(p, "_lmv_grad_cb") for k, p in m2.named_parameters() if k.startswith(FROZEN))
        x = torch.randn(4, 3, 64, 64, device=DEV); y = torch.randint(0, 10, (4,), device=DEV)
        for _ in range(2):
            for m, o, s in ((m1, o1, None), (m2, o2, sync)):
                torch.manual_seed(7)
                o.zero_grad()
                with torch.autocast("cuda", torch.bfloat16):
                    loss = torch.nn.functional.cross_entropy(m(x), y)
                loss.backward()
                if s is not None:
                    assert len(s._work) == len(s.bounds), "a chunk waited for a block that never reports"
                    s.finish()
                o.step()
        torch.cuda.synchronize()
        for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(p1, p2), (n, float((p1 - p2).abs().max()))
    finally:
        if created:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------
# (8) memory
def test_peak_memory_drops_by_the_arena_difference(monkeypatch):
    """Base 224 x 224, bf16, B = 32, forward + backward with an image that requires grad: everything frozen peaks lower than everything trainable by at least
    the saved-set difference of lmv_block_arena_bytes summed over the natively scheduled blocks (the bound is computed here, from the shapes the run saw)."""
    from lemevit_amd._lib import lib, BlockDesc
    M = Mod()
    B = 32
    seen = []
    real = M.native_block_forward

    def spy(kind, x, c, H, W, names, P, masks, save, *a, **k):
        if save:
            seen.append((kind, x.shape[0], H, W, c.shape[1], x.shape[2], P["mlp.0.weight"].shape[0], bool(k.get("data_only", False))))
        return real(kind, x, c, H, W, names, P, masks, save, *a, **k)
    monkeypatch.setattr(M, "native_block_forward", spy)
    img0 = det_tensor((B, 3, 224, 224), "frozen.mem.img", 12)

    def peak(frozen):
        m = _model("lemevit_base", 1000, 7, drop_path_rate=0.0).train()
        if frozen:
            m.requires_grad_(False)
        img = img0.to(DEV).requires_grad_(True)
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        seen.clear()
        with torch.autocast("cuda", torch.bfloat16):
            out = m(img)
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        assert img.grad is not None and torch.isfinite(img.grad).all()
        return torch.cuda.max_memory_allocated() - base, list(seen)

    p_frozen, blocks = peak(True)
    p_train, blocks_t = peak(False)
    assert blocks and all(b[-1] for b in blocks) and not any(b[-1] for b in blocks_t) and len(blocks) == len(blocks_t)
    bound = 0
    for kind, b, H, W, Mt, C, hid, _ in blocks:
        d = BlockDesc()
        d.kind, d.dtype, d.B, d.H, d.W, d.M, d.C, d.hidden = {"S": 0, "D": 1, "C": 2}[kind], 1, b, H, W, Mt, C, hid
        full = lib.lmv_block_arena_bytes(ctypes.byref(d))
        d.flags = 4
        bound += full - lib.lmv_block_arena_bytes(ctypes.byref(d))
    print(f"peak: trainable {p_train / 2**20:.0f} MiB, frozen {p_frozen / 2**20:.0f} MiB, difference {(p_train - p_frozen) / 2**20:.0f} MiB; "
          f"arena difference over {len(blocks)} blocks {bound / 2**20:.0f} MiB")
    assert bound > 0 and p_train - p_frozen >= bound, (p_train, p_frozen, bound)


@pytest.mark.parametrize("kind,C,h,Hs", [("D", 96, 3, 14), ("S", 192, 6, 7)])
def test_frozen_block_does_not_keep_its_input(kind, C, h, Hs):
    """x is read by the position convolution's weight gradient alone: an unchecked frozen block keeps its shape only (lmv_block_bwd gets NULL), so the
    producer's tensor goes back to the allocator once nobody else holds it; a checkpointed or a trainable block keeps it.  dx / dc are unchanged."""
    import weakref
    from lemevit_amd.blocks import PARAM_NAMES
    M = Mod()
    B, N = 3, Hs * Hs
    x0 = det_tensor((B, N, C), "x", 6).to(DEV, torch.bfloat16).requires_grad_(True); c0 = det_tensor((B, 16, C), "c", 6).to(DEV, torch.bfloat16).requires_grad_(True)
    gx = det_tensor((B, N, C), "gx", 6).to(DEV, torch.bfloat16)

    def run(frozen, ckpt):
        blk = load(_block(kind, C, h), "blk.", 11)
        blk.requires_grad_(not frozen)
        allp = dict(blk.named_parameters())
        x0.grad = c0.grad = None
        x = x0 * 1                      # a non-leaf input, as between two blocks of a stage
        alive = weakref.ref(x)
        xo, co = M.run_block(kind, x, c0, Hs, Hs, {n: allp[n] for n in PARAM_NAMES[kind]}, (None,) * 4, ckpt=ckpt)
        del x
        kept = alive() is not None
        ((xo.float() * gx.float()).sum() + co.float().sum()).backward()
        torch.cuda.synchronize()
        return kept, x0.grad.clone(), c0.grad.clone()

    kept, dx, dc = run(True, False)
    kept_c, dx_c, dc_c = run(True, True)
    kept_t, _, _ = run(False, False)
    assert not kept and kept_c and kept_t, (kept, kept_c, kept_t)
    assert torch.equal(dx, dx_c) and torch.equal(dc, dc_c)
