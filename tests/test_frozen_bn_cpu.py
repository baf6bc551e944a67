"""Training through frozen BatchNorm without a GPU: the new C-ABI symbols are declared, exported and bound; the new entry points refuse bad arguments before any
launch; the float64 restatements that tests/test_frozen_bn_gpu.py holds the kernels to agree with autograd through conv2d -> batch_norm(eval) -> gelu and through
the classifier tail; and the oracle meets the reference's eval-mode fixture (frozenbn_tiny_96: the fp32 class of the project, 1e-5 of max-abs for logits and full
gradients as in test_input_grad_cpu.py, 3e-4 for the gradient norms as in test_oracle_in_chans_train_step)."""
import ctypes
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CI_TAP, TAP_CI = 0, 1


# ------------------------------------------------------------------------------------------------
# float64 restatements of the new kernels (the GPU tests compare the kernels with these on identical operands)
# ------------------------------------------------------------------------------------------------
def fold_ref(w, b, gamma, beta, mean, var, eps, KP, layout):
    """lmv_conv_bn_fold: (wm [Co, KP], bf [Co], s [Co]) in float64."""
    w, gamma, beta, mean, var = (t.double() for t in (w, gamma, beta, mean, var))
    Co, Cin = w.shape[:2]
    r = 1.0 / torch.sqrt(var + eps)
    s = gamma * r
    ws = w * s[:, None, None, None]
    wm = torch.zeros(Co, KP, dtype=torch.float64)
    wm[:, :9 * Cin] = ws.reshape(Co, 9 * Cin) if layout == CI_TAP else ws.permute(0, 2, 3, 1).reshape(Co, 9 * Cin)
    b0 = torch.zeros(Co, dtype=torch.float64) if b is None else b.double()
    return wm, (b0 - mean) * s + beta, s


def fold_bwd_ref(dwm, dbf, w, b, gamma, mean, var, eps, layout):
    """lmv_conv_bn_fold_bwd: (dW [Co, Cin, 3, 3], db, dgamma, dbeta) in float64."""
    dwm, dbf, w, gamma, mean, var = (t.double() for t in (dwm, dbf, w, gamma, mean, var))
    Co, Cin = w.shape[:2]
    r = 1.0 / torch.sqrt(var + eps)
    s = gamma * r
    d = dwm[:, :9 * Cin]
    dwf = d.reshape(Co, Cin, 3, 3) if layout == CI_TAP else d.reshape(Co, 3, 3, Cin).permute(0, 3, 1, 2)
    b0 = torch.zeros(Co, dtype=torch.float64) if b is None else b.double()
    return dwf * s[:, None, None, None], dbf * s, r * ((dwf * w).sum((1, 2, 3)) + dbf * (b0 - mean)), dbf.clone()


def gelu_bwd_ref(a, w, bias, da):
    """lmv_linear_fwd(LMV_ACT_GELU_BWD): da * GELU'(a w^T + bias) in float64."""
    z = a.double() @ w.double().t() + (0.0 if bias is None else bias.double())
    return da.double() * (0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi))


def patches_ref(x, KP, layout):
    """The patch matrix of a 3 x 3 / stride-2 / padding-1 convolution, [B Ho Wo, KP], in either column order."""
    B, Ci, H, W = x.shape
    cols = F.unfold(x, 3, padding=1, stride=2)                      # [B, Ci * 9, Ho Wo], column order ci * 9 + tap
    p = cols.transpose(1, 2).reshape(-1, Ci * 9)
    if layout == TAP_CI:
        p = p.reshape(-1, Ci, 9).transpose(1, 2).reshape(-1, 9 * Ci)
    out = torch.zeros(p.shape[0], KP, dtype=x.dtype)
    out[:, :9 * Ci] = p
    return out


def test_restatements_agree_with_autograd():
    dd = torch.float64
    for layout, Ci, Co, bias, gelu in [(CI_TAP, 3, 8, True, True), (CI_TAP, 13, 16, False, True), (TAP_CI, 8, 16, True, False), (TAP_CI, 16, 8, False, False)]:
        torch.manual_seed(Ci)
        B, H, W, eps = 2, 11, 8, 1e-5
        x = torch.randn(B, Ci, H, W, dtype=dd, requires_grad=True)
        w = torch.randn(Co, Ci, 3, 3, dtype=dd, requires_grad=True)
        b = torch.randn(Co, dtype=dd, requires_grad=True) if bias else None
        g = torch.randn(Co, dtype=dd, requires_grad=True); be = torch.randn(Co, dtype=dd, requires_grad=True)
        mu = torch.randn(Co, dtype=dd); var = torch.rand(Co, dtype=dd) + 0.5
        y = F.batch_norm(F.conv2d(x, w, b, 2, 1), mu, var, g, be, False, 0.1, eps)
        y = F.gelu(y) if gelu else y
        da = torch.randn_like(y)
        y.backward(da)
        # the fold route, as the model's node runs it: fold -> GEMM on the patch matrix -> (GELU' from recomputed z) -> weight-gradient GEMM -> fold_bwd
        KP = (9 * Ci + 31) // 32 * 32
        wm, bf, s = fold_ref(w.detach(), None if b is None else b.detach(), g.detach(), be.detach(), mu, var, eps, KP, layout)
        assert bool((wm[:, 9 * Ci:] == 0).all())
        p = patches_ref(x.detach(), KP, layout)
        z = p @ wm.t() + bf
        a = F.gelu(z) if gelu else z
        yr = y.detach().permute(0, 2, 3, 1).reshape(-1, Co)
        dar = da.permute(0, 2, 3, 1).reshape(-1, Co)
        dz = gelu_bwd_ref(p, wm, bf, dar) if gelu else dar
        dW, db, dg, dbe = fold_bwd_ref(dz.t() @ p, dz.sum(0), w.detach(), None if b is None else b.detach(), g.detach(), mu, var, eps, layout)
        for name, u, v in [("y", a, yr), ("dW", dW, w.grad), ("dgamma", dg, g.grad), ("dbeta", dbe, be.grad)] + ([("db", db, b.grad)] if bias else []):
            err = float((u - v).abs().max() / v.abs().max())
            assert err < 1e-12, (layout, Ci, name, err)


def tail_bwd_ref(dpooled, x, gamma, mean, var, eps):
    """The eval form of the classifier tail: (dx [B, L, C], dgamma, dbeta) in float64."""
    dpooled, x, gamma, mean, var = (t.double() for t in (dpooled, x, gamma, mean, var))
    r = 1.0 / torch.sqrt(var + eps)
    L = x.shape[1]
    return (dpooled * gamma * r / L)[:, None, :].expand_as(x), (dpooled * (x.mean(1) - mean) * r).sum(0), dpooled.sum(0)


def test_tail_restatement_agrees_with_autograd():
    torch.manual_seed(1)
    dd = torch.float64
    B, L, C, eps = 3, 49, 16, 1e-5
    xt = torch.randn(B, L, C, dtype=dd, requires_grad=True)
    g = torch.randn(C, dtype=dd, requires_grad=True); be = torch.randn(C, dtype=dd, requires_grad=True)
    mu = torch.randn(C, dtype=dd); var = torch.rand(C, dtype=dd) + 0.5
    p = F.batch_norm(xt.transpose(1, 2).reshape(B, C, 7, 7), mu, var, g, be, False, 0.1, eps).flatten(2).mean(-1)
    dp = torch.randn_like(p)
    p.backward(dp)
    dx, dg, dbe = tail_bwd_ref(dp, xt.detach(), g.detach(), mu, var, eps)
    for name, u, v in [("dx", dx, xt.grad), ("dgamma", dg, g.grad), ("dbeta", dbe, be.grad)]:
        assert float((u - v).abs().max() / v.abs().max()) < 1e-12, name


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_bound():
    from lemevit_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    assert re.search(r"#define LMV_ABI_VERSION 14\b", src) and "LMV_ACT_GELU_BWD = 3" in src
    assert "LMV_FOLD_CI_TAP = 0" in src and "LMV_FOLD_TAP_CI = 1" in src
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n, nargs in [("lmv_conv_bn_fold", 16), ("lmv_conv_bn_fold_bwd", 17)]:
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(raw, n) and n in _lib.SIGNATURES
        fn = getattr(_lib.lib, n)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    assert (_lib.ACT_GELU_BWD, ops.ACT_GELU_BWD, ops.FOLD_CI_TAP, ops.FOLD_TAP_CI) == (3, 3, 0, 1)
    assert callable(ops.conv_bn_fold) and callable(ops.conv_bn_fold_bwd)


def test_new_entry_points_refuse_bad_arguments():
    from lemevit_amd import _lib
    lib = _lib.lib
    p = 1 << 20          # (a non-null, aligned address: no launch happens on any of these calls)

    def fold(Co=32, Cin=3, KP=32, layout=0, wm=p, w=p, dtype=1):
        return lib.lmv_conv_bn_fold(w, p, p, p, p, p, 1e-5, Co, Cin, KP, layout, wm, p, p, dtype, None)

    def fold_bwd(Co=32, Cin=3, KP=32, layout=0, dwm=p):
        return lib.lmv_conv_bn_fold_bwd(dwm, p, p, p, p, p, p, 1e-5, Co, Cin, KP, layout, p, p, p, p, None)

    for fn, name in [(fold, b"conv_bn_fold"), (fold_bwd, b"conv_bn_fold_bwd")]:
        for kw, word in [(dict(KP=24), b"9 Cin"), (dict(Cin=4, KP=32), b"9 Cin"), (dict(Co=12), b"multiple of 8"), (dict(layout=2), b"layout"), (dict(layout=-1), b"layout"),
                         (dict(Co=0), b"bad shape"), (dict(Cin=0), b"bad shape")]:
            assert fn(**kw) == -1 and name in lib.lmv_last_error() and word in lib.lmv_last_error(), (name, kw, lib.lmv_last_error())
    assert fold(w=None) == -1 and fold(wm=None) == -1 and fold(wm=p + 8) == -1 and fold_bwd(dwm=None) == -1
    assert fold(dtype=7) == -2

    q = (_lib.LinearProblem * 1)()
    q[0].a = q[0].w = q[0].out = p
    q[0].rows = 64
    assert lib.lmv_linear_fwd(q, 1, 32, 32, _lib.ACT_GELU_BWD, 1, None) == -1 and b"aux" in lib.lmv_last_error()
    q[0].aux = p
    assert lib.lmv_linear_fwd(q, 1, 32, 40, _lib.ACT_GELU_BWD, 1, None) == -1 and b"multiple of 32" in lib.lmv_last_error()
    assert lib.lmv_linear_fwd(q, 1, 136, 32, _lib.ACT_GELU_BWD, 1, None) == -1 and b"at most 128" in lib.lmv_last_error()
    q[0].res = p
    assert lib.lmv_linear_fwd(q, 1, 32, 32, _lib.ACT_GELU_BWD, 1, None) == -1 and b"residual" in lib.lmv_last_error()
    q[0].res = None
    assert lib.lmv_linear_fwd(q, 1, 32, 32, _lib.ACT_GELU_BWD, 7, None) == -2
    assert lib.lmv_linear_fwd(q, 1, 32, 32, 4, 1, None) == -1 and b"act must be" in lib.lmv_last_error()


def test_switch_and_predicates():
    """LMV_FROZEN_BN is a module-level switch beside LMV_STEM / LMV_CONV_IMPLICIT; the pairing predicate takes only a BatchNorm2d in eval mode that tracks running
    statistics, is affine and holds fp32 parameters and buffers."""
    import lemevit_amd.model as M
    nn = torch.nn
    assert M._FROZEN_BN is True and M._STEM is True and M._CONV_IMPLICIT is True
    bn = nn.BatchNorm2d(16)
    assert not M._bn_frozen(bn)                                   # training mode
    assert M._bn_frozen(bn.eval())
    assert not M._bn_frozen(nn.BatchNorm2d(16, affine=False).eval())
    assert not M._bn_frozen(nn.BatchNorm2d(16, track_running_stats=False).eval())
    assert not M._bn_frozen(nn.BatchNorm2d(16).eval().to(torch.bfloat16))
    assert not M._bn_frozen(nn.GroupNorm(2, 16).eval()) and not M._bn_frozen(None)
    old = M._FROZEN_BN
    try:
        M._FROZEN_BN = False
        assert not M._bn_frozen(bn)
    finally:
        M._FROZEN_BN = old


# ------------------------------------------------------------------------------------------------
# the oracle against the reference's fixture
# ------------------------------------------------------------------------------------------------
def _close(out, ref, tol, what):
    out = np.asarray(out.detach().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max() / mx
    print(f"{what}: rel max-abs err {err:.2e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.0e} of max-abs {mx:.3e}"


def test_oracle_meets_frozen_bn_fixture(golden):
    meta, g = golden("frozenbn_tiny_96")
    cfg = O.VARIANTS[meta["variant"]]
    sd = fill_state_dict(O.state_dict_spec(cfg, meta["num_classes"]), meta["seed"])
    for k, v in sd.items():
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), meta["img"], meta["img_seed"])
    logits = O.lemevit_forward(sd, cfg, img, train=False)
    loss = F.cross_entropy(logits, torch.tensor(meta["target"]))
    loss.backward()
    _close(logits.detach(), g["logits"], 1e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    assert len(meta["bn_params"]) == 12 and "norm.weight" in meta["bn_params"]          # five stem / transition BatchNorms and the final one
    for k in meta["bn_params"] + ["downsample_layers.0.0.weight"]:
        _close(sd[k].grad, g["grad." + k], 1e-5, "grad " + k)
    gn = np.array([float(sd[k].grad.norm()) if sd[k].grad is not None else 0.0 for k in meta["param_names"]], dtype=np.float32)
    assert np.all(np.abs(gn - g["grad_norms"]) <= 3e-4 * np.maximum(1.0, np.abs(g["grad_norms"]))), np.abs(gn - g["grad_norms"]).max()
