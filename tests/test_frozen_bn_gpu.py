"""Training through frozen BatchNorm on a real MI355X: the fold kernels and the GELU-backward GEMM of csrc/convbn.hip through the C ABI against float64 restatements
on identical operands (tests/test_frozen_bn_cpu.py holds those to autograd), then the model paths that reach them: no stock batch_norm / gelu call is left, every
parameter gradient against float64 autograd through the oracle with the switch on AND off, the reference's eval-mode fixture, the saved set of the stem, frozen
parameters, run-to-run determinism.

Kernel tolerances are the project's (tests/test_input_grad_gpu.py, kernel_close): fp32 1e-5, bf16 1e-3 of the output's max-abs, one bf16 rounding of the OUTPUT on top
where the output is stored in bf16.  Model tolerances are test_train_step_fp32's (logits 2e-5, gradients 2e-4 of each tensor's max-abs, gradient norms 1e-3) and, in
bf16, the statistics and bounds of test_dense_backward_large."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict
from oracle import lemevit_oracle as O
from test_frozen_bn_cpu import CI_TAP, TAP_CI, fold_bwd_ref, fold_ref, gelu_bwd_ref
from test_input_grad_gpu import close, kernel_close

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
# the golden Tiny dense configuration and the reduced one of the dense backward tests (tests/test_dense_large_gpu.py)
TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
REDUCED = dict(TINY, depth=[1, 1, 1, 2, 1], drop_path_rate=0.0)


def L():
    import lemevit_amd
    return lemevit_amd


def ops():
    from lemevit_amd import ops as _ops
    return _ops


def Mod():
    import lemevit_amd.model as M
    return M


def _backbone(cfg, seed, **kw):
    m = Mod().LeMeViTBackbone(**cfg, **kw)
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m.to(DEV)


def _classifier(seed=41, **kw):
    m = L().create_model("lemevit_tiny", num_classes=10, **kw)
    m.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------
# 1. the fold kernels
def _kp(cin, layout, dtype):
    if layout == CI_TAP:
        return (9 * cin + 31) // 32 * 32
    return 9 * cin if (dtype == torch.float32 and cin % 8 == 0) else (9 * cin + 63) // 64 * 64


def _fold_operands(cin, co, bias, tag):
    w = det_tensor((co, cin, 3, 3), tag + ".w", 7)
    b = det_tensor((co,), tag + ".b", 7) if bias else None
    gamma = det_tensor((co,), tag + ".g", 7) + 1.5
    beta = det_tensor((co,), tag + ".be", 7)
    mean = det_tensor((co,), tag + ".mu", 7)
    var = det_tensor((co,), tag + ".var", 7).abs() + 0.25
    return w, b, gamma, beta, mean, var


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", [CI_TAP, TAP_CI], ids=["ci_tap", "tap_ci"])
def test_conv_bn_fold_kernels(layout, dtype):
    eps = 1e-5
    dev = lambda t: None if t is None else t.to(DEV)
    for cin in [1, 3, 4, 13, 32, 64, 192]:
        for co in [32, 48, 96, 320]:
            for bias in (True, False):
                tag = f"fold.{cin}.{co}"
                w, b, gamma, beta, mean, var = _fold_operands(cin, co, bias, tag)
                KP = _kp(cin, layout, dtype)
                wm, bf, s = ops().conv_bn_fold(dev(w), dev(b), dev(gamma), dev(beta), dev(mean), dev(var), eps, dtype, KP, layout)
                rwm, rbf, rs = fold_ref(w, b, gamma, beta, mean, var, eps, KP, layout)
                assert wm.dtype == dtype and wm.shape == (co, KP) and bf.dtype == s.dtype == torch.float32
                what = f"fold cin={cin} co={co} bias={bias}"
                kernel_close(wm, rwm, torch.float32, what + " wm")
                kernel_close(bf, rbf, torch.float32, what + " bf")
                kernel_close(s, rs, torch.float32, what + " s")
                assert not bool(wm[:, 9 * cin:].any()), what + ": padding columns must be exactly zero"
                dwm = det_tensor((co, KP), tag + ".dwm", 7)
                dbf = det_tensor((co,), tag + ".dbf", 7)
                got = ops().conv_bn_fold_bwd(dev(dwm), dev(dbf), dev(w), dev(b), dev(gamma), dev(mean), dev(var), eps, layout)
                again = ops().conv_bn_fold_bwd(dev(dwm), dev(dbf), dev(w), dev(b), dev(gamma), dev(mean), dev(var), eps, layout)
                ref = fold_bwd_ref(dwm, dbf, w, b, gamma, mean, var, eps, layout)
                for name, g_, a_, r_ in zip(("dW", "db", "dgamma", "dbeta"), got, again, ref):
                    assert g_.dtype == torch.float32 and torch.equal(g_, a_), what + f" {name}: a second launch differs"
                    kernel_close(g_, r_, torch.float32, what + " " + name)
    # each output is optional
    w, b, gamma, beta, mean, var = (t.to(DEV) for t in _fold_operands(3, 32, True, "fold.opt"))
    dwm, dbf = det_tensor((32, 32), "fold.opt.dwm", 7).to(DEV), det_tensor((32,), "fold.opt.dbf", 7).to(DEV)
    full = ops().conv_bn_fold_bwd(dwm, dbf, w, b, gamma, mean, var, eps, layout)
    for k in range(4):
        want = [j == k for j in range(4)]
        part = ops().conv_bn_fold_bwd(dwm, dbf, w, b, gamma, mean, var, eps, layout, want)
        assert [p is not None for p in part] == want and torch.equal(part[k], full[k])


# ------------------------------------------------------------------------------------------------
# 2. the GELU backward that recomputes its pre-activation
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [32, 48, 96])
@pytest.mark.parametrize("K", [32, 128, 288])
def test_gelu_bwd_epilogue(K, N, dtype):
    rows = ((97 + 1) // 2) * ((131 + 1) // 2)          # the patch rows of a 97 x 131 image: 3 234, not a multiple of any tile
    assert rows % 16 != 0
    a = (det_tensor((rows, K), f"gbwd.a.{K}", 8) * (2.0 / K ** 0.5)).to(dtype)
    w = det_tensor((N, K), f"gbwd.w.{N}.{K}", 8).to(dtype)
    bias = det_tensor((N,), f"gbwd.b.{N}", 8)
    da = det_tensor((rows, N), f"gbwd.da.{N}", 8).to(dtype)
    out = torch.full((rows + 16, N), float("nan"), device=DEV, dtype=dtype)          # rows behind M must stay untouched
    P = ops().Prob(a.to(DEV), w.to(DEV), out[:rows], bias=bias.to(DEV), aux=da.to(DEV))
    ops().linear_fwd([P], N, K, ops().ACT_GELU_BWD)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[rows:]).all()), "wrote behind the last row"
    kernel_close(out[:rows], gelu_bwd_ref(a, w, bias, da), dtype, f"gelu_bwd K={K} N={N} {dtype}")
    # the forward it pairs with: linear_fwd(ACT_GELU) without a pre-activation copy
    y = torch.empty((rows, N), device=DEV, dtype=dtype)
    ops().linear_fwd([ops().Prob(a.to(DEV), w.to(DEV), y, bias=bias.to(DEV))], N, K, ops().ACT_GELU)
    kernel_close(y, F.gelu(a.double() @ w.double().t() + bias.double()), dtype, f"gelu fwd K={K} N={N} {dtype}")


# ------------------------------------------------------------------------------------------------
# 3. no stock kernels
def _forbid(monkeypatch):
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called: a frozen BatchNorm / its GELU left the native kernels")
        return f
    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse("torch.nn.functional.batch_norm"))
    monkeypatch.setattr(torch.nn.functional, "gelu", refuse("torch.nn.functional.gelu"))
    monkeypatch.setattr(ops(), "batchnorm_apply_fwd", refuse("ops.batchnorm_apply_fwd"))


@pytest.mark.parametrize("ck", [[], [0, 1, 2, 3, 4]], ids=["plain", "checkpointed"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_no_stock_kernels_backbone(bf16, ck, monkeypatch):
    m = _backbone(TINY, 3, use_checkpoint_stages=ck).train()
    img = det_tensor((2, 3, 96, 160), "frozenbn.dense.img", 6).to(DEV)
    _forbid(monkeypatch)
    with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
        outs = m(img)
    sum((o.float() ** 2).mean() for o in outs).backward()
    torch.cuda.synchronize()
    bn = [p for seq in m.downsample_layers for mod in seq.modules() if isinstance(mod, torch.nn.BatchNorm2d) for p in mod.parameters()]
    assert len(bn) == 10 and all(p.grad is not None and torch.isfinite(p.grad).all() and bool(p.grad.any()) for p in bn)


@pytest.mark.parametrize("ck", [[], [0, 1, 2, 3, 4]], ids=["plain", "checkpointed"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_no_stock_kernels_classifier(bf16, ck, monkeypatch):
    m = _classifier(use_checkpoint_stages=ck).eval()
    img = det_tensor((2, 3, 96, 96), "frozenbn.cls.img", 6).to(DEV).requires_grad_(True)
    _forbid(monkeypatch)
    with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
        logits = m(img)
    logits.float().logsumexp(1).sum().backward()
    torch.cuda.synchronize()
    assert img.grad is not None and torch.isfinite(img.grad).all() and bool(img.grad.any())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in (m.norm.weight, m.norm.bias))


# ------------------------------------------------------------------------------------------------
# 4. gradients against float64 autograd through the oracle, new path and glue path
def _oracle_sd(m):
    return {k: (v.detach().cpu().double().requires_grad_("running" not in k) if v.dtype.is_floating_point else v.detach().cpu()) for k, v in m.state_dict().items()}


def _hold_gradients(m, ref_sd, dtype, must_have, what):
    """test_dense_backward_large's comparison: fp32 2e-4 of each tensor's max-abs; bf16 whole-gradient rel-L2 / cosine, per-tensor median / 90th percentile, worst cosine."""
    gmax = max(float(v.grad.abs().max()) for v in ref_sd.values() if getattr(v, "grad", None) is not None)
    errs, seen = [], set()
    for k, p in m.named_parameters():
        r = ref_sd[k].grad
        if r is None:
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        assert p.grad is not None, k
        gq = p.grad.detach().double().cpu()
        assert torch.isfinite(gq).all(), k
        if float(r.abs().max()) <= 1e-5 * gmax:                         # mathematically zero gradient: rounding noise on both sides, held to a coarse bound
            assert float(gq.abs().max()) <= (2e-4 if dtype == torch.float32 else 2e-2) * gmax, (k, float(gq.abs().max()), gmax)
            continue
        seen.add(k)
        errs.append((float((gq - r).abs().max() / r.abs().max()), float((gq - r).norm() / r.norm()), float(F.cosine_similarity(gq.flatten(), r.flatten(), dim=0)), k))
    errs.sort(reverse=True)
    missing = [k for k in must_have if k not in seen]
    assert not missing, f"{what}: no (non-zero) reference gradient for {missing}"
    print(f"{what} {dtype}: {len(errs)} tensors, largest per-tensor errors (max-abs, rel-L2, cosine):", [(k, f"{e:.2e}", f"{l2:.2e}", f"{c:.5f}") for e, l2, c, k in errs[:6]])
    print(f"{what} {dtype}: BatchNorm tensors:", [(k, f"{e:.2e}") for e, _, _, k in errs if k in must_have])
    if dtype == torch.float32:
        bad = [(k, e) for e, _, _, k in errs if e > 2e-4]
        assert not bad, bad
        return
    es = sorted(e for e, _, _, _ in errs)
    med, p90 = es[len(es) // 2], es[len(es) * 9 // 10]
    worst_cos = min((c, k) for _, _, c, k in errs)
    names = [k for _, _, _, k in errs]
    params = dict(m.named_parameters())
    gall = torch.cat([params[k].grad.detach().double().cpu().flatten() for k in names])
    rall = torch.cat([ref_sd[k].grad.flatten() for k in names])
    gl2 = float((gall - rall).norm() / rall.norm())
    gcos = float(F.cosine_similarity(gall, rall, dim=0))
    print(f"  whole-gradient rel-L2 {gl2:.2e} (bound 3e-2), cosine {gcos:.6f} (>= 0.9995); per tensor median {med:.2e} (2e-2), 90th percentile {p90:.2e} (8e-2), "
          f"worst cosine {worst_cos[0]:.4f} ({worst_cos[1]}; >= 0.90)")
    assert gl2 <= 3e-2 and gcos >= 0.9995, (gl2, gcos)
    assert med <= 2e-2 and p90 <= 8e-2, (med, p90)
    assert worst_cos[0] >= 0.90, worst_cos


_dense_ref = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_backbone_gradients_vs_oracle(dtype, monkeypatch):
    """The reduced dense backbone of test_dense_backward_large at 512 x 512, train() (norm layers frozen): every parameter gradient, gamma and beta of the five stem /
    transition BatchNorms included, with the fold (default) and with LMV_FROZEN_BN off.  Both paths are right; each is held to the oracle, not to the other."""
    H = W = 512
    m = _backbone(REDUCED, 3).train()
    img = det_tensor((1, 3, H, W), f"dense_large.grad.{H}x{W}.img", 6)
    bn = [n + "." + s for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) and n.startswith("downsample_layers") for s in ("weight", "bias")]
    assert len(bn) == 10
    if "sd" not in _dense_ref:
        ref_sd = _oracle_sd(m)
        refs = O.lemevit_dense_forward(ref_sd, REDUCED, img.double())
        gs = [det_tensor(tuple(r.shape), f"dense_large.grad.g{i}", 6) for i, r in enumerate(refs)]
        sum((r * g.double()).sum() for r, g in zip(refs, gs)).backward()
        _dense_ref.update(sd=ref_sd, gs=gs, outs=[r.detach() for r in refs])
    ref_sd, gs = _dense_ref["sd"], _dense_ref["gs"]
    for on in (True, False):
        monkeypatch.setattr(Mod(), "_FROZEN_BN", on)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
            outs = m(img.to(DEV))
        sum((o.float() * g.to(DEV)).sum() for o, g in zip(outs, gs)).backward()
        for i, (o, r) in enumerate(zip(outs, _dense_ref["outs"])):
            close(o, r, 1e-5 if dtype == torch.float32 else 2e-2, f"train-mode out{i} (LMV_FROZEN_BN={int(on)})")
        _hold_gradients(m, ref_sd, dtype, bn, f"dense backbone 512x512 LMV_FROZEN_BN={int(on)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_classifier_gradients_vs_oracle(dtype, monkeypatch):
    """create_model('lemevit_tiny').eval() under autograd (cross-entropy; the image requires grad): every parameter gradient, `norm` and the five stem / transition
    BatchNorms included, against O.lemevit_forward(train=False) in float64; switch on and off."""
    cfg = O.VARIANTS["lemevit_tiny"]
    m = _classifier(41).eval()
    img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5)
    tgt = torch.tensor([1, 7, 3, 3])
    bn = [n + "." + s for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d) for s in ("weight", "bias")]
    assert len(bn) == 12
    ref_sd = _oracle_sd(m)
    rimg = img.double().requires_grad_(True)
    F.cross_entropy(O.lemevit_forward(ref_sd, cfg, rimg, train=False), tgt).backward()
    for on in (True, False):
        monkeypatch.setattr(Mod(), "_FROZEN_BN", on)
        m.zero_grad(set_to_none=True)
        x = img.to(DEV).requires_grad_(True)
        with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
            loss = F.cross_entropy(m(x).float(), tgt.to(DEV))
        loss.backward()
        _hold_gradients(m, ref_sd, dtype, bn, f"classifier eval 96x96 LMV_FROZEN_BN={int(on)}")
        if dtype == torch.float32:
            close(x.grad, rimg.grad, 2e-4, f"image gradient (LMV_FROZEN_BN={int(on)})")


# ------------------------------------------------------------------------------------------------
# 5. the reference's fixture
def test_reference_fixture_fp32(golden):
    meta, g = golden("frozenbn_tiny_96")
    m = _classifier(meta["seed"]).eval()
    img = det_tensor((meta["B"], 3, meta["res"], meta["res"]), meta["img"], meta["img_seed"]).to(DEV)
    logits = m(img)
    loss = F.cross_entropy(logits, torch.tensor(meta["target"], device=DEV))
    loss.backward()
    close(logits, g["logits"], 2e-5, "logits")
    # cross-entropy moves by at most twice the largest logit error (|d logsumexp| <= max |d logit|, plus the target logit's own), so the logits' bound carries over
    print(f"loss {loss.item():.6f} vs {float(g['loss']):.6f}")
    assert abs(loss.item() - float(g["loss"])) <= 2 * 2e-5 * float(np.abs(g["logits"]).max())
    params = dict(m.named_parameters())
    gn = np.array([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in meta["param_names"]])
    bad = np.abs(gn - g["grad_norms"]) > 1e-3 * np.maximum(1.0, np.abs(g["grad_norms"]))
    assert not bad.any(), [(meta["param_names"][i], gn[i], g["grad_norms"][i]) for i in np.nonzero(bad)[0][:5]]
    assert len(meta["bn_params"]) == 12
    for k in meta["bn_params"] + ["downsample_layers.0.0.weight"]:
        close(params[k].grad, g["grad." + k], 2e-4, "grad " + k)


# ------------------------------------------------------------------------------------------------
# 6. what the stem keeps for the backward pass
def test_stem_saved_set():
    """Tiny backbone, 2 x 3 x 800 x 1344, bf16 autocast, no checkpointing: across the stem call the allocation grows by the patch matrix of the first convolution, the
    map between the two convolutions and the stem's output -- no pre-BatchNorm or pre-GELU map.  8 MiB cover the allocator's granularity (and the folded operands)."""
    m = _backbone(TINY, 3).train()
    B, H, W = 2, 800, 1344
    img = det_tensor((B, 3, H, W), "ckpt.dense.img", 6).to(DEV)
    Cm, Co = m.downsample_layers[0][0].out_channels, m.downsample_layers[0][3].out_channels
    rows1, rows2 = B * (H // 2) * (W // 2), B * (H // 4) * (W // 4)
    bound = rows1 * 32 * 2 + rows1 * Cm * 2 + rows2 * Co * 2 + (8 << 20)
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.autocast("cuda", torch.bfloat16):
        y = m._run_downsample(m.downsample_layers[0], img)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"stem saved set: {grown / 1e6:.1f} MB (bound {bound / 1e6:.1f} MB)")
    assert y.requires_grad and tuple(y.shape) == (B, Co, H // 4, W // 4)
    assert grown <= bound, (grown, bound)


# ------------------------------------------------------------------------------------------------
# 7. frozen parameters
class _DwCalls:
    """(N, K) of the weight-gradient launches made through ops.linear_dw / ops.conv3x3s2_dw."""

    def __init__(self, monkeypatch):
        self.calls = []
        lin, conv = ops().linear_dw, ops().conv3x3s2_dw

        def linear_dw(probs, N, K, *a, **k):
            self.calls.append((N, K))
            return lin(probs, N, K, *a, **k)

        def conv3x3s2_dw(dy, x, dwm, dbias):
            self.calls.append(tuple(dwm.shape))
            return conv(dy, x, dwm, dbias)

        monkeypatch.setattr(ops(), "linear_dw", linear_dw)
        monkeypatch.setattr(ops(), "conv3x3s2_dw", conv3x3s2_dw)


def test_frozen_parameters(monkeypatch):
    img = det_tensor((2, 3, 96, 160), "frozenbn.dense.img", 6).to(DEV)
    calls = _DwCalls(monkeypatch)
    # bf16 autocast: the mode whose gradients reproduce bit for bit from run to run (the fp32 block kernels of stages 0 - 2 do not), so that
    # "unchanged bit for bit" compares this change and not the run-to-run spread of the cotangents that reach the transitions.
    # (K, N) of the weight-gradient GEMMs of the stem (K = 32; 9 * 32 padded to 320) and of the three transitions (9 * 64, 9 * 128, 9 * 192): no block launch has such a pair
    conv_k = {32: 32, 320: 64, 576: 128, 1152: 192, 1728: 320}

    def run(freeze_bn, freeze_conv):
        m = _backbone(TINY, 3, frozen_stages=[0]).train()
        for seq in m.downsample_layers:
            for mod in seq.modules():
                if isinstance(mod, torch.nn.BatchNorm2d) and freeze_bn or isinstance(mod, torch.nn.Conv2d) and freeze_conv:
                    mod.requires_grad_(False)
        calls.calls.clear()
        with torch.autocast("cuda", torch.bfloat16):
            outs = m(img)
        sum((o.float() ** 2).mean() for o in outs).backward()
        torch.cuda.synchronize()
        n = sum(1 for N, K in calls.calls if conv_k.get(K) == N)
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}, n

    g0, n0 = run(False, False)
    g1, n1 = run(True, False)
    g2, n2 = run(True, True)
    assert n0 == 5 and n1 == 5, (n0, n1)
    probe = Mod().LeMeViTBackbone(**TINY)
    kinds = {n: type(mod) for n, mod in probe.named_modules()}
    bn = [k for k in g0 if k.startswith("downsample_layers") and kinds[k.rsplit(".", 1)[0]] is torch.nn.BatchNorm2d]
    conv = [k for k in g0 if k.startswith("downsample_layers") and kinds[k.rsplit(".", 1)[0]] is torch.nn.Conv2d]
    assert len(bn) == 10 and len(conv) == 10, (bn, conv)
    assert all(g0[k] is not None for k in bn + conv)
    assert all(g1[k] is None for k in bn), "a BatchNorm parameter that does not require grad got a gradient"
    assert all(torch.equal(g0[k], g1[k]) for k in conv), "the convolution gradients moved when the BatchNorm parameters were frozen"
    assert not any(k.startswith("stages.0.") and g is not None for k, g in g1.items())
    assert all(g2[k] is None for k in bn + conv)
    assert n2 == 0, f"{n2} weight-gradient launches for frozen convolutions"
    rest = [k for k in g1 if k not in bn + conv and g1[k] is not None]
    assert rest and all(torch.equal(g1[k], g2[k]) for k in rest)


# ------------------------------------------------------------------------------------------------
# 8. determinism
def test_bf16_gradients_bit_identical_run_to_run():
    img = det_tensor((2, 3, 96, 160), "frozenbn.dense.img", 6).to(DEV)
    grads = []
    for _ in range(2):
        m = _backbone(TINY, 3).train()
        with torch.autocast("cuda", torch.bfloat16):
            outs = m(img)
        sum((o.float() ** 2).mean() for o in outs).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and any(k.startswith("downsample_layers.0.1.") for k in grads[0])
    bad = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not bad, f"gradients differ between two runs: {bad[:8]}"
