"""Image gradients and in_chans != 3 on a real MI355X: the patch-matrix kernel for any channel count and the one-launch data gradient of the first stem
convolution (csrc/conv1.hip) through the C ABI against float64 restatements on identical operands, then the model paths that reach them: the train step with an
image that requires grad (reference fixtures and the CPU oracle), other channel counts, the checkpointed stem, the dense backbone.

Kernel tolerances are those of tests/test_ops_gpu.py (fp32 1e-5, bf16 1e-3 of the output's max-abs; one bf16 rounding of the OUTPUT on top where the output is stored
in bf16): lmv_conv3x3s2_nchw_dx has no rounded intermediate, so the 4e-3 of the two-launch convolution gradient does not apply.  Model tolerances are
test_train_step_fp32's (logits 2e-5, gradients 2e-4, gradient norms 1e-3, running statistics 1e-5)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from detfill import det_tensor, fill_state_dict, sample
from oracle import lemevit_oracle as O

DEV = "cuda:0"
FIRST = "downsample_layers.0.0.weight"
DTYPES = [torch.float32, torch.bfloat16]


def L():
    import lemevit_amd
    return lemevit_amd


def ops():
    from lemevit_amd import ops as _ops
    return _ops


def kernel_close(out, ref, compute, what):
    """test_ops_gpu.assert_close with the output rounding allowed only where the output IS bf16."""
    out_bf16 = out.dtype == torch.bfloat16
    out = out.detach().to("cpu", torch.float64)
    ref = ref.to(torch.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out).all(), what + ": non-finite output"
    mx = max(float(ref.abs().max()), 1e-30)
    err = (out - ref).abs()
    bound = (1e-5 if compute == torch.float32 else 1e-3) * mx + (ref.abs() * 2.0 ** -8 if out_bf16 else 0.0)
    bad = err > bound
    print(f"{what}: max-abs err {float(err.max()) / mx:.2e} of max-abs")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {float((err - bound).max()):.3e} over (max-abs {mx:.3e})"


def close(out, ref, tol, what):
    out = np.asarray(out.detach().float().cpu().numpy() if torch.is_tensor(out) else out, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.isfinite(out).all(), what
    mx = max(np.abs(ref).max(), 1e-30)
    err = np.abs(out - ref).max() / mx
    print(f"{what}: rel max-abs err {err:.2e}")
    assert err <= tol, f"{what}: max-abs err {err:.3e} > {tol:.0e} of {mx:.3e}"


def shapes(cin):
    return [(1, cin, 97, 131), (3, cin, 8, 5), (2, cin, 1, 7), (2, cin, 12, 9)]          # odd x odd, tiny, one row, H even / W odd


def kp_of(cin):
    return (9 * cin + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------
# 5. the patch matrix
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", [1, 2, 4, 6, 13])
def test_im2col_nchw(dtype, cin):
    o = ops()
    for shape in shapes(cin):
        B, _, H, W = shape
        x = det_tensor(shape, "img", 5).to(DEV)
        KP = kp_of(cin)
        for src in (x, x.contiguous(memory_format=torch.channels_last), x.to(torch.bfloat16)):
            p = o.im2col3x3s2_nchw(src, dtype)
            want = F.unfold(src.double(), 3, padding=1, stride=2).transpose(1, 2).reshape(-1, 9 * cin)
            assert p.shape == (B * ((H + 1) // 2) * ((W + 1) // 2), KP) and p.dtype == dtype
            assert torch.equal(p[:, :9 * cin].double().cpu(), want.to(dtype).double().cpu()), ("patch values", shape)
            assert not bool(p[:, 9 * cin:].any()), "padding columns must be zero"
        p = o.im2col3x3s2_nchw(x, dtype, KP + 32)          # a wider KP: more zero columns
        assert p.shape[1] == KP + 32 and not bool(p[:, 9 * cin:].any())
        Co = 48
        w = det_tensor((Co, cin, 3, 3), "w", 5, 0.3).to(DEV); b = det_tensor((Co,), "b", 5, 0.1).to(DEV)
        wm = torch.zeros(Co, KP, device=DEV, dtype=dtype); wm[:, :9 * cin] = w.reshape(Co, 9 * cin).to(dtype)
        p = o.im2col3x3s2_nchw(x, dtype)
        y = torch.empty(p.shape[0], Co, device=DEV, dtype=dtype)
        o.linear_fwd([o.Prob(p, wm, y, bias=b)], Co, KP)
        conv = F.conv2d(x.to(dtype).double().cpu(), w.to(dtype).double().cpu(), b.double().cpu(), stride=2, padding=1)
        kernel_close(y, conv.permute(0, 2, 3, 1).reshape(-1, Co), dtype, f"conv1 as GEMM {shape}")


# ------------------------------------------------------------------------------------------------
# 6. the data gradient
def _dx_abi(dy, wm, out):
    from lemevit_amd._lib import lib, check
    o = ops()
    B, cin, H, W = out.shape
    sb, sc, sh, sw = out.stride()
    check(lib.lmv_conv3x3s2_nchw_dx(dy.data_ptr(), wm.data_ptr(), out.data_ptr(), o.dtype_code(out), B, cin, H, W, wm.shape[0], wm.shape[1], sb, sc, sh, sw, o.dtype_code(dy),
                                    torch.cuda.current_stream().cuda_stream), "lmv_conv3x3s2_nchw_dx")
    return out


def _dx_case(dtype, shape, Co):
    B, cin, H, W = shape
    Ho, Wo, KP = (H + 1) // 2, (W + 1) // 2, kp_of(cin)
    dy = det_tensor((B, Co, Ho, Wo), "dy", 7).to(dtype)                      # NCHW-shaped values of the output gradient
    w = det_tensor((Co, cin, 3, 3), "w", 7, 0.3).to(dtype)
    ref = torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), stride=2, padding=1)          # float64, the identical (rounded) operands
    g = dy.permute(0, 2, 3, 1).reshape(-1, Co).contiguous().to(DEV)
    wm = torch.zeros(Co, KP, dtype=dtype); wm[:, :9 * cin] = w.reshape(Co, 9 * cin)
    wm = wm.to(DEV)
    first = None
    for odt in DTYPES:
        for fmt in (torch.contiguous_format, torch.channels_last):
            out = torch.full(shape, float("nan"), device=DEV, dtype=odt).contiguous(memory_format=fmt)
            _dx_abi(g, wm, out)
            assert not bool(torch.isnan(out).any()), f"{shape} Co={Co}: elements left unwritten"
            kernel_close(out, ref, dtype, f"dx {shape} Co={Co} {dtype} -> {odt} {fmt}")
            again = _dx_abi(g, wm, torch.full(shape, float("nan"), device=DEV, dtype=odt).contiguous(memory_format=fmt))
            assert torch.equal(out, again), "two launches must agree bit for bit"
            if odt == torch.float32:
                first = out if first is None else first
                assert torch.equal(first, out), "the memory format of dx must not change its values"
    like = torch.empty(shape, device=DEV).contiguous(memory_format=torch.channels_last)
    dx = ops().conv3x3s2_nchw_dx(g, wm, like=like)
    assert dx.shape == like.shape and dx.dtype == like.dtype and dx.stride() == like.stride() and torch.equal(dx, first)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Co", [8, 32, 48])
@pytest.mark.parametrize("cin", [1, 3, 4, 13, 31])
def test_conv3x3s2_nchw_dx(dtype, cin, Co):
    for shape in shapes(cin):
        _dx_case(dtype, shape, Co)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3x3s2_nchw_dx_image_size(dtype):
    _dx_case(dtype, (2, 3, 224, 224), 48)
    _dx_case(dtype, (1, 4, 70, 38), 64)          # several tiles with ragged edges on both axes, Co = 64


# ------------------------------------------------------------------------------------------------
# 7. the autograd node
@pytest.mark.parametrize("cin", [3, 4])
def test_stem_conv1_node_with_and_without_image_grad(monkeypatch, cin):
    import lemevit_amd.model as M
    o = ops()
    calls = []
    real = o.conv3x3s2_nchw_dx
    monkeypatch.setattr(o, "conv3x3s2_nchw_dx", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    Co = 48
    x = det_tensor((3, cin, 50, 38), "x", 3).to(DEV)
    gy = det_tensor((3, Co, 25, 19), "gy", 3).to(DEV).to(torch.bfloat16)
    res = []
    for need in (False, True):
        w = det_tensor((Co, cin, 3, 3), "w", 3, 0.3).to(DEV).requires_grad_(True)
        b = det_tensor((Co,), "b", 3, 0.1).to(DEV).requires_grad_(True)
        xi = x.clone().requires_grad_(need)
        M.new_training_pass()
        y = M._conv3x3s2(xi, w, b, torch.bfloat16)
        n0 = len(calls)
        y.backward(gy)
        assert len(calls) - n0 == (1 if need else 0), "exactly one data-gradient launch, and only when the image asks for it"
        res.append((y.detach(), w.grad, b.grad, xi.grad))
    (y0, dw0, db0, dx0), (y1, dw1, db1, dx1) = res
    assert torch.equal(y0, y1) and torch.equal(dw0, dw1) and torch.equal(db0, db1) and dx0 is None
    assert dx1.shape == x.shape and dx1.dtype == x.dtype
    wq = det_tensor((Co, cin, 3, 3), "w", 3, 0.3).to(torch.bfloat16).double()
    ref = torch.nn.grad.conv2d_input(x.shape, wq, gy.double().cpu(), stride=2, padding=1)
    kernel_close(dx1, ref, torch.bfloat16, "node dx")


@pytest.mark.parametrize("shape,Co,form", [((3, 3, 50, 38), 48, "image"), ((3, 4, 50, 38), 48, "image"), ((2, 8, 5, 6), 16, "patch"), ((64, 64, 9, 7), 128, "implicit")])
def test_frozen_plain_convolution_keeps_no_gather(monkeypatch, shape, Co, form):
    """One saved-set rule for every form of the convolution node: a plain convolution whose weight and bias are frozen gives the same y and dX bit for bit, launches no
    weight-gradient GEMM and keeps neither its patch matrix nor (implicit form) its NHWC map for the backward pass; a trainable one keeps it."""
    import lemevit_amd.model as M
    o = ops()
    dw_calls = []
    for name in ("linear_dw", "conv3x3s2_dw"):
        monkeypatch.setattr(o, name, lambda *a, _real=getattr(o, name), **k: (dw_calls.append(1), _real(*a, **k))[1])
    B, cin, H, W = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    KP = kp_of(cin) if cin % 8 else (9 * cin + 63) // 64 * 64
    x = det_tensor(shape, "x", 3).to(DEV)
    if form != "image":
        assert o.conv3x3s2_implicit_ok(x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous(), Co, KP) == (form == "implicit")
    gather = (B, H, W, cin) if form == "implicit" else (B * Ho * Wo, KP)
    gy = det_tensor((B, Co, Ho, Wo), "gy", 3).to(DEV).to(torch.bfloat16)
    res = []
    for trainable in (True, False):
        w = det_tensor((Co, cin, 3, 3), "w", 3, 0.3).to(DEV).requires_grad_(trainable)
        b = det_tensor((Co,), "b", 3, 0.1).to(DEV).requires_grad_(trainable)
        xi = x.clone().requires_grad_(True)
        M.new_training_pass()
        y = M._conv3x3s2(xi, w, b, torch.bfloat16)
        assert y.grad_fn.form == form
        kept = [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
        n0 = len(dw_calls)
        y.backward(gy)
        res.append((y.detach(), xi.grad, w.grad, b.grad, kept, len(dw_calls) - n0))
    (y1, dx1, dw1, db1, kept1, n1), (y0, dx0, dw0, db0, kept0, n0) = res
    assert gather in kept1 and n1 == 1 and dw1 is not None and db1 is not None, "the trainable convolution keeps its gather for ONE weight-gradient launch"
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and dx0.shape == x.shape
    assert n0 == 0, "a frozen convolution launches no weight-gradient GEMM"
    assert gather not in kept0, f"a frozen convolution keeps its gather: {kept0}"
    assert dw0 is None and db0 is None


# ------------------------------------------------------------------------------------------------
# 8. / 9. the model against the reference's fixtures
def _model(variant, num_classes, seed, **kw):
    m = L().create_model(variant, num_classes=num_classes, **kw)
    spec = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(fill_state_dict(spec, seed))
    return m.to(DEV)


def _check_train_fixture(m, meta, g, logits, loss):
    close(logits, g["logits"], 2e-5, "logits")
    assert abs(loss.item() - float(g["loss"])) < 2e-5
    params = dict(m.named_parameters())
    gn = np.array([float(params[k].grad.norm()) if params[k].grad is not None else 0.0 for k in meta["param_names"]])
    bad = np.abs(gn - g["grad_norms"]) > 1e-3 * np.maximum(1.0, np.abs(g["grad_norms"]))
    assert not bad.any(), [(meta["param_names"][i], gn[i], g["grad_norms"][i]) for i in np.nonzero(bad)[0][:5]]
    for k in g:
        if k.startswith("grad.") and k != "grad_norms":
            close(params[k[5:]].grad, g[k], 2e-4, k)
        if k.startswith("stat."):
            close(m.state_dict()[k[5:]], g[k], 1e-5, k)


def test_image_gradient_fp32_train(golden):
    meta, g = golden("inputgrad_tiny_96")
    tmeta, t = golden("train_tiny_96")
    m = _model("lemevit_tiny", 10, meta["seed"], drop_path_rate=0.0).train()
    img = det_tensor((4, 3, 96, 96), meta["img"], meta["img_seed"]).to(DEV).requires_grad_(True)
    logits = m(img)
    loss = F.cross_entropy(logits, torch.tensor(meta["target"], device=DEV))
    loss.backward()
    assert img.grad is not None and img.grad.shape == img.shape and img.grad.dtype == torch.float32
    close(img.grad, g["dimg"], 2e-4, "img.grad")
    close(dict(m.named_parameters())[FIRST].grad, g["grad." + FIRST], 2e-4, "grad " + FIRST)
    _check_train_fixture(m, tmeta, t, logits, loss)


def test_image_gradient_does_not_move_the_bf16_step():
    """bf16 (the fp32 step does not reproduce itself bit for bit in stages 0 - 2): logits, loss and every parameter gradient are the same bits whether or
    not the image requires grad."""
    outs = []
    for need in (False, True):
        m = _model("lemevit_tiny", 10, 41, drop_path_rate=0.0).train()
        img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5).to(DEV).requires_grad_(need)
        with torch.autocast("cuda", torch.bfloat16):
            logits = m(img)
            loss = F.cross_entropy(logits, torch.tensor([1, 7, 3, 3], device=DEV))
        loss.backward()
        outs.append((logits.detach(), loss.detach(), {k: p.grad for k, p in m.named_parameters()}, img.grad))
    (l0, s0, g0, d0), (l1, s1, g1, d1) = outs
    assert torch.equal(l0, l1) and torch.equal(s0, s1) and d0 is None and d1 is not None and torch.isfinite(d1).all() and float(d1.abs().max()) > 0
    for k in g0:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]), k


def test_image_gradient_fp32_eval(golden):
    meta, g = golden("inputgrad_tiny_96_eval")
    m = _model("lemevit_tiny", 10, meta["seed"], drop_path_rate=0.0).eval()
    img = det_tensor((4, 3, 96, 96), meta["img"], meta["img_seed"]).to(DEV).requires_grad_(True)
    logits = m(img)
    logits[:, torch.tensor(meta["target"], device=DEV)].sum().backward()
    close(logits, g["logits"], 2e-5, "logits")
    close(img.grad, g["dimg"], 2e-4, "img.grad")


def _oracle_train(meta, img_cpu, num_classes):
    cfg = O.VARIANTS[meta["variant"]]
    sd = fill_state_dict(O.state_dict_spec(cfg, num_classes, in_chans=img_cpu.shape[1]), meta["seed"])
    for k, v in sd.items():
        if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
    x = img_cpu.clone().requires_grad_(True)
    logits = O.lemevit_forward(sd, cfg, x, train=True)
    F.cross_entropy(logits, torch.tensor(meta["target"])).backward()
    return logits.detach(), x.grad, sd


@pytest.mark.parametrize("name", ["train_tiny_c4_96", "train_tiny_c13_96"])
def test_in_chans_train_step_fp32(golden, name):
    meta, g = golden(name)
    cin = meta["in_chans"]
    m = _model("lemevit_tiny", 10, meta["seed"], in_chans=cin, drop_path_rate=0.0).train()
    img_cpu = det_tensor((meta["B"], cin, 96, 96), name + ".img", 5)
    img = img_cpu.to(DEV).requires_grad_(True)
    logits = m(img)
    loss = F.cross_entropy(logits, torch.tensor(meta["target"], device=DEV))
    loss.backward()
    dimg_ref = g.pop("dimg")
    _check_train_fixture(m, meta, g, logits, loss)
    close(sample(img.grad, meta["dimg_sampled"]) if meta["dimg_sampled"] else img.grad, dimg_ref, 2e-4, "img.grad vs the reference")
    _, dref, _ = _oracle_train(meta, img_cpu, 10)
    close(img.grad, dref, 2e-4, "img.grad (full) vs the oracle")


def test_one_channel_inference(golden):
    meta, g = golden("model_tiny_c1_224")
    m = _model("lemevit_tiny", 1000, meta["seed"], in_chans=1).eval()
    img = det_tensor((1, 1, 224, 224), "model_tiny_c1_224.img", 4).to(DEV)
    with torch.no_grad():
        close(m(img), g["logits"], 1e-5, "fp32 logits")
        with torch.autocast("cuda", torch.bfloat16):
            close(m(img).float(), g["logits"], 3e-2, "bf16 no-grad logits (folded per-launch stem)")


def test_in_chans_8_routes_to_the_nhwc_convolution():
    meta = dict(variant="lemevit_tiny", seed=41, target=[1, 7])
    m = _model("lemevit_tiny", 10, 41, in_chans=8, drop_path_rate=0.0).train()
    img_cpu = det_tensor((2, 8, 96, 96), "c8.img", 5)
    img = img_cpu.to(DEV).requires_grad_(True)
    logits = m(img)
    F.cross_entropy(logits, torch.tensor([1, 7], device=DEV)).backward()
    lref, dref, sd = _oracle_train(meta, img_cpu, 10)
    close(logits, lref, 2e-5, "logits")
    close(img.grad, dref, 2e-4, "img.grad")
    close(dict(m.named_parameters())[FIRST].grad, sd[FIRST].grad, 2e-4, "grad " + FIRST)


def test_in_chans_33_is_refused():
    m = L().create_model("lemevit_tiny", num_classes=10, in_chans=33).to(DEV).train()
    with pytest.raises(NotImplementedError, match="1 .. 32 input channels"):
        m(torch.zeros(1, 33, 64, 64, device=DEV))


# ------------------------------------------------------------------------------------------------
# 10. the headline configuration
def test_base_224_bf16_image_gradient_vs_oracle():
    """Base 224 x 224, bf16 autocast, train mode, reference initialisation, B = 4 (test_base_224_bf16_gradients_vs_oracle's set-up) with an image that requires grad, against the
    oracle's fp32 autograd.  Bounds: that test's whole-gradient rel-L2 3e-2 and cosine 0.9995, and the end-to-end bf16 max-abs bound 5e-2; the reference's own bf16 autocast
    against its own fp32 on this case gives rel-L2 2.27e-2, cosine 0.99976, max-abs 2.17e-2."""
    cfg = O.VARIANTS["lemevit_base"]
    torch.manual_seed(0)
    m = L().create_model("lemevit_base", num_classes=1000, drop_path_rate=0.0).to(DEV).train()
    img = det_tensor((4, 3, 224, 224), "basegrad.img", 5)
    tgt = torch.tensor([3, 141, 592, 653])
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x = img.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        loss = F.cross_entropy(m(x), tgt.to(DEV))
    loss.backward()
    xr = img.clone().requires_grad_(True)
    ref_loss = F.cross_entropy(O.lemevit_forward(sd, cfg, xr, train=True), tgt)
    ref_loss.backward()
    gq, r = x.grad.detach().float().cpu().double(), xr.grad.double()
    assert torch.isfinite(gq).all()
    l2 = float((gq - r).norm() / r.norm())
    cos = float(F.cosine_similarity(gq.flatten(), r.flatten(), dim=0))
    mx = float((gq - r).abs().max() / r.abs().max())
    print(f"Base 224 bf16 image gradient vs oracle: rel-L2 {l2:.2e}, cosine {cos:.5f}, max-abs {mx:.2e} of max-abs; loss {loss.item():.5f} vs {ref_loss.item():.5f}")
    assert l2 <= 3e-2 and cos >= 0.9995 and mx <= 5e-2, (l2, cos, mx)


# ------------------------------------------------------------------------------------------------
# 11. the checkpointed stem
def test_checkpointed_stem_gives_the_image_gradient(golden):
    _, g = golden("inputgrad_tiny_96")

    def run(ck, bf16):
        m = _model("lemevit_tiny", 10, 41, drop_path_rate=0.0, use_checkpoint_stages=ck).train()
        img = det_tensor((4, 3, 96, 96), "train_tiny_96.img", 5).to(DEV).requires_grad_(True)
        with torch.autocast("cuda", torch.bfloat16, enabled=bf16):
            logits = m(img)
            loss = F.cross_entropy(logits, torch.tensor([1, 7, 3, 3], device=DEV))
        loss.backward()
        return logits.detach(), img.grad, {k: p.grad for k, p in m.named_parameters()}

    (l0, d0, g0), (l1, d1, g1) = run([], True), run([0, 1, 2, 3, 4], True)
    assert torch.equal(l0, l1) and torch.equal(d0, d1), "checkpointing must not change a bit of the bf16 step"
    for k in g0:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]), k
    _, d32, _ = run([0, 1, 2, 3, 4], False)
    close(d32, g["dimg"], 2e-4, "img.grad, fp32, every stage checkpointed")


# ------------------------------------------------------------------------------------------------
# 12. the dense backbone
def test_dense_backbone_in_chans_4(golden):
    from lemevit_amd.model import LeMeViTBackbone
    meta, _ = golden("dense_tiny_160x96")
    cfg = meta["cfg"]
    m = LeMeViTBackbone(in_chans=4, **cfg)
    spec = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = fill_state_dict(spec, meta["seed"])
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    img_cpu = det_tensor((2, 4, 160, 96), "dense_c4.img", 6)
    img = img_cpu.to(DEV).requires_grad_(True)
    outs = m(img)
    xr = img_cpu.clone().requires_grad_(True)
    refs = O.lemevit_dense_forward(sd, cfg, xr)
    gs = [det_tensor(tuple(r.shape), f"dense_c4.g{i}", 6) for i, r in enumerate(refs)]
    sum((o * gi.to(DEV)).sum() for o, gi in zip(outs, gs)).backward()
    sum((r * gi).sum() for r, gi in zip(refs, gs)).backward()
    assert len(outs) == 4
    for i, (o, r) in enumerate(zip(outs, refs)):
        close(o, r, 1e-5, f"out{i}")
    close(img.grad, xr.grad, 2e-4, "img.grad")
