"""Native mixup / cutmix (lmv_mix_images) and the fused soft-target cross-entropy (lmv_soft_ce) on a real MI355X, against a float64 restatement of timm's
formulas (x * lam + x.flip(0) * (1 - lam) / the pasted box; mixup_target; sum(-t * log_softmax(x)).mean()) written here in plain torch on the CPU; then
autograd through the loss modules, one LeMeViT-Tiny train step and a captured step whose replays mix differently."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def Lm():
    import lemevit_amd
    return lemevit_amd


def R():
    from lemevit_amd import recipe
    return recipe


# ================================================================================================================================================
# lmv_mix_images
# ================================================================================================================================================
SHAPES = [(6, 3, 20, 30), (5, 4, 17, 33), (6, 3, 17, 33), (5, 4, 20, 30)]          # C H W = 1800 / 2244 / 1683 / 2400: 16-byte stores for both / fp32 only / neither / both


def tables(B, H, W):
    """Two hand-made tables.  A: mixup 0.3 | interior box | box in the top-left corner | identity (its partner has a box: different records within a pair) |
    w = 0 | the whole image.  B: one pixel | a full row band | mixup 0.3 (the middle image of B = 5: mixed with itself) | box in the bottom-right corner |
    w = 1 without a box | box touching the top and the right border."""
    a = [(0.3, 0, 0, 0, 0, 0.3), (1.0, 5, 12, 7, 19, 0.6), (1.0, 0, 6, 0, 9, 0.9), (1.0, 0, 0, 0, 0, 1.0), (0.0, 0, 0, 0, 0, 0.0), (1.0, 0, H, 0, W, 0.0)]
    b = [(1.0, 3, 4, 5, 6, 0.99), (1.0, 4, 9, 0, W, 0.7), (0.3, 0, 0, 0, 0, 0.3), (1.0, H - 5, H, W - 7, W, 0.8), (1.0, 0, 0, 0, 0, 1.0), (1.0, 0, 5, W - 4, W, 0.9)]
    return [R().make_records(t[:B]) for t in (a, b)]


@functools.lru_cache(maxsize=None)
def images(shape, kind):
    """The same values in every layout (computed once): contiguous, channels-last, and a slice with W stride 2."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H)
    if kind == torch.uint8:
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    else:
        x = torch.randn(shape, generator=g).clamp_(-4.0, 4.0).to(kind)
    wide = torch.zeros((B, C, H, 2 * W + 1), dtype=x.dtype)
    wide[..., 1::2] = x
    xd = x.to(DEV)
    return x, dict(contiguous=xd, channels_last=xd.contiguous(memory_format=torch.channels_last), sliced=wide.to(DEV)[..., 1::2])


def mix_reference(x, rec, scale, shift):
    """float64: inside the box the partner, elsewhere w * self + (1 - w) * partner; then * scale + shift; and the mask of the pixels that take ONE image as it is"""
    B, C, H, W = x.shape
    x64 = x.double()
    p64 = x64.flip(0)
    out = torch.empty_like(x64)
    copy_of = torch.zeros(x.shape, dtype=torch.int8)          # 1: a copy of the image itself, 2: a copy of the partner, 0: computed
    yy, xx = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    for b in range(B):
        r = rec[b]
        w = float(r["w"])
        box = (yy >= int(r["yl"])) & (yy < int(r["yh"])) & (xx >= int(r["xl"])) & (xx < int(r["xh"]))
        out[b] = torch.where(box, p64[b], w * x64[b] + (1.0 - w) * p64[b])
        copy_of[b] = torch.where(box, 2, 1 if w == 1.0 else 0).to(torch.int8).expand(C, H, W)
    if scale is not None:
        out = out * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    return out, copy_of


AFFINE_F = ([0.5, 0.75, 1.0, 0.25], [-0.5, 0.25, 1.0, 0.0])                                                  # |scale| <= 1: the rounding of the mix is not amplified
AFFINE_U8 = ([1 / (255 * s) for s in (0.229, 0.224, 0.225, 0.25)], [-m / s for m, s in zip((0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25))])   # PrefetchLoader on 0..255 data


@pytest.mark.parametrize("in_dtype", [torch.uint8, torch.float32, torch.bfloat16], ids=["u8", "f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_images(shape, in_dtype):
    """Every layout x output type x (with / without scale and shift) x both tables against float64.  Bounds, derived: the fp32 result is three roundings of
    w * a + (1 - w) * b (1 - w, the product, the fused sum) and one more for the affine map, each <= 2^-24 of a term no larger than max(1, |ref|) once
    |scale| <= 1 (0..255 data: the terms reach 255, the scale is ~1 / 58): |err| <= 2^-21 max(1, |ref|); a bf16 result adds one rounding: 2^-8 |ref| + 2^-21.
    Where a pixel takes one image as it is (box, or w == 1), with equal dtypes and no affine map, it is a copy.  Two launches agree bit for bit; the input
    is left alone."""
    ops = Lm().ops
    B, C, H, W = shape
    host, layouts = images(shape, in_dtype)
    aff = AFFINE_U8 if in_dtype == torch.uint8 else AFFINE_F
    scale, shift = (torch.tensor(v[:C], dtype=torch.float32) for v in aff)
    worst = {}
    for rec in tables(B, H, W):
        packed = R().pack_records(rec)
        table = packed.to(DEV)
        refs = {False: mix_reference(host, rec, None, None), True: mix_reference(host, rec, scale, shift)}
        for lname, x in layouts.items():
            assert (lname == "contiguous") == x.is_contiguous()
            before = x.clone()
            for out_dtype in (torch.float32, torch.bfloat16):
                for affine in (False, True):
                    kw = dict(scale=scale.to(DEV), shift=shift.to(DEV)) if affine else {}
                    out = ops.mix_images(x, table, out_dtype, records=packed, **kw)
                    again = ops.mix_images(x, table, out_dtype, **kw)
                    assert out.shape == x.shape and out.dtype == out_dtype and out.is_contiguous() and torch.equal(out, again)
                    ref, copy_of = refs[affine]
                    err = (out.double().cpu() - ref).abs()
                    bound = 2.0 ** -21 * ref.abs().clamp(min=1.0) if out_dtype == torch.float32 else 2.0 ** -8 * ref.abs() + 2.0 ** -21
                    key = (str(out_dtype)[6:], affine)
                    worst[key] = max(worst.get(key, 0.0), float((err / bound).max()))
                    assert bool((err <= bound).all()), (lname, out_dtype, affine, float((err / bound).max()))
                    if not affine and out_dtype == in_dtype:
                        oc, hp = out.cpu(), host.flip(0)
                        assert torch.equal(oc[copy_of == 1], host[copy_of == 1]) and torch.equal(oc[copy_of == 2], hp[copy_of == 2])
            assert torch.equal(x, before)
    print(f"mix_images {shape} {in_dtype}: worst error / bound {worst}")


def test_mix_images_default_dtype_and_errors():
    ops = Lm().ops
    rec = R().pack_records(R().make_records([(1.0, 0, 0, 0, 0, 1.0)] * 2))
    x = torch.zeros(2, 3, 4, 6, device=DEV)
    assert ops.mix_images(x.to(torch.uint8), rec.to(DEV)).dtype == torch.float32 and ops.mix_images(x.bfloat16(), rec.to(DEV)).dtype == torch.bfloat16
    with pytest.raises(TypeError):
        ops.mix_images(x.half(), rec.to(DEV))
    with pytest.raises(TypeError):
        ops.mix_images(x, rec.to(DEV)[:1])
    bad = R().pack_records(R().make_records([(1.0, 0, 5, 0, 3, 1.0)] * 2))          # yh = 5 > H = 4
    with pytest.raises(RuntimeError, match="outside"):
        ops.mix_images(x, bad.to(DEV), records=bad)


# ================================================================================================================================================
# lmv_soft_ce
# ================================================================================================================================================
CE_SHAPES = [(1, 10), (6, 51), (5, 1000), (4, 1003)]
LAMS = [0.0, 0.37, 1.0, 0.62, 0.25, 0.9]


@functools.lru_cache(maxsize=None)
def ce_inputs(B, N, dtype, scaled):
    g = torch.Generator().manual_seed(B * 7919 + N)
    x = torch.randn((B, N), generator=g) * (1.0 if not scaled else 30.0)
    if scaled:
        x = x.clamp_(-80.0, 80.0)
        x[0, 0], x[0, N - 1] = 80.0, -80.0
    x = x.to(dtype)
    labels = torch.randint(0, N, (B,), generator=g)
    if B > 1:
        labels[B - 1] = labels[0]                       # row 0 and its partner carry the same label
    dense = torch.softmax(torch.randn((B, N), generator=g) * 2.0, dim=-1).float()          # a random row-stochastic target
    Np = (N + 7) // 8 * 8 if N % 8 else N + 8
    padded = torch.full((B, Np), 7.0, dtype=dtype)      # (the padding is not part of the logits: whatever it holds must not matter)
    padded[:, :N] = x
    rec = R().make_records([(1.0, 0, 0, 0, 0, lt) for lt in LAMS[:B]])
    return x, labels, dense, padded, rec


def ce_reference(x, t64):
    """float64 on the already rounded logits: per-row losses, their mean, d mean / d logits"""
    x64 = x.double()
    logp = F.log_softmax(x64, dim=-1)
    row = -(t64 * logp).sum(-1)
    grad = (logp.exp() * t64.sum(-1, keepdim=True) - t64) / x.shape[0]
    return row, row.mean(), grad


def torch_fp32_error(x, t64, ref_loss, ref_grad):
    """PyTorch's own fp32 GPU log_softmax-based soft-target loss and gradient on the same inputs: its distance from float64"""
    xg = x.float().to(DEV).requires_grad_(True)
    loss = torch.sum(-t64.float().to(DEV) * F.log_softmax(xg, dim=-1), dim=-1).mean()
    loss.backward()
    return abs(float(loss.detach().double().cpu()) - float(ref_loss)), float((xg.grad.double().cpu() - ref_grad).abs().max())


def check_ce(name, x_dev, x_host, t64, run, dtype):
    """run(want_grad) -> (loss, row, dlogits); the checks of the module docstring of this section"""
    ref_row, ref_loss, ref_grad = ce_reference(x_host, t64)
    te_loss, te_grad = torch_fp32_error(x_host, t64, ref_loss, ref_grad)
    loss, row, dlog = run(True)
    loss2, row2, dlog2 = run(True)
    loss0, row0, none = run(False)
    assert none is None and torch.equal(loss0, loss) and torch.equal(row0, row)
    assert torch.equal(loss, loss2) and torch.equal(row, row2) and torch.equal(dlog, dlog2)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and row.dtype == torch.float32 and dlog.dtype == dtype and dlog.is_contiguous()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(row).all()) and bool(torch.isfinite(dlog.float()).all())
    e_loss = abs(float(loss.double().cpu()) - float(ref_loss))
    e_row = (row.double().cpu() - ref_row).abs()
    allow_loss = max(2 * te_loss, 1e-6 * max(1.0, abs(float(ref_loss))))
    allow_row = torch.maximum(torch.full_like(ref_row, 2 * te_loss), 1e-6 * ref_row.abs().clamp(min=1.0))
    e_grad = (dlog.double().cpu() - ref_grad).abs()
    if dtype == torch.float32:
        allow_grad = torch.maximum(torch.full_like(ref_grad, 2 * te_grad), 1e-6 * ref_grad.abs().clamp(min=1.0))
    else:
        allow_grad = 2.0 ** -8 * ref_grad.abs() + 1e-7
    print(f"soft_ce {name}: loss error {e_loss:.3e} (torch fp32 {te_loss:.3e}, allowed {allow_loss:.3e}); dlogits error {float(e_grad.max()):.3e} (torch fp32 {te_grad:.3e}), "
          f"worst error / allowed {float((e_grad / allow_grad).max()):.3f}")
    assert e_loss <= allow_loss
    assert bool((e_row <= allow_row).all()), float((e_row / allow_row).max())
    assert bool((e_grad <= allow_grad).all()), float((e_grad / allow_grad).max())
    assert abs(float(row.double().mean().cpu()) - float(loss.double().cpu())) <= (1e-6 if abs(float(ref_loss)) < 16.0 else 1e-6 * abs(float(ref_loss)))          # (+-80 logits: relative)


def mixed_target64(labels, lam, N, s):
    off = s / N
    on = 1.0 - s + off
    B = labels.shape[0]

    def one_hot(y):
        return torch.full((B, N), off, dtype=torch.float64).scatter_(1, y.view(B, 1), on)
    lam = torch.as_tensor(lam, dtype=torch.float64).view(B, 1)
    return one_hot(labels) * lam + one_hot(labels.flip(0)) * (1.0 - lam)


@pytest.mark.parametrize("layout", ["contiguous", "padded"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N", CE_SHAPES)
def test_soft_ce(B, N, dtype, layout):
    """Sparse form with the table (lam_t 0 / 0.37 / 1 / ..., a row whose partner has its label, smoothing 0 and 0.1), without it (= F.cross_entropy with
    label_smoothing), and the dense form on a random row-stochastic target; contiguous logits and the [:, :N] view of a buffer padded to the next multiple of 8
    (the classifier tail's layout).  fp32 dlogits and all losses: within max(2 x the error of PyTorch's fp32 GPU log_softmax-based loss / gradient on the same
    inputs, 1e-6 max(1, |ref|)); bf16 dlogits: one bf16 rounding, 2^-8 |ref| + 1e-7."""
    ops = Lm().ops
    x, labels, dense, padded, rec = ce_inputs(B, N, dtype, False)
    xd = x.to(DEV) if layout == "contiguous" else padded.to(DEV)[:, :N]
    assert layout == "contiguous" or B == 1 or not xd.is_contiguous()
    yd, table = labels.to(DEV), R().pack_records(rec).to(DEV)
    lam = rec["lam_t"].astype("float64")
    for s in (0.0, 0.1):
        check_ce(f"[{B}, {N}] {dtype} {layout} table s={s}", xd, x, mixed_target64(labels, lam, N, s),
                 lambda g: ops.soft_ce(xd, labels=yd, table=table, smoothing=s, want_grad=g), dtype)
        t_plain = mixed_target64(labels, [1.0] * B, N, s)
        check_ce(f"[{B}, {N}] {dtype} {layout} labels s={s}", xd, x, t_plain, lambda g: ops.soft_ce(xd, labels=yd, smoothing=s, want_grad=g), dtype)
        ce64 = F.cross_entropy(x.double(), labels, label_smoothing=s)
        assert abs(float(ce_reference(x, t_plain)[1]) - float(ce64)) <= 1e-12 * max(1.0, float(ce64))          # the restatement IS F.cross_entropy in float64
    for tdt in (torch.float32, torch.bfloat16):
        t = dense.to(tdt)
        check_ce(f"[{B}, {N}] {dtype} {layout} dense {tdt}", xd, x, t.double(), lambda g: ops.soft_ce(xd, target=t.to(DEV), want_grad=g), dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_soft_ce_large_logits_and_stray_labels(dtype):
    """Logits scaled to +-80: the log-sum-exp is taken around the row maximum, everything stays finite and inside the same bounds.  A label outside [0, N)
    carries no one-hot mass (MixedTarget.dense() says the same) and is never used as an index."""
    ops = Lm().ops
    B, N = 6, 51
    x, labels, dense, padded, rec = ce_inputs(B, N, dtype, True)
    xd, yd, table = padded.to(DEV)[:, :N], labels.to(DEV), R().pack_records(rec).to(DEV)
    lam = rec["lam_t"].astype("float64")
    check_ce(f"+-80 {dtype} table", xd, x, mixed_target64(labels, lam, N, 0.1), lambda g: ops.soft_ce(xd, labels=yd, table=table, smoothing=0.1, want_grad=g), dtype)
    check_ce(f"+-80 {dtype} dense", xd, x, dense.double(), lambda g: ops.soft_ce(xd, target=dense.to(DEV), want_grad=g), dtype)
    stray = labels.clone()
    stray[1], stray[3] = N, -3          # (their partners, rows 4 and 2, keep valid labels)
    t64 = R().MixedTarget(stray, R().pack_records(rec), 0.1, N).dense(torch.float64)
    assert abs(float(t64[1].sum()) - (0.1 + 0.9 * (1 - LAMS[1]))) < 1e-6          # row 1 keeps the smoothing floor and its partner's share only
    x1, _, _, p1, _ = ce_inputs(B, N, dtype, False)
    x1d = p1.to(DEV)[:, :N]
    check_ce(f"stray labels {dtype}", x1d, x1, t64, lambda g: ops.soft_ce(x1d, labels=stray.to(DEV), table=table, smoothing=0.1, want_grad=g), dtype)


# ================================================================================================================================================
# autograd, the model, capture
# ================================================================================================================================================
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_through_the_loss_modules(dtype):
    """A leaf logits tensor, upstream gradient 0.5: logits.grad == dlogits * 0.5 exactly; reduction='none' rows and their gradient; logits that do not require
    grad take the loss-only form; the three target forms agree with each other."""
    L, ops = Lm(), Lm().ops
    B, N = 6, 51
    x, labels, dense, padded, rec = ce_inputs(B, N, dtype, False)
    yd, table = labels.to(DEV), R().pack_records(rec).to(DEV)
    tgt = L.MixedTarget(yd, table, 0.1, N)
    leaf = padded.to(DEV).requires_grad_(True)
    loss = L.SoftTargetCrossEntropy()(leaf[:, :N], tgt)
    (loss * 0.5).backward()
    want_loss, want_row, dlog = ops.soft_ce(leaf.detach()[:, :N], labels=yd, table=table, smoothing=0.1)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(leaf.grad[:, :N], dlog * 0.5) and float(leaf.grad[:, N:].abs().max()) == 0.0
    assert loss.requires_grad and loss.dtype == torch.float32
    frozen = L.SoftTargetCrossEntropy()(leaf.detach()[:, :N], tgt)
    assert not frozen.requires_grad and torch.equal(frozen, want_loss)
    leaf2 = x.to(DEV).requires_grad_(True)
    rows = L.SoftTargetCrossEntropy(reduction="none")(leaf2, tgt)
    assert torch.equal(rows.detach(), want_row)
    gr = torch.linspace(0.5, 1.5, B, device=DEV)
    (rows * gr).sum().backward()
    want = dlog.float() * (gr * B).view(B, 1)
    assert float((leaf2.grad.float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    d1 = L.SoftTargetCrossEntropy()(x.to(DEV), tgt.dense().to(DEV))
    assert abs(float(d1) - float(want_loss)) <= 1e-5 * max(1.0, abs(float(want_loss)))
    ls = L.LabelSmoothingCrossEntropy(0.1)(x.to(DEV), yd)
    ref = F.cross_entropy(x.double(), labels, label_smoothing=0.1)
    assert abs(float(ls) - float(ref)) <= 1e-5 * max(1.0, float(ref))
    plain = L.SoftTargetCrossEntropy()(x.to(DEV), yd)
    assert abs(float(plain) - float(F.cross_entropy(x.double(), labels))) <= 1e-5 * max(1.0, float(ref))


def _tiny():
    torch.manual_seed(0)
    return Lm().create_model("lemevit_tiny", num_classes=51, drop_path_rate=0.0).to(DEV).train()


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(5)
    return torch.randn((4, 3, 64, 64), generator=g).to(DEV), torch.tensor([3, 50, 17, 3], device=DEV)


def _loss64(logits, t64):
    return float(ce_reference(logits.detach().cpu(), t64)[1])


def test_train_step_with_mixup_and_native_loss():
    """One LeMeViT-Tiny step (51 classes, 64 x 64, B = 4, bf16 autocast) with Mixup + SoftTargetCrossEntropy against the same step with the float64-derived dense
    target and PyTorch's log_softmax-based soft-target loss on the same mixed images.  Loss: each side against float64 on its own logits, the native error within
    max(2 x PyTorch's, 1e-6 max(1, |ref|)).  Head-weight gradient: within 3e-2 of its max-abs, the budget tests/test_model_gpu.py gives bf16 gradients
    (test_block_backward_bf16_vs_oracle; the two sides differ by bf16 roundings of dlogits, up to 2^-8 relative per term)."""
    L = Lm()
    m = _tiny()
    x, y = _batch()
    mix = L.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=51, seed=3)
    xm, tgt = mix(x, y)
    assert xm.shape == x.shape and not torch.equal(xm, x) and tgt.table is mix.table
    rec = mix.records.numpy().view(R().RECORD_DTYPE).reshape(-1)
    t64 = mixed_target64(y.cpu(), rec["lam_t"].astype("float64"), 51, 0.1)
    assert float((tgt.dense(torch.float64).cpu() - t64).abs().max()) <= 1e-12
    with torch.autocast("cuda", torch.bfloat16):
        la = m(xm)
        loss_a = L.SoftTargetCrossEntropy()(la, tgt)
    assert la.dtype == torch.bfloat16 and not la.is_contiguous()          # the [:, :51] view of the 56-column padded logits
    loss_a.backward()
    ga = m.head.weight.grad.detach().clone()
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", torch.bfloat16):
        lb = m(xm)
        loss_b = torch.sum(-t64.float().to(DEV) * F.log_softmax(lb.float(), dim=-1), dim=-1).mean()
    loss_b.backward()
    gb = m.head.weight.grad.detach().clone()
    ref_a, ref_b = _loss64(la, t64), _loss64(lb, t64)
    err_a, err_b = abs(float(loss_a) - ref_a), abs(float(loss_b) - ref_b)
    gerr = float((ga - gb).abs().max()) / float(gb.abs().max())
    print(f"train step: native loss {float(loss_a):.7f} (error {err_a:.3e}), torch loss {float(loss_b):.7f} (error {err_b:.3e}); head-weight gradient difference {gerr:.3e} of max-abs")
    assert err_a <= max(2 * err_b, 1e-6 * max(1.0, abs(ref_a)))
    assert torch.isfinite(ga).all() and float(gb.abs().max()) > 0 and gerr <= 3e-2


def test_captured_step_mixes_differently_at_every_replay():
    """GraphedStep over {mix, forward, loss, backward, FlatAdamW.step} with before_replay=mix.draw: two replays with different seeded draws.  Each replay's loss
    equals the loss of an eager forward from the parameters that replay started from and the records it drew -- the same kernels on the same inputs: within
    1e-6 max(1, |loss|), the floor of the fp32 bound -- while the records of the capture give another loss there: the table is read, not baked in."""
    L, ops = Lm(), Lm().ops
    from lemevit_amd.graph import GraphedStep
    m = _tiny()
    opt = L.FlatAdamW(m, lr=1e-3, eps=1e-3, weight_decay=0.05)
    x, y = _batch()
    mix = L.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=51, seed=11)
    crit = L.SoftTargetCrossEntropy()
    out = torch.zeros((), device=DEV)

    def forward(table):
        with torch.autocast("cuda", torch.bfloat16):
            return crit(m(ops.mix_images(x, table)), L.MixedTarget(y, table, 0.1, 51))

    def step():
        opt.zero_grad(set_to_none=True)
        xm, tgt = mix(x, y)
        with torch.autocast("cuda", torch.bfloat16):
            loss = crit(m(xm), tgt)
        loss.backward()
        opt.step()
        out.copy_(loss.detach())

    g = GraphedStep(step, warmup=1, before_replay=mix.draw)
    captured = mix.records.clone()
    runs = []
    for _ in range(2):
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        g()
        torch.cuda.synchronize()
        runs.append((start, mix.records.clone(), float(out)))
    ops.check_stage_errors("graph replay", sync=False)
    assert not torch.equal(runs[0][1], runs[1][1]) and not torch.equal(runs[0][1], captured)
    assert runs[0][2] != runs[1][2]
    for k, (start, records, loss) in enumerate(runs):
        m.load_state_dict(start)
        eager = float(forward(records.to(DEV)))
        stale = float(forward(captured.to(DEV)))
        print(f"replay {k}: captured loss {loss:.7f}, eager loss with the same records {eager:.7f}, with the records of the capture {stale:.7f}")
        assert abs(loss - eager) <= 1e-6 * max(1.0, abs(eager))
        assert abs(loss - stale) > 1e-4 * max(1.0, abs(eager)), "control: the records of the capture must give another loss"
