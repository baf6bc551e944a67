"""Dense-prediction losses and metrics on a real MI355X: lmv_dense_loss_fwd / lmv_dense_loss_bwd (csrc/dense.hip) and the surface built on them (lemevit_amd.dense)
against ``reference_dense``, the numpy float64 restatement that tests/test_dense_loss_cpu.py holds to the reference's own functions.  ``pred``, ``T_k``,
``n_valid`` and the confusion matrix are integers and must be equal.  Losses and ``I / P`` hold the bound tests/test_recipe_gpu.py uses for lmv_soft_ce:
max(2 x the error of PyTorch's own fp32 GPU evaluation of the same formulas on the same inputs against float64, 1e-6 max(1, |ref|)) -- the factor 2 because two
correct fp32 evaluations differ by their summation order.  fp32 ``dlogits``: the same rule with the floor 1e-6 x the largest |reference gradient| of the case
(gradients scale with 1 / D: an absolute floor would say nothing); bf16 ``dlogits``: 2^-8 |ref| on top of that (the rounding of the stored value).

The forward pass runs at most 1024 workgroups (DN_MAX_WG in csrc/dense.hip) of 256 threads (K <= 16), a thread owning 4 (fp32) or 8 (bf16) pixels: one sweep of the
grid covers 1 048 576 fp32 or 2 097 152 bf16 pixels.  BIG_SHAPE has 2 129 920: every thread of either dtype goes round its grid-stride loop more than once."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG_SHAPE = (2, 2, 1024, 1040)
SHAPES = [(1, 2, 1, 1), (2, 2, 5, 7), (3, 3, 16, 16), (1, 5, 33, 31), (2, 9, 6, 10), (2, 19, 24, 40), (1, 64, 9, 11), (8, 2, 256, 256), BIG_SHAPE]
SWEEP_PIXELS = {torch.float32: 1024 * 256 * 4, torch.bfloat16: 1024 * 256 * 8}
BIG = 1e30          # what the planes around the view are filled with


def Lm():
    import lemevit_amd
    return lemevit_amd


def Dn():
    from lemevit_amd import dense
    return dense


def weights(K):
    return [0.5 + 1.5 * k / (K - 1) for k in range(K)]


def modes(K):
    """(name, arguments): CE, CE with an ignore index INSIDE [0, K), focal gamma = 2 with alpha, dice only, jaccard only, the reference's hybrid, and all terms at
    once -- the three avg modes and both ignore conventions of the issue (255 and K) among them"""
    w = weights(K)
    return [("ce", dict(ignore_index=255, avg="valid")), ("ce-ignore-1", dict(ignore_index=1, avg="valid")),
            ("focal", dict(gamma=2.0, alpha=w, ignore_index=K, avg="weight")), ("dice", dict(ce=0.0, dice=1.0, ignore_index=255)),
            ("jaccard", dict(ce=0.0, jaccard=1.0, ignore_index=K)), ("hybrid", dict(ce=1.0, dice=1.0, ignore_index=255, avg="all")),
            ("everything", dict(ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha=w, ignore_index=K, avg="valid"))]


@functools.lru_cache(maxsize=None)
def inputs(shape, ldtype):
    """fp32 logits (randn x 3) and a label map with about a fifth of the pixels ignored: a tenth labelled 255, a tenth labelled K; int64 maps also hold the stray
    labels -1 and K + 3"""
    B, K, H, W = shape
    g = torch.Generator().manual_seed(B * 7919 + K * 131 + H * 17 + W)
    x = torch.randn(shape, generator=g) * 3
    y = torch.randint(0, K, (B, H, W), generator=g)
    r = torch.rand((B, H, W), generator=g)
    y[r < 0.1] = 255
    y[(r >= 0.1) & (r < 0.2)] = K
    if ldtype == torch.int64:
        y[(r >= 0.2) & (r < 0.21)] = -1
        y[(r >= 0.21) & (r < 0.22)] = K + 3
    return x, y.to(ldtype)


def on_device(x, layout):
    """contiguous, or the [:, 1:K+1] view of a [B, K + 2, H, W] buffer whose two other planes hold BIG"""
    if layout == "contiguous":
        return x.to(DEV)
    B, K, H, W = x.shape
    wide = torch.full((B, K + 2, H, W), BIG, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    v = wide.to(DEV)[:, 1:K + 1]
    assert not v.is_contiguous() or B == 1          # (one image: torch ignores the batch stride)
    return v


def torch_dense(x, y, ce=1.0, dice=0.0, jaccard=0.0, gamma=0.0, alpha=None, ignore_index=None, avg="valid", eps=1e-7):
    """The stated formulas in plain torch (the restatement of tests/test_dense_loss_cpu.py), differentiable, in the dtype and on the device of ``x``"""
    B, K = x.shape[:2]
    y = y.reshape(B, -1).long()
    valid = (y >= 0) & (y < K)
    if ignore_index is not None:
        valid &= y != ignore_index
    ys = torch.where(valid, y, torch.zeros_like(y))
    logp = F.log_softmax(x.reshape(B, K, -1), dim=1)
    p = logp.exp()
    logpt = logp.gather(1, ys[:, None])[:, 0]
    a = torch.ones(K, dtype=x.dtype, device=x.device) if alpha is None else torch.tensor(alpha, dtype=torch.float32).to(x.device, x.dtype)
    f = a[ys]
    if gamma > 0:
        f = f * (1 - logpt.detach().exp()) ** gamma
    vm = valid.to(x.dtype)
    onehot = F.one_hot(ys, K).permute(0, 2, 1).to(x.dtype) * vm[:, None]
    I, P, T = (p * onehot).sum((0, 2)), (p * vm[:, None]).sum((0, 2)), onehot.sum((0, 2))
    Dn_ = {"valid": vm.sum(), "all": torch.tensor(float(y.numel()), dtype=x.dtype, device=x.device), "weight": (a * T).sum()}[avg]
    ce_v = (f * -logpt * vm).sum() / Dn_ if float(Dn_) > 0 else (logpt * 0).sum()
    dice_v = 1 - (2 * I / (P + T + eps)).mean()
    jac_v = 1 - (I / (P + T - I + eps)).mean()
    return ce * ce_v + dice * dice_v + jaccard * jac_v, dict(ce=ce_v, dice=dice_v, jaccard=jac_v, I=I, P=P, T=T)


def op_kwargs(kw, K):
    o = dict(kw)
    o["w_ce"], o["w_dice"], o["w_jac"] = o.pop("ce", 1.0), o.pop("dice", 0.0), o.pop("jaccard", 0.0)
    if o.get("alpha") is not None:
        o["alpha"] = torch.tensor(o["alpha"], dtype=torch.float32, device=DEV)
    return o


def check_dense(name, xd, yd, x, y, kw, gout=None):
    """x: the host copy of the logits in their own dtype; kw: reference_dense's arguments.  Integers equal, everything else within the bound of the module
    docstring (the measured errors are printed next to the allowance); two calls agree bit for bit in every output."""
    ops = Lm().ops
    B, K, H, W = x.shape
    ref = Dn().reference_dense(x, y, gout=1.0 if gout is None else gout, **kw)
    xt = x.float().to(DEV).requires_grad_(True)
    t_loss, t_parts = torch_dense(xt, y.to(DEV), **kw)
    (t_loss * (1.0 if gout is None else gout)).backward()
    okw = op_kwargs(kw, K)
    gt = None if gout is None else torch.tensor(gout, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        pred = torch.full((B, H * W), 77, dtype=torch.uint8, device=DEV)
        conf = torch.zeros((K, K), dtype=torch.int64, device=DEV)
        meter = torch.zeros(2, dtype=torch.float64, device=DEV)
        stats = ops.dense_loss_fwd(xd, yd, pred=pred, conf=conf, meter=meter, **okw)
        dl = ops.dense_loss_bwd(xd, yd, stats, gout=gt, **okw)
        assert dl.dtype == x.dtype and tuple(dl.shape) == tuple(x.shape) and dl.is_contiguous() and tuple(stats.shape) == (6 + 5 * K,)
        runs.append((stats.cpu(), pred.cpu(), conf.cpu(), meter.cpu(), dl.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.bfloat16 else a.view(torch.int16), b.view(torch.uint8) if b.dtype != torch.bfloat16 else b.view(torch.int16)), \
            f"{name}: two calls differ"
    stats, pred, conf, meter, dl = runs[0]
    st = stats.double().numpy()
    # integers: equal
    assert np.array_equal(pred.numpy().reshape(B, H, W), ref["pred"]), name
    assert np.array_equal(st[6 + 4 * K:], ref["T"].astype(np.float64)) and st[4] == ref["n_valid"], (name, st[6 + 4 * K:], ref["T"])
    assert np.array_equal(conf.numpy(), ref["conf"]) and float(meter[1]) == ref["n_valid"], name
    # losses, I, P
    got = dict(loss=st[0], ce=st[1], dice=st[2], jaccard=st[3], I=st[6 + 2 * K:6 + 3 * K], P=st[6 + 3 * K:6 + 4 * K])
    tor = dict(loss=t_loss, **{k: t_parts[k] for k in ("ce", "dice", "jaccard", "I", "P")})
    for k, g in got.items():
        r = np.asarray(ref[k], dtype=np.float64)
        te = np.abs(tor[k].detach().double().cpu().numpy() - r)
        allow = np.maximum(2 * te, 1e-6 * np.maximum(1.0, np.abs(r)))
        err = np.abs(np.asarray(g) - r)
        print(f"dense {name} {k}: error {float(err.max()):.3e} (torch fp32 {float(te.max()):.3e}, allowed {float(allow.min()):.3e})")
        assert bool((err <= allow).all()), (name, k, float(err.max()), float(allow.min()))
    assert abs(st[5] - ref["inv_D"]) <= 2.0 ** -23 * ref["inv_D"], name
    assert abs(float(meter[0]) - ref["nll_sum"]) <= 1e-6 * max(1.0, ref["nll_sum"]), (name, float(meter[0]), ref["nll_sum"])          # the floor of the bound alone
    # dlogits
    rg = ref["dlogits"]
    gmax = float(np.abs(rg).max())
    te = float(np.abs(xt.grad.double().cpu().numpy() - rg).max())
    allow = np.full(rg.shape, max(2 * te, 1e-6 * gmax))
    if x.dtype == torch.bfloat16:
        allow = allow + 2.0 ** -8 * np.abs(rg)
    err = np.abs(dl.double().numpy() - rg)
    print(f"dense {name} dlogits: error {float(err.max()):.3e} of {gmax:.3e} (torch fp32 {te:.3e}, allowed {float(allow.min()):.3e})")
    assert bool((err <= allow).all()), (name, float(err.max()), float(allow.min()), gmax)
    ign = ~((y.reshape(B, -1).long() >= 0) & (y.reshape(B, -1).long() < K) & (y.reshape(B, -1).long() != kw.get("ignore_index", -1))).numpy()
    assert not dl.float().numpy().reshape(B, K, -1).transpose(0, 2, 1)[ign].any(), f"{name}: an ignored pixel has a gradient"
    return ref, stats, dl


@pytest.mark.parametrize("layout", ["contiguous", "view"])
@pytest.mark.parametrize("ldtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_loss(shape, dtype, ldtype, layout):
    B, K, H, W = shape
    x32, y = inputs(shape, ldtype)
    x = x32.to(dtype)
    if shape == BIG_SHAPE:
        assert B * H * W > SWEEP_PIXELS[dtype] and K <= 16          # more pixels than one sweep of the capped grid covers
    xd, yd = on_device(x, layout), y.to(DEV)
    npix = B * H * W
    for name, kw in modes(K):
        ref, _, _ = check_dense(f"{list(shape)} {dtype} {ldtype} {layout} {name}", xd, yd, x, y, kw, gout=0.4 if name == "everything" else None)
        if npix >= 256:
            assert 0.7 * B * H * W <= ref["n_valid"] < 0.9 * B * H * W or name == "ce-ignore-1"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_dense_loss_special_calls(dtype):
    """An all-ignored call (loss 0, zero gradient, nothing counted); an image of a single class (absent classes in dice and jaccard); logits at +-80."""
    ops = Lm().ops
    shape = (2, 3, 7, 9)
    x32, _ = inputs(shape, torch.int64)
    x = x32.to(dtype)
    xd = x.to(DEV)
    none = torch.full((2, 7, 9), 255, dtype=torch.int64)
    none[0, 0, :4] = torch.tensor([-1, 3, 6, 1 << 40])
    for kw in (dict(ignore_index=255), dict(ignore_index=255, avg="weight", alpha=weights(3), gamma=2.0), dict(ignore_index=255, avg="all")):
        ref, stats, dl = check_dense(f"all ignored {dtype} {kw}", xd, none.to(DEV), x, none, kw)
        assert ref["n_valid"] == 0 and stats[:2].tolist() == [0.0, 0.0] and float(stats[4]) == 0.0 and not dl.float().any() and not stats[6:].any()
        assert float(stats[5]) == (float(np.float32(1.0 / 126)) if kw.get("avg") == "all" else 0.0)          # D = B H W is not 0; the other two are
    one = torch.full((2, 7, 9), 1, dtype=torch.uint8)
    for kw in (dict(ce=0.0, dice=1.0), dict(ce=0.0, jaccard=1.0), dict(ce=1.0, dice=1.0, jaccard=1.0, avg="all")):
        ref, stats, dl = check_dense(f"single class {dtype} {kw}", xd, one.to(DEV), x, one, kw)
        assert ref["T"].tolist() == [0, 126, 0] and stats[6 + 2 * 3:6 + 3 * 3].tolist()[0::2] == [0.0, 0.0] and bool(torch.isfinite(dl.float()).all())
    g = torch.Generator().manual_seed(5)
    far = (torch.randint(0, 2, shape, generator=g).float() * 160 - 80).to(dtype)          # every logit is +80 or -80
    y = torch.randint(0, 3, (2, 7, 9), generator=g)
    for kw in (dict(), dict(gamma=2.0, alpha=weights(3), avg="weight"), dict(ce=1.0, dice=1.0, jaccard=0.5, avg="all")):
        ref, stats, dl = check_dense(f"+-80 {dtype} {kw}", far.to(DEV), y.to(DEV), far, y, kw)
        assert np.isfinite(ref["loss"]) and ref["ce"] > 10.0 and bool(torch.isfinite(stats).all()) and bool(torch.isfinite(dl.float()).all())


def test_argmax_rule_and_views_are_read_in_place():
    """NaN, signed zeros and ties in the argmax map (ignored pixels included); the two paths of the pass -- 16-byte loads and element loads -- give the same bits:
    the same planes at a 16-byte aligned and at a misaligned offset of one buffer."""
    ops = Lm().ops
    nan = float("nan")
    x = torch.tensor([[0.0, nan, 1.0, -0.0, 2.0, 2.0], [-0.0, nan, 1.0, 0.0, 2.0, -1.0], [0.0, 2.0, nan, -0.0, 1.0, 2.0]]).reshape(1, 3, 2, 3)
    y = torch.tensor([[[0, 1, 255, 2, 1, 0]]]).reshape(1, 2, 3)
    pred = torch.zeros((1, 6), dtype=torch.uint8, device=DEV)
    ops.dense_loss_fwd(x.to(DEV), y.to(DEV), pred=pred)
    want = Dn().reference_dense(x, y)["pred"].reshape(-1).tolist()
    assert want == [0, 0, 2, 0, 0, 0] and pred.cpu().reshape(-1).tolist() == want
    for dtype, K, HW in ((torch.float32, 3, 64), (torch.bfloat16, 5, 128), (torch.float32, 19, 32)):
        g = torch.Generator().manual_seed(K)
        planes = (torch.randn(2, K, 1, HW, generator=g) * 3).to(dtype)
        yv = torch.randint(0, K, (2, 1, HW), generator=g).to(DEV)
        buf = torch.full((2, K + 1, 1, HW), BIG, dtype=dtype, device=DEV)
        flat = buf.view(-1)
        outs = []
        for off in (0, 1):          # element offset 1: no plane is 16-byte aligned any more
            v = torch.as_strided(flat, (2, K, 1, HW), ((K + 1) * HW, HW, HW, 1), off)
            v.copy_(planes)
            kw = dict(w_ce=1.0, w_dice=1.0, w_jac=0.5, gamma=2.0)
            pred = torch.zeros((2, HW), dtype=torch.uint8, device=DEV)
            st = ops.dense_loss_fwd(v, yv, pred=pred, **kw)
            outs.append((st.cpu(), pred.cpu(), ops.dense_loss_bwd(v, yv, st, **kw).cpu()))
            flat.fill_(BIG)
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1]), (dtype, K)
        assert torch.equal(outs[0][2].view(torch.uint8), outs[1][2].view(torch.uint8)), (dtype, K)


class _Spy:
    """lib with every entry point wrapped: records the names it is called with"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, n):
        f = getattr(self._lib, n)

        def g(*a):
            self.calls.append(n)
            return f(*a)
        return g


def test_dense_loss_autograd(monkeypatch):
    """DenseLoss under autograd: backward() gives the ops-level dlogits bit for bit; (0.4 * loss).backward() and a two-element prediction list scale and sum as
    stated with ONE lmv_dense_loss_fwd and ONE lmv_dense_loss_bwd per prediction and no other library call; crit.last; the drop-ins equal DenseLoss with the
    corresponding settings; [B, 1, H, W] and uint8 targets."""
    L, dense, ops = Lm(), Dn(), Lm().ops
    shape = (2, 3, 16, 20)
    x32, y = inputs(shape, torch.int64)
    w = weights(3)
    xa = x32.to(DEV).requires_grad_(True)
    xb = on_device(x32.flip(0).bfloat16(), "view").detach().requires_grad_(True)
    yd = y.to(DEV)
    crit = dense.DenseLoss(ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha=w, ignore_index=255, avg="weight")
    okw = dict(ignore_index=255, alpha=torch.tensor(w, device=DEV), gamma=2.0, w_ce=0.7, w_dice=0.4, w_jac=0.5, avg="weight")
    loss = crit(xa, yd)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    loss.backward()
    st = ops.dense_loss_fwd(xa.detach(), yd, **okw)
    assert torch.equal(loss.detach().view(torch.int32), st[0].view(torch.int32))
    assert torch.equal(xa.grad.view(torch.int32), ops.dense_loss_bwd(xa.detach(), yd, st, **okw).view(torch.int32))
    assert sorted(crit.last) == ["ce", "dice", "jaccard", "n_valid"] and all(v.is_cuda and v.dim() == 0 for v in crit.last.values())
    assert [float(crit.last[k]) for k in ("ce", "dice", "jaccard", "n_valid")] == st[1:5].tolist()
    # a list of two predictions, scaled: three launches (two forward, one backward) per prediction, nothing else from the library
    xa.grad = None
    spy = _Spy(ops.lib)
    monkeypatch.setattr(ops, "lib", spy)
    total = crit([xa, xb], yd[:, None])
    (0.4 * total).backward()
    monkeypatch.undo()
    launches = [c for c in spy.calls if c != "lmv_dense_loss_workspace_bytes"]
    assert launches == ["lmv_dense_loss_fwd", "lmv_dense_loss_fwd", "lmv_dense_loss_bwd", "lmv_dense_loss_bwd"], spy.calls
    sb = ops.dense_loss_fwd(xb.detach(), yd, **okw)
    assert torch.equal(total.detach().view(torch.int32), (st[0] + sb[0]).view(torch.int32))
    g04 = torch.tensor(0.4, device=DEV)
    assert torch.equal(xa.grad.view(torch.int32), ops.dense_loss_bwd(xa.detach(), yd, st, gout=g04, **okw).view(torch.int32))
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad.view(torch.int16), ops.dense_loss_bwd(xb.detach(), yd, sb, gout=g04, **okw).view(torch.int16))
    # the drop-ins
    y8 = y.clamp(0, 2).to(torch.uint8).to(DEV)[:, None]          # the reference's functions know no ignored pixel

    def same(a, b):
        return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    xs = [xa.detach(), xb.detach()]
    assert same(dense.hybrid_loss(xs, y8), dense.DenseLoss(ce=1.0, dice=1.0, avg="all")(xs, y8))
    assert same(dense.dice_loss(xs[0], y8), dense.DenseLoss(ce=0.0, dice=1.0)(xs[0], y8)) and same(dense.dice_loss(xs[1], y8, eps=1e-3), dense.DenseLoss(ce=0.0, dice=1.0, eps=1e-3)(xs[1], y8))
    assert same(dense.jaccard_loss(xs[0], y8), dense.DenseLoss(ce=0.0, jaccard=1.0)(xs[0], y8))
    assert same(dense.FocalLoss(gamma=2, alpha=w)(xs[0], y8), dense.DenseLoss(gamma=2.0, alpha=w, avg="all")(xs[0], y8))
    assert same(dense.FocalLoss()(xs[1], y8), dense.DenseLoss(avg="all")(xs[1], y8))
    assert same(dense.FocalLoss(size_average=False)(xs[0], y8), dense.DenseLoss(avg="all")(xs[0], y8) * float(2 * 16 * 20))
    assert same(dense.DenseCrossEntropy(ignore_index=255, loss_weight=0.4, class_weight=w)(xs[0], yd), dense.DenseLoss(ce=0.4, alpha=w, ignore_index=255)(xs[0], yd))
    assert same(dense.DenseCrossEntropy(ignore_index=255, avg_non_ignore=False)(xs[1], yd), dense.DenseLoss(ignore_index=255, avg="all")(xs[1], yd))
    with pytest.raises(ValueError):
        crit(xa.detach().contiguous(memory_format=torch.channels_last), yd)
    with pytest.raises(ValueError):
        crit(xa.detach()[:, :2], yd)          # alpha holds three weights


def test_seg_meter(monkeypatch):
    """Three batches of different shapes (fp32 contiguous, a bf16 view, fp32 with uint8 labels) against the numpy matrix; compute() against the host formulas;
    meter= inside the loss call leaves the same state as a separate update; merge adds states; a known shape allocates nothing and copies nothing."""
    dense, ops = Dn(), Lm().ops
    K = 5
    batches = []
    for i, (shape, dtype, ldtype, layout) in enumerate([((2, K, 33, 31), torch.float32, torch.int64, "contiguous"), ((3, K, 16, 24), torch.bfloat16, torch.int64, "view"),
                                                        ((1, K, 40, 40), torch.float32, torch.uint8, "contiguous")]):
        x32, y = inputs(shape, ldtype)
        x = x32.to(dtype)
        batches.append((on_device(x, layout), y.to(DEV), x, y))
    meter = dense.SegMeter(K, ignore_index=255)
    conf, nll, n = np.zeros((K, K), dtype=np.int64), 0.0, 0
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a copy path was taken")))
    for xd, yd, x, y in batches:
        meter.update(xd, yd)
        ref = dense.reference_dense(x, y, ignore_index=255)
        assert meter.pred.dtype == torch.uint8 and np.array_equal(meter.pred.cpu().numpy(), ref["pred"])
        conf += ref["conf"]
        nll += ref["nll_sum"]
        n += ref["n_valid"]
    monkeypatch.undo()
    assert meter.conf.is_cuda and meter.conf.dtype == torch.int64 and np.array_equal(meter.conf.cpu().numpy(), conf)
    assert meter.loss.dtype == torch.float64 and float(meter.loss[1]) == n and abs(float(meter.loss[0]) - nll) <= 1e-6 * nll
    got, want = meter.compute(), dense.seg_metrics(conf, (float(meter.loss[0]), float(n)))
    assert list(got) == ["loss", "aAcc", "IoU", "Acc", "Precision", "F1", "mIoU", "mAcc", "count"] and got["count"] == n
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True), k
    tp = np.diag(conf).astype(np.float64)
    assert got["aAcc"] == tp.sum() / conf.sum() and np.array_equal(got["IoU"], tp / (conf.sum(0) + conf.sum(1) - tp)) and abs(got["mIoU"] - float(np.mean(got["IoU"]))) <= 1e-15
    # a known shape allocates nothing
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    meter.update(batches[0][0], batches[0][1])
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    # meter= inside the loss call == a separate update
    xd, yd, x, y = batches[1]
    a, b = dense.SegMeter(K, ignore_index=255), dense.SegMeter(K, ignore_index=255)
    crit = dense.DenseLoss(ce=1.0, dice=1.0, ignore_index=255)
    plain = crit(xd, yd)
    with_meter = crit([batches[1][0], xd], yd, meter=a)          # the meter sees the last prediction of a list, once
    b.update(xd, yd)
    assert torch.equal(a.conf, b.conf) and torch.equal(a.loss.view(torch.int64), b.loss.view(torch.int64)) and torch.equal(a.pred, b.pred)
    assert torch.equal(with_meter.view(torch.int32), (plain + plain).view(torch.int32))
    with pytest.raises(ValueError, match="must agree"):
        dense.DenseLoss()(xd, yd, meter=a)
    # merge adds states; two classes give eval.py's numbers
    m = dense.SegMeter(K, ignore_index=255).merge([a.state, b.state, (b.conf.cpu(), b.loss.cpu())])
    assert torch.equal(m.conf, 3 * a.conf) and torch.equal(m.loss, 3 * a.loss)
    x2, y2 = inputs((2, 2, 5, 7), torch.uint8)
    m2 = dense.SegMeter(2)
    m2.update(x2.to(DEV), y2.to(DEV))
    r2 = dense.reference_dense(x2, y2)
    c2 = m2.compute()
    assert (c2["tn"], c2["fp"], c2["fn"], c2["tp"]) == tuple(int(v) for v in r2["conf"].reshape(-1)) and c2["count"] == r2["n_valid"]
    with pytest.raises(ValueError):
        m2.update(batches[0][0], batches[0][1])          # five classes


def test_seg_meter_captured():
    """After one eager update, meter.update(static_logits, static_labels) is captured on one stream (no parallel branches); three replays over refilled static
    tensors leave the state of an eager meter over the same three batches exactly.  Capture without the eager update raises."""
    dense = Dn()
    shape = (2, 5, 33, 31)
    x, y = inputs(shape, torch.int64)
    batches = [(x, y), (x.flip(0).contiguous(), y.flip(0).contiguous()), (x.roll(7, 3), y.roll(3, 2))]
    eager = dense.SegMeter(5, ignore_index=255)
    for xb, yb in batches:
        eager.update(xb.to(DEV), yb.to(DEV))
    sx, sy = torch.zeros_like(x, device=DEV), torch.zeros_like(y, device=DEV)
    cold, other = dense.SegMeter(5, ignore_index=255), dense.SegMeter(5, ignore_index=255)
    other.update(sx[:1], sy[:1])          # a state, but no buffers for this shape
    meter = dense.SegMeter(5, ignore_index=255)
    meter.update(sx, sy)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="eager update first"):          # (raised before anything is allocated or launched: the capture goes on)
            cold.update(sx, sy)
        with pytest.raises(RuntimeError, match="eager update first"):
            other.update(sx, sy)
        meter.update(sx, sy)
    for xb, yb in batches:
        sx.copy_(xb)
        sy.copy_(yb)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(meter.conf, eager.conf) and torch.equal(meter.loss.view(torch.int64), eager.loss.view(torch.int64)), (meter.loss.tolist(), eager.loss.tolist())
    assert int(meter.conf.sum()) == int(meter.loss[1]) > 0
