"""The dense losses on LOW-RESOLUTION logits on a real MI355X: lmv_dense_up_loss_fwd / lmv_dense_up_loss_bwd (csrc/dense.hip) and the surface built on them
(``DenseLoss(upsample=True)``, ``SegMeter(upsample=True)``, ``predict``) against ``reference_dense(upsample=)``, the numpy float64 oracle that
tests/test_dense_up_cpu.py holds to PyTorch's own float64 ``F.interpolate`` and autograd.

Integers (``T_k``, ``n_valid``, ``meter[1]``) must be equal.  ``pred`` must equal the oracle's at every pixel whose oracle margin (top-1 minus top-2 interpolated
logit) is at least 1e-4 max(1, |top logit|) -- an fp32 interpolation cannot order two logits closer than its own rounding; the pixels left out may be at most 0.5 %
of a case.  ``conf`` must equal the histogram of (label, the device's own pred) exactly.  Losses, ``I``, ``P`` and ``meter[0]`` hold the bound of
tests/test_dense_loss_gpu.py: max(2 x the error of PyTorch's own fp32 GPU evaluation -- fp32 ``F.interpolate``, then the stated formulas -- against float64,
1e-6 max(1, |ref|)); ``dlogits`` the same with the floor 1e-6 x the largest |reference gradient|, plus 2^-8 |ref| for a bf16 result (its rounding).

Shapes: CASES together reach the register path (K <= 5) and the generic one, whole and partial chunks of 4 output pixels, label rows at odd alignments
(W = 37), integer and non-integer ratios, 16 x, the clamps of a 1 x 1 input and of equal sizes, several backward tiles with neighbours on all sides
(40 x 44 input: 5 x 6 tiles of 8 x 8), K = 64 (the backward pass then reads its taps from global memory: the logits tile no longer fits into LDS next to the
rest; every other case stages it), and more chunks than one sweep of the capped forward grid takes (1024 workgroups x 256 threads x 4 pixels = 1 048 576 <
4 x 512 x 544)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dense_loss_gpu import BIG, DEV, op_kwargs, torch_dense, weights

pytestmark = pytest.mark.gpu

# (B, K, h, w), (H, W), align_corners
CASES = [((2, 2, 8, 8), (32, 32), True), ((2, 5, 7, 9), (28, 36), False), ((2, 5, 7, 9), (28, 36), True), ((2, 5, 7, 9), (30, 37), False),
         ((1, 6, 5, 6), (80, 96), False), ((1, 19, 3, 4), (12, 16), False), ((1, 3, 1, 1), (4, 4), False), ((1, 3, 8, 8), (8, 8), False),
         ((1, 3, 40, 44), (160, 176), False), ((1, 64, 9, 11), (36, 44), False), ((4, 2, 128, 136), (512, 544), True)]
BIG_CASE = CASES[-1]


def case_id(c):
    return "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])) + ("-ac" if c[2] else "")


def Lm():
    import lemevit_amd
    return lemevit_amd


def Dn():
    from lemevit_amd import dense
    return dense


def modes(K):
    w = weights(K)
    return [("ce", dict(ignore_index=255, avg="valid"), None), ("hybrid", dict(ce=1.0, dice=1.0, ignore_index=255, avg="all"), None),
            ("everything", dict(ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha=w, ignore_index=K, avg="valid"), 0.4)]


@functools.lru_cache(maxsize=None)
def inputs(shape, size, ldtype):
    """fp32 logits (randn x 3) and a label map as tests/test_dense_loss_gpu.py draws it: a tenth labelled 255, a tenth labelled K; int64 maps also hold the stray
    labels -1 and K + 3"""
    B, K, h, w = shape
    H, W = size
    g = torch.Generator().manual_seed(B * 7919 + K * 131 + h * 17 + w + H * 3 + W)
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
    """contiguous, or the [:, 1:K+1] view of a [B, K + 2, h, w] buffer whose two other planes hold BIG"""
    if layout == "contiguous":
        return x.to(DEV)
    B, K, h, w = x.shape
    wide = torch.full((B, K + 2, h, w), BIG, dtype=x.dtype)
    wide[:, 1:K + 1] = x
    return wide.to(DEV)[:, 1:K + 1]


@functools.lru_cache(maxsize=None)
def expected(shape, size, align, dtype, ldtype, mode):
    """(the float64 oracle, the errors of PyTorch's fp32 GPU evaluation of the same thing against it): computed once, shared by both layouts, never modified"""
    K = shape[1]
    x32, y = inputs(shape, size, ldtype)
    x = x32.to(dtype)
    name, kw, gout = [m for m in modes(K) if m[0] == mode][0]
    ref = Dn().reference_dense(x, y, upsample=size, align_corners=align, gout=1.0 if gout is None else gout, **kw)
    xt = x.float().to(DEV).requires_grad_(True)          # (a bf16 input: its values in fp32, interpolated in fp32 and not rounded back -- what the kernels do)
    zt = F.interpolate(xt, size=size, mode="bilinear", align_corners=align)
    t_loss, t_parts = torch_dense(zt, y.to(DEV), **kw)
    (t_loss * (1.0 if gout is None else gout)).backward()
    yl = y.to(DEV).long().reshape(shape[0], -1)
    valid = (yl >= 0) & (yl < K) & (yl != kw["ignore_index"])
    logp = F.log_softmax(zt.detach().reshape(shape[0], K, -1), dim=1).gather(1, torch.where(valid, yl, torch.zeros_like(yl))[:, None])[:, 0]
    tor = dict(loss=t_loss, nll_sum=-(logp * valid).sum(), **{k: t_parts[k] for k in ("ce", "dice", "jaccard", "I", "P")})
    te = {k: np.abs(v.detach().double().cpu().numpy() - np.asarray(ref[k], dtype=np.float64)) for k, v in tor.items()}
    te["dlogits"] = float(np.abs(xt.grad.double().cpu().numpy() - ref["dlogits"]).max())
    return ref, te


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.uint8)


def check_up(name, xd, yd, x, y, size, align, ref, te, kw, gout):
    ops = Lm().ops
    B, K, h, w = x.shape
    H, W = size
    okw = op_kwargs(kw, K)
    gt = None if gout is None else torch.tensor(gout, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        pred = torch.full((B, H * W), 77, dtype=torch.uint8, device=DEV)
        conf = torch.zeros((K, K), dtype=torch.int64, device=DEV)
        meter = torch.zeros(2, dtype=torch.float64, device=DEV)
        stats = ops.dense_up_loss_fwd(xd, yd, align, pred=pred, conf=conf, meter=meter, **okw)
        dl = ops.dense_up_loss_bwd(xd, yd, stats, align, gout=gt, **okw)
        assert dl.dtype == x.dtype and tuple(dl.shape) == tuple(x.shape) and dl.is_contiguous() and tuple(stats.shape) == (6 + 5 * K,)
        runs.append((stats.cpu(), pred.cpu(), conf.cpu(), meter.cpu(), dl.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(bits(a), bits(b)), f"{name}: two calls differ"
    stats, pred, conf, meter, dl = runs[0]
    st = stats.double().numpy()
    # integers: equal
    assert np.array_equal(st[6 + 4 * K:], ref["T"].astype(np.float64)) and st[4] == ref["n_valid"] and float(meter[1]) == ref["n_valid"], (name, st[6 + 4 * K:], ref["T"])
    # pred: equal wherever the oracle's margin is decisive
    top = ref["z"].max(1)
    decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(top))
    share = 1.0 - float(decisive.mean())
    p = pred.numpy().reshape(B, H, W)
    print(f"dense_up {name} pred: {100 * share:.4f} % of the pixels left out, {int((p != ref['pred'])[decisive].sum())} differ")
    assert share <= 0.005, (name, share)
    assert np.array_equal(p[decisive], ref["pred"][decisive]), name
    # conf: the histogram of (label, the device's own pred) over the valid pixels
    yl = y.long().numpy().reshape(B, H, W)
    valid = (yl >= 0) & (yl < K) & (yl != kw["ignore_index"])
    want = np.bincount(yl[valid] * K + p[valid].astype(np.int64), minlength=K * K).reshape(K, K)
    assert np.array_equal(conf.numpy(), want), name
    # losses, I, P, meter[0]
    got = dict(loss=st[0], ce=st[1], dice=st[2], jaccard=st[3], I=st[6 + 2 * K:6 + 3 * K], P=st[6 + 3 * K:6 + 4 * K], nll_sum=float(meter[0]))
    for k, g in got.items():
        r = np.asarray(ref[k], dtype=np.float64)
        allow = np.maximum(2 * te[k], 1e-6 * np.maximum(1.0, np.abs(r)))
        err = np.abs(np.asarray(g) - r)
        print(f"dense_up {name} {k}: error {float(err.max()):.3e} (torch fp32 {float(te[k].max()):.3e}, allowed {float(allow.min()):.3e})")
        assert bool((err <= allow).all()), (name, k, float(err.max()), float(allow.min()))
    assert abs(st[5] - ref["inv_D"]) <= 2.0 ** -23 * ref["inv_D"], name
    # dlogits
    rg = ref["dlogits"]
    gmax = float(np.abs(rg).max())
    allow = np.full(rg.shape, max(2 * te["dlogits"], 1e-6 * gmax))
    if x.dtype == torch.bfloat16:
        allow = allow + 2.0 ** -8 * np.abs(rg)
    err = np.abs(dl.double().numpy() - rg)
    print(f"dense_up {name} dlogits: error {float(err.max()):.3e} of {gmax:.3e} (torch fp32 {te['dlogits']:.3e}, allowed {float(allow.min()):.3e})")
    assert bool((err <= allow).all()), (name, float(err.max()), float(allow.min()), gmax)


@pytest.mark.parametrize("layout", ["contiguous", "view"])
@pytest.mark.parametrize("ldtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_up_loss(case, dtype, ldtype, layout):
    shape, size, align = case
    B, K, h, w = shape
    if case == BIG_CASE:
        assert B * size[0] * size[1] > 1024 * 256 * 4 and K <= 16          # more output pixels than one sweep of the capped grid covers
    x32, y = inputs(shape, size, ldtype)
    x = x32.to(dtype)
    xd, yd = on_device(x, layout), y.to(DEV)
    for mode, kw, gout in modes(K):
        ref, te = expected(shape, size, align, dtype, ldtype, mode)
        check_up(f"{case_id(case)} {dtype} {ldtype} {layout} {mode}", xd, yd, x, y, size, align, ref, te, kw, gout)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4], CASES[8]], ids=case_id)
def test_ignored_pixels_give_no_gradient(case, dtype):
    """A label map that is ignored everywhere outside ONE output row: dlogits is exact zero on every input row that this row's two taps do not touch."""
    ops, dense = Lm().ops, Dn()
    shape, size, align = case
    B, K, h, w = shape
    x32, y = inputs(shape, size, torch.int64)
    for Y in (0, size[0] // 2 + 1, size[0] - 1):
        only = torch.full_like(y, 255)
        only[:, Y] = y[:, Y].clamp(0, K - 1)
        taps = np.nonzero(dense._up_matrix(size[0], h, align)[Y])[0]
        src = (Y + 0.5) * h / size[0] - 0.5
        assert not align and (src < 0 or abs(src - round(src)) > 1e-3), "choose a row whose taps do not depend on rounding"
        xd, yd = x32.to(dtype).to(DEV), only.to(DEV)
        kw = dict(w_ce=1.0, w_dice=1.0, ignore_index=255)
        st = ops.dense_up_loss_fwd(xd, yd, align, **kw)
        dl = ops.dense_up_loss_bwd(xd, yd, st, align, **kw).float().cpu()
        rows = torch.ones(h, dtype=torch.bool)
        rows[torch.as_tensor(taps)] = False
        assert float(st[4]) == B * size[1] and bool(dl[:, :, ~rows].any())
        assert not bool(dl[:, :, rows].any()), (case_id(case), Y, taps)


def test_dense_loss_upsample_autograd():
    """DenseLoss(upsample=True) under autograd gives ops.dense_up_loss_bwd's result bit for bit; a list with one low-resolution and one full-resolution prediction
    sums both (the second through the plain kernels); the drop-ins match the oracle; upsample=False still refuses a size mismatch."""
    dense, ops = Dn(), Lm().ops
    shape, size = (2, 3, 10, 12), (40, 48)
    x32, y = inputs(shape, size, torch.int64)
    w = weights(3)
    yd = y.to(DEV)
    xa = x32.to(DEV).requires_grad_(True)
    xf = torch.randn((2, 3) + size, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    crit = dense.DenseLoss(ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha=w, ignore_index=255, avg="weight", upsample=True, align_corners=True)
    okw = dict(ignore_index=255, alpha=torch.tensor(w, device=DEV), gamma=2.0, w_ce=0.7, w_dice=0.4, w_jac=0.5, avg="weight")
    loss = crit(xa, yd)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (0.4 * loss).backward()
    st = ops.dense_up_loss_fwd(xa.detach(), yd, True, **okw)
    g04 = torch.tensor(0.4, device=DEV)
    assert torch.equal(loss.detach().view(torch.int32), st[0].view(torch.int32))
    assert tuple(xa.grad.shape) == shape and torch.equal(xa.grad.view(torch.int32), ops.dense_up_loss_bwd(xa.detach(), yd, st, True, gout=g04, **okw).view(torch.int32))
    ref = dense.reference_dense(x32, y, ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha=w, ignore_index=255, avg="weight", upsample=size, align_corners=True)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
    # a list: low resolution + full resolution, bf16 low resolution in a view
    xa.grad = None
    xb = on_device(x32.flip(0).bfloat16(), "view").detach().requires_grad_(True)
    total = crit([xa, xf, xb], yd[:, None])
    total.backward()
    sf = ops.dense_loss_fwd(xf.detach(), yd, **okw)
    sb = ops.dense_up_loss_fwd(xb.detach(), yd, True, **okw)
    assert torch.equal(total.detach().view(torch.int32), (st[0] + sf[0] + sb[0]).view(torch.int32))
    assert torch.equal(xa.grad.view(torch.int32), ops.dense_up_loss_bwd(xa.detach(), yd, st, True, **okw).view(torch.int32))
    assert torch.equal(xf.grad.view(torch.int32), ops.dense_loss_bwd(xf.detach(), yd, sf, **okw).view(torch.int32))
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad.view(torch.int16), ops.dense_up_loss_bwd(xb.detach(), yd, sb, True, **okw).view(torch.int16))
    # the drop-ins against the oracle
    y8 = y.clamp(0, 2).to(torch.uint8)
    for ac in (False, True):
        got = dense.hybrid_loss([xa.detach(), xf.detach()], y8.to(DEV)[:, None], upsample=True, align_corners=ac)
        want = dense.reference_dense(x32, y8, ce=1.0, dice=1.0, avg="all", upsample=size, align_corners=ac)["loss"] + \
            dense.reference_dense(xf.detach().cpu(), y8, ce=1.0, dice=1.0, avg="all")["loss"]
        assert abs(float(got) - want) <= 1e-5 * want, (ac, float(got), want)
        got = dense.DenseCrossEntropy(ignore_index=255, loss_weight=0.4, class_weight=w, upsample=True, align_corners=ac)(xa.detach(), yd)
        want = dense.reference_dense(x32, y, ce=0.4, alpha=w, ignore_index=255, upsample=size, align_corners=ac)["loss"]
        assert abs(float(got) - want) <= 1e-5 * want, (ac, float(got), want)
    # without the option a size mismatch raises, as before
    for call in (lambda: dense.DenseLoss()(xa.detach(), yd), lambda: dense.hybrid_loss([xa.detach()], yd), lambda: dense.SegMeter(3).update(xa.detach(), yd),
                 lambda: ops.dense_loss_fwd(xa.detach(), yd)):
        with pytest.raises(ValueError, match="labels must be"):
            call()
    with pytest.raises(ValueError, match="upsampling only"):
        crit(xf.detach(), yd[:, :10, :12].contiguous())


def test_seg_meter_upsample_and_predict():
    """SegMeter(upsample=True).update leaves what DenseLoss(upsample=True)(.., meter=) leaves; predict gives the meter's pred; a known shape allocates nothing."""
    dense = Dn()
    K = 5
    a, b = dense.SegMeter(K, ignore_index=255, upsample=True), dense.SegMeter(K, ignore_index=255, upsample=True)
    crit = dense.DenseLoss(ignore_index=255, upsample=True)
    for shape, size, dtype, ldtype, layout in [((2, K, 7, 9), (30, 37), torch.float32, torch.int64, "contiguous"), ((3, K, 8, 6), (32, 24), torch.bfloat16, torch.uint8, "view"),
                                               ((1, K, 12, 12), (12, 12), torch.float32, torch.int64, "contiguous")]:
        x32, y = inputs(shape, size, ldtype)
        xd, yd = on_device(x32.to(dtype), layout), y.to(DEV)
        a.update(xd, yd)
        crit(xd, yd, meter=b)
        ref = dense.reference_dense(x32.to(dtype), y, ignore_index=255, upsample=size)
        assert a.pred.dtype == torch.uint8 and tuple(a.pred.shape) == (shape[0],) + size and torch.equal(a.pred, b.pred)
        decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(ref["z"].max(1)))
        assert np.array_equal(a.pred.cpu().numpy()[decisive], ref["pred"][decisive])
        assert torch.equal(dense.predict(xd, size=size), a.pred)
        assert torch.equal(a.conf, b.conf) and torch.equal(a.loss.view(torch.int64), b.loss.view(torch.int64))
    assert int(a.conf.sum()) == int(a.loss[1]) > 0
    x32, y = inputs((2, K, 7, 9), (30, 37), torch.int64)
    xd, yd = x32.to(DEV), y.to(DEV)
    assert torch.equal(dense.predict(xd), xd.argmax(1).to(torch.uint8))          # size=None: the logits' own size
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    a.update(xd, yd)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before


def test_upsample_captured():
    """After one eager call, DenseLoss(upsample=True) forward + backward and SegMeter(upsample=True).update are captured on one stream; replays over refilled static
    tensors equal the eager results bit for bit."""
    dense = Dn()
    shape, size = (2, 5, 7, 9), (30, 37)
    x, y = inputs(shape, size, torch.int64)
    batches = [(x, y), (x.flip(0).contiguous(), y.flip(0).contiguous()), (x.roll(3, 3), y.roll(5, 2))]
    crit = dense.DenseLoss(ce=1.0, dice=1.0, ignore_index=255, upsample=True)
    eager_meter = dense.SegMeter(5, ignore_index=255, upsample=True)
    eager = []
    for xb, yb in batches:
        xe = xb.to(DEV).requires_grad_(True)
        loss = crit(xe, yb.to(DEV))
        loss.backward()
        eager_meter.update(xe.detach(), yb.to(DEV))
        eager.append((loss.detach().clone(), xe.grad.clone()))
    sx, sy = torch.zeros_like(x, device=DEV).requires_grad_(True), torch.zeros_like(y, device=DEV)
    meter = dense.SegMeter(5, ignore_index=255, upsample=True)
    meter.update(sx.detach(), sy)
    meter.reset()
    cold = dense.SegMeter(5, ignore_index=255, upsample=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="eager update first"):
            cold.update(sx.detach(), sy)
        sloss = crit(sx, sy)
        sloss.backward()
        meter.update(sx.detach(), sy)
    for (xb, yb), (eloss, egrad) in zip(batches, eager):
        with torch.no_grad():
            sx.copy_(xb)
        sy.copy_(yb)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sloss.detach().view(torch.int32), eloss.view(torch.int32)) and torch.equal(sx.grad.view(torch.int32), egrad.view(torch.int32))
    assert torch.equal(meter.conf, eager_meter.conf) and torch.equal(meter.loss.view(torch.int64), eager_meter.loss.view(torch.int64))
    assert int(meter.conf.sum()) == int(meter.loss[1]) > 0


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 7, 6, 12)], ids=["register-path", "generic-path"])
def test_equal_size_up_forward_is_the_plain_forward(shape):
    """At ``size == (h, w)``, ``align_corners=False`` and ``W % 4 == 0`` the upsampling forward IS the plain forward, bit for bit, in ``stats``, ``pred``, ``conf``
    and ``meter``: both taps of either axis fall on the pixel itself with weight 1 and 0, so the interpolation returns the logit exactly; both kernels cut the
    same chunks of 4 pixels into the same workgroup rows; and per pixel both go through the same code (csrc/dense.hip: DN_PIXEL on the register path, dn_pixel_tail,
    dn_store_pred, dn_write_row) in the same order.  fp32 only (a bf16 chunk is 8 pixels in the plain kernel, 4 here: another partition of the sums) and the
    forward only (the two backward passes form ``sum_k p_k g_k`` in different orders on purpose)."""
    ops = Lm().ops
    B, K, h, w = shape
    assert w % 4 == 0
    g = torch.Generator().manual_seed(K * 131 + h * 17 + w)
    xd = (torch.randn(shape, generator=g) * 3).to(DEV)
    y = torch.randint(0, K, (B, h, w), generator=g)
    y[torch.rand((B, h, w), generator=g) < 0.1] = 255
    yd = y.to(torch.uint8).to(DEV)
    for mode, kw, _ in modes(K):
        okw = op_kwargs(kw, K)
        got = []
        for fwd in (lambda **out: ops.dense_up_loss_fwd(xd, yd, False, size=(h, w), **okw, **out), lambda **out: ops.dense_loss_fwd(xd, yd, **okw, **out)):
            out = dict(pred=torch.full((B, h * w), 77, dtype=torch.uint8, device=DEV), conf=torch.zeros((K, K), dtype=torch.int64, device=DEV),
                       meter=torch.zeros(2, dtype=torch.float64, device=DEV))
            got.append(dict(out, stats=fwd(**out)))
        for name in ("stats", "pred", "conf", "meter"):
            assert torch.equal(bits(got[0][name]), bits(got[1][name])), (mode, name)
        assert int(got[0]["conf"].sum()) == int(got[0]["meter"][1]) > 0
