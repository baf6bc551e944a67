"""Sliding-window dense inference on a real MI355X: lmv_dense_slide_fwd (csrc/dense.hip) and the surface built on it (``slide_predict``, ``SegMeter.update_slide``,
``slide_inference``) against ``reference_slide``, the numpy float64 oracle that tests/test_dense_slide_cpu.py holds to mmseg's loop written with PyTorch's own
float64 ``F.interpolate`` / ``F.pad``.

The bounds are those of tests/test_dense_up_gpu.py.  Integers (``n_valid``, ``meter[1]``) must be equal.  ``pred`` must equal the oracle's at every pixel whose
oracle margin (top-1 minus top-2 mean logit) is at least 1e-4 max(1, |top logit|); the pixels left out may be at most 0.5 % of a case
(tests/test_dense_slide_cpu.py checks that cap with the oracle alone).  ``conf`` must equal the histogram of (label, the device's own pred) exactly.
``mean_logits``, ``meter[0]`` and the loss hold max(2 x the error of PyTorch's own fp32 GPU evaluation of the literal loop -- ``F.interpolate``, ``F.pad``, ``+=``,
``/``, then ``log_softmax`` -- against float64, 1e-6 max(1, |ref|)); for the map the error of PyTorch's evaluation is its largest over the map.

CASES together reach: a shifted last window, up to 3 x 4 covering windows with an odd W and partial chunks, an image below the crop on one axis with a
non-integer ratio, K = 6 (a register instance above the other kernels' 5), the generic path with the LDS stash (K = 19, bf16), K = 64 (with labels and a
confusion matrix the stash no longer fits: the re-interpolating form; prediction only: the stash), and more chunks than one sweep of the capped grid
(2 x 768 x 192 = 294 912 > 1024 workgroups x 256 threads)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_dense_loss_gpu import BIG, DEV

pytestmark = pytest.mark.gpu

# B, K, (H, W), crop, stride, (h, w), align_corners, dtype
CASES = [(2, 2, (40, 52), 24, 16, (6, 6), False, torch.float32),
         (1, 5, (37, 45), (16, 20), 8, (4, 5), True, torch.float32),
         (1, 6, (20, 70), 32, 24, (7, 9), False, torch.float32),
         (1, 19, (48, 48), 32, 16, (8, 8), False, torch.bfloat16),
         (1, 64, (24, 24), 16, 8, (4, 4), False, torch.float32),
         (2, 2, (768, 768), 512, 384, (128, 128), False, torch.float32)]
BIG_CASE = CASES[-1]
IGNORE = 255


def case_id(c):
    B, K, size, crop, stride, lo, align, dtype = c
    return f"{B}x{K}x{size[0]}x{size[1]}-c{crop}-s{stride}-{lo[0]}x{lo[1]}{'-ac' if align else ''}-{'bf16' if dtype == torch.bfloat16 else 'f32'}".replace(" ", "")


def Dn():
    from lemevit_amd import dense
    return dense


def grid_of(case):
    return Dn().slide_grid(case[2], case[3], case[4])


@functools.lru_cache(maxsize=None)
def inputs(case, ldtype):
    """window logits [G, B, K, h, w] (randn x 3, rounded to the case's dtype) and a label map as tests/test_dense_up_gpu.py draws it: a tenth labelled 255, a tenth
    labelled K; int64 maps also hold the stray labels -1 and K + 3"""
    B, K, (H, W), crop, stride, (h, w), align, dtype = case
    G = len(grid_of(case))
    g = torch.Generator().manual_seed(B * 7919 + K * 131 + h * 17 + w + H * 3 + W)
    x = (torch.randn((G, B, K, h, w), generator=g) * 3).to(dtype)
    y = torch.randint(0, K, (B, H, W), generator=g)
    r = torch.rand((B, H, W), generator=g)
    y[r < 0.1] = 255
    y[(r >= 0.1) & (r < 0.2)] = K
    if ldtype == torch.int64:
        y[(r >= 0.2) & (r < 0.21)] = -1
        y[(r >= 0.21) & (r < 0.22)] = K + 3
    return x, y.to(ldtype)


def on_device(x, layout):
    """contiguous, or the [:, :, 1:K+1] view of a [G, B, K + 2, h, w] buffer whose two other planes hold BIG"""
    if layout == "contiguous":
        return x.to(DEV)
    G, B, K, h, w = x.shape
    wide = torch.full((G, B, K + 2, h, w), BIG, dtype=x.dtype)
    wide[:, :, 1:K + 1] = x
    return wide.to(DEV)[:, :, 1:K + 1]


def torch_loop(x, grid, align):
    """mmseg's loop in stock PyTorch, in the dtype and on the device of ``x`` [G, B, K, h, w]: resize, pad, +=, count, divide"""
    G, B, K = x.shape[:3]
    preds = x.new_zeros((B, K, grid.H, grid.W))
    count_mat = x.new_zeros((B, 1, grid.H, grid.W))
    for g, (y1, y2, x1, x2) in enumerate(grid.boxes()):
        crop_seg_logit = F.interpolate(x[g], size=(y2 - y1, x2 - x1), mode="bilinear", align_corners=align)
        preds += F.pad(crop_seg_logit, (x1, grid.W - x2, y1, grid.H - y2))
        count_mat[:, :, y1:y2, x1:x2] += 1
    return preds / count_mat


@functools.lru_cache(maxsize=None)
def expected(case, ldtype):
    """(the float64 oracle, the errors of PyTorch's fp32 GPU evaluation of the literal loop against it): computed once, shared by both layouts, never modified"""
    B, K, size, crop, stride, lo, align, dtype = case
    x, y = inputs(case, ldtype)
    grid = grid_of(case)
    ref = Dn().reference_slide(x, grid, align_corners=align, labels=y, ignore_index=IGNORE)
    ref["loss"] = ref["nll_sum"] / ref["n_valid"]
    zt = torch_loop(x.float().to(DEV), grid, align)          # (a bf16 input: its values in fp32, not rounded back -- what the kernel does)
    yl = y.to(DEV).long().reshape(B, -1)
    valid = (yl >= 0) & (yl < K) & (yl != IGNORE)
    logp = F.log_softmax(zt.reshape(B, K, -1), dim=1).gather(1, torch.where(valid, yl, torch.zeros_like(yl))[:, None])[:, 0]
    t_nll = -(logp * valid).sum()
    te = dict(z=float(np.abs(zt.double().cpu().numpy() - ref["z"]).max()), nll_sum=abs(float(t_nll.double()) - ref["nll_sum"]),
              loss=abs(float((t_nll / valid.sum()).double()) - ref["loss"]))
    return ref, te


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.uint8)


def run(xd, yd, grid, align, K, with_mean=True):
    from lemevit_amd import ops
    B = xd.shape[1]
    pred = torch.full((B, grid.H * grid.W), 77, dtype=torch.uint8, device=DEV)
    mean = torch.full((B, K, grid.H, grid.W), 7.0, dtype=torch.float32, device=DEV) if with_mean else None
    conf = torch.zeros((K, K), dtype=torch.int64, device=DEV)
    meter = torch.zeros(2, dtype=torch.float64, device=DEV)
    stats = ops.dense_slide_fwd(xd, grid.ys, grid.xs, grid.window, (grid.H, grid.W), yd, align, IGNORE, pred=pred, mean_logits=mean, conf=conf, meter=meter)
    assert tuple(stats.shape) == (6 + 5 * K,)
    return dict(stats=stats.cpu(), pred=pred.cpu(), conf=conf.cpu(), meter=meter.cpu(), **({"mean": mean.cpu()} if with_mean else {}))


def check_slide(name, xd, yd, y, grid, align, K, ref, te):
    B, H, W = y.shape
    a, b = run(xd, yd, grid, align, K), run(xd, yd, grid, align, K)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{name}: two calls differ in {k}"
    c = run(xd, yd, grid, align, K, with_mean=False)          # without the map: the same bits everywhere else
    for k in c:
        assert torch.equal(bits(a[k]), bits(c[k])), f"{name}: {k} depends on whether mean_logits is written"
    st = a["stats"].double().numpy()
    # integers: equal
    assert st[4] == ref["n_valid"] and float(a["meter"][1]) == ref["n_valid"], (name, st[4], ref["n_valid"])
    # pred: equal wherever the oracle's margin is decisive
    decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(ref["z"].max(1)))
    share = 1.0 - float(decisive.mean())
    p = a["pred"].numpy().reshape(B, H, W)
    print(f"dense_slide {name} pred: {100 * share:.4f} % of the pixels left out, {int((p != ref['pred'])[decisive].sum())} differ")
    assert share <= 0.005, (name, share)
    assert np.array_equal(p[decisive], ref["pred"][decisive]), name
    # conf: the histogram of (label, the device's own pred) over the valid pixels
    yl = y.long().numpy()
    valid = (yl >= 0) & (yl < K) & (yl != IGNORE)
    want = np.bincount(yl[valid] * K + p[valid].astype(np.int64), minlength=K * K).reshape(K, K)
    assert np.array_equal(a["conf"].numpy(), want), name
    # mean_logits, meter[0], the loss
    for k, got in (("z", a["mean"].double().numpy()), ("nll_sum", float(a["meter"][0])), ("loss", st[0])):
        r = np.asarray(ref[k], dtype=np.float64)
        allow = np.maximum(2 * te[k], 1e-6 * np.maximum(1.0, np.abs(r)))
        err = np.abs(np.asarray(got) - r)
        print(f"dense_slide {name} {k}: error {float(err.max()):.3e} (torch fp32 {te[k]:.3e}, allowed {float(allow.min()):.3e})")
        assert bool((err <= allow).all()), (name, k, float(err.max()), float(allow.min()))
    assert st[1] == st[0] and abs(st[5] * ref["n_valid"] - 1.0) <= 2.0 ** -23          # plain cross-entropy over the valid pixels


@pytest.mark.parametrize("layout", ["contiguous", "view"])
@pytest.mark.parametrize("ldtype", [torch.int64, torch.uint8], ids=["i64", "u8"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_slide(case, ldtype, layout):
    B, K, size, crop, stride, lo, align, dtype = case
    grid = grid_of(case)
    if case == BIG_CASE:
        assert B * size[0] * ((size[1] + 3) // 4) > 1024 * 256 and K <= 16          # more chunks than one sweep of the capped grid takes
    x, y = inputs(case, ldtype)
    ref, te = expected(case, ldtype)
    check_slide(f"{case_id(case)} {ldtype} {layout}", on_device(x, layout), y.to(DEV), y, grid, align, K, ref, te)


@pytest.mark.parametrize("case", CASES[:5], ids=case_id)
def test_slide_predict_is_the_labelled_pass(case):
    """Prediction only (K = 64: with the stash) gives the bits of the pass with labels, map included"""
    dense = Dn()
    B, K, size, crop, stride, lo, align, dtype = case
    grid = grid_of(case)
    x, y = inputs(case, torch.uint8)
    xd = on_device(x, "view")
    full = run(xd, y.to(DEV), grid, align, K)
    pred, mean = dense.slide_predict(xd, grid, align, return_logits=True)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (B,) + size and mean.dtype == torch.float32 and tuple(mean.shape) == (B, K) + size
    assert torch.equal(pred.cpu().reshape(B, -1), full["pred"]) and torch.equal(bits(mean.cpu()), bits(full["mean"]))
    assert torch.equal(dense.slide_predict(xd, grid, align), pred)


@pytest.mark.parametrize("align", [False, True], ids=["half-pixel", "align-corners"])
@pytest.mark.parametrize("B,K,size,crop,stride,dtype", [(2, 2, (40, 52), 24, 16, torch.float32), (1, 5, (37, 45), (16, 20), 8, torch.float32),
                                                       (1, 6, (20, 70), 32, 24, torch.bfloat16), (1, 19, (48, 48), 32, 16, torch.float32)],
                         ids=["K2", "K5", "K6-bf16", "K19"])
def test_full_resolution_logits_are_the_literal_loop_bit_for_bit(B, K, size, crop, stride, dtype, align):
    """With (h, w) equal to the window every weight is 0 or 1: ``mean_logits`` is the sum in window order and one division, the bits of the literal fp32 loop"""
    dense = Dn()
    grid = dense.slide_grid(size, crop, stride)
    g = torch.Generator().manual_seed(K * 131 + size[1])
    x = (torch.randn((len(grid), B, K) + grid.window, generator=g) * 3).to(dtype)
    xd = on_device(x, "view")
    pred, mean = dense.slide_predict(xd, grid, align, return_logits=True)
    want = torch_loop(xd.float(), grid, align)
    assert int(Dn().reference_slide(x, grid)["count"].max()) >= 2
    assert torch.equal(mean.view(torch.int32), want.view(torch.int32))
    assert torch.equal(pred, want.argmax(1).to(torch.uint8))          # (torch's argmax takes the first index of a tie as well; randn x 3 holds no NaN)


@pytest.mark.parametrize("K,dtype,ldtype", [(3, torch.float32, torch.int64), (6, torch.float32, torch.uint8), (6, torch.bfloat16, torch.int64),
                                            (19, torch.float32, torch.uint8)], ids=["K3", "K6", "K6-bf16", "K19"])
def test_one_window_is_the_upsampling_path(K, dtype, ldtype):
    """The image equals the crop: one window, count 1.  ``pred`` is ``dense.predict``'s and the meter state ``SegMeter(upsample=True).update``'s, bit for bit."""
    dense = Dn()
    B, size, lo = 2, (32, 36), (8, 9)
    grid = dense.slide_grid(size, size, (16, 16))
    assert len(grid) == 1 and grid.window == size
    g = torch.Generator().manual_seed(K)
    x = (torch.randn((1, B, K) + lo, generator=g) * 3).to(dtype)
    y = torch.randint(0, K, (B,) + size, generator=g)
    y[torch.rand((B,) + size, generator=g) < 0.1] = IGNORE
    xd, yd = x.to(DEV), y.to(ldtype).to(DEV)
    assert torch.equal(dense.slide_predict(xd, grid), dense.predict(xd[0], size=size))
    a, b = dense.SegMeter(K, ignore_index=IGNORE), dense.SegMeter(K, ignore_index=IGNORE, upsample=True)
    for _ in range(2):
        a.update_slide(xd, grid, yd)
        b.update(xd[0], yd)
    assert torch.equal(a.pred, b.pred) and torch.equal(a.conf, b.conf) and torch.equal(a.loss.view(torch.int64), b.loss.view(torch.int64))
    assert int(a.conf.sum()) == int(a.loss[1]) > 0


def test_update_slide_allocates_nothing_and_can_be_captured():
    """``update_slide`` allocates nothing after its first call for a shape; captured on one stream (after one eager call), its replays over refilled static tensors
    leave the ``conf`` / ``loss`` bits of the eager updates."""
    dense = Dn()
    case = CASES[2]
    B, K, size, crop, stride, lo, align, dtype = case
    grid = grid_of(case)
    x, y = inputs(case, torch.int64)
    batches = [(x, y), (x.flip(0).contiguous(), y.flip(1).contiguous()), (x.roll(2, 4), y.roll(5, 2))]
    eager = dense.SegMeter(K, ignore_index=IGNORE, align_corners=align)
    for xb, yb in batches:
        eager.update_slide(xb.to(DEV), grid, yb.to(DEV))
    xd, yd = x.to(DEV), y.to(DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    eager.update_slide(xd, grid, yd)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    ref = dense.reference_slide(x, grid, align, labels=y, ignore_index=IGNORE)
    decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(ref["z"].max(1)))
    assert eager.pred.dtype == torch.uint8 and tuple(eager.pred.shape) == (B,) + size and np.array_equal(eager.pred.cpu().numpy()[decisive], ref["pred"][decisive])
    eager.reset()
    for xb, yb in batches:
        eager.update_slide(xb.to(DEV), grid, yb.to(DEV))
    sx, sy = torch.zeros_like(x, device=DEV), torch.zeros_like(y, device=DEV)
    meter = dense.SegMeter(K, ignore_index=IGNORE, align_corners=align)
    meter.update_slide(sx, grid, sy)
    meter.reset()
    cold = dense.SegMeter(K, ignore_index=IGNORE, align_corners=align)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="eager update first"):
            cold.update_slide(sx, grid, sy)
        meter.update_slide(sx, grid, sy)
    for xb, yb in batches:
        sx.copy_(xb)
        sy.copy_(yb)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(meter.conf, eager.conf) and torch.equal(meter.loss.view(torch.int64), eager.loss.view(torch.int64))
    assert int(meter.conf.sum()) == int(meter.loss[1]) > 0


def test_slide_inference_end_to_end():
    """A small fixed ``fn`` (1 x 1 convolution, 4 x average pooling) on a 2 x 3 x 40 x 52 image: ``slide_inference`` gives ``slide_predict`` on the logits ``fn`` gives
    per crop, the same bits with 1 and with 3 windows per call, and with a meter what ``update_slide`` leaves."""
    dense = Dn()
    torch.manual_seed(0)
    K = 4
    fn = torch.nn.Sequential(torch.nn.Conv2d(3, K, 1), torch.nn.AvgPool2d(4)).to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    img = torch.randn((2, 3, 40, 52), generator=g).to(DEV)
    y = torch.randint(0, K, (2, 40, 52), generator=g)
    y[torch.rand((2, 40, 52), generator=g) < 0.1] = IGNORE
    yd = y.to(DEV)
    grid = dense.slide_grid((40, 52), 24, 16)
    with torch.no_grad():
        stack = torch.stack([fn(img[:, :, y1:y2, x1:x2]) for y1, y2, x1, x2 in grid.boxes()])
        assert tuple(stack.shape) == (6, 2, K, 6, 6)
        want, want_mean = dense.slide_predict(stack, grid, return_logits=True)
        one = dense.slide_inference(fn, img, 24, 16)
        three, mean3 = dense.slide_inference(fn, img, 24, 16, windows_per_call=3, return_logits=True)
        four = dense.slide_inference(fn, img, 24, 16, windows_per_call=4)          # a last group of two windows
    assert one.dtype == torch.uint8 and tuple(one.shape) == (2, 40, 52)
    assert torch.equal(one, want) and torch.equal(three, want) and torch.equal(four, want) and torch.equal(mean3.view(torch.int32), want_mean.view(torch.int32))
    ref = dense.reference_slide(stack, grid, labels=y, ignore_index=IGNORE)
    decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(ref["z"].max(1)))
    assert np.array_equal(one.cpu().numpy()[decisive], ref["pred"][decisive])
    a, b = dense.SegMeter(K, ignore_index=IGNORE), dense.SegMeter(K, ignore_index=IGNORE)
    with torch.no_grad():
        got = dense.slide_inference(fn, img, 24, 16, windows_per_call=3, meter=a, target=yd)
    b.update_slide(stack, grid, yd)
    assert torch.equal(got, want) and torch.equal(a.conf, b.conf) and torch.equal(a.loss.view(torch.int64), b.loss.view(torch.int64)) and int(a.loss[1]) == ref["n_valid"]
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    with torch.no_grad():
        dense.slide_inference(lambda c: stack[0], img, 24, 16, meter=a, target=yd)          # the stack of a known shape is kept: only fn allocates
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
