"""Native validation metrics on a real MI355X: lmv_eval_logits / lmv_meter_add (csrc/metrics.hip) and the surface built on them (lemevit_amd.metrics) against
``reference_metrics``, the numpy restatement that tests/test_metrics_cpu.py holds to the stock formulas.  Ranks and predictions are integers and must be equal;
the per-row loss is held to the bound tests/test_recipe_gpu.py uses for lmv_soft_ce, max(2 x the error of PyTorch's own fp32 GPU F.cross_entropy on the same
inputs against float64, 1e-6 max(1, |ref|)).  The logits carry PLANTED ranks (see the CPU file); after rounding to bf16 some rows tie at the label, which is why
bf16 is held to the stated tie rule of ``reference_metrics`` and only fp32 additionally to timm's formula."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (3, 5), (5, 63), (4, 64), (6, 65), (130, 1000), (7, 1003), (16, 21841)]          # one lane, a part of a wave, 63 / 64 / 65, several workgroups, ImageNet-21k
PLANT = (0, 1, 4, 5, 2, 0, 17, 10 ** 9)
BIG = 1e30          # what the padding behind column N is filled with


def Lm():
    import lemevit_amd
    return lemevit_amd


def M():
    from lemevit_amd import metrics
    return metrics


@functools.lru_cache(maxsize=None)
def planted(B, N):
    """The inputs of tests/test_metrics_cpu.py: row b's label sits at rank min(PLANT[b % 8], N - 1)"""
    g = torch.Generator().manual_seed(B * 7919 + N)
    x = torch.randn(B, N, generator=g)
    y = torch.randint(0, N, (B,), generator=g)
    for b in range(B):
        if N == 1:
            continue
        t, yb = min(PLANT[b % 8], N - 1), int(y[b])
        o = torch.cat([x[b, :yb], x[b, yb + 1:]]).sort(descending=True).values
        x[b, yb] = o[0] + 1 if t == 0 else (o[N - 2] - 1 if t == N - 1 else (o[t - 1] + o[t]) / 2)
    return x, y


def timm_correct(output, target, topk):
    maxk = min(max(topk), output.size(1))
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.reshape(1, -1).expand_as(pred.t()))
    return [int(correct[:min(k, maxk)].reshape(-1).float().sum(0)) for k in topk]


def on_device(x, layout):
    """contiguous, or the [:, :N] view of a buffer padded to the next multiple of 8 (at least one column) and filled with BIG: the classifier tail's layout"""
    if layout == "contiguous":
        return x.to(DEV)
    B, N = x.shape
    wide = torch.full((B, (N + 8) // 8 * 8), BIG, dtype=x.dtype)
    wide[:, :N] = x
    return wide.to(DEV)[:, :N]


def check_eval(name, xd, yd, x, y, r=1):
    """x: the host copy of the logits in their own dtype.  Every K: rank / pred equal to the reference, the loss within the bound; two launches agree bit for bit."""
    ops = Lm().ops
    G, N = x.shape[0] // r, x.shape[1]
    Kmax = min(16, N)
    ref = M().reference_metrics(x, y, (1,), tta=r, k_pred=Kmax)
    on = ref["rank"] >= 0
    v = torch.from_numpy(ref["values"])          # what the loss is taken of (the fp32 mean for r > 1)
    ys = torch.where(torch.from_numpy(on), y, torch.zeros_like(y))
    t_row = F.cross_entropy(v.to(DEV), ys.to(DEV), reduction="none").double().cpu().numpy()
    finite = on & np.isfinite(ref["row_loss"])
    te = float(np.abs(t_row[finite] - ref["row_loss"][finite]).max()) if finite.any() else 0.0
    allow = np.maximum(2 * te, 1e-6 * np.maximum(1.0, np.abs(ref["row_loss"])))
    first = None
    for K in sorted({0, 1, min(5, N), Kmax}):
        row, rank, pred = ops.eval_logits(xd, yd, r, K)
        assert row.dtype == torch.float32 and tuple(row.shape) == (G,) and rank.dtype == torch.int32 and tuple(rank.shape) == (G,)
        assert (pred is None) if K == 0 else (pred.dtype == torch.int32 and tuple(pred.shape) == (G, K))
        got_row, got_rank = row.double().cpu().numpy(), rank.cpu().numpy()
        assert np.array_equal(got_rank, ref["rank"]), (name, K, got_rank.tolist(), ref["rank"].tolist())
        if K:
            assert np.array_equal(pred.cpu().numpy(), ref["pred"][:, :K]), (name, K)
        with np.errstate(invalid="ignore"):
            err = np.abs(got_row - ref["row_loss"])
        if first is None:
            print(f"eval_logits {name}: largest row-loss error {float(err[finite].max()) if finite.any() else 0.0:.3e} (torch fp32 {te:.3e}, allowed {float(allow[finite].min()) if finite.any() else 0.0:.3e})")
        assert bool((err[finite] <= allow[finite]).all()), (name, K, float((err[finite] / allow[finite]).max()))
        rest = ~finite
        assert np.array_equal(np.isnan(got_row[rest]), np.isnan(ref["row_loss"][rest])) and np.array_equal(got_row[rest & ~np.isnan(got_row)], ref["row_loss"][rest & ~np.isnan(got_row)]), name
        assert np.array_equal(got_row[~on], np.zeros(int((~on).sum())))
        bits = (row.view(torch.int32).cpu(), rank.cpu())
        if first is None:
            first = bits
        assert torch.equal(bits[0], first[0]) and torch.equal(bits[1], first[1]), f"{name}: two launches differ"
    return ref


@pytest.mark.parametrize("layout", ["contiguous", "padded"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_eval_logits(B, N, dtype, layout):
    x32, y = planted(B, N)
    x = x32.to(dtype)
    ref = check_eval(f"[{B}, {N}] {dtype} {layout}", on_device(x, layout), y.to(DEV), x, y)
    if dtype == torch.float32:          # no ties at the label: timm's formula holds too
        topk = (1, min(5, N))
        assert [int((ref["rank"] < k).sum()) for k in topk] == timm_correct(x32, y, topk)
        assert ref["rank"].tolist() == [min(PLANT[b % 8], N - 1) for b in range(B)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_eval_logits_special_rows_and_ignored_labels(dtype):
    """The rows of the CPU test: constant, NaN (also at the label), signed zeros, -inf except two entries (label on a finite one: finite loss; on -inf: +inf),
    each once more with an ignored label (-1, N); and a constant row wider than a wave."""
    inf, nan = float("inf"), float("nan")
    rows = [([0.25] * 7, 4), ([1.0, 3.0, nan, 2.0, -1.0, 0.5, 0.0], 1), ([1.0, nan, 3.0, nan, 0.0, 0.0, 0.0], 3), ([-0.0, 0.0, -1.0, 0.0, -0.0, 1.0, -0.0], 4),
            ([-inf, -inf, 2.0, -inf, 3.0, -inf, -inf], 3), ([-inf, -inf, 2.0, -inf, 3.0, -inf, -inf], 2)]
    x = torch.tensor([r[0] for r in rows] * 2, dtype=torch.float32).to(dtype)
    y = torch.tensor([r[1] for r in rows] + [-1, 7, -5, 1 << 40, -1, 7])
    for layout in ("contiguous", "padded"):
        ref = check_eval(f"special rows {dtype} {layout}", on_device(x, layout), y.to(DEV), x, y)
        assert ref["rank"].tolist() == [4, 1, 1, 4, 4, 1] + [-1] * 6 and ref["count"] == 6
        assert np.isfinite(ref["row_loss"][5]) and ref["row_loss"][4] == inf and np.isnan(ref["row_loss"][1])
    c = torch.full((3, 200), -2.5).to(dtype)
    yc = torch.tensor([0, 100, 199])
    ref = check_eval(f"constant rows {dtype}", c.to(DEV), yc.to(DEV), c, yc)
    assert ref["rank"].tolist() == [0, 100, 199] and all(p.tolist() == list(range(16)) for p in ref["pred"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("G,N", [(12, 65), (8, 1000)])
def test_eval_logits_tta(G, N, r, dtype):
    """reduce_factor r: the device forms the fp32 mean by the stated expression, the same in every sweep -- ranks, predictions and bits of two launches as the
    reference's; labels at planted ranks of the mean, two of them ignored"""
    g = torch.Generator().manual_seed(G * 7919 + N + r)
    x = torch.randn(G * r, N, generator=g).to(dtype)
    mean = torch.from_numpy(M().reference_metrics(x, torch.zeros(G, dtype=torch.int64), (1,), tta=r)["values"])
    y = mean.argsort(dim=1, descending=True, stable=True)[torch.arange(G), torch.tensor([min(PLANT[b % 8], N - 1) for b in range(G)])]
    y[3], y[G - 1] = -1, N
    for layout in ("contiguous", "padded"):
        ref = check_eval(f"tta {r} [{G * r}, {N}] {dtype} {layout}", on_device(x, layout), y.to(DEV), x, y, r)
        assert ref["count"] == G - 2
    with pytest.raises(ValueError):
        Lm().ops.eval_logits(x.to(DEV)[:-1], y.to(DEV), r)


def test_accuracy_is_timm_accuracy():
    for B, N in [(130, 1000), (7, 1003), (3, 5)]:
        x, y = planted(B, N)
        topk = (1, min(5, N))
        acc = Lm().accuracy(x.to(DEV), y.to(DEV), topk=topk)
        assert isinstance(acc, list) and len(acc) == 2 and all(a.is_cuda and a.dim() == 0 and a.dtype == torch.float32 for a in acc)
        counts = [float(a) * B / 100.0 for a in acc]
        assert all(abs(c - round(c)) < 1e-3 for c in counts) and [round(c) for c in counts] == timm_correct(x, y, topk)
    with pytest.raises(ValueError):
        Lm().accuracy(x.to(DEV), y.to(DEV), topk=(1, 6))


class _Spy:
    """lib with one entry point wrapped: records the arguments it is called with"""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, []

    def __getattr__(self, n):
        f = getattr(self._lib, n)
        if n != self._name:
            return f

        def g(*a):
            self.calls.append(a)
            return f(*a)
        return g


def test_eval_meter(monkeypatch):
    """Three updates (130, 130, 7 rows; fp32, bf16 padded, fp32) against the reference of each: counts exact, the loss within 1e-6 relative of the float64 mean
    of the fp32 row losses; keep_predictions; update_loss; reset; the keys of compute(); a strided view is read in place; no allocation for a known shape."""
    ops = Lm().ops
    xa, ya = planted(130, 1000)
    xb = xa.flip(0).bfloat16()
    yb = ya.flip(0).clone()
    yb[5] = -1
    xc, yc = planted(7, 1000)
    meter = M().EvalMeter(topk=(1, 5), keep_predictions=3)
    spy = _Spy(ops.lib, "lmv_eval_logits")
    monkeypatch.setattr(ops, "lib", spy)
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a copy path was taken")))
    batches = [(on_device(xa, "contiguous"), ya, xa), (on_device(xb, "padded"), yb, xb), (on_device(xc, "padded"), yc, xc)]
    labels = [b[1].to(DEV) for b in batches]
    row_sum, want = 0.0, torch.zeros(4, dtype=torch.float64)
    for (xd, y, x), yd in zip(batches, labels):
        meter.update(xd, yd)
        assert spy.calls[-1][0] == xd.data_ptr() and spy.calls[-1][2] == xd.stride(0)          # the view itself, with its row stride
        ref = M().reference_metrics(x, y, (1, 5), k_pred=3)
        assert np.array_equal(meter.rank.cpu().numpy(), ref["rank"]) and np.array_equal(meter.pred.cpu().numpy(), ref["pred"])
        row_sum += float(meter.row_loss.double().sum())
        want += ref["state"]
    monkeypatch.undo()
    state = meter.state.cpu()
    assert meter.state.is_cuda and state.dtype == torch.float64 and state[1:].tolist() == want[1:].tolist() and state[1] == 266.0
    assert abs(float(state[0]) - row_sum) <= 1e-6 * abs(row_sum)
    got = meter.compute()
    assert list(got) == ["loss", "top1", "top5", "count"] and got["count"] == 266
    assert got["top1"] == 100.0 * float(want[2]) / 266 and got["top5"] == 100.0 * float(want[3]) / 266 and abs(got["loss"] - row_sum / 266) <= 1e-6 * row_sum / 266
    # a known shape allocates nothing
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    meter.update(batches[0][0], labels[0])
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    meter.reset()
    assert meter.state.cpu().tolist() == [0.0] * 4
    # the scalar mode: losses_m.update(loss.item(), n) without the .item()
    l1, l2 = torch.tensor(0.75, device=DEV), torch.tensor(2.5, device=DEV)
    meter.update_loss(l1, 128)
    meter.update_loss(l2, 7)
    s = meter.state.cpu().tolist()
    assert s == [0.75 * 128 + 2.5 * 7, 135.0, 0.0, 0.0] and meter.compute()["loss"] == (0.75 * 128 + 2.5 * 7) / 135
    with pytest.raises(ValueError):
        meter.update(batches[0][0][:, :4], labels[0])
    # tta through the meter
    xt = torch.randn(12, 65, generator=torch.Generator().manual_seed(3))
    yt = torch.tensor([5, 64, 0, -1])
    mt = M().EvalMeter(topk=(1, 2, 5), tta=3)
    mt.update(xt.to(DEV), yt.to(DEV))
    assert mt.state.cpu()[1:].tolist() == M().reference_metrics(xt, yt, (1, 2, 5), tta=3)["state"][1:].tolist()


def test_eval_meter_captured():
    """After one eager update, meter.update(static_logits, static_labels) is captured on one stream; three replays over refilled static tensors leave the
    state of an eager meter over the same three batches, bit for bit.  Capture without the eager update raises."""
    x, y = planted(130, 1000)
    batches = [(x, y), (x.flip(0).contiguous(), y.flip(0).contiguous()), (x.roll(7, 0), y.roll(3, 0))]
    eager = M().EvalMeter(topk=(1, 5))
    for xb, yb in batches:
        eager.update(xb.to(DEV), yb.to(DEV))
    sx, sy = torch.zeros_like(x, device=DEV), torch.zeros_like(y, device=DEV)
    cold, other = M().EvalMeter(topk=(1, 5)), M().EvalMeter(topk=(1, 5))
    other.update(sx[:7], sy[:7])          # a state, but no buffers for 130 rows
    meter = M().EvalMeter(topk=(1, 5))
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
    assert torch.equal(meter.state.view(torch.int64), eager.state.view(torch.int64)), (meter.state.tolist(), eager.state.tolist())
    assert meter.state[1] == 390.0 and meter.state[2] > 0


def test_validate():
    """lemevit_tiny, 10 classes, 96 x 96, batches of 4, 4 and 2 with one ignored label: validate() equals reference_metrics of the model's own logits, collected
    in a second pass -- counts exact, the loss within max(2 x the error of PyTorch's fp32 GPU F.cross_entropy on those logits, 1e-6 max(1, |ref|)); the
    training flag is restored; a uint8 loader batch goes through ``preprocess``."""
    L = Lm()
    torch.manual_seed(0)
    model = L.create_model("lemevit_tiny", num_classes=10, drop_path_rate=0.0).to(DEV).train()
    g = torch.Generator().manual_seed(11)
    sizes = (4, 4, 2)
    loader = [(torch.randn((b, 3, 96, 96), generator=g), torch.randint(0, 10, (b,), generator=g)) for b in sizes]
    loader[2][1][1] = -1
    got = L.validate(model, loader, topk=(1, 5))
    assert model.training and list(got) == ["loss", "top1", "top5"]
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits = torch.cat([model(xb.to(DEV)).cpu() for xb, _ in loader])
    labels = torch.cat([yb for _, yb in loader])
    assert logits.dtype == torch.bfloat16 and tuple(logits.shape) == (10, 10)
    ref = M().reference_metrics(logits, labels, (1, 5))
    t_loss = float(F.cross_entropy(logits.float().to(DEV), labels.to(DEV), ignore_index=-1))
    te = abs(t_loss - ref["loss"])
    print(f"validate: loss {got['loss']:.7f} (reference {ref['loss']:.7f}, torch fp32 error {te:.3e}), top1 {got['top1']:.2f}, top5 {got['top5']:.2f}")
    assert ref["count"] == 9 and got["top1"] == 100.0 * ref["hits"][1] / 9 and got["top5"] == 100.0 * ref["hits"][5] / 9
    assert abs(got["loss"] - ref["loss"]) <= max(2 * te, 1e-6 * max(1.0, abs(ref["loss"])))
    # eval-mode model stays in eval mode; a uint8 batch through the one-launch normalise-and-cast
    u8 = [(torch.randint(0, 256, (b, 3, 96, 96), generator=g, dtype=torch.uint8), torch.randint(0, 10, (b,), generator=g)) for b in (4, 2)]
    pre = L.RandomErasing(0.0, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], out_dtype=torch.bfloat16)
    out = L.validate(model, u8, preprocess=pre, log_interval=1, logger=type("Log", (), {"info": staticmethod(print)}))
    assert not model.training and np.isfinite(out["loss"]) and 0.0 <= out["top1"] <= out["top5"] <= 100.0
