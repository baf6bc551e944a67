"""Host half of the native validation metrics (lemevit_amd.metrics, lmv_eval_logits / lmv_meter_add in csrc/metrics.hip) without a GPU: the numpy restatement
``reference_metrics`` -- the oracle of tests/test_metrics_gpu.py -- against the stock formulas (timm.utils.accuracy restated here, F.cross_entropy in float64)
on logits with PLANTED ranks (random labels on random logits give essentially no hits: a broken rank would pass), the stated order on special rows, ignored
labels, the --tta mean, EvalMeter.merge under a 2-rank gloo group, and the ABI: both symbols declared, exported and bound, argument validation before any launch."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 5), (5, 63), (4, 64), (6, 65), (130, 1000), (7, 1003), (16, 21841)]
PLANT = (0, 1, 4, 5, 2, 0, 17, 10 ** 9)


def M():
    from lemevit_amd import metrics
    return metrics


def planted(B, N):
    """randn logits and random labels; row b's label value moved so that its rank among the others is min(PLANT[b % 8], N - 1): midway between its would-be
    neighbours in the descending sort of the other entries, +1 above the top for rank 0, -1 below the bottom for the last rank"""
    g = torch.Generator().manual_seed(B * 7919 + N)
    x = torch.randn(B, N, generator=g)
    y = torch.randint(0, N, (B,), generator=g)
    want = [min(PLANT[b % 8], N - 1) for b in range(B)]
    for b in range(B):
        if N == 1:
            continue
        t, yb = want[b], int(y[b])
        o = torch.cat([x[b, :yb], x[b, yb + 1:]]).sort(descending=True).values
        x[b, yb] = o[0] + 1 if t == 0 else (o[N - 2] - 1 if t == N - 1 else (o[t - 1] + o[t]) / 2)
    return x, y, want


def timm_correct(output, target, topk):
    """timm.utils.accuracy up to its scaling: the number of rows whose label is among the top k, per k"""
    maxk = min(max(topk), output.size(1))
    _, pred = output.topk(maxk, 1, True, True)
    correct = pred.t().eq(target.reshape(1, -1).expand_as(pred.t()))
    return [int(correct[:min(k, maxk)].reshape(-1).float().sum(0)) for k in topk]


@pytest.mark.parametrize("B,N", SHAPES)
def test_reference_against_stock_formulas(B, N):
    x, y, want = planted(B, N)
    rows = torch.arange(B)
    assert int((x == x[rows, y][:, None]).sum()) == B, "precondition: no logit ties with its label's"
    topk = (1, min(5, N))
    K = min(16, N)
    m = M().reference_metrics(x, y, topk, k_pred=K)
    assert m["rank"].dtype == np.int32 and m["rank"].tolist() == want          # every planted rank is met
    assert [m["hits"][k] for k in topk] == timm_correct(x, y, topk)
    for k in topk:          # ... on every row, not only in the sum
        assert np.array_equal(m["rank"] < k, x.topk(k, 1, True, True).indices.eq(y[:, None]).any(1).numpy())
    assert np.array_equal(m["pred"], x.topk(K, 1, True, True).indices.numpy())          # (no ties within these rows' top K either)
    ce = F.cross_entropy(x.double(), y, reduction="none").numpy()
    assert np.all(np.abs(m["row_loss"] - ce) <= 1e-12 * np.maximum(1.0, np.abs(ce)))
    assert m["count"] == B and abs(m["loss"] - ce.mean()) <= 1e-12 * max(1.0, ce.mean())
    assert m["state"].dtype == torch.float64 and m["state"].tolist()[1:] == [float(B)] + [float(m["hits"][k]) for k in topk]
    if (B, N) == (130, 1000):
        assert (m["hits"][1], m["hits"][5]) == (33, 82)


def special_rows():
    """(name, row, label, rank, first classes of the order, loss finite / nan)"""
    inf, nan = float("inf"), float("nan")
    return [("constant", [0.25] * 7, 4, 4, [0, 1, 2, 3, 4, 5, 6], "finite"),
            ("one NaN", [1.0, 3.0, nan, 2.0, -1.0, 0.5, 0.0], 1, 1, [2, 1, 3, 0, 5, 6, 4], "nan"),
            ("NaN at the label, another behind it", [1.0, nan, 3.0, nan, 0.0, 0.0, 0.0], 3, 1, [1, 3, 2, 0, 4, 5, 6], "nan"),
            ("signed zeros", [-0.0, 0.0, -1.0, 0.0, -0.0, 1.0, -0.0], 4, 4, [5, 0, 1, 3, 4, 6, 2], "finite"),
            ("-inf except two", [-inf, -inf, 2.0, -inf, 3.0, -inf, -inf], 3, 4, [4, 2, 0, 1, 3, 5, 6], "inf"),
            ("-inf except two, label finite", [-inf, -inf, 2.0, -inf, 3.0, -inf, -inf], 2, 1, [4, 2, 0, 1, 3, 5, 6], "finite")]


def test_the_order_on_special_rows():
    rows = special_rows()
    x = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    y = torch.tensor([r[2] for r in rows])
    m = M().reference_metrics(x, y, (1, 5), k_pred=7)
    for i, (name, _, _, rank, order, loss) in enumerate(rows):
        assert int(m["rank"][i]) == rank, name
        assert m["pred"][i].tolist() == order, name
        got = float(m["row_loss"][i])
        assert {"finite": np.isfinite(got), "nan": np.isnan(got), "inf": got == np.inf}[loss], (name, got)
    two = float(m["row_loss"][5])
    assert abs(two - np.log1p(np.exp(1.0))) <= 1e-12          # lse(2, 3) - 2 = log(1 + e)
    # a constant row of any width: rank == label and the predictions are 0 .. K - 1
    for N in (1, 64, 65, 200):
        c = M().reference_metrics(torch.full((3, N), -2.5), torch.tensor([0, N // 2, N - 1]), (1,), k_pred=min(16, N))
        assert c["rank"].tolist() == [0, N // 2, N - 1] and all(p.tolist() == list(range(min(16, N))) for p in c["pred"])
        assert np.all(np.abs(c["row_loss"] - np.log(N)) <= 1e-12)


def test_ignored_labels_are_counted_nowhere():
    x, y, _ = planted(6, 65)
    y2 = y.clone()
    y2[1], y2[4] = -1, 65
    keep = torch.tensor([0, 2, 3, 5])
    m, sub = M().reference_metrics(x, y2, (1, 5), k_pred=3), M().reference_metrics(x[keep], y[keep], (1, 5), k_pred=3)
    assert m["rank"][[1, 4]].tolist() == [-1, -1] and m["row_loss"][[1, 4]].tolist() == [0.0, 0.0]
    assert m["count"] == 4 and m["hits"] == sub["hits"] and m["loss"] == sub["loss"] and torch.equal(m["state"], sub["state"])
    assert np.array_equal(m["pred"][[0, 2, 3, 5]], sub["pred"]) and np.array_equal(m["pred"][1], x[1].topk(3).indices.numpy())          # pred is still written
    none = M().reference_metrics(x, torch.full((6,), -1), (1, 5))
    assert none["count"] == 0 and none["state"].tolist() == [0.0, 0.0, 0.0, 0.0] and np.isnan(none["loss"])


@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("G,N", [(12, 65), (8, 1000)])
def test_tta_mean(G, N, r):
    """--tta: reference_metrics(x, y, tta=r) against output.unfold(0, r, r).mean(2) evaluated in float64.  The fp32 mean differs from the float64 one by at
    most r roundings of 2^-24 relative to the partial sums (r - 1 additions and the product; r a power of two: the product is exact), so the loss, whose
    derivative with respect to the values has 1-norm <= 2, is within 2 r 2^-24 max|partial sum|.  The labels are placed at planted ranks of the float64 mean;
    the ranks must be equal when r is a power of two, and for r = 3 wherever the label's float64 gap to both neighbours exceeds that rounding."""
    g = torch.Generator().manual_seed(G * 7919 + N + r)
    x = torch.randn(G * r, N, generator=g)
    mean64 = x.double().unfold(0, r, r).mean(dim=2)
    order = mean64.argsort(1, descending=True)
    want = [min(PLANT[b % 8], N - 1) for b in range(G)]
    y = order[torch.arange(G), torch.tensor(want)]
    m = M().reference_metrics(x, y, (1, 5), tta=r, k_pred=5)
    assert m["values"].dtype == np.float32 and m["values"].shape == (G, N)
    bound = r * 2.0 ** -24 * float(x.double().abs().unfold(0, r, r).sum(2).max())
    assert np.abs(m["values"].astype(np.float64) - mean64.numpy()).max() <= bound
    ce = F.cross_entropy(mean64, y, reduction="none").numpy()
    assert np.abs(m["row_loss"] - ce).max() <= 2 * bound
    srt = mean64.sort(1, descending=True).values
    gap = torch.stack([(srt[b, max(t - 1, 0)] - srt[b, t]).abs() + (t == 0) for b, t in enumerate(want)]).minimum(
        torch.stack([(srt[b, t] - srt[b, min(t + 1, N - 1)]).abs() + (t == N - 1) for b, t in enumerate(want)]))
    clear = (gap > 2 * bound).numpy()
    if r in (2, 4):
        assert m["rank"].tolist() == want
    assert clear.sum() >= G - 1 and np.array_equal(m["rank"][clear], np.array(want)[clear])
    one = M().reference_metrics(x, y.repeat_interleave(r), (1, 5))          # tta = 1: no arithmetic touches the values
    assert np.array_equal(one["values"].view(np.uint32), x.numpy().view(np.uint32))
    with pytest.raises(ValueError):
        M().reference_metrics(x[:-1], y, (1, 5), tta=r)


# ---- EvalMeter.merge / all_reduce under gloo ---------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _merge_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from lemevit_amd import dist as D
    from lemevit_amd import metrics
    D.init_distributed("gloo")
    x, y, _ = planted(130, 1000)
    y[7], y[100] = -1, 1000          # one ignored row in each half
    half = slice(0, 65) if rank == 0 else slice(65, 130)
    m = metrics.reference_metrics(x[half], y[half], (1, 5))
    meter = metrics.EvalMeter(topk=(1, 5)).merge([m["state"]])
    meter.all_reduce()
    torch.save(dict(state=meter.state, mine=m["state"], metrics=meter.compute()), out + f".{rank}")
    torch.distributed.destroy_process_group()


def test_eval_meter_merge_two_ranks(tmp_path):
    """The states of two halves, summed by ONE all-reduce (gloo, CPU tensors), equal the state of the whole: the integer entries exactly, the loss sum within
    float64 rounding; merge() of the two states on one process gives the same bits as the all-reduce."""
    out = str(tmp_path / "m.pt")
    mp.spawn(_merge_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    x, y, _ = planted(130, 1000)
    y[7], y[100] = -1, 1000
    whole = M().reference_metrics(x, y, (1, 5))
    assert torch.equal(r0["state"], r1["state"]) and r0["state"].dtype == torch.float64
    assert r0["state"][1:].tolist() == whole["state"][1:].tolist() and r0["state"][1] == 128.0
    assert abs(float(r0["state"][0] - whole["state"][0])) <= 1e-12 * float(whole["state"][0])
    merged = M().EvalMeter(topk=(1, 5)).merge([r0["mine"], r1["mine"]])
    assert torch.equal(merged.state, r0["state"])
    got = merged.compute()
    assert list(got) == ["loss", "top1", "top5", "count"] and got == r0["metrics"] and got["count"] == 128
    assert got["top1"] == 100.0 * whole["hits"][1] / 128 and got["top5"] == 100.0 * whole["hits"][5] / 128 and abs(got["loss"] - whole["loss"]) <= 1e-12 * whole["loss"]
    merged.reset()
    assert merged.state.tolist() == [0.0] * 4
    with pytest.raises(TypeError):
        merged.merge([torch.zeros(3, dtype=torch.float64)])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_version():
    import lemevit_amd
    from lemevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lmv_eval_logits", "lmv_meter_add"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} not declared"
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14 and re.search(r"#define\s+LMV_ABI_VERSION\s+14\b", src)          # a pure addition
    assert re.search(r"#define\s+LMV_EVAL_MAX_PRED\s+16\b", src) and re.search(r"#define\s+LMV_METER_MAX_K\s+8\b", src)
    assert (_lib.EVAL_MAX_PRED, _lib.METER_MAX_K) == (16, 8)
    assert len(_lib.SIGNATURES["lmv_eval_logits"][1]) == 12 and len(_lib.SIGNATURES["lmv_meter_add"][1]) == 9
    assert "metrics.hip" in open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()
    for name in ("accuracy", "EvalMeter", "validate", "reference_metrics"):
        assert getattr(lemevit_amd, name) is getattr(lemevit_amd.metrics, name) and name in lemevit_amd.__all__


def test_argument_validation_without_gpu():
    """Each refusal returns LMV_ERR_SHAPE (-1) with its message before any launch; the buffers are host memory that is never touched."""
    from lemevit_amd._lib import lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    F32, BF16 = 0, 1

    def ev(logits=p, dtype=F32, ls=5, B=4, N=5, labels=p, r=1, row=p, rank=p, pred=p, K=0):
        rc = lib.lmv_eval_logits(logits, dtype, ls, B, N, labels, r, row, rank, pred, K, None)
        return rc, lib.lmv_last_error().decode()

    for kw, msg in [(dict(logits=None), "null"), (dict(labels=None), "null"), (dict(row=None), "null"), (dict(rank=None), "null"),
                    (dict(B=0), "bad shape"), (dict(N=0), "bad shape"), (dict(r=3), "reduce_factor"), (dict(r=0), "reduce_factor"), (dict(ls=4), "row stride"),
                    (dict(dtype=2), "dtype"), (dict(dtype=7), "dtype"), (dict(K=17, N=40, ls=40), "outside 0 .. 16"), (dict(K=-1), "outside 0 .. 16"),
                    (dict(K=6), "predictions of N = 5"), (dict(K=2, pred=None), "null pred"),
                    (dict(logits=p + 2), "misaligned"), (dict(logits=p + 1, dtype=BF16), "misaligned"), (dict(labels=p + 4), "misaligned"),
                    (dict(row=p + 2), "misaligned"), (dict(rank=p + 1), "misaligned"), (dict(pred=p + 2, K=1), "misaligned")]:
        rc, err = ev(**kw)
        assert rc == -1 and msg in err and err.startswith("eval_logits:"), (kw, rc, err)

    ks = (ctypes.c_int32 * 8)(1, 5, 1, 1, 1, 1, 1, 1)

    def ma(state=p, row=p, rank=p, rows=4, k=ks, nk=2, loss=None, n=0):
        rc = lib.lmv_meter_add(state, row, rank, rows, k, nk, loss, n, None)
        return rc, lib.lmv_last_error().decode()

    bad = (ctypes.c_int32 * 8)(1, 0, 1, 1, 1, 1, 1, 1)
    for kw, msg in [(dict(state=None), "null state"), (dict(nk=9), "outside 0 .. 8"), (dict(nk=-1), "outside 0 .. 8"), (dict(k=None), "null ks"), (dict(k=bad), "ks[1] = 0 < 1"),
                    (dict(row=None, rank=None), "exactly one"), (dict(loss=p), "exactly one"), (dict(rank=None), "come together"), (dict(row=None), "come together"),
                    (dict(rows=0), "rows = 0"), (dict(row=None, rank=None, loss=p, n=0), "n = 0"),
                    (dict(state=p + 4), "misaligned"), (dict(row=p + 2), "misaligned"), (dict(rank=p + 2), "misaligned"), (dict(row=None, rank=None, loss=p + 2, n=1), "misaligned")]:
        rc, err = ma(**kw)
        assert rc == -1 and msg in err and err.startswith("meter_add:"), (kw, rc, err)


def test_python_side_refusals_without_gpu():
    """ops.eval_logits / ops.meter_add and the metrics surface raise on the Python side for what the ABI would refuse (and never compute on the CPU)."""
    from lemevit_amd import ops
    metrics = M()
    x, y = torch.randn(4, 5), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.eval_logits(x, y)
    with pytest.raises(ValueError):
        ops.eval_logits(torch.randn(4), y)
    st = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.meter_add(st, ks=range(1, 10))
    with pytest.raises(ValueError):
        ops.meter_add(st, ks=(1, 0))
    with pytest.raises(TypeError):
        ops.meter_add(torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.int32), (1, 5))
    with pytest.raises(ValueError, match="exactly one"):
        ops.meter_add(st, ks=(1, 5))
    with pytest.raises(ValueError, match="come together"):
        ops.meter_add(st, row_loss=torch.zeros(4), ks=(1, 5))
    with pytest.raises(ValueError):
        ops.meter_add(st, ks=(1, 5), loss=torch.zeros(()), n=0)
    with pytest.raises(ValueError, match="top-6 of 5"):
        metrics.accuracy(x, y, topk=(1, 6))
    with pytest.raises(ValueError):
        metrics.EvalMeter(topk=())
    with pytest.raises(ValueError):
        metrics.EvalMeter(topk=range(1, 10))
    with pytest.raises(ValueError):
        metrics.EvalMeter(keep_predictions=17)
    with pytest.raises(ValueError):
        metrics.EvalMeter(tta=0)
    with pytest.raises(ValueError, match="top-5 of 4"):
        metrics.EvalMeter().update(torch.randn(4, 4), y)
    with pytest.raises(RuntimeError):
        metrics.EvalMeter().compute()
