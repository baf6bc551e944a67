"""Host half of the dense-prediction losses and metrics (lemevit_amd.dense, lmv_dense_loss_fwd / lmv_dense_loss_bwd in csrc/dense.hip) without a GPU: the numpy
restatement ``reference_dense`` -- the oracle of tests/test_dense_loss_gpu.py -- against the reference's own functions (tests/golden/dense_loss.npz, written by
gen_dense_loss_golden.py from change_detection/utils/metrics.py), against ``F.cross_entropy`` in float64 for the three ``avg`` modes and against autograd through a
plain-torch float64 restatement of the stated formulas; ``SegMeter.compute()`` on hand-written matrices; and the ABI: the symbols declared, exported and bound
with the header's argument counts, every refusal before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gen_dense_loss_golden import ALPHA, GAMMA, SHAPES, case_name, dense_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lmv_dense_loss_workspace_bytes", "lmv_dense_loss_fwd", "lmv_dense_loss_bwd")


def D():
    from lemevit_amd import dense
    return dense


def torch_dense(x, y, ce=1.0, dice=0.0, jaccard=0.0, gamma=0.0, alpha=None, ignore_index=None, avg="valid", eps=1e-7):
    """The stated formulas in plain torch, differentiable, in the dtype and on the device of ``x`` (include/lemevit_hip.h; the reference's FocalLoss / dice_loss /
    jaccard_loss with a valid mask in front of every sum).  Returns (loss, dict(ce, dice, jaccard, I, P, T))."""
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
    Dn = {"valid": vm.sum(), "all": torch.tensor(float(y.numel()), dtype=x.dtype, device=x.device), "weight": (a * T).sum()}[avg]
    ce_v = (f * -logpt * vm).sum() / Dn if float(Dn) > 0 else (logpt * 0).sum()
    dice_v = 1 - (2 * I / (P + T + eps)).mean()
    jac_v = 1 - (I / (P + T - I + eps)).mean()
    return ce * ce_v + dice * dice_v + jaccard * jac_v, dict(ce=ce_v, dice=dice_v, jaccard=jac_v, I=I, P=P, T=T)


# ---- the golden file: the reference's own functions --------------------------------------------------------------------------------------------------
GOLDEN_MODES = [("focal0", lambda K: dict(ce=1.0, avg="all")), ("focal2", lambda K: dict(ce=1.0, gamma=float(GAMMA), alpha=ALPHA[K], avg="all")),
                ("dice", lambda K: dict(ce=0.0, dice=1.0)), ("jaccard", lambda K: dict(ce=0.0, jaccard=1.0))]


@pytest.mark.parametrize("shape", SHAPES, ids=case_name)
def test_reference_reproduces_the_golden_file(golden, shape):
    """float64 cases: losses and gradients within 1e-12 max(1, |ref|).  float32 cases: the reference evaluated the same functions in float32, so its output is the
    float64 value up to float32 rounding: the loss (a mean of O(1) terms, each a few float32 operations) within 4 ulp of max(1, |loss|), 4 x 2^-23.  A gradient
    element is p_k (g_k - sum_j p_j g_j) + w_ce f (p_k - [y = k]) / D: its terms are bounded by S = 2 max_k (|u_k| + |v_k|) + w_ce max(alpha) / D, and u_k, v_k
    come from I_k, P_k, sums of N = B H W probabilities that float32 may accumulate one by one (N - 1 roundings of 2^-24), followed by at most 16 roundings of the
    softmax, the quotient rule and the products: within (N + 16) 2^-24 S."""
    meta, arr = golden("dense_loss")
    assert meta["kind"] == "dense_loss" and [tuple(c["shape"]) for c in meta["cases"]] == SHAPES and meta["gamma"] == GAMMA
    K = shape[1]
    x, y = dense_case(shape)
    assert x.dtype == torch.float64 and torch.equal(x, x.float().double()) and sorted(set(y.reshape(-1).tolist())) == list(range(K))
    for name, kw in GOLDEN_MODES:
        r = D().reference_dense(x, y, **kw(K))
        for tag in ("f64", "f32"):
            L, G = arr[f"{case_name(shape)}.{tag}.{name}"], arr[f"{case_name(shape)}.{tag}.{name}.grad"]
            assert G.shape == tuple(shape) and G.dtype == (np.float64 if tag == "f64" else np.float32)
            el, eg = abs(r["loss"] - float(L)), float(np.abs(r["dlogits"] - G).max())
            if tag == "f64":
                bl, bg = 1e-12 * max(1.0, abs(float(L))), 1e-12
                assert np.all(np.abs(r["dlogits"] - G) <= 1e-12 * np.maximum(1.0, np.abs(G))), (name, eg)
            else:
                S = 2 * float((np.abs(r["u"]) + np.abs(r["v"])).max()) + kw(K)["ce"] * max(kw(K).get("alpha") or [1.0]) * r["inv_D"]
                bl, bg = 4 * 2.0 ** -23 * max(1.0, abs(float(L))), (np.prod(shape) // K + 16) * 2.0 ** -24 * S
            assert el <= bl and eg <= bg, (name, tag, el, bl, eg, bg)
    # hybrid_loss is focal0 + dice on every prediction
    h = D().reference_dense(x, y, ce=1.0, dice=1.0, avg="all")
    want = float(arr[f"{case_name(shape)}.f64.focal0"]) + float(arr[f"{case_name(shape)}.f64.dice"])
    assert abs(h["loss"] - want) <= 1e-12 * max(1.0, abs(want))
    assert np.abs(h["dlogits"] - arr[f"{case_name(shape)}.f64.focal0.grad"] - arr[f"{case_name(shape)}.f64.dice.grad"]).max() <= 1e-12


def ignored_case(B, K, H, W, seed, ignore):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, K, H, W, generator=g) * 3).double()
    y = torch.randint(0, K, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.2] = ignore
    return x, y


@pytest.mark.parametrize("B,K,H,W,ignore", [(2, 2, 5, 7, 255), (1, 5, 9, 4, 5), (3, 19, 3, 3, 255), (2, 4, 6, 6, 1)])
def test_reference_ce_is_torch_cross_entropy(B, K, H, W, ignore):
    x, y = ignored_case(B, K, H, W, B * 100 + K, ignore)
    w = [0.5 + 0.25 * k for k in range(K)]
    ref = D().reference_dense
    valid = F.cross_entropy(x, y, ignore_index=ignore)
    r = ref(x, y, ignore_index=ignore, avg="valid")
    assert abs(r["ce"] - float(valid)) <= 1e-12 * max(1.0, float(valid)) and r["loss"] == r["ce"] and r["n_valid"] == int((y != ignore).sum())
    alls = F.cross_entropy(x, y, ignore_index=ignore, reduction="sum") / (B * H * W)
    assert abs(ref(x, y, ignore_index=ignore, avg="all")["ce"] - float(alls)) <= 1e-12 * max(1.0, float(alls))
    wt = F.cross_entropy(x, y, ignore_index=ignore, weight=torch.tensor(w, dtype=torch.float32).double())
    assert abs(ref(x, y, ignore_index=ignore, avg="weight", alpha=w)["ce"] - float(wt)) <= 1e-12 * max(1.0, float(wt))
    # weighted, averaged over the valid pixels: what DenseCrossEntropy(class_weight=) asks for
    wv = F.cross_entropy(x, y, ignore_index=ignore, weight=torch.tensor(w, dtype=torch.float32).double(), reduction="sum") / r["n_valid"]
    assert abs(ref(x, y, ignore_index=ignore, avg="valid", alpha=w)["ce"] - float(wv)) <= 1e-12 * max(1.0, float(wv))
    # labels outside [0, K) are ignored whatever ignore_index says, and pred / conf follow the argmax
    y2 = y.clone()
    y2[y2 == ignore] = -1
    r2 = ref(x, y2, avg="valid")
    assert r2["ce"] == r["ce"] and np.array_equal(r2["conf"], r["conf"]) and int(r["conf"].sum()) == r["n_valid"]
    assert np.array_equal(r["pred"], x.argmax(1).numpy().astype(np.uint8)) and np.array_equal(r["T"], r["conf"].sum(1))


@pytest.mark.parametrize("mode", [dict(), dict(gamma=2.0, alpha="w", avg="weight"), dict(ce=0.0, dice=1.0), dict(ce=0.0, jaccard=1.0), dict(dice=1.0, avg="all"),
                                  dict(ce=0.7, dice=0.4, jaccard=0.5, gamma=2.0, alpha="w", avg="valid")], ids=["ce", "focal", "dice", "jaccard", "hybrid", "everything"])
def test_closed_form_gradient_is_autograd(mode):
    for B, K, H, W, ignore in [(2, 2, 5, 7, 255), (1, 5, 9, 4, 5), (2, 4, 6, 6, 1)]:
        x, y = ignored_case(B, K, H, W, 7 * K + H, ignore)
        kw = dict(mode)
        if kw.get("alpha") == "w":
            kw["alpha"] = [0.5 + 0.25 * k for k in range(K)]
        xt = x.clone().requires_grad_(True)
        loss, parts = torch_dense(xt, y, ignore_index=ignore, **kw)
        loss.backward()
        r = D().reference_dense(x, y, ignore_index=ignore, gout=0.4, **kw)
        assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
        for k in ("I", "P", "T"):
            assert np.abs(r[k] - parts[k].detach().numpy()).max() <= 1e-12 * max(1.0, float(parts[k].detach().abs().max()))
        g = 0.4 * xt.grad.numpy()
        assert np.abs(r["dlogits"] - g).max() <= 1e-12 * max(1.0, float(np.abs(g).max())), mode
        assert not r["dlogits"].reshape(B, K, -1).transpose(0, 2, 1)[(y.reshape(B, -1) == ignore).numpy()].any()          # ignored pixels: exact zeros
        st = r["stats"]
        assert st.shape == (6 + 5 * K,) and st[0] == r["loss"] and st[4] == r["n_valid"] and st[5] == r["inv_D"] and np.array_equal(st[6 + 4 * K:], r["T"])


def test_reference_edge_cases():
    ref = D().reference_dense
    x, y = ignored_case(2, 3, 4, 5, 1, 255)
    none = ref(x, torch.full_like(y, 255), ignore_index=255, dice=1.0)
    assert none["ce"] == 0.0 and none["n_valid"] == 0 and none["inv_D"] == 0.0 and not none["dlogits"].any() and not none["conf"].any() and none["dice"] == 1.0
    one = ref(x, torch.full_like(y, 1), ce=0.0, dice=1.0, jaccard=1.0)          # a single class in the image: the absent classes' terms are 0
    assert one["T"].tolist() == [0, 40, 0] and one["I"][0] == 0.0 and one["I"][2] == 0.0 and np.isfinite(one["dlogits"]).all()
    big = ref(torch.tensor([80.0, -80.0, 80.0, -80.0]).reshape(1, 2, 1, 2), torch.tensor([[[0, 0]]]))          # pixels (80, 80) and (-80, -80): p = 1 / 2
    assert abs(big["ce"] - np.log(2.0)) <= 1e-12
    far = ref(torch.tensor([80.0, -80.0]).reshape(1, 2, 1, 1), torch.tensor([[[1]]]))
    assert abs(far["ce"] - 160.0) <= 1e-12 and far["pred"].tolist() == [[[0]]]
    nan = float("nan")
    tie = ref(torch.tensor([[0.0, nan, 1.0, -0.0], [-0.0, nan, 1.0, 0.0], [0.0, 2.0, nan, -0.0]]).reshape(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
    assert tie["pred"].reshape(-1).tolist() == [0, 0, 2, 0]          # -0 == +0: the first; a NaN beats every number, the first NaN wins


# ---- SegMeter.compute ----------------------------------------------------------------------------------------------------------------------------------
def test_seg_meter_arithmetic():
    dense = D()
    conf = torch.tensor([[50, 10], [5, 35]])          # conf[label, prediction]: tn = 50, fp = 10, fn = 5, tp = 35
    m = dense.SegMeter(2).merge([(conf, torch.tensor([25.0, 100.0], dtype=torch.float64))]).compute()
    assert (m["tn"], m["fp"], m["fn"], m["tp"]) == (50, 10, 5, 35) and m["count"] == 100 and m["loss"] == 0.25 and m["aAcc"] == 0.85
    P, R = 35 / 45, 35 / 40
    assert m["precision"] == P and m["recall"] == R and m["f1"] == 2 * P * R / (R + P)          # eval.py:64-67
    assert m["IoU"].tolist() == [50 / 65, 35 / 50] and m["Acc"].tolist() == [50 / 60, 35 / 40] and m["Precision"].tolist() == [50 / 55, 35 / 45]
    assert m["mIoU"] == (50 / 65 + 35 / 50) / 2 and m["mAcc"] == (50 / 60 + 35 / 40) / 2 and abs(m["F1"][1] - m["f1"]) <= 1e-15
    # three classes, class 2 absent from labels and predictions: NaN per class, left out of the means
    c3 = torch.tensor([[8, 2, 0], [1, 9, 0], [0, 0, 0]])
    meter = dense.SegMeter(3, ignore_index=255)
    meter.merge([(c3, torch.tensor([4.0, 20.0], dtype=torch.float64)), (c3, torch.tensor([6.0, 20.0], dtype=torch.float64))])
    assert torch.equal(meter.state[0], 2 * c3) and meter.state[1].tolist() == [10.0, 40.0]
    m3 = meter.compute()
    assert np.isnan(m3["IoU"][2]) and np.isnan(m3["Acc"][2]) and np.isnan(m3["Precision"][2]) and np.isnan(m3["F1"][2]) and "tp" not in m3
    assert m3["IoU"][:2].tolist() == [16 / 22, 18 / 24] and m3["mIoU"] == (16 / 22 + 18 / 24) / 2 and m3["mAcc"] == (0.8 + 0.9) / 2 and m3["aAcc"] == 34 / 40
    assert m3["loss"] == 0.25 and m3["count"] == 40
    # a class that is predicted but never labelled: IoU 0 (it counts), recall NaN (it does not)
    c4 = dense.seg_metrics(np.array([[5, 0, 1], [0, 4, 0], [0, 0, 0]]), (0.0, 0.0))
    assert c4["IoU"][2] == 0.0 and np.isnan(c4["Acc"][2]) and c4["mIoU"] == (5 / 6 + 1.0 + 0.0) / 3 and c4["mAcc"] == (5 / 6 + 1.0) / 2 and np.isnan(c4["loss"])
    meter.reset()
    assert not meter.state[0].any() and meter.state[1].tolist() == [0.0, 0.0]
    with pytest.raises(TypeError):
        meter.merge([(conf, torch.zeros(2, dtype=torch.float64))])
    with pytest.raises(RuntimeError):
        dense.SegMeter(2).compute()
    with pytest.raises(ValueError):
        dense.SegMeter(1)
    with pytest.raises(ValueError):
        dense.SegMeter(65)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_counts():
    import lemevit_amd
    from lemevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl, f"{name} not declared"
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 24, 21]
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14 and re.search(r"#define\s+LMV_ABI_VERSION\s+14\b", src)          # a pure addition
    assert re.search(r"#define\s+LMV_DENSE_MAX_CLASSES\s+64\b", src) and re.search(r"#define\s+LMV_DENSE_STATS_HEAD\s+6\b", src)
    assert (_lib.DENSE_MAX_CLASSES, _lib.DENSE_STATS_HEAD) == (64, 6)
    assert re.search(r"LMV_DENSE_LABEL_I64\s*=\s*0,\s*LMV_DENSE_LABEL_U8\s*=\s*1", src) and (_lib.DENSE_LABEL_I64, _lib.DENSE_LABEL_U8) == (0, 1)
    assert re.search(r"LMV_DENSE_AVG_VALID\s*=\s*0,\s*LMV_DENSE_AVG_ALL\s*=\s*1,\s*LMV_DENSE_AVG_WEIGHT\s*=\s*2", src)
    assert (_lib.DENSE_AVG_VALID, _lib.DENSE_AVG_ALL, _lib.DENSE_AVG_WEIGHT) == (0, 1, 2)
    assert "dense.hip" in open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()
    for name in ("DenseLoss", "SegMeter", "hybrid_loss", "dice_loss", "jaccard_loss", "FocalLoss", "DenseCrossEntropy", "reference_dense"):
        assert getattr(lemevit_amd, name) is getattr(lemevit_amd.dense, name) and name in lemevit_amd.__all__
    assert all(hasattr(lemevit_amd.ops, n) for n in ("dense_loss_fwd", "dense_loss_bwd", "dense_workspace"))
    ws = _lib.lib.lmv_dense_loss_workspace_bytes
    assert ws(1, 2, 1) == 9 * 4 and ws(8, 2, 256 * 256) == 512 * 9 * 4 and ws(10, 5, 512 * 512) == 1024 * 18 * 4 and ws(1, 64, 99) == 195 * 4
    assert ws(0, 2, 4) == 0 and ws(1, 1, 4) == 0 and ws(1, 65, 4) == 0 and ws(2, 2, 1 << 30) == 0


def test_argument_validation_without_gpu():
    """Each refusal the header lists returns LMV_ERR_SHAPE (-1) with a message that starts ``dense_loss`` before any launch; the buffers are host memory that is
    never touched."""
    from lemevit_amd._lib import lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0 or p % 8 == 0
    F32, BF16 = 0, 1
    big = 1 << 20

    def common(kw):
        a = dict(logits=p, dtype=F32, sb=24, sc=12, B=2, K=2, HW=12, labels=p, ldtype=0, ignore=255, alpha=None, gamma=0.0, w_ce=1.0, w_dice=0.0, w_jac=0.0,
                 eps=1e-7, avg=0)
        a.update(kw)
        return [a[k] for k in ("logits", "dtype", "sb", "sc", "B", "K", "HW", "labels", "ldtype", "ignore", "alpha", "gamma", "w_ce", "w_dice", "w_jac", "eps", "avg")]

    def fwd(**kw):
        t = dict(ws=p, ws_bytes=big, stats=p, pred=None, conf=None, meter=None)
        t.update({k: kw.pop(k) for k in list(kw) if k in t})
        rc = lib.lmv_dense_loss_fwd(*common(kw), t["ws"], t["ws_bytes"], t["stats"], t["pred"], t["conf"], t["meter"], None)
        return rc, lib.lmv_last_error().decode()

    def bwd(**kw):
        t = dict(stats=p, gout=None, dl=p)
        t.update({k: kw.pop(k) for k in list(kw) if k in t})
        rc = lib.lmv_dense_loss_bwd(*common(kw), t["stats"], t["gout"], t["dl"], None)
        return rc, lib.lmv_last_error().decode()

    shared = [(dict(logits=None), "null"), (dict(labels=None), "null"), (dict(K=1, sb=12), "outside 2 .. 64"), (dict(K=65, sb=12 * 65), "outside 2 .. 64"),
              (dict(B=0), "bad shape"), (dict(HW=0), "bad shape"), (dict(B=2, HW=1 << 30, sc=1 << 30, sb=1 << 31), "bad shape"),
              (dict(dtype=2), "logits dtype"), (dict(dtype=7), "logits dtype"), (dict(ldtype=2), "label dtype"), (dict(ldtype=-1), "label dtype"),
              (dict(sc=11), "class stride"), (dict(sb=23), "batch stride"), (dict(K=3, sb=35), "batch stride"),
              (dict(w_ce=-1.0), "negative loss weight"), (dict(w_dice=-0.5), "negative loss weight"), (dict(w_jac=-2.0), "negative loss weight"),
              (dict(w_ce=float("nan")), "negative loss weight"), (dict(gamma=-1.0), "gamma"), (dict(eps=0.0), "eps"), (dict(eps=-1e-7), "eps"),
              (dict(avg=3), "avg_mode"), (dict(avg=-1), "avg_mode"),
              (dict(logits=p + 2), "misaligned"), (dict(logits=p + 1, dtype=BF16), "misaligned"), (dict(labels=p + 4), "misaligned"), (dict(alpha=p + 2), "misaligned")]
    for call, name, extra in [(fwd, "dense_loss_fwd", [(dict(ws=None), "null"), (dict(stats=None), "null"), (dict(ws_bytes=35), "workspace of 35 bytes"),
                                                       (dict(ws_bytes=0), "workspace of 0 bytes"), (dict(ws=p + 2), "misaligned"), (dict(stats=p + 1), "misaligned"),
                                                       (dict(conf=p + 4), "misaligned"), (dict(meter=p + 4), "misaligned")]),
                              (bwd, "dense_loss_bwd", [(dict(stats=None), "null"), (dict(dl=None), "null"), (dict(stats=p + 2), "misaligned"), (dict(gout=p + 2), "misaligned"),
                                                       (dict(dl=p + 2), "misaligned"), (dict(dl=p + 1, dtype=BF16), "misaligned")])]:
        for kw, msg in shared + extra:
            rc, err = call(**dict(kw))
            assert rc == -1 and msg in err and err.startswith(name + ":"), (name, kw, rc, err)
    assert fwd(labels=p + 1, ldtype=1, K=70, sb=12 * 70)[0] == -1          # (uint8 labels need no alignment: the refusal here is K)


def test_python_side_refusals_without_gpu():
    """ops.dense_* and the dense surface raise on the Python side for what the ABI would refuse (and never compute on the CPU)."""
    from lemevit_amd import ops
    dense = D()
    x, y = torch.randn(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dense_loss_fwd(x, y)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dense_loss_bwd(x, y, torch.zeros(21))
    with pytest.raises(RuntimeError, match="GPU"):
        dense.DenseLoss()(x, y)
    with pytest.raises(RuntimeError, match="GPU"):
        dense.hybrid_loss([x, x], y[:, None])
    with pytest.raises(RuntimeError, match="GPU"):
        dense.SegMeter(3).update(x, y)
    with pytest.raises(ValueError, match="B, K, H, W"):
        ops.dense_loss_fwd(x[0], y)
    with pytest.raises(ValueError):
        ops.dense_workspace(0, 2, 16, "cpu")
    with pytest.raises(ValueError):
        ops.dense_workspace(1, 65, 16, "cpu")
    for kw in (dict(ce=-1.0), dict(dice=-1.0), dict(jaccard=-1.0), dict(gamma=-0.5), dict(eps=0.0), dict(avg="mean")):
        with pytest.raises(ValueError):
            dense.DenseLoss(**kw)
    with pytest.raises(ValueError, match="an empty list"):
        dense.DenseLoss()([], y)
    with pytest.raises(ValueError, match="classes"):
        dense.SegMeter(2)._check(3, None)
    with pytest.raises(ValueError, match="must agree"):
        dense.SegMeter(3, ignore_index=255)._check(3, None)
    f = dense.FocalLoss(gamma=2, alpha=0.25)
    assert f.crit.alpha.dtype == torch.float32 and f.crit.alpha.tolist() == [0.25, 0.75] and f.crit.avg == "all" and f.crit.gamma == 2.0
    c = dense.DenseCrossEntropy(ignore_index=255, loss_weight=0.4, class_weight=[1.0, 2.0, 3.0], avg_non_ignore=False)
    assert c.crit.ce == 0.4 and c.crit.avg == "all" and c.crit.ignore_index == 255 and c.crit.alpha.tolist() == [1.0, 2.0, 3.0]
    assert dense.DenseCrossEntropy().crit.avg == "valid" and dense.DenseCrossEntropy().crit.ignore_index == -100
