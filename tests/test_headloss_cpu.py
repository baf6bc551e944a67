"""The head losses without a GPU (lemevit_amd/detection.py: rpn_head_loss, bbox_head_loss; csrc/headloss.hip): the conditions the generated inputs must meet, the
float64 oracles against central differences of their own losses and against the stock formulations run in float64 on the CPU, the averaging rule by hand, and
the argument checks of the four entry points (LMV_ERR_SHAPE and the message prefixes)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen_headloss_golden as gen  # noqa: E402
from lemevit_amd import detection as det  # noqa: E402


def rpn_oracle(c, gout=None, **over):
    kw = dict(cls_scores=c["cls_scores"], bbox_preds=c["bbox_preds"])
    kw.update(over)
    return det.reference_rpn_head_loss(kw["cls_scores"], kw["bbox_preds"], c["anchors"], c["gts"], c["gt_inds"], c["mask"], c["counts"], (0.0,) * 6, gen.RPN_STDS,
                                       gen.RPN_BETA, 1.0, 1.0, gout)


def rcnn_oracle(c, gout=None, **over):
    kw = dict(cls_score=c["cls_score"], bbox_pred=c["bbox_pred"])
    kw.update(over)
    return det.reference_bbox_head_loss(kw["cls_score"], kw["bbox_pred"], c["rois"], c["gts"], c["s_gt_inds"], c["s_labels"], c["counts"], (0.0,) * 5, gen.RCNN_STDS,
                                        c["K"], gen.RCNN_BETA, 1.0, 1.0, gout)


def test_generated_conditions():
    """every condition the issue sets for the generated inputs"""
    seen = dict(no_pos=False, no_sample=False, count0=False, empty_level=False)
    for name in gen.RPN_CASES:
        c = gen.rpn_case(name)
        m, ind, cnt, offs = c["mask"].numpy(), c["gt_inds"].numpy(), c["counts"].numpy(), c["offsets"]
        assert c["N"] == offs[-1] == sum(h * w * c["A"] for h, w in c["levels"]) and m.shape == (c["B"], c["N"]) and set(np.unique(m)) <= {0, 1, 2}
        assert m[0, 0] != 0 and (m[0, -1] != 0 or name == "i")          # the first and the last element (case i: its last level is the one without a sample)
        pos0 = ind[0][m[0] == 1]
        assert {-1, 0, int(cnt[0]) + 1} <= set(pos0.tolist())          # mask == 1 rows that are not live
        assert ((pos0 >= 1) & (pos0 <= cnt[0])).any()                   # ... and live ones
        for b in range(c["B"]):
            seen["no_pos"] |= bool((m[b] == 1).sum() == 0 and (m[b] != 0).sum() > 0)
            seen["no_sample"] |= bool((m[b] != 0).sum() == 0)
            seen["count0"] |= bool(cnt[b] == 0 and (m[b] == 1).sum() > 0)
        for l in range(len(c["levels"])):
            seen["empty_level"] |= bool((m[:, offs[l]:offs[l + 1]] != 0).sum() == 0)
    assert all(seen.values()), seen
    ii = gen.rpn_case("ii")
    n0 = int(ii["offsets"][1])
    assert n0 == 1653 and n0 > 1024 and n0 % 16 != 0 and ii["N"] % 16 != 0 and gen.rpn_case("i")["N"] % 16 == 0
    assert (ii["mask"].numpy()[0, 1024:n0] != 0).any() and (ii["mask"].numpy()[0, n0:] != 0).any()          # past the first wave's span, and on the second level
    assert gen.rpn_case("iii")["A"] == 1
    assert {gen.RCNN_CASES[f"r{R}"][0] for R in (1, 63, 64, 65, 257, 1000)} == {1, 63, 64, 65, 257, 1000}
    assert gen.RCNN_CASES["c15"][1:3] == (15, 15) and gen.RCNN_CASES["k1"][1] == 1
    for name in gen.RCNN_CASES:
        for bf16 in (False, True):
            c = gen.rcnn_case(name, bf16)
            z, lab, roi = c["cls_score"].double().numpy(), c["s_labels"].numpy(), c["rois"].numpy()
            top = np.sort(z, 1)[:, -2:]
            assert (top[:, 1] - top[:, 0] >= gen.GAP).all()
            assert ((lab == -1) == (roi[:, 0] == -1)).all()
            if bf16:
                assert torch.equal(c["cls_score"].bfloat16().float(), c["cls_score"]) and torch.equal(c["bbox_pred"].bfloat16().float(), c["bbox_pred"])
    assert (gen.rcnn_case("r257")["s_labels"].numpy() == -1).any()
    o = rcnn_oracle(gen.rcnn_case("nopos"))
    assert o["n_live"] == 0 and o["n_valid"] == 65 and o["loss_bbox"] == 0.0 and o["loss_cls"] > 0
    o = rcnn_oracle(gen.rcnn_case("allpad"))
    assert o["n_valid"] == 0 and o["loss_cls"] == 0.0 and o["acc"] == 0.0 and not o["dcls"].any()
    o = rcnn_oracle(gen.rcnn_case("r1000"))
    assert 0 < o["n_live"] < o["n_valid"] < 1000
    for bf16 in (False, True):
        c = gen.rpn_case("i", bf16)
        assert all(torch.equal(t.bfloat16().float(), t) for t in c["cls_scores"] + c["bbox_preds"]) == bf16


def _directional(loss_of, x0, grads, rng, h=1e-6, n=6):
    """central differences of a scalar loss along n random +-1 directions over all inputs against <gradient, direction>; the largest error relative to that
    directional derivative"""
    worst = 0.0
    for _ in range(n):
        v = [rng.choice([-1.0, 1.0], size=x.shape) for x in x0]
        fd = (loss_of([x + h * d for x, d in zip(x0, v)]) - loss_of([x - h * d for x, d in zip(x0, v)])) / (2 * h)
        an = sum(float((g * d).sum()) for g, d in zip(grads, v))          # the directional derivative that fd estimates
        assert an != 0.0
        worst = max(worst, abs(fd - an) / abs(an))
    return worst


@pytest.mark.parametrize("name", list(gen.RPN_CASES))
def test_rpn_oracle_gradient_is_the_derivative(name):
    """the analytic gradient of the RPN oracle against central differences of sum_i gout_i loss_i in float64 (relative 1e-6), every loss with its own gout"""
    c = gen.rpn_case(name)
    L = len(c["levels"])
    rng = np.random.default_rng(5)
    gout = rng.uniform(0.5, 2.0, 2 * L)
    x0 = [t.double().numpy() for t in c["cls_scores"] + c["bbox_preds"]]
    o = rpn_oracle(c, gout)

    def loss_of(xs):
        r = rpn_oracle(c, cls_scores=xs[:L], bbox_preds=xs[L:])
        return float((gout[:L] * r["loss_cls"]).sum() + (gout[L:] * r["loss_bbox"]).sum())
    assert _directional(loss_of, x0, o["dcls"] + o["dreg"], rng) <= 1e-6
    # single elements: a sampled positive's logit and its six deltas
    b, e = 0, int(np.nonzero((c["mask"].numpy()[0] == 1) & (c["gt_inds"].numpy()[0] >= 1) & (c["gt_inds"].numpy()[0] <= int(c["counts"][0])))[0][0])
    l = int(np.searchsorted(c["offsets"], e, side="right") - 1)
    H, W = c["levels"][l]
    r = e - int(c["offsets"][l])
    pos, a = divmod(r, c["A"])
    hh, ww = divmod(pos, W)
    for which, ch in [(l, a)] + [(L + l, a * 6 + d) for d in range(6)]:
        def at(delta):
            xs = [x.copy() for x in x0]
            xs[which][b, ch, hh, ww] += delta
            return loss_of(xs)
        fd = (at(1e-6) - at(-1e-6)) / 2e-6
        an = (o["dcls"] + o["dreg"])[which][b, ch, hh, ww]
        assert an != 0.0 and abs(fd - an) <= 1e-6 * abs(an), (which, ch, fd, an)


@pytest.mark.parametrize("name", ["r65", "r257", "c15", "k1", "nopos"])
def test_rcnn_oracle_gradient_is_the_derivative(name):
    c = gen.rcnn_case(name)
    rng = np.random.default_rng(6)
    gout = rng.uniform(0.5, 2.0, 2)
    x0 = [c["cls_score"].double().numpy(), c["bbox_pred"].double().numpy()]
    o = rcnn_oracle(c, gout)

    def loss_of(xs):
        r = rcnn_oracle(c, cls_score=xs[0], bbox_pred=xs[1])
        return float(gout[0] * r["loss_cls"] + gout[1] * r["loss_bbox"])
    assert _directional(loss_of, x0, [o["dcls"], o["dbbox"]], rng) <= 1e-6
    live = (c["s_labels"].numpy() >= 0) & (c["s_labels"].numpy() < c["K"]) & (np.abs(o["dbbox"]).sum(1) > 0)
    if live.any():          # single elements of a live row: the label's logit, the largest other logit, and the five deltas of the chosen set
        r, lab = int(np.nonzero(live)[0][0]), int(c["s_labels"][np.nonzero(live)[0][0]])
        base = 0 if c["C"] == 1 else 5 * lab
        other = int(np.argsort(np.where(np.arange(c["K"] + 1) == lab, -np.inf, x0[0][r]))[-1])          # the largest other logit: a derivative above the round-off of fd
        for which, col in [(0, lab), (0, other)] + [(1, base + d) for d in range(5)]:
            def at(delta):
                xs = [x.copy() for x in x0]
                xs[which][r, col] += delta
                return loss_of(xs)
            fd = (at(1e-4) - at(-1e-4)) / 2e-4          # (h = 1e-4: the loss is O(10), so its round-off over 2 h stays below 1e-6 of a derivative of 1e-3)
            an = (o["dcls"], o["dbbox"])[which][r, col]
            assert an != 0.0 and abs(fd - an) <= 1e-6 * abs(an), (which, col, fd, an)
    else:
        assert name == "nopos"
    pad = c["s_labels"].numpy() < 0
    assert not o["dcls"][pad].any() and not o["dbbox"][pad].any()
    if c["C"] > 1:          # only the label's set of a live row
        nz = np.abs(o["dbbox"]).reshape(c["R"], c["C"], 5).sum(2) > 0
        assert (nz.sum(1) <= 1).all() and nz.any() and (np.nonzero(nz)[1] == c["s_labels"].numpy()[np.nonzero(nz)[0]]).all()


def _err(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if ref.size else 0.0
    return 0.0 if x.size == 0 or np.array_equal(x, ref) else float(np.abs(x - ref).max() / scale) if scale > 0 else float("inf")


@pytest.mark.parametrize("name", list(gen.RPN_CASES))
def test_rpn_stock_float64_agrees_with_oracle(name):
    """the stock formulation in float64 on the CPU and the oracle: losses (|x - ref| / S, S = the oracle's loss: every term is non-negative) and autograd's
    gradients against the analytic ones, 1e-12"""
    c = gen.rpn_case(name)
    L = len(c["levels"])
    gout = np.linspace(0.5, 1.5, 2 * L)
    maps = [t.double().requires_grad_() for t in c["cls_scores"] + c["bbox_preds"]]
    out = det.rpn_head_loss_torch(maps[:L], maps[L:], c["anchors"].double(), c["gts"].double(), c["gt_inds"], c["mask"], c["counts"], (0.0,) * 6, gen.RPN_STDS,
                                  gen.RPN_BETA)
    o = rpn_oracle(c, gout)
    for l in range(L):
        for got, ref in ((out["loss_rpn_cls"][l], o["loss_cls"][l]), (out["loss_rpn_bbox"][l], o["loss_bbox"][l])):
            assert abs(float(got.detach()) - ref) <= 1e-12 * ref, (name, l, float(got.detach()), ref)
    g = torch.from_numpy(gout)
    ((out["loss_rpn_cls"] * g[:L]).sum() + (out["loss_rpn_bbox"] * g[L:]).sum()).backward()
    for m, ref in zip(maps, o["dcls"] + o["dreg"]):
        assert _err(m.grad.numpy(), ref) <= 1e-12


@pytest.mark.parametrize("name", list(gen.RCNN_CASES))
def test_rcnn_stock_float64_agrees_with_oracle(name):
    c = gen.rcnn_case(name)
    z, p = c["cls_score"].double().requires_grad_(), c["bbox_pred"].double().requires_grad_()
    out = det.bbox_head_loss_torch(z, p, c["rois"].double(), c["gts"].double(), c["s_gt_inds"], c["s_labels"], c["counts"], (0.0,) * 5, gen.RCNN_STDS, c["K"],
                                   c["C"] == 1, gen.RCNN_BETA)
    o = rcnn_oracle(c, np.array([0.75, 1.25]))
    assert abs(float(out["loss_cls"]) - o["loss_cls"]) <= 1e-12 * o["loss_cls"] and abs(float(out["loss_bbox"]) - o["loss_bbox"]) <= 1e-12 * o["loss_bbox"]
    assert float(out["acc"]) == o["acc"] and not out["acc"].requires_grad
    (0.75 * out["loss_cls"] + 1.25 * out["loss_bbox"]).backward()
    assert _err(z.grad.numpy(), o["dcls"]) <= 1e-12 and _err(p.grad.numpy(), o["dbbox"]) <= 1e-12


def test_avg_rule_by_hand():
    """num_total_samples with an image that has no positive (case i): avg = max(27, 1) + max(7, 1) + max(0, 1) + max(40, 1) = 75, not 74"""
    c = gen.rpn_case("i")
    m = c["mask"].numpy()
    assert (m == 1).sum(1).tolist() == [27, 0] and (m == 2).sum(1).tolist() == [7, 40]
    o = rpn_oracle(c)
    assert o["avg"] == 27 + 7 + 1 + 40 == 75 and o["n_pos"] == 27 and o["n_neg"] == 47
    z = c["cls_scores"][0].double().permute(0, 2, 3, 1).reshape(2, -1).numpy()
    m0 = m[:, :z.shape[1]]
    terms = np.maximum(z, 0) - z * (m0 == 1) + np.log1p(np.exp(-np.abs(z)))
    assert abs(o["loss_cls"][0] - terms[m0 != 0].sum() / 75.0) <= 1e-15
    assert o["loss_cls"][2] == 0.0 and o["loss_bbox"][2] == 0.0 and not o["dcls"][2].any() and not o["dreg"][2].any()          # the level without a sample
    # the same losses on a mask without the negatives: loss_bbox scales by the ratio of the two avg
    c2 = dict(c, mask=torch.from_numpy(np.where(m == 1, 1, 0).astype(np.uint8)))
    o2 = rpn_oracle(c2)
    assert o2["avg"] == 27 + 1 + 1 + 1 and np.allclose(o2["loss_bbox"] * o2["avg"], o["loss_bbox"] * o["avg"], rtol=1e-14, atol=0)


def test_symbols():
    """the entry points are declared in include/lemevit_hip.h, exported and bound; the header states the constants; the ABI version stays 14"""
    from lemevit_amd import _lib
    import lemevit_amd
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lmv_rpn_loss_fwd", "lmv_rpn_loss_bwd", "lmv_rcnn_loss_fwd", "lmv_rcnn_loss_bwd"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    for name in ("lmv_rpn_loss_workspace_bytes", "lmv_rcnn_loss_workspace_bytes"):
        assert re.search(r"\bsize_t " + name + r"\(", src) and hasattr(raw, name) and name in _lib.SIGNATURES
    assert int(re.search(r"#define LMV_RPN_LOSS_MAX_LEVELS (\d+)", src).group(1)) == _lib.RPN_LOSS_MAX_LEVELS
    assert int(re.search(r"#define LMV_RCNN_LOSS_STATS (\d+)", src).group(1)) == _lib.RCNN_LOSS_STATS
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    mk = open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()
    assert "headloss.hip" in mk and re.search(r"coder\.o headloss\.o: coder_rules\.h", mk)
    assert '#include "coder_rules.h"' in open(os.path.join(ROOT, "lemevit_amd", "csrc", "coder.hip")).read()
    assert _lib.lib.lmv_rpn_loss_workspace_bytes(8, 261888) == 8 * 256 * 48 and _lib.lib.lmv_rpn_loss_workspace_bytes(0, 10) == 0
    assert _lib.lib.lmv_rcnn_loss_workspace_bytes(4096) == 64 * 32 and _lib.lib.lmv_rcnn_loss_workspace_bytes(0) == 0 and _lib.lib.lmv_rcnn_loss_workspace_bytes(-1) == 0
    for name in ("rpn_head_loss", "bbox_head_loss", "rpn_head_loss_torch", "bbox_head_loss_torch", "reference_rpn_head_loss", "reference_bbox_head_loss"):
        assert getattr(lemevit_amd, name) is getattr(det, name) and name in lemevit_amd.__all__


def test_refusals_without_gpu():
    """Argument validation happens before any launch: LMV_ERR_SHAPE and a message that starts with the entry point's name"""
    from lemevit_amd import _lib
    from lemevit_amd._lib import lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    F = ctypes.c_float
    m6, s6, m5, s5 = (F * 6)(), (F * 6)(1, 1, 1, 1, 0.5, 0.5), (F * 5)(), (F * 5)(0.1, 0.1, 0.2, 0.2, 0.1)
    nan6 = (F * 6)(0, 0, float("nan"), 0, 0, 0)
    nan, inf = float("nan"), float("inf")

    def level(H=5, W=7, A=3, cls=p, reg=p, dcls=p, dreg=p, cls_stride=None, reg_stride=None):
        lv = _lib.RpnLossLevel()
        lv.cls, lv.reg, lv.dcls, lv.dreg, lv.H, lv.W = cls, reg, dcls, dreg, H, W
        st = lambda ch: (ctypes.c_int64 * 4)(ch * H * W, H * W, W, 1)          # noqa: E731
        lv.cls_stride, lv.reg_stride = cls_stride or st(A), reg_stride or st(6 * A)
        lv.dcls_stride, lv.dreg_stride = st(A), st(6 * A)
        return lv

    def table(*lv):
        return (_lib.RpnLossLevel * len(lv))(*lv)

    def rpn(bwd=False, levels=None, L=1, A=3, dtype=0, B=2, mask=p, anchors=p, a_s=4, a_b=0, gts=p, gs=5, Gmax=4, counts=None, inds=p, kind=0, means=m6, stds=s6,
            beta=1 / 9, wc=1.0, wb=1.0, ws=p, ws_bytes=1 << 12, stats=p, gout=None):
        levels = table(level()) if levels is None else levels
        head = (levels, L, A, dtype, B, mask, anchors, a_s, a_b, gts, gs, Gmax, counts, inds, kind, means, stds, beta, wc, wb)
        return lib.lmv_rpn_loss_bwd(*head, stats, gout, None) if bwd else lib.lmv_rpn_loss_fwd(*head, ws, ws_bytes, stats, None)

    def rcnn(bwd=False, cls=p, cs=16, box=p, bs=5, dtype=0, R=8, K=15, C=1, rois=p, rs=6, inds=p, labels=p, gts=p, gs=5, B=2, Gmax=4, counts=None, kind=1, means=m5,
             stds=s5, beta=1.0, wc=1.0, wb=1.0, ws=p, ws_bytes=1 << 12, stats=p, gout=None, dcls=p, dcs=16, dbox=p, dbs=5):
        head = (cls, cs, box, bs, dtype, R, K, C, rois, rs, inds, labels, gts, gs, B, Gmax, counts, kind, means, stds, beta, wc, wb)
        return lib.lmv_rcnn_loss_bwd(*head, stats, gout, dcls, dcs, dbox, dbs, None) if bwd else lib.lmv_rcnn_loss_fwd(*head, ws, ws_bytes, stats, None)

    def msg():
        return lib.lmv_last_error()

    for bwd, prefix in ((False, b"rpn_loss_fwd"), (True, b"rpn_loss_bwd")):
        assert rpn(bwd, kind=1) == -1 and msg().startswith(prefix) and b"unknown kind" in msg()
        assert rpn(bwd, dtype=2) == -1 and msg().startswith(prefix) and b"unknown dtype" in msg()
        assert rpn(bwd, L=0) == -1 and b"levels" in msg() and rpn(bwd, L=6) == -1 and rpn(bwd, levels=ctypes.cast(None, ctypes.POINTER(_lib.RpnLossLevel))) == -1
        assert rpn(bwd, A=0) == -1 and b"anchors per position" in msg() and rpn(bwd, B=0) == -1 and b"images" in msg() and rpn(bwd, B=4097) == -1
        assert rpn(bwd, Gmax=-1) == -1 and rpn(bwd, a_s=3) == -1 and b"row strides" in msg() and rpn(bwd, gs=4) == -1 and rpn(bwd, a_b=-1) == -1
        for beta in (0.0, -1.0, nan, inf):
            assert rpn(bwd, beta=beta) == -1 and b"beta" in msg()
        assert rpn(bwd, wc=-1.0) == -1 and b"loss weight" in msg() and rpn(bwd, wb=nan) == -1 and b"loss weight" in msg()
        assert rpn(bwd, means=None) == -1 and b"null means" in msg() and rpn(bwd, stds=nan6) == -1 and b"NaN" in msg()
        assert rpn(bwd, levels=table(level(H=0))) == -1 and b"positions" in msg()
        assert rpn(bwd, levels=table(level(cls=None))) == -1 and b"null class map" in msg() and rpn(bwd, levels=table(level(reg=None))) == -1
        assert rpn(bwd, levels=table(level(cls=p + 2))) == -1 and b"misaligned" in msg() and rpn(bwd, dtype=1, levels=table(level(reg=p + 1))) == -1
        assert rpn(bwd, levels=table(level(cls_stride=(ctypes.c_int64 * 4)(104, 35, 7, 1)))) == -1 and b"smaller than the extent" in msg()          # batch stride < 105
        assert rpn(bwd, levels=table(level(reg_stride=(ctypes.c_int64 * 4)(630, 35, 7, 0)))) == -1 and b"smaller than the extent" in msg()
        assert rpn(bwd, levels=table(level(H=1024, W=1024), level(H=1024, W=1024)), L=2, A=1) == -1 and b"exceeds" in msg()
        assert rpn(bwd, mask=None) == -1 and b"null mask" in msg() and rpn(bwd, anchors=None) == -1 and rpn(bwd, inds=None) == -1 and rpn(bwd, gts=None) == -1
        assert rpn(bwd, inds=p + 4) == -1 and b"misaligned" in msg() and rpn(bwd, stats=None) == -1 and msg().startswith(prefix)
    assert rpn(ws=None) == -1 and b"workspace" in msg() and rpn(ws_bytes=95) == -1 and b"workspace" in msg() and rpn(ws=p + 8) == -1 and msg().startswith(b"rpn_loss_fwd")
    assert rpn(True, levels=table(level(dcls=None))) == -1 and b"null class gradient" in msg() and rpn(True, gout=p + 2) == -1

    for bwd, prefix in ((False, b"rcnn_loss_fwd"), (True, b"rcnn_loss_bwd")):
        assert rcnn(bwd, kind=0) == -1 and msg().startswith(prefix) and b"unknown kind" in msg() and rcnn(bwd, dtype=3) == -1 and b"unknown dtype" in msg()
        assert rcnn(bwd, R=-1) == -1 and rcnn(bwd, R=(1 << 20) + 1) == -1 and b"rows" in msg()
        assert rcnn(bwd, K=0) == -1 and b"classes" in msg() and rcnn(bwd, K=128, cs=129) == -1 and rcnn(bwd, C=2) == -1 and b"delta sets" in msg()
        assert rcnn(bwd, B=0) == -1 and rcnn(bwd, Gmax=-1) == -1
        assert rcnn(bwd, cs=15) == -1 and b"row strides" in msg() and rcnn(bwd, C=15, bs=74) == -1 and rcnn(bwd, rs=5) == -1 and rcnn(bwd, gs=4) == -1
        for beta in (0.0, nan, inf):
            assert rcnn(bwd, beta=beta) == -1 and b"beta" in msg()
        assert rcnn(bwd, wc=nan) == -1 and rcnn(bwd, wb=-0.5) == -1 and b"loss weight" in msg()
        assert rcnn(bwd, means=None) == -1 and rcnn(bwd, cls=None) == -1 and b"null cls_score" in msg() and rcnn(bwd, labels=None) == -1 and rcnn(bwd, gts=None) == -1
        assert rcnn(bwd, cls=p + 2) == -1 and b"misaligned" in msg() and rcnn(bwd, labels=p + 4) == -1 and rcnn(bwd, stats=None) == -1 and msg().startswith(prefix)
    assert rcnn(ws=None) == -1 and b"workspace" in msg() and rcnn(ws_bytes=31) == -1 and rcnn(R=65, ws_bytes=63) == -1 and b"workspace" in msg()
    assert rcnn(True, dcs=15) == -1 and b"gradient row strides" in msg() and rcnn(True, dcls=None) == -1 and rcnn(True, dbox=p + 1) == -1 and b"misaligned" in msg()
    assert rcnn(True, R=0, cls=None, box=None, rois=None, inds=None, labels=None, dcls=None, dbox=None) == 0          # nothing to write: no launch


def test_python_checks_without_gpu():
    """the wrappers' own checks come before any pointer is taken; there is no CPU fallback"""
    from lemevit_amd import ops
    c = gen.rpn_case("iii")
    args = (c["cls_scores"], c["bbox_preds"], c["anchors"], c["gts"], c["gt_inds"], c["mask"], c["counts"])
    with pytest.raises((RuntimeError, TypeError), match="GPU"):
        det.rpn_head_loss(*args)
    with pytest.raises(ValueError, match="MidpointOffsetCoder"):
        det.rpn_head_loss(*args, coder=det.OBB2OBBDeltaXYWHTCoder())
    with pytest.raises(ValueError, match="beta"):
        det.rpn_head_loss(*args, beta=0.0)
    with pytest.raises(ValueError, match="loss weight"):
        det.rpn_head_loss(*args, loss_weight_cls=-1.0)
    with pytest.raises(ValueError, match="levels"):
        det.rpn_head_loss(c["cls_scores"], c["bbox_preds"][:1], *args[2:])
    r = gen.rcnn_case("r65")
    rargs = (r["cls_score"], r["bbox_pred"], r["rois"], r["gts"], r["s_gt_inds"], r["s_labels"], r["counts"])
    with pytest.raises(RuntimeError, match="GPU"):
        det.bbox_head_loss(*rargs)
    with pytest.raises(ValueError, match="num_classes"):
        det.bbox_head_loss(*rargs, num_classes=14)
    with pytest.raises(ValueError, match="reg_class_agnostic"):
        det.bbox_head_loss(*rargs, reg_class_agnostic=False)
    with pytest.raises(ValueError):
        ops.rpn_loss_workspace_bytes(0, 10)
    assert ops.rpn_loss_workspace_bytes(8, 261888) == 98304 and ops.rcnn_loss_workspace_bytes(4096) == 2048
