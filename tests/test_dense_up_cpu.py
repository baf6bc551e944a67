"""The dense losses on low-resolution logits, without a GPU: ``reference_dense(upsample=)`` (the numpy float64 oracle of tests/test_dense_up_gpu.py) against
PyTorch's own float64 ``F.interpolate`` + autograd, the argument refusals of lmv_dense_up_loss_fwd / _bwd (before any launch, on host buffers that are never
touched) and the Python-side refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GEOMETRIES = [((7, 9), (28, 36)), ((7, 9), (30, 37)), ((5, 6), (80, 96)), ((3, 1), (7, 5)), ((1, 1), (4, 4)), ((8, 8), (8, 8))]
IDS = ["x".join(map(str, a)) + "-" + "x".join(map(str, b)) for a, b in GEOMETRIES]


def D():
    from lemevit_amd import dense
    return dense


def draw(lo, hi, K=4, B=2, seed=0):
    g = torch.Generator().manual_seed(seed + lo[0] * 131 + hi[1])
    x = torch.randn((B, K) + lo, generator=g, dtype=torch.float64) * 3
    y = torch.randint(0, K, (B,) + hi, generator=g)
    y[torch.rand((B,) + hi, generator=g) < 0.1] = 255
    return x, y


def torch_terms(z, y, K, ignore, eps=1e-7):
    """dice and jaccard over the valid pixels, written out (include/lemevit_hip.h); z: [B, K, H, W] float64"""
    valid = (y != ignore).reshape(y.shape[0], -1)
    ys = torch.where(valid, y.reshape(y.shape[0], -1), torch.zeros_like(y.reshape(y.shape[0], -1)))
    p = F.softmax(z.reshape(z.shape[0], K, -1), dim=1)
    onehot = F.one_hot(ys, K).permute(0, 2, 1).double() * valid[:, None]
    I, P, T = (p * onehot).sum((0, 2)), (p * valid[:, None]).sum((0, 2)), onehot.sum((0, 2))
    return 1 - (2 * I / (P + T + eps)).mean(), 1 - (I / (P + T - I + eps)).mean()


@pytest.mark.parametrize("align", [False, True], ids=["half-pixel", "align-corners"])
@pytest.mark.parametrize("lo,hi", GEOMETRIES, ids=IDS)
def test_oracle_is_torch_interpolate_and_autograd(lo, hi, align):
    dense, K = D(), 4
    x, y = draw(lo, hi, K)
    zi = F.interpolate(x, size=hi, mode="bilinear", align_corners=align)
    for kw in (dict(ignore_index=255), dict(ce=0.0, dice=1.0, ignore_index=255), dict(ce=0.0, jaccard=1.0, ignore_index=255),
               dict(ce=1.0, dice=0.5, jaccard=0.25, ignore_index=255)):
        ref = dense.reference_dense(x, y, upsample=hi, align_corners=align, gout=0.4, **kw)
        assert ref["z"].shape == (2, K) + hi and float(np.abs(ref["z"] - zi.numpy()).max()) <= 1e-12
        assert ref["dlogits"].shape == (2, K) + lo and ref["margin"].shape == (2,) + hi and ref["pred"].shape == (2,) + hi
        xt = x.clone().requires_grad_(True)
        zt = F.interpolate(xt, size=hi, mode="bilinear", align_corners=align)
        dice, jac = torch_terms(zt, y, K, 255)
        loss = kw.get("ce", 1.0) * F.cross_entropy(zt, y, ignore_index=255) + kw.get("dice", 0.0) * dice + kw.get("jaccard", 0.0) * jac
        (0.4 * loss).backward()
        assert abs(ref["loss"] - float(loss.detach())) <= 1e-10, (kw, ref["loss"], float(loss.detach()))
        assert float(np.abs(ref["dlogits"] - xt.grad.numpy()).max()) <= 1e-10, kw
        srt = np.sort(zi.numpy(), axis=1)
        assert np.array_equal(ref["margin"], srt[:, -1] - srt[:, -2]) or float(np.abs(ref["margin"] - (srt[:, -1] - srt[:, -2])).max()) <= 1e-12


def test_oracle_at_the_logits_own_size_is_the_plain_oracle():
    dense = D()
    x, y = draw((6, 7), (6, 7), 3)
    a, b = dense.reference_dense(x, y, ignore_index=255, dice=1.0), dense.reference_dense(x, y, ignore_index=255, dice=1.0, upsample=(6, 7), align_corners=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    with pytest.raises(ValueError, match="upsampling only"):
        dense.reference_dense(x, y[:, :5], upsample=(5, 7))


def test_abi_additions():
    import lemevit_amd
    from lemevit_amd import _lib
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lmv_dense_up_loss_workspace_bytes", "lmv_dense_up_loss_fwd", "lmv_dense_up_loss_bwd")] == [4, 28, 25]
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14          # a pure addition: detected by symbol
    ws = _lib.lib.lmv_dense_up_loss_workspace_bytes
    # chunks of 4 pixels never cross an output row: 37 columns are 10 chunks a row
    assert ws(1, 2, 1, 1) == 9 * 4 and ws(2, 5, 30, 37) == 3 * 18 * 4 and ws(10, 6, 512, 512) == 1024 * 21 * 4 and ws(1, 64, 9, 11) == 195 * 4 * 1
    assert ws(0, 2, 4, 4) == 0 and ws(1, 1, 4, 4) == 0 and ws(1, 65, 4, 4) == 0 and ws(2, 2, 1 << 15, 1 << 15) == 0 and ws(1, 2, 0, 4) == 0
    assert "predict" in lemevit_amd.dense.__all__
    assert all(hasattr(lemevit_amd.ops, n) for n in ("dense_up_loss_fwd", "dense_up_loss_bwd", "dense_up_workspace"))


def test_argument_validation_without_gpu():
    """Each refusal the header lists returns LMV_ERR_SHAPE (-1) with a message that starts ``dense_up_loss`` before any launch; the buffers are host memory that is
    never touched."""
    from lemevit_amd._lib import lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    F32, BF16 = 0, 1
    big = 1 << 20

    def common(kw):
        a = dict(logits=p, dtype=F32, sb=24, sc=12, B=2, K=2, h=3, w=4, H=6, W=8, align=0, labels=p, ldtype=0, ignore=255, alpha=None, gamma=0.0, w_ce=1.0,
                 w_dice=0.0, w_jac=0.0, eps=1e-7, avg=0)
        a.update(kw)
        return [a[k] for k in ("logits", "dtype", "sb", "sc", "B", "K", "h", "w", "H", "W", "align", "labels", "ldtype", "ignore", "alpha", "gamma", "w_ce", "w_dice",
                               "w_jac", "eps", "avg")]

    def fwd(**kw):
        t = dict(ws=p, ws_bytes=big, stats=p, pred=None, conf=None, meter=None)
        t.update({k: kw.pop(k) for k in list(kw) if k in t})
        rc = lib.lmv_dense_up_loss_fwd(*common(kw), t["ws"], t["ws_bytes"], t["stats"], t["pred"], t["conf"], t["meter"], None)
        return rc, lib.lmv_last_error().decode()

    def bwd(**kw):
        t = dict(stats=p, gout=None, dl=p)
        t.update({k: kw.pop(k) for k in list(kw) if k in t})
        rc = lib.lmv_dense_up_loss_bwd(*common(kw), t["stats"], t["gout"], t["dl"], None)
        return rc, lib.lmv_last_error().decode()

    shared = [(dict(logits=None), "null"), (dict(labels=None), "null"), (dict(K=1, sb=12), "outside 2 .. 64"), (dict(K=65, sb=12 * 65), "outside 2 .. 64"),
              (dict(B=0), "bad shape"), (dict(dtype=2), "logits dtype"), (dict(dtype=7), "logits dtype"), (dict(ldtype=2), "label dtype"), (dict(ldtype=-1), "label dtype"),
              (dict(sc=11), "class stride"), (dict(sb=23), "batch stride"), (dict(K=3, sb=35), "batch stride"),
              (dict(w_ce=-1.0), "negative loss weight"), (dict(w_dice=-0.5), "negative loss weight"), (dict(w_jac=-2.0), "negative loss weight"),
              (dict(w_ce=float("nan")), "negative loss weight"), (dict(gamma=-1.0), "gamma"), (dict(eps=0.0), "eps"), (dict(eps=-1e-7), "eps"),
              (dict(avg=3), "avg_mode"), (dict(avg=-1), "avg_mode"),
              (dict(logits=p + 2), "misaligned"), (dict(logits=p + 1, dtype=BF16), "misaligned"), (dict(labels=p + 4), "misaligned"), (dict(alpha=p + 2), "misaligned"),
              # what the upsampling adds
              (dict(h=0), "bad sizes"), (dict(w=0), "bad sizes"), (dict(h=-1), "bad sizes"), (dict(H=2), "bad sizes"), (dict(W=3), "bad sizes"),
              (dict(H=1 << 15, W=1 << 15), "B H W < 2^31"), (dict(B=1, sb=24, H=1 << 16, W=1 << 15), "B H W < 2^31"),
              (dict(align=2), "align_corners"), (dict(align=-1), "align_corners")]
    for call, name, extra in [(fwd, "dense_up_loss_fwd", [(dict(ws=None), "null"), (dict(stats=None), "null"), (dict(ws_bytes=35), "workspace of 35 bytes"),
                                                          (dict(ws_bytes=0), "workspace of 0 bytes"), (dict(ws=p + 2), "misaligned"), (dict(stats=p + 1), "misaligned"),
                                                          (dict(conf=p + 4), "misaligned"), (dict(meter=p + 4), "misaligned"),
                                                          (dict(labels=None, pred=None), "null labels and null pred"),
                                                          (dict(labels=None, pred=p, K=1, sb=12), "outside 2 .. 64"), (dict(labels=None, pred=p, H=2), "bad sizes")]),
                              (bwd, "dense_up_loss_bwd", [(dict(stats=None), "null"), (dict(dl=None), "null"), (dict(stats=p + 2), "misaligned"), (dict(gout=p + 2), "misaligned"),
                                                          (dict(dl=p + 2), "misaligned"), (dict(dl=p + 1, dtype=BF16), "misaligned")])]:
        for kw, msg in shared + extra:
            rc, err = call(**dict(kw))
            assert rc == -1 and msg in err and err.startswith(name + ":"), (name, kw, rc, err)


def test_python_side_refusals_without_gpu():
    """ops.dense_up_* and the surface raise on the Python side for what the ABI would refuse, and never compute on the CPU."""
    from lemevit_amd import ops
    dense = D()
    x, y = torch.randn(2, 3, 4, 5), torch.zeros(2, 8, 10, dtype=torch.int64)
    for call in (lambda: ops.dense_up_loss_fwd(x, y), lambda: ops.dense_up_loss_bwd(x, y, torch.zeros(21)), lambda: dense.DenseLoss(upsample=True)(x, y),
                 lambda: dense.hybrid_loss([x, x], y[:, None], upsample=True, align_corners=True), lambda: dense.DenseCrossEntropy(upsample=True)(x, y),
                 lambda: dense.SegMeter(3, upsample=True).update(x, y), lambda: dense.predict(x, size=(8, 10))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(ValueError):
        ops.dense_up_workspace(0, 2, 16, 16, "cpu")
    with pytest.raises(ValueError):
        ops.dense_up_workspace(1, 65, 16, 16, "cpu")
    with pytest.raises(ValueError, match="B, K, h, w"):
        dense.predict(x[0])
    crit = dense.DenseLoss(upsample=True, align_corners=True)
    assert crit.upsample and crit.align_corners and not dense.DenseLoss().upsample
    m = dense.SegMeter(3, upsample=True)
    assert m.upsample and not m.align_corners and not dense.SegMeter(3).upsample


def test_size_and_layout_refusals():
    """``upsample=True`` with H < h (no downsampling) and channels-last logits are refused by the argument checks, which come before the question of the device."""
    from lemevit_amd import ops
    dense = D()
    x, small = torch.randn(2, 3, 8, 10), torch.zeros(2, 4, 10, dtype=torch.int64)          # H = 4 < h = 8
    for call in (lambda: ops.dense_up_loss_fwd(x, small), lambda: ops.dense_up_loss_bwd(x, small, torch.zeros(21)), lambda: dense.DenseLoss(upsample=True)(x, small),
                 lambda: dense.predict(x, size=(8, 9)),
                 lambda: dense.hybrid_loss([x], small, upsample=True)):
        with pytest.raises(ValueError, match="upsampling only"):
            call()
    y = torch.zeros(2, 16, 20, dtype=torch.int64)
    cl = torch.randn(2, 3, 8, 10).contiguous(memory_format=torch.channels_last)
    for call in (lambda: ops.dense_up_loss_fwd(cl, y), lambda: dense.DenseLoss(upsample=True)(cl, y), lambda: dense.predict(cl, size=(16, 20))):
        with pytest.raises(ValueError, match="channels-last"):
            call()
    with pytest.raises(ValueError, match="size"):
        ops.dense_up_loss_fwd(x, None)
