"""Sliding-window dense inference, without a GPU: ``slide_grid`` against mmseg's window rule, ``reference_slide`` (the numpy float64 oracle of
tests/test_dense_slide_gpu.py) against mmseg's ``slide_inference`` loop written out with PyTorch's own float64 ``F.interpolate`` / ``F.pad``, the ABI additions, and
the argument refusals of lmv_dense_slide_fwd (before any launch, on host buffers that are never touched)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# (H, W), crop, stride -> ys, xs, window
GRIDS = [((40, 52), 24, 16, (0, 16), (0, 16, 28), (24, 24)),
         ((37, 45), (16, 20), 8, (0, 8, 16, 21), (0, 8, 16, 24, 25), (16, 20)),
         ((20, 70), 32, 24, (0,), (0, 24, 38), (20, 32)),
         ((32, 48), (32, 48), (16, 16), (0,), (0,), (32, 48))]


def D():
    from lemevit_amd import dense
    return dense


def mmseg_loop(x, size, crop, stride, align):
    """``EncoderDecoder.slide_inference`` restated: x [G, B, K, h, w] are the ``crop_seg_logit``s in front of the resize, in the loop's own order"""
    (h_img, w_img), (h_crop, w_crop), (h_stride, w_stride) = size, crop, stride
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    G, B, K = x.shape[:3]
    preds = x.new_zeros((B, K, h_img, w_img))
    count_mat = x.new_zeros((B, 1, h_img, w_img))
    g = 0
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1, x1 = h_idx * h_stride, w_idx * w_stride
            y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
            y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
            crop_seg_logit = F.interpolate(x[g], size=(y2 - y1, x2 - x1), mode="bilinear", align_corners=align)
            preds += F.pad(crop_seg_logit, (int(x1), int(preds.shape[3] - x2), int(y1), int(preds.shape[2] - y2)))
            count_mat[:, :, y1:y2, x1:x2] += 1
            g += 1
    assert g == G and (count_mat == 0).sum() == 0
    return preds / count_mat, count_mat


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


@pytest.mark.parametrize("size,crop,stride,ys,xs,window", GRIDS, ids=["shifted-last", "dense-overlap", "below-the-crop", "one-window"])
def test_slide_grid_is_mmsegs_rule(size, crop, stride, ys, xs, window):
    g = D().slide_grid(size, crop, stride)
    assert (g.H, g.W) == size and g.ys == ys and g.xs == xs and g.window == window and len(g) == len(ys) * len(xs)
    assert g.boxes() == [(y, y + window[0], x, x + window[1]) for y in ys for x in xs]
    assert list(g.c_ys) == list(ys) and list(g.c_xs) == list(xs)
    for bad in (lambda: D().slide_grid(size, crop, 0), lambda: D().slide_grid(size, 8, 9), lambda: D().slide_grid((0, 4), crop, stride)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("align", [False, True], ids=["half-pixel", "align-corners"])
@pytest.mark.parametrize("size,crop,stride,lo", [(GRIDS[0][0], 24, 16, (6, 6)), (GRIDS[1][0], (16, 20), 8, (4, 5)), (GRIDS[2][0], 32, 24, (7, 9)),
                                                 (GRIDS[3][0], (32, 48), 16, (8, 12)), (GRIDS[0][0], 24, 16, (24, 24))],
                         ids=["shifted-last", "dense-overlap", "below-the-crop", "one-window", "full-resolution"])
def test_oracle_is_the_literal_loop(size, crop, stride, lo, align):
    dense, B, K = D(), 2, 4
    grid = dense.slide_grid(size, crop, stride)
    gen = torch.Generator().manual_seed(size[0] * 131 + lo[1])
    x = torch.randn((len(grid), B, K) + lo, generator=gen, dtype=torch.float64) * 3
    y = torch.randint(0, K, (B,) + size, generator=gen)
    y[torch.rand((B,) + size, generator=gen) < 0.1] = 255
    want, count = mmseg_loop(x, size, pair(crop), pair(stride), align)
    ref = dense.reference_slide(x, grid, align_corners=align, labels=y, ignore_index=255)
    assert ref["z"].shape == (B, K) + size and float(np.abs(ref["z"] - want.numpy()).max()) <= 1e-12
    assert np.array_equal(ref["count"], count[0, 0].numpy().astype(np.int64)) and ref["count"].max() >= (2 if len(grid) > 1 else 1)
    assert np.array_equal(ref["pred"], want.argmax(1).numpy().astype(np.uint8))
    srt = np.sort(ref["z"], axis=1)
    assert np.array_equal(ref["margin"], srt[:, -1] - srt[:, -2])
    valid = y != 255
    assert ref["n_valid"] == int(valid.sum())
    nll = F.cross_entropy(want, y, ignore_index=255, reduction="sum")
    assert abs(ref["nll_sum"] - float(nll)) <= 1e-9 * float(nll)
    conf = np.bincount((y[valid] * K + want.argmax(1)[valid]).numpy(), minlength=K * K).reshape(K, K)
    assert np.array_equal(ref["conf"], conf)
    assert sorted(dense.reference_slide(x, grid, align_corners=align)) == ["count", "margin", "pred", "z"]
    with pytest.raises(ValueError):
        dense.reference_slide(x[1:], grid)


def test_abi_additions():
    import lemevit_amd
    from lemevit_amd import _lib
    assert [len(_lib.SIGNATURES[n][1]) for n in ("lmv_dense_slide_workspace_bytes", "lmv_dense_slide_fwd")] == [4, 29]
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14          # a pure addition: detected by symbol
    assert _lib.DENSE_SLIDE_MAX_GRID == 64
    ws, up = _lib.lib.lmv_dense_slide_workspace_bytes, _lib.lib.lmv_dense_up_loss_workspace_bytes
    for args in ((1, 2, 1, 1), (2, 5, 30, 37), (1, 6, 1536, 1536), (1, 64, 24, 24), (0, 2, 4, 4), (1, 65, 4, 4), (2, 2, 1 << 15, 1 << 15)):
        assert ws(*args) == up(*args)          # the chunks and the rows of the upsampling forward
    assert ws(1, 6, 1536, 1536) == 1024 * 21 * 4
    header = open(__import__("os").path.join(__import__("os").path.dirname(lemevit_amd.__file__), "..", "include", "lemevit_hip.h")).read()
    assert "lmv_dense_slide_fwd(" in header and "lmv_dense_slide_workspace_bytes(" in header and "#define LMV_DENSE_SLIDE_MAX_GRID 64" in header
    assert "#define LMV_ABI_VERSION 14" in header
    for n in ("SlideGrid", "slide_grid", "slide_predict", "slide_inference", "reference_slide"):
        assert n in lemevit_amd.dense.__all__ and n in lemevit_amd.__all__ and getattr(lemevit_amd, n) is getattr(lemevit_amd.dense, n)
    assert all(hasattr(lemevit_amd.ops, n) for n in ("dense_slide_fwd", "dense_slide_workspace")) and hasattr(lemevit_amd.SegMeter, "update_slide")


def test_argument_validation_without_gpu():
    """Each refusal the header lists returns LMV_ERR_SHAPE (-1) with a message that starts ``dense_slide`` before any launch; the buffers are host memory that is
    never touched."""
    from lemevit_amd._lib import lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    F32, BF16 = 0, 1

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def call(**kw):
        # 2 x 3 windows of 6 x 8 pixels over a 10 x 20 image, logits 3 x 4, B = 2, K = 2
        a = dict(logits=p, dtype=F32, sg=48, sb=24, sc=12, B=2, K=2, h=3, w=4, ys=ints(0, 4), gy=2, xs=ints(0, 6, 12), gx=3, wh=6, ww=8, H=10, W=20, align=0,
                 labels=p, ldtype=0, ignore=255, ws=p, ws_bytes=1 << 20, stats=p, pred=None, mean=None, conf=None, meter=None)
        a.update(kw)
        keep = [a["ys"], a["xs"]]
        ys, xs = (None if o is None else ctypes.addressof(o) for o in keep)
        rc = lib.lmv_dense_slide_fwd(a["logits"], a["dtype"], a["sg"], a["sb"], a["sc"], a["B"], a["K"], a["h"], a["w"], ys, a["gy"], xs, a["gx"], a["wh"], a["ww"],
                                     a["H"], a["W"], a["align"], a["labels"], a["ldtype"], a["ignore"], a["ws"], a["ws_bytes"], a["stats"], a["pred"], a["mean"],
                                     a["conf"], a["meter"], None)
        return rc, lib.lmv_last_error().decode()

    many = ints(*range(65))
    cases = [  # everything lmv_dense_up_loss_fwd refuses
        (dict(logits=None), "null"), (dict(labels=None), "null labels, null pred and null mean_logits"), (dict(K=1, sb=12), "outside 2 .. 64"),
        (dict(K=65, sb=12 * 65, sg=24 * 65), "outside 2 .. 64"), (dict(B=0), "bad shape"), (dict(dtype=2), "logits dtype"), (dict(ldtype=2), "label dtype"),
        (dict(ldtype=-1), "label dtype"), (dict(sc=11), "class stride"), (dict(sb=23), "batch stride"), (dict(K=3, sb=35), "batch stride"),
        (dict(logits=p + 2), "misaligned"), (dict(logits=p + 1, dtype=BF16), "misaligned"), (dict(labels=p + 4), "misaligned"),
        (dict(h=0), "bad sizes"), (dict(w=0), "bad sizes"), (dict(h=-1), "bad sizes"), (dict(align=2), "align_corners"), (dict(align=-1), "align_corners"),
        (dict(ws=None), "null"), (dict(stats=None), "null"), (dict(ws_bytes=35), "workspace of 35 bytes"), (dict(ws_bytes=0), "workspace of 0 bytes"),
        (dict(ws=p + 2), "misaligned"), (dict(stats=p + 1), "misaligned"), (dict(conf=p + 4), "misaligned"), (dict(meter=p + 4), "misaligned"),
        (dict(labels=None, pred=p, K=1, sb=12), "outside 2 .. 64"), (dict(labels=None, mean=p, h=0), "bad sizes"),
        # downsampling: h > wh, w > ww
        (dict(h=7, sc=28, sb=56, sg=112), "upsampling only"), (dict(w=9, sc=27, sb=54, sg=108), "upsampling only"),
        # the grid
        (dict(gy=0), "outside 1 .. 64"), (dict(gx=0), "outside 1 .. 64"), (dict(gy=65, ys=many), "outside 1 .. 64"), (dict(gx=65, xs=many), "outside 1 .. 64"),
        (dict(gy=-1), "outside 1 .. 64"), (dict(ys=None), "null window origins"), (dict(xs=None), "null window origins"),
        (dict(ys=ints(0, 0)), "not strictly increasing"), (dict(xs=ints(0, 12, 6)), "not strictly increasing"), (dict(xs=ints(0, 6, 6)), "not strictly increasing"),
        (dict(ys=ints(1, 4)), "not at 0"), (dict(xs=ints(2, 6, 12)), "not at 0"), (dict(ys=ints(-4, 4)), "not at 0"),
        (dict(ys=ints(0, 3)), "the image at 10"), (dict(ys=ints(0, 5)), "the image at 10"), (dict(xs=ints(0, 6, 11)), "the image at 20"), (dict(H=11), "the image at 11"),
        (dict(W=19), "the image at 19"), (dict(gy=1, ys=ints(0)), "the image at 10"),
        (dict(xs=ints(0, 3, 12)), "leave pixels uncovered"), (dict(ys=ints(0, 7), H=13), "leave pixels uncovered"),
        # the image and the rest
        (dict(H=0, gy=1, ys=ints(0), wh=0), "bad sizes"), (dict(B=1 << 10, H=1 << 11, W=1 << 10), "B H W < 2^31"),
        (dict(sg=47), "window stride"), (dict(B=1, sg=23), "window stride"), (dict(mean=p + 2), "misaligned")]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == -1 and msg in err and err.startswith("dense_slide_fwd:"), (kw, rc, err)


def test_python_side_refusals_without_gpu():
    """ops.dense_slide_fwd and the surface raise on the Python side for what the ABI would refuse, and never compute on the CPU."""
    from lemevit_amd import ops
    dense = D()
    grid = dense.slide_grid((40, 52), 24, 16)
    x, y = torch.randn(6, 2, 3, 6, 6), torch.zeros(2, 40, 52, dtype=torch.int64)
    fn = torch.nn.AvgPool2d(4)
    for call in (lambda: dense.slide_predict(x, grid), lambda: dense.SegMeter(3).update_slide(x, grid, y), lambda: dense.slide_inference(fn, torch.randn(2, 3, 40, 52), 24, 16),
                 lambda: ops.dense_slide_fwd(x, grid.ys, grid.xs, grid.window, (40, 52), y)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    for call, msg in ((lambda: dense.slide_predict(x[:5], grid), "windows"), (lambda: dense.slide_predict(x[0], grid), "windows"),
                      (lambda: dense.slide_predict(torch.randn(6, 2, 3, 25, 6), grid), "upsampling only"),
                      (lambda: dense.slide_predict(x.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3), grid), "channels-last"),
                      (lambda: dense.slide_predict(torch.randn(6, 2, 65, 6, 6), grid), "outside 2 .. 64"),
                      (lambda: ops.dense_slide_fwd(x, grid.ys, grid.xs, grid.window, (40, 52), y[:, :39].contiguous()), "labels must be"),
                      (lambda: dense.SegMeter(4).update_slide(x, grid, y), "classes"),
                      (lambda: ops.dense_slide_fwd(x, grid.ys, grid.xs, grid.window, (40, 52)), "nothing to compute"),
                      (lambda: dense.slide_inference(fn, torch.randn(2, 3, 40, 52), 24, 16, meter=dense.SegMeter(3)), "come together"),
                      (lambda: dense.slide_inference(fn, torch.randn(2, 3, 40, 52), 24, 16, windows_per_call=0), "windows_per_call"),
                      (lambda: dense.SlideGrid(8, 8 * 65, (0,), tuple(range(0, 8 * 65, 8)), (8, 8)), "per axis")):
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(ValueError):
        ops.dense_slide_workspace(0, 2, 16, 16, "cpu")


def test_gpu_cases_leave_out_few_pixels():
    """With the oracle alone: in every case of tests/test_dense_slide_gpu.py the pixels whose margin is below 1e-4 max(1, |top|) -- where ``pred`` is not compared --
    stay under the 0.5 % cap."""
    from test_dense_slide_gpu import CASES, IGNORE, case_id, grid_of, inputs
    for case in CASES:
        for ldtype in (torch.int64, torch.uint8):
            x, y = inputs(case, ldtype)
            ref = D().reference_slide(x, grid_of(case), align_corners=case[6], labels=y, ignore_index=IGNORE)
            decisive = ref["margin"] >= 1e-4 * np.maximum(1.0, np.abs(ref["z"].max(1)))
            assert 1.0 - float(decisive.mean()) <= 0.005, (case_id(case), 1.0 - float(decisive.mean()))
            assert 0 < ref["n_valid"] < y.numel()
