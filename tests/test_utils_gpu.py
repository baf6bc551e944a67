"""The utility entry points of csrc/misc.hip that only model-level tests reached: the classifier tail's token means and their gradient, the two-segment
DropPath scaling, the batched transpose, the EMA update and the NHWC patch gather / scatter of the 3x3 / stride-2 convolutions -- each against a float64 (or
bit-exact torch) restatement on the rounded operands the kernel reads, under the assert_close rule of test_ops_gpu.py unless a tighter one is stated."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor
from test_ops_gpu import DTYPES, assert_close, dev, ops


def _bits(t):
    """the raw words of a tensor (so that 'bit for bit' also tells -0 from +0 and compares NaN)"""
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


MEAN_SHAPES = [(3, 3136, 16, 64), (2, 49, 16, 320), (5, 7, 3, 8), (2, 9, 16, 512), (300, 8, 16, 64)]      # B, L, M, C


def _mean_inputs(B, L, M, C_, dtype):
    """x and c with a per-channel offset of about 0.5 (means away from zero), rounded to dtype"""
    off = 0.5 + 0.25 * det_tensor((C_,), "tm.off", 7)
    x = (det_tensor((B, L, C_), "tm.x", 7) + off).to(dtype)
    c = (det_tensor((B, M, C_), "tm.c", 7) - off).to(dtype)
    return x, c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_c", [True, False], ids=["xc", "x_only"])
@pytest.mark.parametrize("B,L,M,C_", MEAN_SHAPES)
def test_token_mean2_fwd(dtype, with_c, B, L, M, C_):
    """lmv_token_mean2_fwd and lmv_token_mean2_affine_fwd: mean over the tokens of x (+ the mean over the tokens of c), the affine form with fp32
    xscale / xshift on the x mean.  L and M walk the unroll-by-8 loop with a tail (49, 7, 9, 3) and without (3136, 8, 16); 300 x 64 channels is more than one
    workgroup of (sample, chunk) items."""
    o = ops()
    x, c = _mean_inputs(B, L, M, C_, dtype)
    xs = (1.0 + 0.3 * det_tensor((C_,), "tm.xs", 7)).float(); xb = (0.2 * det_tensor((C_,), "tm.xb", 7)).float()
    mx, mc = x.double().mean(1), (c.double().mean(1) if with_c else 0.0)
    cg = c.to(dev()) if with_c else None
    assert_close(o.token_mean2_fwd(x.to(dev()), cg), mx + mc, dtype, "token_mean2_fwd")
    out = o.token_mean2_affine_fwd(x.to(dev()), cg, xs.to(dev()), xb.to(dev()))
    assert_close(out, xs.double() * mx + xb.double() + mc, dtype, "token_mean2_affine_fwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,M,C_", MEAN_SHAPES + [(B, L, 0, C_) for B, L, _, C_ in MEAN_SHAPES])
def test_token_mean2_bwd(dtype, B, L, M, C_):
    """lmv_token_mean2_bwd: dx[b, l, :] = g[b, :] / L and dc[b, m, :] = g[b, :] / M, every element (the buffers start as NaN).
    The kernel multiplies g by the fp32 reciprocal of the count and rounds the product to the dtype: two fp32 roundings (2^-24 of the value each) and the
    output rounding (none in fp32, half a bf16 ulp = at most 2^-8 of the value in bf16).  That is the bound, elementwise; where the count is a power of two the reciprocal is exact
    and the result must equal g / count rounded once to the dtype, bit for bit.  All tokens of a sample get the same row."""
    from lemevit_amd._lib import check, lib
    o = ops()
    g = det_tensor((B, C_), "tm.g", 7).to(dtype)
    gg = g.to(dev())
    dx = torch.full((B, L, C_), float("nan"), device=dev(), dtype=dtype)
    dc = torch.full((B, M, C_), float("nan"), device=dev(), dtype=dtype) if M else None
    check(lib.lmv_token_mean2_bwd(gg.data_ptr(), dx.data_ptr(), L, None if dc is None else dc.data_ptr(), M, C_, B, o.dtype_code(gg),
                                  torch.cuda.current_stream().cuda_stream), "lmv_token_mean2_bwd")
    rel = 2.0 ** -23 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    for what, got, n in (("dx", dx, L), ("dc", dc, M)):
        if got is None:
            continue
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), f"token_mean2_bwd {what}: unwritten or non-finite element"
        assert torch.equal(_bits(got), _bits(got[:, :1].expand_as(got))), f"token_mean2_bwd {what}: the tokens of a sample differ"
        ref = g.double() / n
        err = (got[:, 0].double() - ref).abs()
        assert bool((err <= rel * ref.abs()).all()), f"token_mean2_bwd {what}: worst error {float((err / ref.abs().clamp_min(1e-300)).max()):.3e} of the value, bound {rel:.3e}"
        if n & (n - 1) == 0:
            assert torch.equal(_bits(got[:, 0]), _bits(ref.to(dtype))), f"token_mean2_bwd {what}: g / {n} must be exact up to the output rounding"
    # the wrapper allocates the same shapes and returns no second gradient without a second segment
    wx, wc = o.token_mean2_bwd(gg, L, M)
    assert torch.equal(_bits(wx), _bits(dx)) and ((wc is None and M == 0) or torch.equal(_bits(wc), _bits(dc)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_scale_multi(dtype):
    """lmv_row_scale_multi with two segments of different row counts and rows_per_sample (one launch), and the wrapper's other routes: a None scale passes its
    tensor through, three scaled tensors or two of different C go tensor by tensor.  Every result equals row_scale of that tensor bit for bit and the float64
    product within the assert_close budget."""
    o = ops()
    B = 4
    x = det_tensor((B, 196, 96), "rs.x", 7).to(dtype); c = det_tensor((B, 16, 96), "rs.c", 7).to(dtype); e = det_tensor((B, 5, 96), "rs.e", 7).to(dtype)
    n = det_tensor((B, 16, 64), "rs.n", 7).to(dtype)
    sc = {k: (0.25 + det_tensor((B,), "rs.s" + k, 7).abs() * 1.5).float() for k in "xcen"}
    src = {"x": x, "c": c, "e": e, "n": n}
    gpu = {k: v.to(dev()) for k, v in src.items()}; sg = {k: v.to(dev()) for k, v in sc.items()}

    def verify(keys, scaled, outs):
        assert len(outs) == len(keys)
        for k, on, y in zip(keys, scaled, outs):
            if not on:
                assert y is gpu[k], f"row_scale_multi: the unscaled tensor {k} must pass through"
                continue
            assert y.data_ptr() != gpu[k].data_ptr()
            assert torch.equal(_bits(y), _bits(o.row_scale(gpu[k], sg[k], src[k].shape[1]))), f"row_scale_multi: {k} differs from row_scale"
            assert_close(y, src[k].double() * sc[k].double()[:, None, None], dtype, f"row_scale_multi {keys} {k}")

    for keys, scaled in ((("x", "c"), (True, True)), (("c", "x"), (True, True)), (("x", "c"), (True, False)), (("x", "c"), (False, True)),
                         (("x", "c", "e"), (True, True, True)), (("x", "c", "e"), (True, False, True)), (("x", "n"), (True, True))):
        outs = o.row_scale_multi([gpu[k] for k in keys], [sg[k] if on else None for k, on in zip(keys, scaled)])
        verify(keys, scaled, outs)
    outs = o.row_scale_multi([gpu["x"], gpu["c"]], [None, None])
    assert outs[0] is gpu["x"] and outs[1] is gpu["c"]


TR_SHAPES = [(64, 64), (1, 8), (65, 63), (384, 1536), (100, 7), (1, 1)]


def _transpose_and_check(o, shapes, tag):
    srcs = [det_tensor(s, f"tr.{tag}{i}", 7).to(torch.bfloat16).to(dev()) for i, s in enumerate(shapes)]
    # every destination is the head of a NaN-filled buffer with one more row: unwritten elements and writes behind the matrix both show
    bufs = [torch.full((c + 1, r), float("nan"), device=dev(), dtype=torch.bfloat16) for r, c in shapes]
    o.transpose_batch([(s, b[:-1]) for s, b in zip(srcs, bufs)])
    for (r, c), s, b in zip(shapes, srcs, bufs):
        assert torch.equal(_bits(b[:-1]), _bits(s.t().contiguous())), f"transpose_batch {tag}: {r} x {c} differs from .t().contiguous()"
        assert bool(torch.isnan(b[-1]).all()), f"transpose_batch {tag}: {r} x {c} wrote behind its destination"


def test_transpose_batch():
    """lmv_transpose_batch (bf16) bit-exact against .t().contiguous(): whole 64 x 64 tiles, ragged tiles in both directions, single rows and columns, one
    element; each shape alone, all in one call, and 50 segments of mixed shapes, which is more than LMV_TRANSPOSE_MAX_SEGS = 48 and takes two launches."""
    o = ops()
    for i, s in enumerate(TR_SHAPES):
        _transpose_and_check(o, [s], f"one{i}.")
    _transpose_and_check(o, TR_SHAPES, "all.")
    many = [((3 + 7 * i) % 130 + 1, (5 + 11 * i) % 90 + 1) for i in range(50)]
    assert len(many) > 48
    _transpose_and_check(o, many, "many.")


@pytest.mark.parametrize("n", [4, 4096 * 3, 1000004, 4 * (2048 * 256 + 5)])
def test_ema_flat(n):
    """lmv_ema_flat: ema <- decay * ema + (1 - decay) * param on flat fp32 buffers (the last n is past 2048 workgroups x 256 threads x 4 elements: the
    grid-stride loop takes a second turn)."""
    o = ops()
    ema0 = det_tensor((n,), "ema.e", 7); p = det_tensor((n,), "ema.p", 7, 2.0)
    pg = p.to(dev())
    d = float(torch.tensor(0.9998, dtype=torch.float32))          # the decay the library receives (a C float)
    e = ema0.to(dev()); ref = ema0.double()
    for step in range(3):
        o.ema_flat(e, pg, 0.9998)
        ref = d * ref + (1.0 - d) * p.double()
        assert_close(e, ref, torch.float32, f"ema_flat step {step + 1}", 1e-5)
    e = ema0.to(dev()); o.ema_flat(e, pg, 1.0)
    assert torch.equal(_bits(e), _bits(ema0)), "ema_flat: decay 1 must leave ema as it is"
    e = ema0.to(dev()); o.ema_flat(e, pg, 0.0)
    assert torch.equal(_bits(e), _bits(p)), "ema_flat: decay 0 must copy param"


def test_ema_flat_refusals():
    o = ops()
    e = torch.zeros(8, device=dev()); p = torch.ones(8, device=dev())
    with pytest.raises(RuntimeError, match="ema_flat"):
        o.ema_flat(e[:6], p[:6], 0.5)                               # n % 4 != 0
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="ema_flat"):
            o.ema_flat(e, p, bad)
    with pytest.raises(TypeError):
        o.ema_flat(e, p[:4], 0.5)
    assert torch.equal(e.cpu(), torch.zeros(8)), "a refused call must not touch ema"


def _taps(Ho, Wo):
    """(tap, row slice, column slice) into the map padded by one pixel on every side: tap (ky, kx) of output pixel (ho, wo) is padded pixel (2 ho + ky, 2 wo + kx)"""
    return [(ky * 3 + kx, slice(ky, ky + 2 * Ho - 1, 2), slice(kx, kx + 2 * Wo - 1, 2)) for ky in range(3) for kx in range(3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad64", [False, True], ids=["KP9C", "KP64"])
@pytest.mark.parametrize("B,H,W,C_", [(2, 5, 6, 8), (1, 9, 7, 64), (3, 14, 14, 16)])
def test_im2col_col2im_nhwc(dtype, pad64, B, H, W, C_):
    """lmv_im2col3x3s2_nhwc / lmv_col2im3x3s2_nhwc called directly, odd H and W included.  patches[(b, ho, wo)][(ky * 3 + kx) * C + ci] =
    x[b, 2 ho - 1 + ky, 2 wo - 1 + kx, ci]: bit-equal to a torch gather from the zero-padded map, the taps outside the map and the columns 9 C .. KP - 1 zero.
    col2im sums the 1, 2 or 4 patch entries that read a pixel (the padding columns, filled with data here, take no part): against the float64 sum rounded
    once to the dtype -- bit-equal in fp32 where there are at most 2 terms (one correctly rounded addition), within assert_close everywhere."""
    o = ops()
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    KP = (9 * C_ + 63) // 64 * 64 if pad64 else 9 * C_
    x = det_tensor((B, H, W, C_), "i2c.x", 7).to(dtype)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    ref = torch.zeros((B, Ho, Wo, KP), dtype=dtype)
    for tap, rs, cs in _taps(Ho, Wo):
        ref[..., tap * C_:(tap + 1) * C_] = xp[:, rs, cs]
    got = o.im2col3x3s2_nhwc(x.to(dev()), KP)
    assert got.shape == (B * Ho * Wo, KP)
    assert torch.equal(_bits(got), _bits(ref.reshape(B * Ho * Wo, KP))), "im2col3x3s2_nhwc differs from the gather"

    dp = det_tensor((B * Ho * Wo, KP), "i2c.dp", 7).to(dtype)
    dp64 = dp.double().reshape(B, Ho, Wo, KP)
    acc = torch.zeros((B, H + 2, W + 2, C_), dtype=torch.float64); cnt = torch.zeros((H + 2, W + 2), dtype=torch.int64)
    for tap, rs, cs in _taps(Ho, Wo):
        acc[:, rs, cs] += dp64[..., tap * C_:(tap + 1) * C_]
        cnt[rs, cs] += 1
    acc, cnt = acc[:, 1:H + 1, 1:W + 1], cnt[1:H + 1, 1:W + 1]
    assert set(cnt.unique().tolist()) == {1, 2, 4}
    dx = o.col2im3x3s2_nhwc(dp.to(dev()), B, H, W, C_)
    assert dx.shape == (B, H, W, C_)
    assert_close(dx, acc, dtype, "col2im3x3s2_nhwc")
    if dtype == torch.float32:
        few = cnt <= 2
        assert torch.equal(_bits(dx.cpu()[:, few]), _bits(acc.float()[:, few])), "col2im3x3s2_nhwc: sums of 1 or 2 terms must be exact up to one rounding"
