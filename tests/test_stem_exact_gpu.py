"""csrc/stem.hip (lmv_stem_fwd, lmv_stem_pack) at the kernel level, on raw operands: w1m [Cm, 32] and w2m [Co, ld2] bf16, b1 / b2 fp32, no BatchNorm folding.

1. An EXACT-INTEGER regime in which nothing rounds anywhere, so the whole output is compared bit for bit with a float64 reference: images in {0 .. 3}, weights in
   {-1, 0, +1}, b1 in [85, 170] (every pre-activation h + b1 lies in [4, 251]: the GELU polynomial is on its identity side, where it returns h (1 - 2^-23) -- see
   tests/test_stem_cpu.py -- and the bf16 store of the tile between the convolutions gives the integer h back), conv2 sums below 2^24.  One wrong tap, weight-fragment
   lane, bias lane, tile-to-image map, stale patch / T1 / prefetch mask, or a computed value where conv2 pads (>= 4 instead of 0) changes an integer.  One case gives
   every workgroup of the persistent grid at least two tiles.
2. Every stride pattern of the images, bit-identical to the contiguous copy.
3. The packer with poison in every column it must not read.
4. A probe that makes the tile between the convolutions (conv1 + bias + GELU) observable element by element, against the erf GELU in float64.
5. The guards of ops.stem_fwd.
The output buffer is pre-filled with NaN everywhere and no NaN may remain."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from detfill import det_tensor

DEV = "cuda:0"
NAN = float("nan")
VARIANTS = [(48, 96), (32, 64)]


# ------------------------------------------------------------------------------------------------
# operands of the exact regime
def _mix(t):
    """int64 tensor -> well-mixed 32-bit values (a multiplicative hash: deterministic, no generator state)."""
    t = (t * 2654435761) & 0xFFFFFFFF
    t = t ^ (t >> 15)
    t = (t * 2246822519) & 0xFFFFFFFF
    return t ^ (t >> 13)


def _exact_images(B, H, W, salt=0):
    """[B, 3, H, W] fp32, integers in {0, 1, 2, 3}: a function of the flat index, so different per image, channel and pixel."""
    n = B * 3 * H * W
    return ((_mix(torch.arange(n, dtype=torch.int64) + 12345 + 1000003 * salt) >> 7) & 3).to(torch.float32).reshape(B, 3, H, W)


@functools.lru_cache(maxsize=None)
def _exact_weights(Cm, Co):
    """(w1m [Cm, 32], w2m [Co, 9 Cm]) bf16 with dense {-1, 0, +1} in the columns the kernel reads (zeros behind column 27 of w1m), b1 in [85, 170], b2 in [-8, 8]."""
    w1m = torch.zeros(Cm, 32)
    w1m[:, :27] = ((_mix(torch.arange(Cm * 27, dtype=torch.int64) + 777) >> 5) % 3 - 1).to(torch.float32).reshape(Cm, 27)
    w2m = ((_mix(torch.arange(Co * 9 * Cm, dtype=torch.int64) + 4242) >> 5) % 3 - 1).to(torch.float32).reshape(Co, 9 * Cm)
    b1 = (85 + (_mix(torch.arange(Cm, dtype=torch.int64) + 99) >> 4) % 86).to(torch.float32)
    b2 = ((_mix(torch.arange(Co, dtype=torch.int64) + 31) >> 3) % 17 - 8).to(torch.float32)
    for w in (w1m[:, :27], w2m):
        assert all(int((w == v).sum()) > w.numel() // 4 for v in (-1.0, 0.0, 1.0)), "the weights must be dense in all three values"
    assert 85 <= float(b1.min()) and float(b1.max()) <= 170 and len(set(b1.tolist())) > Cm // 2
    return w1m.to(torch.bfloat16), w2m.to(torch.bfloat16), b1, b2


def _conv_weights(w1m, w2m, Cm, Co):
    """The matrices as Conv2d weights in float64: w1m columns are (ci, ky, kx), w2m columns are (ky, kx, ci)."""
    W1 = w1m[:, :27].double().reshape(Cm, 3, 3, 3)
    W2 = w2m[:, :9 * Cm].double().reshape(Co, 3, 3, Cm).permute(0, 3, 1, 2).contiguous()
    return W1, W2


def _ref_exact(x, Cm, Co):
    """x [B, 3, H, W] on the CPU -> the reference [B, H/4, W/4, Co] bf16, after asserting the ranges the exactness argument rests on."""
    w1m, w2m, b1, b2 = _exact_weights(Cm, Co)
    W1, W2 = _conv_weights(w1m, w2m, Cm, Co)
    with torch.no_grad():
        h = F.conv2d(x.double(), W1, b1.double(), 2, 1)
        lo, hi = float(h.min()), float(h.max())
        assert lo >= 4.0 and hi <= 256.0, (lo, hi)          # the GELU's identity side, and integers a bf16 holds
        y = F.conv2d(h, W2, b2.double(), 2, 1)
        assert float(y.abs().max()) < 2.0 ** 24 and bool((y == y.round()).all())          # exact in fp32 in any order of accumulation
    return y.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _exact_case(B, H, W, Cm, Co):
    x = _exact_images(B, H, W)
    return x, _ref_exact(x, Cm, Co)


@functools.lru_cache(maxsize=None)
def _exact_dev(Cm, Co):
    """(wpk, b1, b2) of the exact regime on the GPU, packed once."""
    from lemevit_amd import ops
    w1m, w2m, b1, b2 = _exact_weights(Cm, Co)
    wpk = ops.stem_pack(w1m.to(DEV), w2m.to(DEV))
    torch.cuda.synchronize()
    return wpk, b1.to(DEV), b2.to(DEV)


# ------------------------------------------------------------------------------------------------
def _launch(x, wpk, b1, b2, Cm, Co):
    """lmv_stem_fwd itself, on x's own strides, into a NaN-filled buffer."""
    from lemevit_amd._lib import LMV_BF16, LMV_F32, check, lib
    B, C3, H, W = x.shape
    assert C3 == 3 and x.is_cuda and wpk.dtype == torch.uint8 and wpk.numel() == lib.lmv_stem_wpk_bytes(Cm, Co)
    assert b1.dtype == torch.float32 and b2.dtype == torch.float32 and b1.is_contiguous() and b2.is_contiguous() and b1.numel() == Cm and b2.numel() == Co
    y = torch.full((B, H // 4, W // 4, Co), NAN, device=DEV, dtype=torch.bfloat16)
    code = {torch.float32: LMV_F32, torch.bfloat16: LMV_BF16}[x.dtype]
    sb, sc, sh, sw = x.stride()
    check(lib.lmv_stem_fwd(x.data_ptr(), code, sb, sc, sh, sw, B, H, W, Cm, Co, wpk.data_ptr(), b1.data_ptr(), b2.data_ptr(), y.data_ptr(),
                           torch.cuda.current_stream().cuda_stream), "lmv_stem_fwd")
    torch.cuda.synchronize()
    n = int(torch.isnan(y).sum())
    assert n == 0, f"{n} of {y.numel()} output elements were not written (or are NaN)"
    return y


def _assert_same(y, ref, what):
    """torch.equal, with a description of where the mismatches are (tiles, rows / columns inside the 8 x 8 tile, channels mod 16) when it fails."""
    y, ref = y.cpu(), ref.cpu()
    assert y.shape == ref.shape and y.dtype == ref.dtype, (what, y.shape, ref.shape)
    if torch.equal(y, ref):
        return
    bad = (y.float() != ref.float()).nonzero()
    b, oy, ox, c = bad.unbind(1)
    tiles = sorted(set(zip(b.tolist(), (oy // 8).tolist(), (ox // 8).tolist())))
    d = (y.float() - ref.float())[y.float() != ref.float()]
    raise AssertionError(f"{what}: {bad.shape[0]} of {y.numel()} elements differ (max |difference| {float(d.abs().max()):g}); {len(tiles)} tiles (image, ty, tx), first {tiles[:8]}; "
                         f"rows in tile {sorted(set((oy % 8).tolist()))}, columns in tile {sorted(set((ox % 8).tolist()))}, "
                         f"channels mod 16 {sorted(set((c % 16).tolist()))}, channel tiles {sorted(set((c // 16).tolist()))}")


def _twice(x, Cm, Co, ref, what, ops3=None):
    wpk, b1, b2 = ops3 if ops3 is not None else _exact_dev(Cm, Co)
    y = _launch(x, wpk, b1, b2, Cm, Co)
    _assert_same(y, ref, what)
    y2 = _launch(x, wpk, b1, b2, Cm, Co)
    assert torch.equal(y, y2), what + ": two runs differ"
    return y


# ------------------------------------------------------------------------------------------------
# 1. exact integers, bit for bit
@pytest.mark.parametrize("Cm,Co", VARIANTS)
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 32, 64), (2, 64, 32), (3, 96, 96), (1, 32, 160)])
def test_stem_exact_integers(B, H, W, Cm, Co):
    """One tile with all four borders; a seam on either axis; an interior tile with every edge kind and a tile index that crosses images; a row of five tiles."""
    x, ref = _exact_case(B, H, W, Cm, Co)
    _twice(x.to(DEV), Cm, Co, ref, f"stem {Cm}->{Co} exact {B}x{H}x{W}")


@pytest.mark.parametrize("Cm,Co", VARIANTS)
def test_stem_exact_persistent_tiles(Cm, Co):
    """More than 4 tiles per compute unit: the launcher starts at most 2 workgroups per compute unit, so EVERY workgroup runs the tile loop at least twice (rewriting
    the patch and T1 over the previous tile's, with the prefetch and its mask of the tile after), some run it once more, and the last generation is ragged.  The grid
    is no multiple of the tiles per image, so the consecutive tiles of a workgroup sit at different positions of their images and have different border masks."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, W = (96, 96) if cus % 9 else (96, 160)
    per = (H // 32) * (W // 32)
    assert cus % per and (2 * cus) % per, (cus, per)
    B = (4 * cus + 7 + per - 1) // per
    ntiles = B * per
    assert ntiles > 4 * cus and ntiles % cus and ntiles % (2 * cus)
    x, ref = _exact_case(B, H, W, Cm, Co)
    _twice(x.to(DEV), Cm, Co, ref, f"stem {Cm}->{Co} exact, {ntiles} tiles on {cus} compute units")


# ------------------------------------------------------------------------------------------------
# 2. layouts
LAYOUTS = ["f32 nchw", "f32 nhwc", "bf16 nchw", "bf16 nhwc", "f32 crop", "bf16 crop", "bf16 crop odd", "batch expand", "bf16 batch expand", "channel expand", "sw = 2", "bf16 sw = 2",
           "sb > 2^31"]


def _layout(name, img):
    """img [B, 3, H, W] fp32 on the GPU -> (x in the layout `name`, the images it must hold, whatever must stay alive)."""
    B, _, H, W = img.shape
    dt = torch.bfloat16 if name.startswith("bf16") else torch.float32
    kind = name[5:] if name.startswith("bf16 ") else name[4:] if name.startswith("f32 ") else name
    src = img.to(dt)
    if kind == "nchw":
        x = src.contiguous()
        assert x.stride() == (3 * H * W, H * W, W, 1)
    elif kind == "nhwc":
        x = src.contiguous(memory_format=torch.channels_last)
        assert x.stride() == (3 * H * W, 1, 3 * W, 3)
    elif kind in ("crop", "crop odd"):
        x0 = 8 if kind == "crop odd" else 7
        big = torch.full((B, 3, H + 11, W + 13), NAN, device=DEV, dtype=dt)
        x = big[:, :, 5:5 + H, x0:x0 + W]
        x.copy_(src)
        assert x.storage_offset() == 5 * (W + 13) + x0 and x.stride(2) == W + 13 and (kind != "crop odd" or x.storage_offset() % 2 == 1)
        assert int(torch.isnan(big).sum()) == big.numel() - x.numel()          # the surroundings stay poisoned
    elif kind == "batch expand":
        src = src[:1].expand(B, 3, H, W)
        x = src[:1].contiguous().expand(B, 3, H, W)
        assert x.stride(0) == 0
    elif kind == "channel expand":
        src = src[:, 1:2].expand(B, 3, H, W)
        x = src[:, :1].contiguous().expand(B, 3, H, W)
        assert x.stride(1) == 0
    elif kind == "sw = 2":
        big = torch.full((B, 3, 2 * H, 2 * W), NAN, device=DEV, dtype=dt)
        x = big[..., ::2, ::2]
        x.copy_(src)
        assert x.stride() == (12 * H * W, 4 * H * W, 4 * W, 2)
    else:
        raise KeyError(name)
    return x, src


@pytest.mark.parametrize("Cm,Co", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stem_exact_layouts(layout, Cm, Co):
    """fp32 / bf16 x NCHW / channels-last; crops of a NaN-filled buffer (a storage offset, a row pitch, for bf16 an odd element offset: the masked loads outside the image
    must not leak a NaN); stride 0 over the batch or the channels; a column stride of 2; a batch stride beyond 2^31 elements.  Each bit-identical to the float64
    reference and to the run on x.contiguous()."""
    B, H, W = 3, 96, 64
    big = x = None
    try:
        if layout == "sb > 2^31":
            B = 2
            img = _exact_images(B, H, W, salt=1).to(DEV)
            sb = 2 ** 31 + 64
            big = torch.empty(sb + 3 * H * W, device=DEV, dtype=torch.bfloat16)          # ~4.3 GB, never filled
            x = big.as_strided((B, 3, H, W), (sb, H * W, W, 1))
            src = img.to(torch.bfloat16)
            for b in range(B):
                x[b].copy_(src[b])
            assert x.stride(0) > 2 ** 31 and x[1].data_ptr() - x[0].data_ptr() == 2 * sb
        else:
            img = _exact_images(B, H, W, salt=1).to(DEV)
            x, src = _layout(layout, img)
        xc = src.contiguous()
        assert x.shape == xc.shape and x.dtype == xc.dtype and xc.is_contiguous()
        if layout != "sb > 2^31":
            assert torch.equal(x, xc)
        ref = _ref_exact(xc.float().cpu(), Cm, Co)
        y = _twice(x, Cm, Co, ref, f"stem {Cm}->{Co} {layout}")
        yc = _twice(xc, Cm, Co, ref, f"stem {Cm}->{Co} {layout}, contiguous copy")
        assert torch.equal(y, yc)
        if "batch expand" in layout:
            assert all(torch.equal(y[0], y[b]) for b in range(1, B))
    finally:
        if big is not None:
            del big, x
            torch.cuda.empty_cache()          # (hand the 4.3 GB back: the rest of the suite shares the device)


# ------------------------------------------------------------------------------------------------
# 3. the packer
@pytest.mark.parametrize("Cm,Co", VARIANTS)
def test_stem_pack_reads_only_its_columns(Cm, Co):
    """Padded ld2 (the GEMM form's multiple of 64) with NaN in the pad columns, NaN in columns 27 .. 31 of w1m: the same packed bytes, and the same output."""
    from lemevit_amd import ops
    from lemevit_amd._lib import lib
    w1m, w2m, b1, b2 = _exact_weights(Cm, Co)
    wpk, b1d, b2d = _exact_dev(Cm, Co)
    assert wpk.dtype == torch.uint8 and wpk.numel() == lib.lmv_stem_wpk_bytes(Cm, Co) == {48: 98304, 32: 40960}[Cm]
    ld2 = (9 * Cm + 63) // 64 * 64
    assert ld2 == {48: 448, 32: 320}[Cm] and w2m.shape[1] == 9 * Cm
    w2p = torch.full((Co, ld2), NAN, dtype=torch.bfloat16)
    w2p[:, :9 * Cm] = w2m
    w1p = w1m.clone()
    w1p[:, 27:] = NAN
    x, ref = _exact_case(2, 64, 32, Cm, Co)
    for what, a, b in [("padded ld2", w1m, w2p), ("poisoned w1m", w1p, w2m), ("both", w1p, w2p)]:
        a, b = a.to(DEV), b.to(DEV)
        assert b.stride(0) == b.shape[1] and int(torch.isnan(a).sum()) + int(torch.isnan(b).sum()) > 0
        got = ops.stem_pack(a, b)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and got.shape == wpk.shape and torch.equal(got, wpk), f"stem_pack {Cm}->{Co}: {what} packs differently"
        _twice(x.to(DEV), Cm, Co, ref, f"stem {Cm}->{Co} packed from {what}", (got, b1d, b2d))
    # lmv_stem_pack itself with an odd ld2 and LIVE values behind the columns (the wrapper takes whole contiguous matrices only)
    from lemevit_amd._lib import check
    wide, w1d = torch.cat([w2m, -w2m[:, :61]], dim=1).to(DEV), w1m.to(DEV)
    got = torch.full_like(wpk, 0xA5)
    check(lib.lmv_stem_pack(w1d.data_ptr(), wide.data_ptr(), wide.stride(0), Cm, Co, got.data_ptr(), torch.cuda.current_stream().cuda_stream), "lmv_stem_pack")
    torch.cuda.synchronize()
    assert wide.stride(0) == 9 * Cm + 61 and torch.equal(got, wpk)


# ------------------------------------------------------------------------------------------------
# 4. the tile between the convolutions, element by element
QUAD = [(1, 1), (1, 2), (2, 1), (2, 2)]          # these four taps of a stride-2 convolution reach every T1 pixel: T1[2 oy - 1 + ky][2 ox - 1 + kx]
EDGE = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)]          # taps that read conv2's zero padding at oy = 0 (ky = 0) and / or ox = 0 (kx = 0)


def _probe_packs(Cm, Co):
    """Lists of Co (ky, kx, ci) -- the one non-zero weight, 1.0, of each output channel.  The first 4 Cm / Co lists walk every (tap of QUAD, ci) once, in a scrambled order."""
    combos = [(ky, kx, ci) for (ky, kx) in QUAD for ci in range(Cm)]
    n = len(combos)
    assert n % Co == 0 and math.gcd(5, n) == 1
    order = [(5 * i + 3) % n for i in range(n)]
    assert sorted(order) == list(range(n))
    packs = [[combos[order[p * Co + co]] for co in range(Co)] for p in range(n // Co)]
    packs.append([EDGE[co % 5] + ((5 * co + 3) % Cm,) for co in range(Co)])
    return packs


@functools.lru_cache(maxsize=None)
def _probe_operands(Cm):
    """Images with full fp32 mantissas; w1m and b1 scaled per channel from narrow to wide so that the pre-activations cover the polynomial's whole range."""
    B, H, W = 2, 64, 96
    x = det_tensor((B, 3, H, W), "stem.exact.t1.img", 5, 2.0)
    scale = torch.tensor([0.06 + 1.7 * ((7 * c + 2) % Cm) / (Cm - 1) for c in range(Cm)])
    w1m = torch.zeros(Cm, 32)
    w1m[:, :27] = det_tensor((Cm, 27), "stem.exact.t1.w1", 5) * scale[:, None]
    w1m = w1m.to(torch.bfloat16)
    b1 = det_tensor((Cm,), "stem.exact.t1.b1", 5, 0.5) * scale
    xb = x.to(torch.bfloat16).double()          # the kernel rounds the images to bf16 (RNE) when it stages the patch
    assert not torch.equal(xb, x.double())
    W1 = w1m[:, :27].double().reshape(Cm, 3, 3, 3)
    with torch.no_grad():
        h = F.conv2d(xb, W1, b1.double(), 2, 1)
        g = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        mag = F.conv2d(xb.abs(), W1.abs(), None, 2, 1)
    assert float(h.min()) < -4.5 and float(h.max()) > 4.5 and float((h.abs() <= 1.0).double().mean()) >= 0.25, (float(h.min()), float(h.max()), float((h.abs() <= 1.0).double().mean()))
    # |error| per T1 element: the bf16 store, the polynomial (csrc/common.h: 1.9e-4), fp32 accumulation of at most 64 terms
    bound = 2.0 ** -8 * g.abs() + 1.9e-4 + 2.0 ** -18 * mag
    return x, w1m, b1, g, bound


@pytest.mark.parametrize("Cm,Co", VARIANTS)
def test_stem_t1_probe(Cm, Co):
    """conv1 + bias + GELU, elementwise: every output channel of conv2 has ONE non-zero weight, 1.0, and b2 = 0, so y[.., co] is the bf16 value of one T1 element.
    Against the erf GELU of the float64 pre-activation (images rounded to bf16 first, as the kernel does), within 2^-8 |ref| + 1.9e-4 + 2^-18 sum |w1| |x| per element;
    where a tap reads conv2's padding the output must be exactly 0.
    Measured on an MI355X: worst error / bound 0.986 at 48 -> 96 and 0.989 at 32 -> 64."""
    from lemevit_amd import ops
    x, w1m, b1, g, bound = _probe_operands(Cm)
    B, _, H, W = x.shape
    xd, w1d, b1d, b2d = x.to(DEV), w1m.to(DEV), b1.to(DEV), torch.zeros(Co, device=DEV)
    seen = torch.zeros(Cm, H // 2, W // 2, dtype=torch.bool)
    worst = 0.0
    packs = _probe_packs(Cm, Co)
    for p, taps in enumerate(packs):
        w2 = torch.zeros(Co, 3, 3, Cm)
        for co, (ky, kx, ci) in enumerate(taps):
            w2[co, ky, kx, ci] = 1.0
        wpk = ops.stem_pack(w1d, w2.reshape(Co, 9 * Cm).to(torch.bfloat16).to(DEV))
        y = _launch(xd, wpk, b1d, b2d, Cm, Co).double().cpu()
        sel = w2.permute(0, 3, 1, 2).double()
        with torch.no_grad():
            ref = F.conv2d(g, sel, None, 2, 1).permute(0, 2, 3, 1)          # a selection: one term per output
            bnd = F.conv2d(bound, sel, None, 2, 1).permute(0, 2, 3, 1)
        err = (y - ref).abs()
        for co, (ky, kx, ci) in enumerate(taps):
            if ky == 0:
                assert bool((y[:, 0, :, co] == 0).all()) and bool((bnd[:, 0, :, co] == 0).all()), f"{Cm}->{Co} pack {p} channel {co}: conv2's top padding is not 0"
            if kx == 0:
                assert bool((y[:, :, 0, co] == 0).all()) and bool((bnd[:, :, 0, co] == 0).all()), f"{Cm}->{Co} pack {p} channel {co}: conv2's left padding is not 0"
            if (ky, kx) in QUAD and p < len(packs) - 1:
                seen[ci, ky - 1::2, kx - 1::2] = True
        live = bnd > 0
        ratio = float((err[live] / bnd[live]).max())
        worst = max(worst, ratio)
        over = err > bnd
        if bool(over.any()):
            b, oy, ox, co = [int(v) for v in np.unravel_index(int((err - bnd).flatten().argmax()), tuple(err.shape))]
            raise AssertionError(f"stem {Cm}->{Co} T1 probe, pack {p}: {int(over.sum())} elements over the bound; worst at image {b} ({oy}, {ox}) channel {co} (tap {taps[co]}): "
                                 f"got {float(y[b, oy, ox, co])!r}, reference {float(ref[b, oy, ox, co])!r}, bound {float(bnd[b, oy, ox, co]):.3e}; worst error / bound {ratio:.3f}")
    assert bool(seen.all()), "the packs do not reach every T1 element"
    print(f"stem {Cm}->{Co} T1 probe: worst error / bound {worst:.3f} over {len(packs)} packs")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------
# 5. ops.stem_fwd
def test_stem_fwd_wrapper_guards_wpk():
    """A pack of the other variant, a buffer of the right size but not uint8, a strided view, fp16 images: ValueError before any launch.  Every buffer here is a device
    buffer at least as large as what the kernel would read for the channels of the call (asserted per call): without the guard the answer would be wrong numbers, not a
    read out of bounds.  And the wrapper on good operands gives the exact reference."""
    from lemevit_amd import ops
    from lemevit_amd._lib import lib
    Cm, Co = 32, 64
    wpk, b1, b2 = _exact_dev(Cm, Co)
    other = _exact_dev(48, 96)[0]
    x, ref = _exact_case(2, 32, 64, Cm, Co)
    xd = x.to(DEV)
    need = lib.lmv_stem_wpk_bytes(Cm, Co)
    assert need == 40960 and other.numel() == 98304 and wpk.numel() == need
    bad = [("the other variant's pack", other, "holds 98304 bytes"), ("bf16, the right size in bytes", torch.zeros(need // 2, device=DEV, dtype=torch.bfloat16), "uint8"),
           ("bf16, the right number of elements", torch.zeros(need, device=DEV, dtype=torch.bfloat16), "uint8"), ("int8", torch.zeros(need, device=DEV, dtype=torch.int8), "uint8"),
           ("a strided view", torch.zeros(2 * need, device=DEV, dtype=torch.uint8)[::2], "strides")]
    for what, w, msg in bad:
        assert w.is_cuda and w.untyped_storage().nbytes() >= need and b1.numel() == Cm and b2.numel() == Co, what
        with pytest.raises(ValueError, match="stem_fwd.*" + msg):
            ops.stem_fwd(xd, w, b1, b2, Cm, Co)
    # the 48 -> 96 call with a buffer that is not its pack (too LARGE: twice what the kernel reads), biases of 48 and 96
    need2 = lib.lmv_stem_wpk_bytes(48, 96)
    big, b1w, b2w = torch.zeros(2 * need2, device=DEV, dtype=torch.uint8), torch.zeros(48, device=DEV), torch.zeros(96, device=DEV)
    assert need2 == 98304 and big.numel() > need2
    with pytest.raises(ValueError, match="stem_fwd.*holds 196608 bytes"):
        ops.stem_fwd(xd, big, b1w, b2w, 48, 96)
    for dt in (torch.float16, torch.float64, torch.uint8):
        with pytest.raises(ValueError, match="stem_fwd"):
            ops.stem_fwd(xd.to(dt), wpk, b1, b2, Cm, Co)
    for xx in (xd, xd.to(torch.bfloat16), xd.contiguous(memory_format=torch.channels_last)):
        y = ops.stem_fwd(xx, wpk, b1, b2, Cm, Co)
        torch.cuda.synchronize()
        _assert_same(y, ref, "ops.stem_fwd")
