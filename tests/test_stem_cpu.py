"""csrc/stem.hip, the parts that need no GPU: lmv_stem_supported / lmv_stem_wpk_bytes answer for exactly the two stems the kernel is instantiated for, and
lmv_stem_fwd / lmv_stem_pack refuse every bad argument on the host, with a message, before any device call (the pointers below are never dereferenced);
and the fp32 facts about the GELU polynomial that tests/test_stem_exact_gpu.py builds its exact regime on."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(48, 96), (32, 64)]
WPK_BYTES = {(48, 96): 98304, (32, 64): 40960}
SHAPE, DTYPE = -1, -2          # LMV_ERR_SHAPE, LMV_ERR_DTYPE (include/lemevit_hip.h)


def _lib():
    from lemevit_amd import _lib as L
    return L


def test_stem_supported_is_the_two_stems_at_multiples_of_32():
    L = _lib()
    sup = L.lib.lmv_stem_supported
    for Cm, Co in VARIANTS:
        for H, W in [(32, 32), (224, 224), (96, 160), (32768, 32768)]:
            assert sup(H, W, Cm, Co, L.LMV_BF16) == 1, (H, W, Cm, Co)
        for H, W in [(48, 32), (32, 48), (32, 0), (0, 32), (-32, 32), (32, -32), (16, 16), (33, 32), (224, 225)]:
            assert sup(H, W, Cm, Co, L.LMV_BF16) == 0, (H, W, Cm, Co)
        assert sup(64, 64, Cm, Co, L.LMV_F32) == 0 and sup(64, 64, Cm, Co, L.LMV_U8) == 0 and sup(64, 64, Cm, Co, 7) == 0
    for Cm, Co in [(40, 80), (48, 64), (32, 96), (96, 48), (64, 128), (0, 0), (48, 0), (-48, -96)]:
        assert sup(64, 64, Cm, Co, L.LMV_BF16) == 0, (Cm, Co)


def test_stem_wpk_bytes_is_the_fragment_count_of_the_geometry():
    L = _lib()
    for (Cm, Co), nb in WPK_BYTES.items():
        # SG2 (csrc/stem.hip): W1_FRAGS = 2 Cm / 16, W2_FRAGS = 3 ceil(3 Cm / 32) Co / 16, 64 lanes x 16 bytes each
        frags = 2 * (Cm // 16) + 3 * ((3 * Cm + 31) // 32) * (Co // 16)
        assert frags * 1024 == nb
        assert L.lib.lmv_stem_wpk_bytes(Cm, Co) == nb
    for Cm, Co in [(40, 80), (48, 64), (32, 96), (96, 48), (0, 0), (96, 192)]:
        assert L.lib.lmv_stem_wpk_bytes(Cm, Co) == 0, (Cm, Co)


X, WPK, B1, B2, Y = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000          # never dereferenced: every case below is refused on the host


def _fwd(L, **kw):
    a = dict(x=X, dt=L.LMV_F32, sb=3 * 64 * 64, sc=64 * 64, sh=64, sw=1, B=2, H=64, W=64, Cm=48, Co=96, wpk=WPK, b1=B1, b2=B2, y=Y)
    a.update(kw)
    rc = L.lib.lmv_stem_fwd(a["x"], a["dt"], a["sb"], a["sc"], a["sh"], a["sw"], a["B"], a["H"], a["W"], a["Cm"], a["Co"], a["wpk"], a["b1"], a["b2"], a["y"], None)
    return rc, L.lib.lmv_last_error().decode(errors="replace")


FWD_CASES = [("40 -> 80 channels", dict(Cm=40, Co=80), DTYPE, "unsupported stem"), ("48 -> 64 channels", dict(Cm=48, Co=64), DTYPE, "unsupported stem"),
             ("H = 48", dict(H=48), DTYPE, "unsupported stem"), ("W = 0", dict(W=0), DTYPE, "unsupported stem"), ("H < 0", dict(H=-64), DTYPE, "unsupported stem"),
             ("dtype code u8", dict(dt=2), DTYPE, "fp32 or bf16"), ("dtype code -1", dict(dt=-1), DTYPE, "fp32 or bf16"), ("dtype code 7", dict(dt=7), DTYPE, "fp32 or bf16"),
             ("null x", dict(x=None), SHAPE, "null or misaligned"), ("null wpk", dict(wpk=None), SHAPE, "null or misaligned"), ("null b1", dict(b1=None), SHAPE, "null or misaligned"),
             ("null b2", dict(b2=None), SHAPE, "null or misaligned"), ("null y", dict(y=None), SHAPE, "null or misaligned"),
             ("misaligned wpk", dict(wpk=WPK + 8), SHAPE, "null or misaligned"), ("misaligned y", dict(y=Y + 2), SHAPE, "null or misaligned"),
             ("misaligned b1", dict(b1=B1 + 4), SHAPE, "null or misaligned"), ("misaligned b2", dict(b2=B2 + 12), SHAPE, "null or misaligned"),
             ("B = 0", dict(B=0), SHAPE, "null or misaligned"), ("B < 0", dict(B=-1), SHAPE, "null or misaligned"),
             ("2^31 tiles", dict(B=2048, H=32768, W=32768), SHAPE, "too many tiles")]


@pytest.mark.parametrize("Cm,Co", VARIANTS)
def test_stem_fwd_refuses_bad_arguments_without_a_launch(Cm, Co):
    L = _lib()
    for dt in (L.LMV_F32, L.LMV_BF16):
        for what, kw, code, msg in FWD_CASES:
            rc, err = _fwd(L, **{"Cm": Cm, "Co": Co, "dt": dt, **kw})
            assert rc == code and err.startswith("stem_fwd") and msg in err, (what, rc, err)
    assert 2048 * (32768 // 32) ** 2 == 1 << 31          # (the tile count of the last case: the first one an int cannot hold)
    # an unaligned IMAGE pointer is fine (any strides, any offset): nothing on the host objects to it -- it is the null wpk that is refused here
    rc, err = _fwd(L, Cm=Cm, Co=Co, x=X + 2, wpk=None)
    assert rc == SHAPE and "null or misaligned" in err


@pytest.mark.parametrize("Cm,Co", VARIANTS)
def test_stem_pack_refuses_bad_arguments_without_a_launch(Cm, Co):
    L = _lib()
    W1, W2, OUT = 0x600000, 0x700000, 0x800000

    def pack(w1=W1, w2=W2, ld2=9 * Cm, cm=Cm, co=Co, out=OUT):
        rc = L.lib.lmv_stem_pack(w1, w2, ld2, cm, co, out, None)
        return rc, L.lib.lmv_last_error().decode(errors="replace")

    for what, kw in [("40 -> 80", dict(cm=40, co=80)), ("swapped", dict(cm=Co, co=Cm)), ("the other Co", dict(co=160 - Co))]:
        rc, err = pack(**kw)
        assert rc == DTYPE and err.startswith("stem_pack") and "not a supported stem" in err, (what, rc, err)
    for what, kw in [("null w1m", dict(w1=None)), ("null w2m", dict(w2=None)), ("null out", dict(out=None)), ("misaligned out", dict(out=OUT + 8)),
                     ("ld2 = 9 Cm - 1", dict(ld2=9 * Cm - 1)), ("ld2 = 0", dict(ld2=0)), ("ld2 < 0", dict(ld2=-9 * Cm))]:
        rc, err = pack(**kw)
        assert rc == SHAPE and err.startswith("stem_pack") and "bad argument" in err, (what, rc, err)


def test_stem_fwd_wrapper_refuses_before_it_touches_the_library():
    """ops.stem_fwd's own checks (images on the GPU, 3 channels) come before anything is allocated or launched."""
    from lemevit_amd import ops
    z = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(ValueError, match="stem_fwd"):
        ops.stem_fwd(torch.zeros(1, 3, 32, 32), z, torch.zeros(48), torch.zeros(96), 48, 96)
    with pytest.raises(TypeError, match="stem_pack"):
        ops.stem_pack(torch.zeros(48, 32), torch.zeros(96, 432))


# ------------------------------------------------------------------------------------------------
# the GELU polynomial in fp32 (gelu_poly2 in csrc/common.h, gelu4 in csrc/stage_common.h): what the clamp gives, and the documented error
COEF = [-1.6300047636032104, 7.93373966217041, -16.877059936523438, 20.921268463134766, -17.09065055847168, 9.8812894821167, -4.233964920043945, 1.595382571220398]


def _coefficients_in_the_sources():
    out = []
    for f in ("common.h", "stage_common.h"):
        src = open(os.path.join(ROOT, "lemevit_amd", "csrc", f)).read()
        out.append(all(repr(c) + "f" in src for c in COEF))
    return out


def _fma32(a, b, c):
    """fl32(a b + c) for fp32 a, b, c: the product of two fp32 values is exact in float64, and the float64 sum is then rounded once more to fp32 (a double
    rounding only on an exact tie of the float64 sum, which the cases below stand clear of: asserted by the caller where it matters)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def test_gelu_polynomial_at_the_clamp_in_fp32():
    assert _coefficients_in_the_sources() == [True, True], "the test's coefficients are not the sources'"
    c = [np.float32(v) for v in COEF]
    assert [float(v) for v in c] == COEF          # fp32 literals
    for s in (np.float32(1.0), np.float32(-1.0)):
        u = np.float32(s * s)
        q = c[0]
        for k in c[1:]:
            q = _fma32(q, u, k)
        phi = _fma32(s, q, np.float32(0.5))
        assert float(q) == 0.5 - 2.0 ** -23          # q(1) = 0.49999988, not 1/2
        assert float(phi) == (1.0 - 2.0 ** -23 if s > 0 else 2.0 ** -23), (float(s), float(phi))
    # hence, for integers h in [4, 256]: bf16(fl32(h (1 - 2^-23))) == h -- the T1 store of the exact regime gives the integer back
    h = torch.arange(4, 257, dtype=torch.float64)
    t1 = (h * (1.0 - 2.0 ** -23)).to(torch.float32)
    assert bool((t1 < h.float()).all()), "fl32(h (1 - 2^-23)) is not below h for some integer h: the clamp value is not what this file documents"
    assert torch.equal(t1.to(torch.bfloat16).double(), h)
    # and GELU(x <= -4) = x 2^-23 is small but not zero
    assert float(np.float32(-4.0) * np.float32(2.0 ** -23)) != 0.0


def test_gelu_polynomial_error_in_float64():
    """The same polynomial with the fp32 coefficients, evaluated in float64 over [-6, 6]: max |GELU error| 1.802e-4, inside the 1.9e-4 of common.h."""
    x = torch.linspace(-6.0, 6.0, 1200001, dtype=torch.float64)
    s = (x * 0.25).clamp(-1.0, 1.0)
    u = s * s
    q = torch.full_like(x, COEF[0])
    for k in COEF[1:]:
        q = q * u + k
    err = float((x * (0.5 + s * q) - 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))).abs().max())
    print(f"gelu polynomial vs erf GELU on [-6, 6], float64: max |error| {err:.4e}")
    assert 1.7e-4 <= err <= 1.9e-4, err
