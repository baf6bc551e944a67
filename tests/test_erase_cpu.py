"""Host half of the native random erasing (lemevit_amd.recipe.RandomErasing, lmv_augment_images in csrc/recipe.hip) without a GPU: Philox4x32-10 against the
Random123 known answers, the fill values against a restatement written here with Python integers, the draws of RandomErasing against a restatement of timm's
``RandomErasing._erase`` (timm.data.random_erasing) over a numpy Generator, and the ABI: the symbol exported and bound, argument validation before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

M32 = 0xffffffff


def R():
    from lemevit_amd import recipe
    return recipe


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def ref_philox(ctr, key):
    """Philox4x32-10 with Python integers (Salmon et al., SC'11)"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def ref_lane(r, lane):
    """Box-Muller: lanes 0, 1 from (r0, r1), lanes 2, 3 from (r2, r3)"""
    ra, rb = r[lane & 2], r[(lane & 2) + 1]
    u1, u2 = ((ra >> 9) + 1) * 2.0 ** -23, (rb >> 8) * 2.0 ** -24
    rad, ang = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
    return rad * (math.sin(ang) if lane & 1 else math.cos(ang))


def ref_noise(key, b, c, y, x):
    return ref_lane(ref_philox((x >> 2, y, c, b), key), x & 3)


def ref_noise_rand(key, b, j, c):
    return ref_lane(ref_philox((j, M32, c, b), key), 0)


def ref_erase(rng, B, H, W, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1, max_count=None, num_splits=0):
    """timm's RandomErasing.__call__ / _erase over a batch: the boxes per image, then the key"""
    max_aspect = max_aspect or 1 / min_aspect
    lo, hi = math.log(min_aspect), math.log(max_aspect)
    max_count = max_count or min_count
    start = B // num_splits if num_splits > 1 else 0
    boxes = [[] for _ in range(B)]
    for i in range(start, B):
        if rng.random() > probability:
            continue
        count = min_count if min_count == max_count else int(rng.integers(min_count, max_count + 1))
        for _ in range(count):
            for _attempt in range(10):
                target_area = rng.uniform(min_area, max_area) * (H * W) / count
                aspect_ratio = math.exp(rng.uniform(lo, hi))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < W and h < H:
                    top = int(rng.integers(0, H - h + 1))
                    left = int(rng.integers(0, W - w + 1))
                    boxes[i].append((top, top + h, left, left + w))
                    break
    key = tuple(int(k) for k in rng.integers(0, 2 ** 32, 2))
    return boxes, key


def boxes_of(arr):
    """[B, 4, 4] -> the non-empty boxes per image"""
    return [[tuple(int(v) for v in bx) for bx in img if bx[1] > bx[0] and bx[3] > bx[2]] for img in arr]


# ---- Philox and the fill values ------------------------------------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((M32,) * 4, (M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    """The Random123 known-answer vectors of philox4x32_10, for the module's restatement and for this file's"""
    assert " ".join("%08x" % int(v) for v in R().philox4x32_10(ctr, key)) == want
    assert " ".join("%08x" % v for v in ref_philox(ctr, key)) == want


def test_philox_broadcasts():
    x = np.arange(37)
    got = R().philox4x32_10((x, 5, x * 3, 2 ** 32 - 1 - x), (0xdeadbeef, 7))
    for i in range(37):
        assert tuple(int(g[i]) for g in got) == ref_philox((i, 5, i * 3, 2 ** 32 - 1 - i), (0xdeadbeef, 7))


def test_erase_noise_equals_the_restatement():
    """Every lane, several rows / channels / images and keys: the float64 values agree to rounding (both sides evaluate the same formula in float64)."""
    for key in [(0, 0), (1, 2), (0x9abcdef0, 0xffffffff)]:
        b, c, y, x = np.meshgrid(np.arange(3), np.arange(2), np.array([0, 5, 223]), np.arange(13), indexing="ij")
        got = R().erase_noise(key, b, c, y, x)
        want = np.vectorize(lambda b_, c_, y_, x_: ref_noise(key, int(b_), int(c_), int(y_), int(x_)))(b, c, y, x)
        assert got.dtype == np.float64 and got.shape == want.shape and np.abs(got - want).max() <= 1e-14
        bb, jj, cc = np.meshgrid(np.arange(3), np.arange(4), np.arange(3), indexing="ij")
        gr = R().erase_noise_rand(key, bb, jj, cc)
        wr = np.vectorize(lambda b_, j_, c_: ref_noise_rand(key, int(b_), int(j_), int(c_)))(bb, jj, cc)
        assert np.abs(gr - wr).max() <= 1e-14
    assert float(R().erase_noise((1, 2), 0, 1, 2, 3)) == pytest.approx(ref_noise((1, 2), 0, 1, 2, 3), abs=1e-14)          # scalars are accepted


@pytest.mark.parametrize("words", [(0, 0, M32, M32), (M32, M32, 0, 0), (0, M32, M32, 0), (0x000001ff, 0x40000000, 0xfffffe00, 0x80000000)])
def test_erase_noise_corner_words(monkeypatch, words):
    """The mapping at the ends of the word range (the generator replaced by one that returns the given words): r = 0 is the smallest u1 = 2^-23, amplitude
    sqrt(46 ln 2) = 5.6467, and u2 = 0; r = ffffffff is u1 = 1 (value 0 whatever the angle) and the largest u2 = 1 - 2^-24."""
    rec = R()
    monkeypatch.setattr(rec, "philox4x32_10", lambda counter, key: tuple(np.full(np.shape(counter[0]), w, dtype=np.uint64) for w in words))
    got = rec.erase_noise((3, 4), 0, 0, 0, np.arange(4))
    want = [ref_lane(words, lane) for lane in range(4)]
    assert np.abs(got - np.array(want)).max() <= 1e-14
    amp = math.sqrt(46.0 * math.log(2.0))
    assert abs(amp - 5.6467) < 1e-4
    if words == (0, 0, M32, M32):
        assert got[0] == pytest.approx(amp, abs=1e-12) and got[1] == 0.0 and got[2] == 0.0 and got[3] == 0.0
    if words == (0, M32, M32, 0):
        assert got[0] == pytest.approx(amp * math.cos(2 * math.pi * (1 - 2.0 ** -24)), abs=1e-12) and abs(got[1]) < 1e-5 * amp * 1.0 and got[2] == 0.0
    assert float(np.abs(got).max()) <= amp + 1e-12


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------------
SETTINGS = [dict(probability=0.25), dict(probability=0.5, min_count=1, max_count=3), dict(probability=1.0, min_count=2, max_count=2, min_area=0.05, max_area=0.2),
            dict(probability=0.7, num_splits=2), dict(probability=1.0, min_aspect=0.5, max_aspect=4.0, max_count=4, min_count=4),
            dict(probability=0.9, num_splits=3, min_count=1, max_count=2)]


@pytest.mark.parametrize("cfg", range(len(SETTINGS)))
@pytest.mark.parametrize("seed", [0, 17])
def test_draw_equals_the_restatement(cfg, seed):
    """Six consecutive draws per setting and seed, B = 8 and B = 5 on a 20 x 30 image: boxes and key equal the restatement's; the geometry holds."""
    H, W = 20, 30
    for B in (8, 5):
        re = R().RandomErasing(mode="pixel", seed=seed, **SETTINGS[cfg])
        rng = np.random.default_rng(seed)
        for _ in range(6):
            boxes = re._boxes(B, H, W)
            key = tuple(int(k) for k in re.rng.integers(0, 2 ** 32, 2))          # (what draw() does after the boxes)
            want_boxes, want_key = ref_erase(rng, B, H, W, **SETTINGS[cfg])
            assert boxes.shape == (B, 4, 4) and boxes.dtype == np.int32
            assert boxes_of(boxes) == want_boxes and key == want_key, (cfg, seed, B)
            for img in boxes_of(boxes):
                for yl, yh, xl, xh in img:
                    assert 0 <= yl and yh <= H and 0 < yh - yl < H and 0 <= xl and xh <= W and 0 < xh - xl < W
            ns = SETTINGS[cfg].get("num_splits", 0)
            if ns > 1:
                assert not boxes[:B // ns].any()
            lo, hi = SETTINGS[cfg].get("min_count", 1), SETTINGS[cfg].get("max_count") or SETTINGS[cfg].get("min_count", 1)
            assert all(len(img) <= hi for img in boxes_of(boxes))
            if SETTINGS[cfg]["probability"] == 1.0:
                assert all(lo <= len(img) for img in boxes_of(boxes))          # (the 20 x 30 image takes every box of these settings within 10 attempts)


def test_count_is_drawn_between_min_and_max():
    re = R().RandomErasing(probability=1.0, min_count=1, max_count=4, min_area=0.02, max_area=0.1, seed=3)
    counts = {len(img) for _ in range(20) for img in boxes_of(re._boxes(8, 32, 32))}
    assert counts == {1, 2, 3, 4}


def test_num_splits_leaves_the_first_part_untouched():
    re = R().RandomErasing(probability=1.0, num_splits=2, seed=5)
    for B in (8, 7):
        b = re._boxes(B, 32, 32)
        assert not b[:B // 2].any() and all(len(img) == 1 for img in boxes_of(b)[B // 2:])


def test_an_image_no_box_fits_comes_back_unerased():
    """H = W = 2 with min_area = max_area = 1: h < 2 needs an aspect below 0.5625 and w < 2 one above 1.78 -- all 10 attempts fail, and they consume their draws"""
    re = R().RandomErasing(probability=1.0, min_area=1.0, max_area=1.0, seed=1)
    rng = np.random.default_rng(1)
    assert not re._boxes(3, 2, 2).any()
    key = tuple(int(k) for k in re.rng.integers(0, 2 ** 32, 2))
    want, want_key = ref_erase(rng, 3, 2, 2, probability=1.0, min_area=1.0, max_area=1.0)
    assert want == [[], [], []] and key == want_key          # both generators are at the same point: 3 x (1 + 10 x 2) draws, then the key


def test_erased_share():
    """probability = 0.25 over 4000 images: the erased share within 0.25 +- 0.035 (5 sigma of the binomial, sigma = 0.0068)"""
    re = R().RandomErasing(probability=0.25, mode="pixel", seed=2024)
    n = sum(len(img) > 0 for _ in range(40) for img in boxes_of(re._boxes(100, 224, 224)))
    assert abs(n / 4000 - 0.25) <= 0.035, n / 4000


def test_draw_fills_a_buffer_off_the_device():
    """draw(..., device='cpu'): one buffer, boxes then key, its views the table and the key; a fresh key at every draw; the shape is remembered for draw()."""
    re = R().RandomErasing(probability=0.6, mode="pixel", seed=4)
    with pytest.raises(RuntimeError):
        re.draw()
    boxes, key = re.draw(6, 20, 30, device="cpu")
    assert re.buffer.dtype == torch.int32 and re.buffer.numel() == 6 * 16 + 2 and tuple(re.table.shape) == (6, 16) and tuple(re.key.shape) == (2,)
    assert re.table.data_ptr() == re.buffer.data_ptr() and re.key.data_ptr() == re.buffer.data_ptr() + 4 * 96
    assert torch.equal(re.table, R().pack_erase_records(boxes)) and torch.equal(re.table, re.records) and re.table.view(6, 4, 4).numpy().tolist() == boxes.tolist()
    assert tuple(int(k) & M32 for k in re.key.tolist()) == key == re.host_key
    first, keys = re.buffer, {key}
    for _ in range(5):
        b2, k2 = re.draw()
        assert re.buffer is first and torch.equal(re.table, R().pack_erase_records(b2))
        keys.add(k2)
    assert len(keys) == 6, "the key changes at every draw"
    re.upload([[(1, 2, 3, 4)], [], [(0, 20, 0, 30), (2, 3, 4, 5)], [], [], []], (7, M32), 20, 30, device="cpu")
    assert re.buffer is first and re.table[2].tolist() == [0, 20, 0, 30, 2, 3, 4, 5] + [0] * 8 and re.key.tolist() == [7, -1]


def test_mixup_draws_both_tables():
    rec = R()
    re = rec.RandomErasing(probability=1.0, mode="pixel", seed=8)
    mix = rec.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", seed=3, random_erasing=re)
    plain = rec.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", seed=3)
    a, b = mix.draw(6, 20, 30, device="cpu"), plain.draw(6, 20, 30, device="cpu")
    assert a.tolist() == b.tolist(), "the erase draws come from the RandomErasing's own generator: the mix records are what they are without it"
    assert re.table is not None and all(len(img) == 1 for img in boxes_of(re.table.view(6, 4, 4).numpy()))
    k1 = re.host_key
    mix.draw()
    assert re.host_key != k1


# ---- errors and binding ------------------------------------------------------------------------------------------------------------------------------
def test_constructor_errors():
    rec = R()
    with pytest.raises(ValueError):
        rec.RandomErasing(max_count=5)
    with pytest.raises(ValueError):
        rec.RandomErasing(mode="noise")
    with pytest.raises(ValueError):
        rec.RandomErasing(mean=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError):
        rec.Mixup(mean=(0.5,), std=(0.5,), random_erasing=rec.RandomErasing(mean=(0.5,), std=(0.5,)))
    assert rec.RandomErasing(max_count=4).max_count == 4 and rec.RandomErasing(min_count=2).max_count == 2
    with pytest.raises(ValueError):
        rec.pack_erase_records([[(0, 1, 0, 1)] * 5])


def test_symbol_exported_and_bound():
    import lemevit_amd
    from lemevit_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "lmv_augment_images") and getattr(_lib.lib, "lmv_augment_images").restype is ctypes.c_int
    assert len(_lib.SIGNATURES["lmv_augment_images"][1]) == 21
    assert ctypes.sizeof(_lib.EraseRecord) == 64 and ops.ERASE_RECORD_WORDS == 16 and _lib.ERASE_MAX_BOXES == 4
    assert ops.ERASE_MODES == {"const": 0, "rand": 1, "pixel": 2}
    assert _lib.ABI_VERSION == 14 and lemevit_amd.RandomErasing is R().RandomErasing and "RandomErasing" in lemevit_amd.__all__
    assert len(_lib.SIGNATURES["lmv_mix_images"][1]) == 17          # the entry points of the mixing pull request are as they were


def test_argument_validation_without_a_device():
    """LMV_ERR_SHAPE and a message before any launch (the device pointers are never dereferenced on these paths)."""
    from lemevit_amd._lib import lib
    H, W = 20, 30
    X, O, T, E, K = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24

    def aug(x=X, out=O, x_dtype=0, out_dtype=0, mix=T, host=None, erase=E, key=K, mode=2, ehost=None, scale=None, shift=None, shape=(1, 3, H, W)):
        return lib.lmv_augment_images(x, x_dtype, 1, 1, 1, 1, out, out_dtype, *shape, mix, host, erase, key, mode, ehost, scale, shift, None)
    # everything lmv_mix_images refuses
    assert aug(x=None) == -1 and b"null image" in lib.lmv_last_error()
    assert aug(out=None) == -1 and b"null image" in lib.lmv_last_error()
    assert aug(x_dtype=5) == -1 and b"dtype" in lib.lmv_last_error()
    assert aug(out_dtype=2) == -1 and b"dtype" in lib.lmv_last_error()
    assert aug(shape=(1, 0, H, W)) == -1 and b"shape" in lib.lmv_last_error()
    assert aug(shape=(0, 3, H, W)) == -1 and b"shape" in lib.lmv_last_error()
    assert aug(scale=T) == -1 and b"scale" in lib.lmv_last_error()
    assert aug(mix=T + 2) == -1 and b"misaligned" in lib.lmv_last_error()
    assert aug(out=O + 2) == -1 and b"misaligned" in lib.lmv_last_error()
    for bad in [(1.0, 0, H + 1, 0, 3, 1.0), (1.0, 0, 3, 0, W + 1, 1.0), (1.0, 5, 4, 0, 3, 1.0), (1.0, -1, 4, 0, 3, 1.0), (1.0, 0, 4, 7, 3, 1.0)]:
        host = R().pack_records(R().make_records([bad]))
        assert aug(host=host.data_ptr()) == -1 and b"outside" in lib.lmv_last_error(), bad
    nan = R().pack_records(R().make_records([(float("nan"), 0, 0, 0, 0, 1.0)]))
    assert aug(host=nan.data_ptr()) == -1 and b"NaN" in lib.lmv_last_error()
    # its own
    for mode in (-1, 3, 7):
        assert aug(mode=mode) == -1 and b"erase mode" in lib.lmv_last_error()
    for mode in (1, 2):
        assert aug(key=None, mode=mode) == -1 and b"key" in lib.lmv_last_error()
    assert aug(erase=E + 1) == -1 and b"misaligned" in lib.lmv_last_error()
    assert aug(key=K + 2) == -1 and b"misaligned" in lib.lmv_last_error()
    for bad in [(0, H + 1, 0, 3), (0, 3, 0, W + 1), (5, 4, 0, 3), (-1, 4, 0, 3), (0, 4, 7, 3), (0, 4, -2, 3)]:
        for slot in (0, 3):
            ehost = R().pack_erase_records([[(1, 2, 3, 4)] * slot + [bad]])
            assert aug(ehost=ehost.data_ptr()) == -1 and b"outside" in lib.lmv_last_error() and (b"box %d" % slot) in lib.lmv_last_error(), (bad, slot)
    two = R().pack_erase_records([[(0, H, 0, W)], [(0, 1, 0, W + 1)]])          # the second image's record is looked at too
    assert aug(ehost=two.data_ptr(), shape=(2, 3, H, W)) == -1 and b"erase record 1" in lib.lmv_last_error()


def test_python_layer_refuses_the_cpu_and_bad_arguments():
    import lemevit_amd as L
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        L.ops.augment_images(x, None, None, None)
    with pytest.raises(RuntimeError, match="GPU"):
        L.RandomErasing(seed=0)(x)
    with pytest.raises(RuntimeError, match="GPU"):
        L.Mixup(seed=0, random_erasing=L.RandomErasing(seed=0))(x, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        L.RandomErasing(seed=0)(x[0])
