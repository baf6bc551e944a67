"""Native random erasing fused into the batch-mixing launch (lmv_augment_images, lemevit_amd.RandomErasing, Mixup(random_erasing=...)) on a real MI355X.
Outside the boxes the launch must give lmv_mix_images' bits; inside, the fill value: 0, or the on-chip noise against a float64 restatement of Philox4x32-10 and
the Box-Muller mapping written here in numpy (independent of lemevit_amd.recipe).  Then layout independence of the noise, its statistics, determinism, the
composition with Mixup, one train step and a captured step whose replays erase differently."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(4, 3, 17, 23), (4, 3, 16, 24), (5, 1, 8, 40), (2, 13, 16, 16)]          # no 16-byte phase, odd rows | vector path | odd B: the middle image is its own partner | many channels
IDS = ["x".join(map(str, s)) for s in SHAPES]
IN_DTYPES = [torch.uint8, torch.float32, torch.bfloat16]
OUT_DTYPES = [torch.float32, torch.bfloat16]
KEY = (0x1234abcd, 0x9e3779b9)
# |fp32 noise - float64| <= 1e-5, derived: the amplitude is at most sqrt(46 ln 2) = 5.65, u1 and u2 are exact in fp32, the angle carries at most ~8e-7 and logf / sqrtf /
# cosf a few ulp each: under 7e-6 in all (the same formula in numpy fp32 over 2^24 samples: 1.9e-6).  A bf16 output adds one rounding: 2^-8 |z| + 1e-5.
TOL32 = 1e-5


def Lm():
    import lemevit_amd
    return lemevit_amd


def R():
    from lemevit_amd import recipe
    return recipe


# ---- the restatement (numpy, float64) ------------------------------------------------------------------------------------------------------------
def ref_philox(c0, c1, c2, c3, key):
    u = np.uint64
    c = [np.asarray(v).astype(u) for v in (c0, c1, c2, c3)]
    k0, k1 = u(key[0]), u(key[1])
    lo32 = u(0xffffffff)
    for _ in range(10):
        p0, p1 = c[0] * u(0xD2511F53), c[2] * u(0xCD9E8D57)
        c = [(p1 >> u(32)) ^ c[1] ^ k0, p1 & lo32, (p0 >> u(32)) ^ c[3] ^ k1, p0 & lo32]
        k0, k1 = (k0 + u(0x9E3779B9)) & lo32, (k1 + u(0xBB67AE85)) & lo32
    return c


def ref_pair(ra, rb):
    u1 = ((ra >> np.uint64(9)) + np.uint64(1)).astype(np.float64) * 2.0 ** -23
    u2 = (rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


@functools.lru_cache(maxsize=None)
def pixel_noise(shape, key=KEY):
    """z64[b, c, y, x] of the 'pixel' mode: counter (x >> 2, y, c, b); lanes 0, 1 from (r0, r1), lanes 2, 3 from (r2, r3)"""
    B, C, H, W = shape
    b, c, y, x = np.meshgrid(np.arange(B), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    r = ref_philox(x >> 2, y, c, b, key)
    z0, z1 = ref_pair(r[0], r[1])
    z2, z3 = ref_pair(r[2], r[3])
    return torch.from_numpy(np.choose(x & 3, [z0, z1, z2, z3]))


def rand_noise(key, b, j, c):
    r = ref_philox(np.array([j]), np.array([0xffffffff]), np.array([c]), np.array([b]), key)
    return float(ref_pair(r[0], r[1])[0][0])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def erase_boxes(B, H, W):
    """Hand-made records (H >= 8, W >= 16).  0: empty -- its partner B - 1 has a box (a box on the partner only) | 1: W - 1 columns, touching the top and the left edge |
    2 (the middle image of B = 5): two overlapping boxes, the second touching the bottom and the right edge | 3: four boxes, two of them overlapping | 4: one column.
    B = 2: the four boxes, then the empty record."""
    rows = [[], [(0, H // 2, 0, W - 1)], [(2, 6, 3, 9), (4, H, 5, W)], [(0, 2, 0, 3), (1, 4, 2, 7), (H - 3, H, W - 5, W), (3, 5, W - 2, W)], [(1, H - 1, 1, 2)]]
    return [rows[3], rows[0]] if B == 2 else rows[:B]


def mix_rows(B, H, W):
    rows = [(0.3, 0, 0, 0, 0, 0.3), (1.0, 1, H - 2, 2, W - 3, 0.6), (0.7, 0, 0, 0, 0, 0.7), (1.0, 0, 0, 0, 0, 1.0), (1.0, 0, H // 2, 0, W // 2, 0.9)]
    return R().make_records(rows[:B])


def box_mask(boxes, shape):
    """[B, 1, H, W] bool: inside any box; and per image the index of the LAST box that holds the pixel (-1: none)"""
    B, C, H, W = shape
    last = torch.full((B, 1, H, W), -1, dtype=torch.int64)
    for b, img in enumerate(boxes):
        for j, (yl, yh, xl, xh) in enumerate(img):
            last[b, 0, yl:yh, xl:xh] = j
    return last >= 0, last


@functools.lru_cache(maxsize=None)
def images(shape, kind):
    """The same values in every layout (made once): contiguous, channels-last, and a slice with W stride 2."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H)
    if kind == torch.uint8:
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    else:
        x = torch.randn(shape, generator=g).clamp_(-4.0, 4.0).to(kind)
    wide = torch.zeros((B, C, H, 2 * W + 1), dtype=x.dtype)
    wide[..., 1::2] = x
    xd = x.to(DEV)
    return dict(contiguous=xd, channels_last=xd.contiguous(memory_format=torch.channels_last), sliced=wide.to(DEV)[..., 1::2])


def affine(C, kind):
    c = torch.arange(C, dtype=torch.float32)
    if kind == torch.uint8:          # PrefetchLoader on 0..255 data
        std = 0.2 + 0.01 * c
        return (1.0 / (255.0 * std)).to(DEV), (-(0.4 + 0.01 * c) / std).to(DEV)
    return (0.5 + 0.03125 * c).to(DEV), (-0.25 + 0.125 * c).to(DEV)


@functools.lru_cache(maxsize=None)
def tables(shape):
    """(mix table, erase table, key, boxes, host erase records) of a shape, on the device"""
    B, C, H, W = shape
    boxes = erase_boxes(B, H, W)
    host = R().pack_erase_records(boxes)
    return R().pack_records(mix_rows(B, H, W)).to(DEV), host.to(DEV), R().pack_erase_key(KEY).to(DEV), boxes, host


def cases(shape):
    """every layout x input dtype x output dtype x (with / without the mix table and the normalisation)"""
    C = shape[1]
    mix = tables(shape)[0]
    for kind in IN_DTYPES:
        for lname, x in images(shape, kind).items():
            for out_dtype in OUT_DTYPES:
                for full in (False, True):
                    sc, sf = affine(C, kind) if full else (None, None)
                    yield f"{lname} {kind} -> {out_dtype} {'mix + affine' if full else 'plain'}", x, (mix if full else None), out_dtype, sc, sf


def base_of(x, mix, out_dtype, sc, sf):
    """what lmv_mix_images gives (identity records where there is no mix table)"""
    B = x.shape[0]
    t = mix if mix is not None else R().pack_records(R().make_records([(1.0, 0, 0, 0, 0, 1.0)] * B)).to(DEV)
    return Lm().ops.mix_images(x, t, out_dtype, sc, sf)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16), b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


def check_fill(out, base, inside, z64, name):
    """outside the boxes the bits of lmv_mix_images; inside the fill value within the bound of the output type"""
    m = inside.to(out.device).expand_as(out)
    assert same_bits(torch.where(m, torch.zeros_like(out), out), torch.where(m, torch.zeros_like(base), base)), f"{name}: changed outside the boxes"
    z = z64.to(out.device).expand_as(out)[m]
    err = (out.double()[m] - z).abs()
    bound = torch.full_like(z, TOL32) if out.dtype == torch.float32 else 2.0 ** -8 * z.abs() + TOL32
    assert bool((err <= bound).all()), (name, float((err / bound).max()))
    return float(err.max()) if err.numel() else 0.0


# ================================================================================================================================================
# 1 - 5: the launch against lmv_mix_images and the restatement
# ================================================================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_without_boxes_it_is_mix_images(shape):
    """erase_table = None, and an all-empty table in every mode: lmv_mix_images' bits for every layout, dtype pair, with and without mix table and normalisation."""
    ops = Lm().ops
    B = shape[0]
    _, _, key, _, _ = tables(shape)
    empty = torch.zeros((B, ops.ERASE_RECORD_WORDS), dtype=torch.int32, device=DEV)
    for name, x, mix, out_dtype, sc, sf in cases(shape):
        before = x.clone()
        base = base_of(x, mix, out_dtype, sc, sf)
        got = ops.augment_images(x, mix, None, None, "const", out_dtype, sc, sf)
        assert got.dtype == out_dtype and got.is_contiguous() and same_bits(got, base), name
        assert same_bits(ops.augment_images(x, mix, None, None, "pixel", out_dtype, sc, sf), base), name          # (no table: no key is asked for)
        for mode in ("const", "rand", "pixel"):
            assert same_bits(ops.augment_images(x, mix, empty, key, mode, out_dtype, sc, sf, erase_records=empty.cpu()), base), (name, mode)
        assert torch.equal(x, before)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_const_mode(shape):
    """lmv_mix_images' bits outside the boxes, exactly 0 inside (no key needed)."""
    ops = Lm().ops
    _, etable, _, boxes, host = tables(shape)
    inside, _ = box_mask(boxes, shape)
    assert inside[0].any() if shape[0] == 2 else (not inside[0].any() and inside[shape[0] - 1].any())          # the record on the partner only
    zero = torch.zeros((), dtype=torch.float64)
    for name, x, mix, out_dtype, sc, sf in cases(shape):
        out = ops.augment_images(x, mix, etable, None, "const", out_dtype, sc, sf, erase_records=host)
        assert check_fill(out, base_of(x, mix, out_dtype, sc, sf), inside, zero, name) == 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pixel_mode(shape):
    """lmv_mix_images' bits outside the boxes; inside |out - z64| <= 1e-5 (fp32) / 2^-8 |z64| + 1e-5 (bf16) against the float64 restatement.  The noise bits do
    not depend on the input's layout or dtype, nor on the mix table or the normalisation in front of the erasing."""
    ops = Lm().ops
    _, etable, key, boxes, host = tables(shape)
    inside, _ = box_mask(boxes, shape)
    z64 = pixel_noise(shape)
    worst, first = {}, {}
    for name, x, mix, out_dtype, sc, sf in cases(shape):
        out = ops.augment_images(x, mix, etable, key, "pixel", out_dtype, sc, sf, erase_records=host)
        e = check_fill(out, base_of(x, mix, out_dtype, sc, sf), inside, z64, name)
        worst[out_dtype] = max(worst.get(out_dtype, 0.0), e)
        noise = out[inside.to(DEV).expand_as(out)]
        assert same_bits(noise, first.setdefault(out_dtype, noise)), f"{name}: the noise depends on more than (key, b, c, y, x)"
    print(f"pixel mode {shape}: largest |out - z64| inside the boxes {worst}")


def launch_into(out, x, erase_table, key, mode):
    """lmv_augment_images into a given output buffer (ops.augment_images allocates its own)"""
    from lemevit_amd import _lib, ops
    codes = {torch.float32: _lib.LMV_F32, torch.bfloat16: _lib.LMV_BF16, torch.uint8: _lib.LMV_U8}
    B, C, H, W = x.shape
    _lib.check(_lib.lib.lmv_augment_images(x.data_ptr(), codes[x.dtype], *x.stride(), out.data_ptr(), codes[out.dtype], B, C, H, W, None, None, erase_table.data_ptr(),
                                           key.data_ptr(), ops.ERASE_MODES[mode], None, None, None, torch.cuda.current_stream().cuda_stream), "lmv_augment_images")


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=["f32", "bf16"])
def test_noise_does_not_depend_on_the_path(out_dtype):
    """One key, one set of boxes: the noise bits at equal (b, c, y, x) agree between the [4, 3, 17, 23] and the [4, 3, 16, 24] batch (no 16-byte phase / head chunks
    and vector stores) over their common pixels, and between an aligned output buffer and one offset by one element (vector stores / element stores)."""
    ops = Lm().ops
    boxes = erase_boxes(4, 16, 23)          # fit both shapes
    etable, key = R().pack_erase_records(boxes).to(DEV), R().pack_erase_key(KEY).to(DEV)
    outs = {}
    for shape in SHAPES[:2]:
        x = images(shape, torch.float32)["contiguous"]
        outs[shape] = ops.augment_images(x, None, etable, key, "pixel", out_dtype)
        buf = torch.zeros(x.numel() + 9, dtype=out_dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        shifted = buf[1:1 + x.numel()].view(shape)
        launch_into(shifted, x, etable, key, "pixel")
        torch.cuda.synchronize()
        assert same_bits(shifted, outs[shape]), f"{shape}: an output buffer offset by one element changes the result"
        assert float(buf[0]) == 0.0 and float(buf[1 + x.numel():].abs().max()) == 0.0, "written outside the output"
    inside = box_mask(boxes, (4, 3, 16, 23))[0].to(DEV).expand(4, 3, 16, 23)
    a, b = outs[SHAPES[0]][:, :, :16, :23][inside], outs[SHAPES[1]][:, :, :16, :23][inside]
    assert a.numel() > 500 and same_bits(a, b)
    z = pixel_noise((4, 3, 16, 23)).to(DEV)[inside]
    assert bool(((a.double() - z).abs() <= (TOL32 if out_dtype == torch.float32 else 2.0 ** -8 * z.abs() + TOL32)).all())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_rand_mode(shape):
    """One value per (box, channel), the box of the highest index winning where two overlap; equal to the restatement within the bound of the pixel mode."""
    ops = Lm().ops
    B, C, H, W = shape
    _, etable, key, boxes, host = tables(shape)
    inside, last = box_mask(boxes, shape)
    z64 = torch.zeros(shape, dtype=torch.float64)
    for b, img in enumerate(boxes):
        for j in range(len(img)):
            for c in range(C):
                z64[b, c][last[b, 0] == j] = rand_noise(KEY, b, j, c)
    for name, x, mix, out_dtype, sc, sf in cases(shape):
        out = ops.augment_images(x, mix, etable, key, "rand", out_dtype, sc, sf, erase_records=host)
        check_fill(out, base_of(x, mix, out_dtype, sc, sf), inside, z64, name)
        for b, img in enumerate(boxes):
            for j in range(len(img)):
                sel = (last[b, 0] == j).to(DEV)
                if bool(sel.any()):
                    for c in range(C):
                        assert out[b, c][sel].unique().numel() == 1, (name, b, j, c)


# ================================================================================================================================================
# 6, 7: statistics and determinism
# ================================================================================================================================================
def test_noise_statistics():
    """[8, 3, 64, 64], one 63 x 63 box per image, fp32: 95 256 samples; |mean| <= 0.02 and |var - 1| <= 0.03 (5 sigma: 0.0162 and 0.0229)."""
    ops = Lm().ops
    shape = (8, 3, 64, 64)
    boxes = [[(b % 2, b % 2 + 63, (b // 2) % 2, (b // 2) % 2 + 63)] for b in range(8)]
    x = torch.zeros(shape, device=DEV)
    out = ops.augment_images(x, None, R().pack_erase_records(boxes).to(DEV), R().pack_erase_key(KEY).to(DEV), "pixel")
    inside = box_mask(boxes, shape)[0].to(DEV).expand(shape)
    z = out[inside].double()
    assert z.numel() == 8 * 3 * 63 * 63 and float(out[~inside].abs().max()) == 0.0
    mean, var = float(z.mean()), float(z.var())
    print(f"noise statistics over {z.numel()} samples: mean {mean:+.5f}, variance {var:.5f}, largest |z| {float(z.abs().max()):.4f}")
    assert abs(mean) <= 0.02 and abs(var - 1.0) <= 0.03
    assert float(z.abs().max()) <= 5.6468
    assert float((out[inside].double() - pixel_noise(shape).to(DEV)[inside]).abs().max()) <= TOL32


def test_determinism_and_the_key():
    """Two launches with one key agree bit for bit; a second key changes more than 99 % of the erased fp32 elements and nothing else."""
    ops = Lm().ops
    shape = SHAPES[1]
    _, etable, key, boxes, _ = tables(shape)
    x = images(shape, torch.float32)["contiguous"]
    a, b = ops.augment_images(x, None, etable, key, "pixel"), ops.augment_images(x, None, etable, key, "pixel")
    assert same_bits(a, b)
    other = ops.augment_images(x, None, etable, R().pack_erase_key((KEY[0] + 1, KEY[1])).to(DEV), "pixel")
    inside = box_mask(boxes, shape)[0].to(DEV).expand(shape)
    changed = float((a[inside] != other[inside]).double().mean())
    assert changed > 0.99 and torch.equal(a[~inside], other[~inside]), changed
    r = ops.augment_images(x, None, etable, R().pack_erase_key((KEY[0] + 1, KEY[1])).to(DEV), "rand")
    assert not torch.equal(r[inside], ops.augment_images(x, None, etable, key, "rand")[inside])


# ================================================================================================================================================
# 8 - 10: Mixup(random_erasing=...), the model, capture
# ================================================================================================================================================
MEAN, STD = [255 * m for m in (0.485, 0.456, 0.406)], [255 * s for s in (0.229, 0.224, 0.225)]


@pytest.mark.parametrize("mode", ["const", "pixel"])
@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=["f32", "bf16"])
def test_mixup_with_random_erasing_is_mixup_then_erasing(mode, out_dtype, monkeypatch):
    """Mixup(mean, std, random_erasing=re) in ONE launch equals Mixup(mean, std) followed by a stand-alone erasing launch under the same records and key, bit for
    bit (uint8 loader batch).  Mixup without random_erasing never reaches ops.augment_images."""
    L, ops = Lm(), Lm().ops
    calls = []
    real = ops.augment_images
    monkeypatch.setattr(ops, "augment_images", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = images(SHAPES[0], torch.uint8)["channels_last"]
    y = torch.tensor([1, 5, 2, 7], device=DEV)
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", num_classes=10, mean=MEAN, std=STD, out_dtype=out_dtype, seed=21)
    re = L.RandomErasing(probability=0.75, mode=mode, min_count=1, max_count=3, seed=4)
    fused, plain = L.Mixup(random_erasing=re, **kw), L.Mixup(**kw)
    mixed, tgt0 = plain(x, y)
    assert calls == [], "Mixup without random_erasing must launch lmv_mix_images"
    out, tgt = fused(x, y)
    assert len(calls) == 1 and torch.equal(fused.records, plain.records) and tgt.table is fused.table
    assert re.records.any(), "precondition: the seed must erase something"
    alone = L.RandomErasing(mode=mode)
    alone.upload(re.records.view(-1, 4, 4).numpy(), re.host_key, x.shape[2], x.shape[3], device=DEV)
    assert torch.equal(alone.table, re.table) and torch.equal(alone.key, re.key)
    two = real(mixed, None, alone.table, alone.key, mode)
    assert out.dtype == out_dtype and same_bits(out, two) and not same_bits(out, mixed)
    with pytest.raises(ValueError):
        L.Mixup(random_erasing=L.RandomErasing(mean=MEAN, std=STD), **kw)


def test_random_erasing_alone():
    """re(x): a draw and one launch, out of place; with mean / std the PrefetchLoader normalisation in front of the erasing; probability 0 is the plain normalise-and-cast."""
    L, ops = Lm(), Lm().ops
    x = images(SHAPES[1], torch.uint8)["contiguous"]
    before = x.clone()
    re = L.RandomErasing(probability=1.0, mode="pixel", mean=MEAN, std=STD, out_dtype=torch.bfloat16, seed=2)
    out = re(x)
    assert torch.equal(x, before) and out.dtype == torch.bfloat16 and tuple(re.table.shape) == (4, 16) and re.table.is_cuda
    boxes = [[tuple(bx) for bx in img if bx[1] > bx[0]] for img in re.records.view(4, 4, 4).tolist()]
    assert all(len(img) == 1 for img in boxes)
    sc, sf = re._affine
    base = base_of(x, None, torch.bfloat16, sc, sf)
    check_fill(out, base, box_mask(boxes, SHAPES[1])[0], pixel_noise(SHAPES[1], re.host_key), "RandomErasing alone")
    k1 = re.host_key
    assert not same_bits(re(x), out) and re.host_key != k1          # a fresh draw at every call
    off = L.RandomErasing(probability=0.0, mode="pixel", mean=MEAN, std=STD, out_dtype=torch.bfloat16, seed=2)
    assert same_bits(off(x), base)


def test_train_step_with_mixup_random_erasing_and_native_loss():
    """One LeMeViT-Tiny step (51 classes, 96 x 96, B = 4, bf16 autocast) with Mixup(..., random_erasing=RandomErasing(0.25, mode='pixel')) and SoftTargetCrossEntropy:
    a finite loss, gradients everywhere, and the model's input is the restatement's noise pasted into ops.mix_images' output (bits outside, 1e-5 inside)."""
    L, ops = Lm(), Lm().ops
    torch.manual_seed(0)
    m = L.create_model("lemevit_tiny", num_classes=51, drop_path_rate=0.0).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn((4, 3, 96, 96), generator=g).to(DEV), torch.tensor([3, 50, 17, 3], device=DEV)
    re = L.RandomErasing(0.25, mode="pixel", seed=1)
    mix = L.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=51, seed=3, random_erasing=re)
    for _ in range(64):          # (probability 0.25 of four images: draw until the batch has an erased image -- seeded, so always the same number of draws)
        xm, tgt = mix(x, y)
        if bool(re.records.any()):
            break
    boxes = [[tuple(bx) for bx in img if bx[1] > bx[0]] for img in re.records.view(4, 4, 4).tolist()]
    inside = box_mask(boxes, x.shape)[0]
    assert 0 < int(inside.sum()) < 4 * 96 * 96
    e = check_fill(xm, ops.mix_images(x, mix.table), inside, pixel_noise(tuple(x.shape), re.host_key), "train step input")
    with torch.autocast("cuda", torch.bfloat16):
        loss = L.SoftTargetCrossEntropy()(m(xm), tgt)
    loss.backward()
    print(f"train step with random erasing: {int(inside.sum())} erased pixels per channel, largest noise error {e:.3e}, loss {float(loss.detach()):.5f}")
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert float(m.head.weight.grad.abs().max()) > 0.0


def test_captured_launch_erases_differently_at_every_replay():
    """GraphedStep over the fused launch with before_replay=mix.draw: three replays give three different batches, each the eager launch under the records and key
    of its draw; a replay without a draw in between repeats the previous batch bit for bit."""
    L, ops = Lm(), Lm().ops
    from lemevit_amd.graph import GraphedStep
    x = images(SHAPES[1], torch.uint8)["contiguous"]
    y = torch.tensor([1, 5, 2, 7], device=DEV)
    re = L.RandomErasing(probability=0.75, mode="pixel", max_count=2, seed=6)
    mix = L.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", num_classes=10, mean=MEAN, std=STD, out_dtype=torch.bfloat16, seed=9, random_erasing=re)
    out = torch.zeros(SHAPES[1], dtype=torch.bfloat16, device=DEV)

    def step():
        out.copy_(mix(x, y)[0])

    g = GraphedStep(step, warmup=1, before_replay=mix.draw)
    captured = (mix.records.clone(), re.records.clone(), re.host_key)
    sc, sf = mix._affine
    runs = []
    for _ in range(3):
        g()
        torch.cuda.synchronize()
        runs.append((out.clone(), mix.records.clone(), re.records.clone(), re.host_key))
    g.graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, runs[-1][0]), "a replay without a draw repeats the previous batch"
    assert runs[0][3] != captured[2] and len({r[3] for r in runs}) == 3
    for i, (got, mrec, erec, key) in enumerate(runs):
        eager = ops.augment_images(x, mrec.to(DEV), erec.to(DEV), R().pack_erase_key(key).to(DEV), "pixel", torch.bfloat16, sc, sf, records=mrec, erase_records=erec)
        assert same_bits(got, eager), f"replay {i}: not the eager launch under the records of its draw"
        for j in range(i):
            assert not same_bits(got, runs[j][0])
    assert any(bool(r[2].any()) for r in runs), "precondition: the seeds must erase something"
