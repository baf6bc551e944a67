"""Host half of the native mixup / cutmix and soft-target loss (lemevit_amd.recipe, csrc/recipe.hip) without a GPU: the draws of Mixup against a restatement of
timm's formulas (timm.data.mixup: Mixup._params_per_batch / _params_per_elem, rand_bbox, rand_bbox_minmax, cutmix_bbox_and_lam, mixup_target) written here in
numpy / float64, the dense form of MixedTarget, and the ABI: both symbols exported and bound, argument validation before any launch."""
import ctypes

import numpy as np
import pytest
import torch

H0, W0 = 20, 30


def R():
    from lemevit_amd import recipe
    return recipe


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def ref_rand_bbox(H, W, lam, cy, cx):
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    return (int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H)), int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W)))


class RefMixup:
    """timm.data.Mixup's parameter draws over a numpy Generator (timm uses the global numpy state; the call ORDER is timm's)."""

    def __init__(self, mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, mode, correct_lam, seed):
        self.ma, self.ca, self.minmax, self.prob, self.sp, self.mode, self.correct = mixup_alpha, (1.0 if cutmix_minmax is not None else cutmix_alpha), cutmix_minmax, prob, switch_prob, mode, correct_lam
        self.rng = np.random.default_rng(seed)
        self.enabled = True

    def per_elem(self, n):
        lam, use = np.ones(n, dtype=np.float32), np.zeros(n, dtype=bool)
        if self.enabled:
            if self.ma > 0 and self.ca > 0:
                use = self.rng.random(n) < self.sp
                mix = np.where(use, self.rng.beta(self.ca, self.ca, size=n), self.rng.beta(self.ma, self.ma, size=n))
            elif self.ma > 0:
                mix = self.rng.beta(self.ma, self.ma, size=n)
            else:
                use = np.ones(n, dtype=bool)
                mix = self.rng.beta(self.ca, self.ca, size=n)
            lam = np.where(self.rng.random(n) < self.prob, mix.astype(np.float32), lam)
        return lam, use

    def per_batch(self):
        lam, use = 1.0, False
        if self.enabled and self.rng.random() < self.prob:
            if self.ma > 0 and self.ca > 0:
                use = self.rng.random() < self.sp
                lam = self.rng.beta(self.ca, self.ca) if use else self.rng.beta(self.ma, self.ma)
            elif self.ma > 0:
                lam = self.rng.beta(self.ma, self.ma)
            else:
                use, lam = True, self.rng.beta(self.ca, self.ca)
            lam = float(lam)
        return lam, use

    def box_and_lam(self, H, W, lam):
        if self.minmax is not None:
            ch = int(self.rng.integers(int(H * self.minmax[0]), int(H * self.minmax[1])))
            cw = int(self.rng.integers(int(W * self.minmax[0]), int(W * self.minmax[1])))
            yl = int(self.rng.integers(0, H - ch)); xl = int(self.rng.integers(0, W - cw))
            box = (yl, yl + ch, xl, xl + cw)
        else:
            cy = int(self.rng.integers(0, H)); cx = int(self.rng.integers(0, W))
            box = ref_rand_bbox(H, W, lam, cy, cx)
        if self.correct or self.minmax is not None:
            lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        return box, lam

    def one(self, H, W, lam, use):
        """what _mix_elem / _mix_pair / _mix_batch do with one (lam, use_cutmix): (image weight, box, target factor)"""
        if lam == 1.0:
            return (1.0, 0, 0, 0, 0, 1.0)
        if use:
            box, lam = self.box_and_lam(H, W, lam)
            return (1.0,) + box + (lam,)
        return (lam, 0, 0, 0, 0, lam)

    def records(self, B, H, W):
        if self.mode == "batch":
            lam, use = self.per_batch()
            return [self.one(H, W, lam, use)] * B
        if self.mode == "elem":
            lam, use = self.per_elem(B)
            return [self.one(H, W, float(lam[i]), bool(use[i])) for i in range(B)]
        lam, use = self.per_elem(B // 2)
        first = [self.one(H, W, float(lam[i]), bool(use[i])) for i in range(B // 2)]
        return first + [(1.0, 0, 0, 0, 0, 1.0)] * (B % 2) + first[::-1]


def ref_mixup_target(labels, num_classes, lam, smoothing):
    """timm.data.mixup.mixup_target in float64"""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off

    def one_hot(y):
        t = np.full((len(y), num_classes), off, dtype=np.float64)
        t[np.arange(len(y)), y] = on
        return t
    lam = np.asarray(lam, dtype=np.float64).reshape(-1, 1)
    return one_hot(labels) * lam + one_hot(labels[::-1]) * (1.0 - lam)


def as_rows(rec):
    return [(np.float32(r["w"]), int(r["yl"]), int(r["yh"]), int(r["xl"]), int(r["xh"]), np.float32(r["lam_t"])) for r in rec]


def same_rows(got, want):
    want = [(np.float32(w), yl, yh, xl, xh, np.float32(lt)) for w, yl, yh, xl, xh, lt in want]
    return as_rows(got) == want


CONFIGS = [dict(mixup_alpha=0.8, cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=0.0), dict(mixup_alpha=0.0, cutmix_alpha=1.0),
           dict(mixup_alpha=0.8, cutmix_alpha=1.0, correct_lam=False), dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.6, switch_prob=0.3),
           dict(mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=(0.2, 0.6))]


# ---- draws -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_draw_equals_the_restatement(mode, cfg):
    """Eight consecutive draws of every configuration and mode, B = 6 and B = 5: the records equal the restatement's, field by field (floats as float32 bits)."""
    kw = dict(mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, correct_lam=True)
    kw.update(CONFIGS[cfg])
    for B in (6, 5):
        mix = R().Mixup(mode=mode, seed=17 + cfg, num_classes=10, **kw)
        ref = RefMixup(kw["mixup_alpha"], kw["cutmix_alpha"], kw["cutmix_minmax"], kw["prob"], kw["switch_prob"], mode, kw["correct_lam"], 17 + cfg)
        for _ in range(8):
            got = mix._records(B, H0, W0)
            want = ref.records(B, H0, W0)
            assert same_rows(got, want), (mode, cfg, B, as_rows(got), want)
            for w, yl, yh, xl, xh, lt in as_rows(got):
                assert 0 <= yl <= yh <= H0 and 0 <= xl <= xh <= W0 and 0.0 <= w <= 1.0 and 0.0 <= lt <= 1.0
                assert w == 1.0 or (yl, yh, xl, xh) == (0, 0, 0, 0)          # a mixup record has no box, a cutmix record has w = 1


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0])
def test_box_geometry(lam):
    """rand_bbox on a 20 x 30 image: int(H sqrt(1 - lam)) x int(W sqrt(1 - lam)) around the centre, clipped; a centre at the border gives a clipped box, lam = 1 an empty one."""
    ch, cw = int(H0 * np.sqrt(1 - lam)), int(W0 * np.sqrt(1 - lam))
    for cy, cx in [(10, 15), (0, 0), (19, 29), (0, 29), (7, 3), (19, 0)]:
        yl, yh, xl, xh = R().bbox(H0, W0, lam, cy, cx)
        assert (yl, yh, xl, xh) == ref_rand_bbox(H0, W0, lam, cy, cx)
        assert (yl, yh, xl, xh) == (max(cy - ch // 2, 0), min(cy + ch // 2, H0), max(cx - cw // 2, 0), min(cx + cw // 2, W0))
        if lam == 1.0:
            assert yh - yl == 0 and xh - xl == 0
    if lam == 0.0:
        assert R().bbox(H0, W0, lam, 10, 15) == (0, H0, 0, W0)
    if lam == 0.25:          # 17 x 25 around (0, 0): clipped to 8 x 12
        assert R().bbox(H0, W0, lam, 0, 0) == (0, 8, 0, 12)


def test_correct_lam_is_one_minus_the_box_share():
    mix = R().Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem", seed=5, num_classes=10)
    raw = R().Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem", seed=5, num_classes=10, correct_lam=False)
    rec, rec_raw = mix._records(64, H0, W0), raw._records(64, H0, W0)
    clipped = 0
    for r, q in zip(rec, rec_raw):
        area = (int(r["yh"]) - int(r["yl"])) * (int(r["xh"]) - int(r["xl"]))
        assert r["lam_t"] == np.float32(1.0 - area / float(H0 * W0)) and r["w"] == np.float32(1.0)
        assert (r["yl"], r["yh"], r["xl"], r["xh"]) == (q["yl"], q["yh"], q["xl"], q["xh"])
        clipped += int(q["lam_t"] != r["lam_t"])
    assert clipped > 0, "the uncorrected factor must differ from the corrected one on some image"


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
def test_identity_records(mode):
    ident = [(1.0, 0, 0, 0, 0, 1.0)] * 6
    off = R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, seed=1)
    off.mixup_enabled = False
    assert same_rows(off._records(6, H0, W0), ident)
    assert same_rows(R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.0, mode=mode, seed=1)._records(6, H0, W0), ident)


def test_pair_mode_gives_both_halves_the_same_record():
    mix = R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair", seed=9)
    seen = set()
    for B in (6, 5, 6, 5):
        rows = as_rows(mix._records(B, H0, W0))
        for i in range(B // 2):
            assert rows[i] == rows[B - 1 - i]
        if B % 2:
            assert rows[B // 2] == (np.float32(1.0), 0, 0, 0, 0, np.float32(1.0))
        seen |= set(rows[:B // 2])
    assert len(seen) > 4, "the pairs of a batch draw their own records"


def test_draw_statistics():
    """2 000 seeded batch-mode draws at the reference's setting (mixup 0.8, cutmix 1.0, switch 0.5): the cutmix share is within 0.05 of switch_prob, every factor in [0, 1]."""
    mix = R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5, mode="batch", seed=2024)
    n, cut = 2000, 0
    for _ in range(n):
        rec = mix._records(2, 224, 224)
        cut += int(mix.last_use_cutmix[0])
        assert 0.0 <= float(rec["w"][0]) <= 1.0 and 0.0 <= float(rec["lam_t"][0]) <= 1.0
    assert abs(cut / n - 0.5) <= 0.05, cut / n
    mix = R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.2, mode="elem", seed=7)
    mix._records(2000, 224, 224)
    assert abs(float(mix.last_use_cutmix.mean()) - 0.2) <= 0.05


def test_draw_fills_a_table_off_the_device():
    """draw(..., device='cpu'): the table is the packed records (the seam that keeps the upload off the GPU); the shape is remembered for draw()."""
    mix = R().Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", seed=3)
    with pytest.raises(RuntimeError):
        mix.draw()
    rec = mix.draw(6, H0, W0, device="cpu")
    assert mix.table.dtype == torch.int32 and tuple(mix.table.shape) == (6, 6) and torch.equal(mix.table, R().pack_records(rec)) and torch.equal(mix.table, mix.records)
    first = mix.table
    rec2 = mix.draw()
    assert mix.table is first and torch.equal(mix.table, R().pack_records(rec2)) and not torch.equal(R().pack_records(rec), R().pack_records(rec2))
    back = mix.table.numpy().view(R().RECORD_DTYPE).reshape(-1)
    assert as_rows(back) == as_rows(rec2)


# ---- the dense target ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B", [6, 5])
def test_dense_target_equals_mixup_target(B, smoothing):
    N = 11
    lams = [0.0, 0.37, 1.0, 0.62, 0.25, 0.9][:B]
    rec = R().make_records([(1.0, 0, 0, 0, 0, lt) for lt in lams])
    labels = np.array([3, 7, 3, 0, 10, 3][:B])
    tgt = R().MixedTarget(torch.from_numpy(labels), R().pack_records(rec), smoothing, N)
    want = ref_mixup_target(labels, N, rec["lam_t"].astype(np.float64), smoothing)
    got = tgt.dense().double().numpy()
    assert got.shape == (B, N) and np.abs(got - want).max() <= 1e-7
    assert np.abs(got.sum(1) - 1.0).max() <= 1e-6
    plain = R().MixedTarget(torch.from_numpy(labels), None, smoothing, N).dense().double().numpy()
    assert np.abs(plain - ref_mixup_target(labels, N, np.ones(B), smoothing)).max() <= 1e-7


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_bound():
    from lemevit_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("lmv_mix_images", "lmv_soft_ce"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES and getattr(_lib.lib, n).restype is ctypes.c_int
    assert len(_lib.SIGNATURES["lmv_mix_images"][1]) == 17 and len(_lib.SIGNATURES["lmv_soft_ce"][1]) == 15
    assert ctypes.sizeof(_lib.MixRecord) == 24 == R().RECORD_DTYPE.itemsize
    assert [n for n, _ in _lib.MixRecord._fields_] == list(R().RECORD_DTYPE.names)


def test_argument_validation_without_a_device():
    """LMV_ERR_SHAPE and a message before any launch (the pointers are never dereferenced on these paths, except the HOST records)."""
    from lemevit_amd._lib import lib
    X, O, T, L = 1 << 20, 1 << 21, 1 << 22, 1 << 23

    def mix(x_dtype=0, out_dtype=0, table=T, host=None, scale=None, shift=None, shape=(1, 3, H0, W0)):
        return lib.lmv_mix_images(X, x_dtype, 1, 1, 1, 1, O, out_dtype, *shape, table, host, scale, shift, None)
    assert mix(table=None) == -1 and b"null table" in lib.lmv_last_error()
    for bad in [(1.0, 0, H0 + 1, 0, 3, 1.0), (1.0, 0, 3, 0, W0 + 1, 1.0), (1.0, 5, 4, 0, 3, 1.0), (1.0, -1, 4, 0, 3, 1.0), (1.0, 0, 4, 7, 3, 1.0)]:
        host = R().pack_records(R().make_records([bad]))
        assert mix(host=host.data_ptr()) == -1 and b"outside" in lib.lmv_last_error(), bad
    assert mix(x_dtype=5) == -1 and b"dtype" in lib.lmv_last_error()
    assert mix(out_dtype=2) == -1 and b"dtype" in lib.lmv_last_error()          # uint8 is an input type only
    assert mix(shape=(1, 0, H0, W0)) == -1 and b"shape" in lib.lmv_last_error()
    assert mix(scale=T) == -1 and b"scale" in lib.lmv_last_error()

    def ce(dtype=0, B=4, N=8, stride=8, labels=L, table=None, smoothing=0.0, target=None, tdtype=0):
        return lib.lmv_soft_ce(X, dtype, stride, B, N, labels, table, smoothing, target, tdtype, stride, O, O + 64, None, None)
    assert ce(N=0) == -1 and b"N >= 1" in lib.lmv_last_error()
    assert ce(dtype=3) == -1 and b"dtype" in lib.lmv_last_error()
    assert ce(dtype=2) == -1 and b"dtype" in lib.lmv_last_error()               # uint8 logits do not exist
    assert ce(stride=7) == -1 and b"stride" in lib.lmv_last_error()
    assert ce(labels=None) == -1 and ce(target=T) == -1 and b"exactly one" in lib.lmv_last_error()
    assert ce(labels=None, target=T, tdtype=4) == -1 and b"target dtype" in lib.lmv_last_error()
    assert ce(smoothing=1.0) == -1 and b"smoothing" in lib.lmv_last_error()


def test_python_layer_refuses_the_cpu_and_other_dtypes():
    import lemevit_amd as L
    rec = R().pack_records(R().make_records([(1.0, 0, 0, 0, 0, 1.0)] * 2))
    with pytest.raises(RuntimeError, match="GPU"):
        L.ops.mix_images(torch.zeros(2, 3, 4, 4), rec)
    with pytest.raises(RuntimeError, match="GPU"):
        L.ops.soft_ce(torch.zeros(2, 5), labels=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        L.Mixup(seed=0)(torch.zeros(2, 3, 4, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        L.SoftTargetCrossEntropy()(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    for crit in (L.SoftTargetCrossEntropy(), L.LabelSmoothingCrossEntropy(0.1)):
        with pytest.raises(TypeError):
            crit(torch.zeros(2, 5, dtype=torch.float16), torch.zeros(2, dtype=torch.int64))
        with pytest.raises(TypeError):
            crit(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        L.Mixup(mixup_alpha=0.0, cutmix_alpha=0.0)
    with pytest.raises(ValueError):
        L.Mixup(mode="half")
