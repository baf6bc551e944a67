"""The two ends of the reference's training step, natively and capturably: mixup / cutmix and random erasing in front of the forward pass and the soft-target
loss behind it.

The reference builds ``timm.data.Mixup`` (main.py:370-389: mixup 0.8, cutmix 1.0, label smoothing 0.1 in every classification config), calls
``mixup_fn(input, target)`` ahead of every forward pass (engine.py:61-62) and picks ``SoftTargetCrossEntropy`` / ``LabelSmoothingCrossEntropy`` for the
loss (main.py:456-466).  Here:

* ``Mixup`` takes timm's constructor keywords.  The random factors and boxes are drawn on the host exactly as timm draws them and uploaded into one small
  DEVICE table; ONE launch of ``lmv_mix_images`` mixes the batch with its flipped self under that table (out of place; optional normalisation and cast
  fused in).  The target is not built: ``MixedTarget`` carries the labels, the table and the smoothing.
* ``SoftTargetCrossEntropy`` / ``LabelSmoothingCrossEntropy`` launch ``lmv_soft_ce`` once: loss and logit gradient in one pass over the logits, straight
  from the strided ``[:, :N]`` view the classifier tail hands out.

* ``RandomErasing`` takes ``timm.data.random_erasing.RandomErasing``'s keywords (the reference's loader runs it behind the ``PrefetchLoader`` normalisation:
  main.py:406-409, reprob 0.25 / remode pixel / recount 1).  The boxes are drawn on the host by timm's procedure and uploaded, with a fresh noise key, into a
  second device table; ONE launch of ``lmv_augment_images`` erases -- and, handed to ``Mixup(random_erasing=...)``, the same single launch mixes, normalises,
  erases and casts.  The noise is generated on the chip from the key and the pixel coordinates; ``erase_noise`` restates it on the host.

Because the kernels read the tables as they run, a captured step mixes (and erases) differently at every replay:
``GraphedStep(step, before_replay=lambda: (mix.draw(), opt.sync_hyper()))``.

The one difference from timm: the input batch is NOT modified (timm mixes and erases in place); use the returned tensor.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor

# lmv_mix_record (include/lemevit_hip.h): inside [yl, yh) x [xl, xh) the partner's pixel, elsewhere w * self + (1 - w) * partner; lam_t: the weight of the image's own label
RECORD_DTYPE = np.dtype([("w", "<f4"), ("yl", "<i4"), ("yh", "<i4"), ("xl", "<i4"), ("xh", "<i4"), ("lam_t", "<f4")])
assert RECORD_DTYPE.itemsize == 4 * ops.MIX_RECORD_WORDS


def make_records(rows: Sequence[Tuple[float, int, int, int, int, float]]) -> np.ndarray:
    """Hand-made records: one ``(w, yl, yh, xl, xh, lam_t)`` per image."""
    return np.array([tuple(r) for r in rows], dtype=RECORD_DTYPE)


def pack_records(records: np.ndarray) -> Tensor:
    """Host records -> the int32 [B, 6] CPU tensor the ops take (a fresh tensor: the floats travel as their bits); ``.to(device)`` makes a table."""
    rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    return torch.from_numpy(rec.view(np.int32).reshape(len(rec), ops.MIX_RECORD_WORDS).copy())


def bbox(H: int, W: int, lam: float, cy: int, cx: int) -> Tuple[int, int, int, int]:
    """timm's ``rand_bbox`` (margin 0) for a given centre: a box of ``int(H sqrt(1 - lam)) x int(W sqrt(1 - lam))`` around (cy, cx), clipped to the image."""
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
    xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
    return yl, yh, xl, xh


# ---- random erasing: the fill values of lmv_augment_images on the host (include/lemevit_hip.h defines them) ----------------------------------------
ERASE_MAX_BOXES = ops.ERASE_RECORD_WORDS // 4
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): ``counter`` four and ``key`` two 32-bit words (ints or broadcastable integer arrays) -> the four result words as uint64
    arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in key]
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]          # (32 x 32 bits: the products fit 64)
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & mask, (p0 >> sh) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & mask, (k[1] + np.uint64(_PHILOX_W1)) & mask]
    return tuple(c)


def _box_muller(ra, rb, odd):
    """The even (cos) or odd (sin) member of the pair two words give, float64"""
    u1 = ((ra >> np.uint64(9)) + np.uint64(1)).astype(np.float64) * 2.0 ** -23
    u2 = (rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return rad * np.where(odd, np.sin(ang), np.cos(ang))


def erase_noise(key, b, c, y, x):
    """The 'pixel' fill value of element (b, c, y, x) under ``key`` (two words), float64; the indices broadcast."""
    b, c, y, x = np.broadcast_arrays(*(np.asarray(v, dtype=np.int64) for v in (b, c, y, x)))
    r = philox4x32_10((x >> 2, y, c, b), key)
    second = (x & 2) != 0
    return _box_muller(np.where(second, r[2], r[0]), np.where(second, r[3], r[1]), (x & 1) != 0)


def erase_noise_rand(key, b, j, c):
    """The 'rand' fill value of box ``j``, channel ``c`` of image ``b`` under ``key``, float64; the indices broadcast."""
    b, j, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.int64) for v in (b, j, c)))
    r = philox4x32_10((j, np.full(b.shape, 0xffffffff, dtype=np.int64), c, b), key)
    return _box_muller(r[0], r[1], np.zeros(b.shape, dtype=bool))


def pack_erase_records(boxes) -> Tensor:
    """Boxes ``[B, <= 4, 4]`` (``yl, yh, xl, xh``; or a list per image of up to four such boxes) -> the int32 [B, 16] CPU tensor the ops take (missing boxes are empty)."""
    out = np.zeros((len(boxes), ERASE_MAX_BOXES, 4), dtype=np.int32)
    for i, bx in enumerate(boxes):
        bx = np.asarray(bx, dtype=np.int64).reshape(-1, 4)
        if len(bx) > ERASE_MAX_BOXES:
            raise ValueError(f"pack_erase_records: image {i} has {len(bx)} boxes, a record holds {ERASE_MAX_BOXES}")
        out[i, :len(bx)] = bx
    return torch.from_numpy(out.reshape(len(boxes), ops.ERASE_RECORD_WORDS))


def pack_erase_key(key) -> Tensor:
    """Two 32-bit key words -> the int32 [2] CPU tensor that carries their bits."""
    return torch.from_numpy(np.array([int(k) & 0xffffffff for k in key], dtype=np.uint32).view(np.int32).copy())


def _affine_vectors(mean, std):
    return 1.0 / np.asarray(std, dtype=np.float64), -np.asarray(mean, dtype=np.float64) / np.asarray(std, dtype=np.float64)


def _affine_on(host, cached, C: int, device, capturing: bool, who: str):
    """The device copies of the per-channel scale and shift (built once per device and channel count, never under capture)"""
    if cached is None or cached[0].device != device or cached[0].numel() != C:
        if capturing:
            raise RuntimeError(f"{who}: the normalisation vectors must exist before capture -- run one eager step first")
        cached = tuple(torch.tensor(np.ascontiguousarray(np.broadcast_to(v, (C,))), dtype=torch.float32).to(device) for v in host)
    return cached


class RandomErasing:
    """``timm.data.random_erasing.RandomErasing`` on the native path (same constructor keywords; timm's ``create_loader`` maps ``re_prob`` / ``re_mode`` /
    ``re_count`` / ``re_split`` of main.py:406-409 onto ``probability`` / ``mode`` / ``max_count`` / ``num_splits``).

    ``erased = re(x)``: draws the boxes on the host (``draw()``; not under graph capture), then ONE ``lmv_augment_images`` launch.  ``x``: [B, C, H, W], uint8 /
    float32 / bfloat16, any strides; it is NOT modified -- the one difference from timm, which erases in place.  ``erased`` is a new contiguous NCHW tensor of
    ``out_dtype`` (default: the input's, float32 for uint8).  ``mean`` / ``std`` (in the units of ``x``) apply ``(x - mean) / std`` in the same launch, ahead of
    the erasing, as timm's ``PrefetchLoader`` does; with both left out and no ``Mixup`` this is also the plain normalise-and-cast of a validation loader when
    ``probability = 0``.  Handed to ``Mixup(random_erasing=re)``, the mix launch does the erasing and this object is not called.

    Modes as in timm: ``const`` (zeros), ``rand`` (one normal per box and channel), ``pixel`` (one normal per element).  The noise comes from the chip: a
    counter-based generator keyed by the pixel's coordinates and a 64-bit key drawn with the boxes (``erase_noise`` / ``erase_noise_rand`` reproduce it);
    overlapping boxes of one image (``max_count`` > 1) write the same 'pixel' noise where timm would draw twice.  At most four boxes per image.

    The draws follow timm's ``_erase`` with the instance's numpy Generator: an image is skipped when ``rng.random() > probability``; ``count`` boxes, each
    with up to 10 attempts at an area ``uniform(min_area, max_area) H W / count`` and a log-uniform aspect ratio, accepted when it is smaller than the image,
    then placed uniformly; with ``num_splits`` > 1 the first ``B // num_splits`` images are never erased.

    Capture: the kernel reads the DEVICE boxes and key, so a captured launch erases with whatever they hold at replay time; under capture nothing is drawn."""

    def __init__(self, probability: float = 0.5, min_area: float = 0.02, max_area: float = 1 / 3, min_aspect: float = 0.3, max_aspect: Optional[float] = None,
                 mode: str = "const", min_count: int = 1, max_count: Optional[int] = None, num_splits: int = 0, device="cuda",
                 mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, out_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None):
        mode = mode.lower()
        if mode not in ops.ERASE_MODES:
            raise ValueError(f"RandomErasing: unknown mode {mode!r} ('const', 'rand' or 'pixel')")
        self.probability, self.min_area, self.max_area = float(probability), float(min_area), float(max_area)
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (float(np.log(min_aspect)), float(np.log(max_aspect)))
        self.min_count, self.max_count = int(min_count), int(max_count or min_count)
        if not 1 <= self.min_count <= self.max_count:
            raise ValueError("RandomErasing: 1 <= min_count <= max_count expected")
        if self.max_count > ERASE_MAX_BOXES:
            raise ValueError(f"RandomErasing: max_count = {self.max_count}: a record holds {ERASE_MAX_BOXES} boxes per image")
        if (mean is None) != (std is None):
            raise ValueError("RandomErasing: mean and std come together")
        self.mode, self.num_splits, self.device, self.out_dtype = mode, int(num_splits), device, out_dtype
        self._affine_host = None if mean is None else _affine_vectors(mean, std)
        self._affine: Optional[Tuple[Tensor, Tensor]] = None
        self.rng = np.random.default_rng(seed)
        self.buffer: Optional[Tensor] = None          # int32 [B * 16 + 2] on the device: the boxes, then the key -- one upload
        self.table: Optional[Tensor] = None           # its views: int32 [B, 16] ...
        self.key: Optional[Tensor] = None             # ... and int32 [2]
        self.records: Optional[Tensor] = None         # the host copy of the table
        self.host_key: Optional[Tuple[int, int]] = None
        self._shape: Optional[Tuple[int, int, int]] = None

    def _boxes(self, B: int, H: int, W: int) -> np.ndarray:
        """The host half of ``draw``: timm's ``_erase`` over the batch -> int32 [B, 4, 4] (``yl, yh, xl, xh``; unused boxes empty).  Nothing touches a device."""
        out = np.zeros((B, ERASE_MAX_BOXES, 4), dtype=np.int32)
        area = H * W
        for i in range(B // self.num_splits if self.num_splits > 1 else 0, B):
            if self.rng.random() > self.probability:
                continue
            count = self.min_count if self.min_count == self.max_count else int(self.rng.integers(self.min_count, self.max_count + 1))
            for j in range(count):
                for _ in range(10):
                    target = self.rng.uniform(self.min_area, self.max_area) * area / count
                    aspect = np.exp(self.rng.uniform(*self.log_aspect_ratio))
                    h, w = int(round(np.sqrt(target * aspect))), int(round(np.sqrt(target / aspect)))
                    if w < W and h < H:
                        top, left = int(self.rng.integers(0, H - h + 1)), int(self.rng.integers(0, W - w + 1))
                        out[i, j] = (top, top + h, left, left + w)
                        break
        return out

    def upload(self, boxes, key, H: int, W: int, device=None) -> None:
        """Put given boxes ([B, <= 4, 4]) and key (two words) into the persistent device buffer: ONE non-blocking copy from a fresh host tensor, stream-ordered
        on the current stream (a replay still in flight keeps reading what it was given)."""
        rec, kw = pack_erase_records(boxes), pack_erase_key(key)
        B = rec.shape[0]
        dev = torch.device(device if device is not None else self.device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        n = B * ops.ERASE_RECORD_WORDS
        if self.buffer is None or self.buffer.numel() != n + 2 or self.buffer.device != dev:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RandomErasing: the table cannot be (re)allocated under graph capture")
            self.buffer = torch.empty((n + 2,), dtype=torch.int32, device=dev)
            self.table, self.key = self.buffer[:n].view(B, ops.ERASE_RECORD_WORDS), self.buffer[n:]
        self.buffer.copy_(torch.cat([rec.reshape(-1), kw]), non_blocking=True)
        self.records, self.host_key, self._shape = rec, tuple(int(k) & 0xffffffff for k in key), (B, int(H), int(W))

    def draw(self, B: Optional[int] = None, H: Optional[int] = None, W: Optional[int] = None, device=None) -> Tuple[np.ndarray, Tuple[int, int]]:
        """Draw fresh boxes and a fresh key and upload them.  Without arguments the shape and device of the last call are used.  Returns ``(boxes, key)``."""
        if B is None:
            if self._shape is None:
                raise RuntimeError("RandomErasing.draw: no shape yet -- call draw(B, H, W) or erase a batch first")
            B, H, W = self._shape
            device = self.buffer.device if device is None else device
        elif H is None or W is None:
            raise ValueError("RandomErasing.draw: give B, H and W together")
        boxes = self._boxes(int(B), int(H), int(W))
        key = tuple(int(k) for k in self.rng.integers(0, 2 ** 32, 2))
        self.upload(boxes, key, H, W, device)
        return boxes, key

    def _ready(self, x: Tensor, capturing: bool) -> None:
        """Draw for this batch, or -- under capture -- insist that the table of an earlier eager step fits it"""
        B, _, H, W = x.shape
        if not capturing:
            self.draw(B, H, W, x.device)
        elif self.buffer is None or self._shape != (B, H, W) or self.buffer.device != x.device:
            raise RuntimeError("RandomErasing: under graph capture the table must exist for this batch shape -- run one eager step (or draw(B, H, W)) first")

    def __call__(self, x: Tensor) -> Tensor:
        if x.dim() != 4:
            raise ValueError(f"RandomErasing: [B, C, H, W] images expected, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
        capturing = torch.cuda.is_current_stream_capturing()
        self._ready(x, capturing)
        scale = shift = None
        if self._affine_host is not None:
            self._affine = _affine_on(self._affine_host, self._affine, x.shape[1], x.device, capturing, "RandomErasing")
            scale, shift = self._affine
        return ops.augment_images(x, None, self.table, self.key, self.mode, self.out_dtype, scale, shift, erase_records=None if capturing else self.records)


class MixedTarget:
    """What ``Mixup`` returns in place of timm's [B, classes] matrix: the labels, the device table and the smoothing.  The loss modules below consume it
    without materialising anything; ``dense()`` gives the matrix (``timm.data.mixup.mixup_target``) to code that wants it."""

    def __init__(self, labels: Tensor, table: Optional[Tensor], smoothing: float, num_classes: int):
        self.labels, self.table, self.smoothing, self.num_classes = labels, table, float(smoothing), int(num_classes)

    def dense(self, dtype: torch.dtype = torch.float32) -> Tensor:
        """``lam_t * one_hot(labels) + (1 - lam_t) * one_hot(labels.flip(0))`` with on = 1 - s + s / N and off = s / N, computed in float64 on the labels' device."""
        y, N = self.labels, self.num_classes
        B = y.shape[0]
        off = self.smoothing / N
        on = 1.0 - self.smoothing + off
        if self.table is None:
            lam = torch.ones(B, dtype=torch.float64, device=y.device)
        else:
            lam = self.table[:, 5].contiguous().view(torch.float32).to(device=y.device, dtype=torch.float64)

        def one_hot(lbl):
            valid = (lbl >= 0) & (lbl < N)          # (a label outside the range carries no one-hot mass, as in the kernel)
            t = torch.full((B, N), off, dtype=torch.float64, device=y.device)
            fill = (off + (on - off) * valid.to(torch.float64)).view(B, 1)
            return t.scatter_(1, lbl.clamp(0, N - 1).view(B, 1), fill)
        lam = lam.view(B, 1)
        return (one_hot(y) * lam + one_hot(y.flip(0)) * (1.0 - lam)).to(dtype)


class Mixup:
    """``timm.data.Mixup`` on the native path (same constructor keywords; main.py:375-389 binds by changing the import).

    ``mixed, target = mix(x, labels)``: draws the per-image records on the host (``draw()``; not under graph capture), then ONE ``lmv_mix_images`` launch.
    ``x``: [B, C, H, W], uint8 / float32 / bfloat16, any strides (contiguous, channels-last, sliced); it is NOT modified -- the one difference from
    timm, which mixes in place.  ``mixed`` is a new contiguous NCHW tensor of ``out_dtype`` (default: the input's, float32 for uint8;
    ``torch.bfloat16`` hands the model its compute type directly).  ``target`` is a ``MixedTarget``.

    ``mean`` / ``std`` (per channel, in the units of ``x``: for 0..255 data pass them times 255, as timm's ``PrefetchLoader`` does): the normalisation
    ``(mixed - mean) / std`` is applied in the same launch.

    Modes as in timm: ``batch`` (one draw per batch), ``elem`` (one per image), ``pair`` (one per pair, both halves alike; the middle image of an odd
    batch stays as it is).  ``mixup_enabled = False`` (engine.py:29-33, ``--mixup-off-epoch``) draws identity records.  An odd batch is accepted (timm
    asserts an even one): the middle image is paired with itself.

    ``random_erasing`` (a ``RandomErasing``): the same single launch (``lmv_augment_images`` in place of ``lmv_mix_images``) also erases, behind the
    normalisation -- timm's order: collate-time mixup, normalise, erase.  ``draw()`` then draws both tables; the ``out_dtype`` is this object's, and
    so is the normalisation (the ``RandomErasing``'s is used when only it carries ``mean`` / ``std``; both carrying them is refused).  Without it nothing changes: the same allocations, draws and launch.

    Capture: the kernels read the DEVICE table, so a captured step mixes with whatever the table holds at replay time --
    ``GraphedStep(step, before_replay=mix.draw)``.  ``draw()`` takes its shape from the last call; ``draw(B, H, W)`` may be called explicitly."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, cutmix_minmax: Optional[Sequence[float]] = None, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch", correct_lam: bool = True, label_smoothing: float = 0.1, num_classes: int = 1000,
                 mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None, out_dtype: Optional[torch.dtype] = None,
                 seed: Optional[int] = None, random_erasing: Optional[RandomErasing] = None):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = float(mixup_alpha), float(cutmix_alpha), cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError("Mixup: cutmix_minmax takes (min, max)")
            self.cutmix_alpha = 1.0          # timm: force cutmix alpha == 1.0 when minmax is active
        if mode not in ("batch", "elem", "pair"):
            raise ValueError(f"Mixup: unknown mode {mode!r} ('batch', 'elem' or 'pair')")
        if not (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0):
            raise ValueError("Mixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax must be set")
        if (mean is None) != (std is None):
            raise ValueError("Mixup: mean and std come together")
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam = float(prob), float(switch_prob), mode, bool(correct_lam)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.mixup_enabled = True
        self.out_dtype = out_dtype
        if random_erasing is not None and mean is not None and random_erasing._affine_host is not None:
            raise ValueError("Mixup: both this object and its random_erasing carry mean / std -- in the fused launch the normalisation belongs to the Mixup")
        self.random_erasing = random_erasing
        self._affine_host = None if mean is None else _affine_vectors(mean, std)
        self._affine: Optional[Tuple[Tensor, Tensor]] = None
        self.rng = np.random.default_rng(seed)
        self.table: Optional[Tensor] = None          # int32 [B, 6] on the device, sized at first use
        self.records: Optional[Tensor] = None        # the host copy of what the table holds (int32 [B, 6])
        self.last_use_cutmix: Optional[np.ndarray] = None
        self._shape: Optional[Tuple[int, int, int]] = None
        self._device: Optional[torch.device] = None

    # ---- the draws: timm's _params_per_batch / _params_per_elem, rand_bbox / rand_bbox_minmax, cutmix_bbox_and_lam -------------------------------
    def _params_per_elem(self, n: int):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = self.rng.random(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n), self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.0:
                lam_mix = self.rng.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            else:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            lam = np.where(self.rng.random(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and self.rng.random() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(self.rng.random() < self.switch_prob)
                lam = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam = self.rng.beta(self.mixup_alpha, self.mixup_alpha)
            else:
                use_cutmix = True
                lam = self.rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam)
        return lam, use_cutmix

    def _cutmix_box(self, H: int, W: int, lam: float):
        """``cutmix_bbox_and_lam``: the box and the (corrected) factor."""
        if self.cutmix_minmax is not None:          # rand_bbox_minmax
            lo, hi = self.cutmix_minmax
            cut_h = int(self.rng.integers(int(H * lo), int(H * hi)))
            cut_w = int(self.rng.integers(int(W * lo), int(W * hi)))
            yl = int(self.rng.integers(0, H - cut_h))
            xl = int(self.rng.integers(0, W - cut_w))
            box = (yl, yl + cut_h, xl, xl + cut_w)
        else:                                        # rand_bbox: a uniform integer centre
            cy, cx = int(self.rng.integers(0, H)), int(self.rng.integers(0, W))
            box = bbox(H, W, lam, cy, cx)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
        return box, lam

    def _record(self, H: int, W: int, lam: float, use_cutmix: bool):
        if lam == 1.0:
            return (1.0, 0, 0, 0, 0, 1.0)
        if use_cutmix:
            box, lam = self._cutmix_box(H, W, lam)
            return (1.0,) + box + (lam,)
        return (lam, 0, 0, 0, 0, lam)

    def _records(self, B: int, H: int, W: int) -> np.ndarray:
        """The host half of ``draw``: one record per image, nothing touches a device."""
        ident = (1.0, 0, 0, 0, 0, 1.0)
        if self.mode == "batch":
            lam, use_cutmix = self._params_per_batch()
            rows = [self._record(H, W, lam, use_cutmix)] * B
            self.last_use_cutmix = np.full(B, bool(use_cutmix and lam != 1.0))
        elif self.mode == "elem":
            lam, use_cutmix = self._params_per_elem(B)
            rows = [self._record(H, W, float(lam[i]), bool(use_cutmix[i])) for i in range(B)]
            self.last_use_cutmix = use_cutmix & (lam != 1.0)
        else:
            half = B // 2
            lam, use_cutmix = self._params_per_elem(half)
            first = [self._record(H, W, float(lam[i]), bool(use_cutmix[i])) for i in range(half)]
            rows = first + [ident] * (B - 2 * half) + first[::-1]
            uc = use_cutmix & (lam != 1.0)
            self.last_use_cutmix = np.concatenate([uc, np.zeros(B - 2 * half, dtype=bool), uc[::-1]])
        return make_records(rows)

    def draw(self, B: Optional[int] = None, H: Optional[int] = None, W: Optional[int] = None, device=None) -> np.ndarray:
        """Draw fresh records and upload them into the persistent device table (stream-ordered on the current stream, from a fresh host tensor, non-blocking:
        a replay still in flight keeps reading what it was given).  Without arguments the shape and device of the last call are used.  Returns the host records."""
        if B is None:
            if self._shape is None:
                raise RuntimeError("Mixup.draw: no shape yet -- call draw(B, H, W) or mix a batch first")
            B, H, W = self._shape
        elif H is None or W is None:
            raise ValueError("Mixup.draw: give B, H and W together")
        dev = torch.device(device) if device is not None else (self._device if self._device is not None else torch.device("cuda"))
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        rec = self._records(int(B), int(H), int(W))
        host = pack_records(rec)
        if self.table is None or self.table.shape[0] != B or self.table.device != dev:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("Mixup.draw: the table cannot be (re)allocated under graph capture")
            self.table = torch.empty((int(B), ops.MIX_RECORD_WORDS), dtype=torch.int32, device=dev)
        self.table.copy_(host, non_blocking=True)
        self.records, self._shape, self._device = host, (int(B), int(H), int(W)), dev
        if self.random_erasing is not None:
            self.random_erasing.draw(B, H, W, dev)
        return rec

    def __call__(self, x: Tensor, labels: Tensor) -> Tuple[Tensor, MixedTarget]:
        if x.dim() != 4:
            raise ValueError(f"Mixup: [B, C, H, W] images expected, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("lemevit_amd: tensors must be on the GPU (no CPU fallback exists)")
        B, C, H, W = x.shape
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.draw(B, H, W, x.device)
        elif self.table is None or self._shape != (B, H, W) or self.table.device != x.device:
            raise RuntimeError("Mixup: under graph capture the table must exist for this batch shape -- run one eager step (or draw(B, H, W)) first")
        re = self.random_erasing
        if re is not None and capturing:
            re._ready(x, True)
        scale = shift = None
        affine_host = self._affine_host if self._affine_host is not None or re is None else re._affine_host
        if affine_host is not None:
            self._affine = _affine_on(affine_host, self._affine, C, x.device, capturing, "Mixup")
            scale, shift = self._affine
        if re is None:
            mixed = ops.mix_images(x, self.table, self.out_dtype, scale, shift, records=None if capturing else self.records)
        else:
            mixed = ops.augment_images(x, self.table, re.table, re.key, re.mode, self.out_dtype, scale, shift, records=None if capturing else self.records,
                                       erase_records=None if capturing else re.records)
        return mixed, MixedTarget(labels, self.table, self.label_smoothing, self.num_classes)


class _SoftCEFn(torch.autograd.Function):
    """One lmv_soft_ce launch in forward (loss, per-row losses and the logit gradient); backward scales the kept gradient by the incoming one."""

    @staticmethod
    def forward(ctx, logits, labels, table, smoothing, target):
        want = ctx.needs_input_grad[0]
        loss, row, dlog = ops.soft_ce(logits.detach(), labels, table, smoothing, target, want_grad=want)
        if want:
            ctx.save_for_backward(dlog)
        ctx.set_materialize_grads(False)          # the unused one of (loss, row) arrives as None, not as a tensor of zeros
        ctx.B = logits.shape[0]
        return loss, row

    @staticmethod
    def backward(ctx, g_loss, g_row):
        (dlog,) = ctx.saved_tensors
        grad = dlog * g_loss.to(dlog.dtype) if g_loss is not None else None
        if g_row is not None:          # reduction="none": row b's loss has the gradient B * dlogits[b]
            part = dlog * (g_row * ctx.B).to(dlog.dtype).view(-1, 1)
            grad = part if grad is None else grad + part
        return grad, None, None, None, None


TargetLike = Union[MixedTarget, Tensor]


def _soft_ce(logits: Tensor, target: TargetLike, smoothing: float, reduction: str) -> Tensor:
    if not torch.is_tensor(logits) or logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"lemevit_amd: the native loss takes float32 or bfloat16 logits, got {getattr(logits, 'dtype', type(logits))}")
    if reduction not in ("mean", "none"):
        raise ValueError(f"lemevit_amd: reduction {reduction!r} is not supported ('mean' or 'none')")
    if isinstance(target, MixedTarget):
        args = (target.labels, target.table, target.smoothing, None)
    elif torch.is_tensor(target) and target.dtype == torch.int64 and target.dim() == 1:
        args = (target, None, smoothing, None)
    elif torch.is_tensor(target) and target.dim() == 2 and target.dtype in (torch.float32, torch.bfloat16):
        args = (None, None, 0.0, target)
    else:
        raise TypeError("lemevit_amd: the target must be a MixedTarget, int64 labels [B] or a float32 / bfloat16 matrix [B, classes]")
    loss, row = _SoftCEFn.apply(logits, *args)
    return loss if reduction == "mean" else row


class SoftTargetCrossEntropy(nn.Module):
    """``timm.loss.SoftTargetCrossEntropy`` on ``lmv_soft_ce``: ``mean_b sum_j -t_bj log_softmax(x)_bj``.  The target is a ``MixedTarget`` (what ``Mixup`` returns:
    nothing is materialised), a dense [B, classes] float32 / bfloat16 matrix, or int64 labels (plain cross-entropy).  float32 and bfloat16 logits; the strided
    ``[:, :N]`` view the classifier tail returns is read without a copy.  Labels are not validated (no host synchronisation): a label outside
    ``[0, classes)`` contributes no one-hot mass.  Logits that do not require grad take the loss-only form of the kernel."""

    def __init__(self, reduction: str = "mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, x: Tensor, target: TargetLike) -> Tensor:
        return _soft_ce(x, target, 0.0, self.reduction)


class LabelSmoothingCrossEntropy(nn.Module):
    """``timm.loss.LabelSmoothingCrossEntropy(smoothing)`` on ``lmv_soft_ce`` (= ``F.cross_entropy(..., label_smoothing=smoothing)``) for int64 labels; a
    ``MixedTarget`` brings its own smoothing, a dense matrix is taken as it is."""

    def __init__(self, smoothing: float = 0.1, reduction: str = "mean"):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError("LabelSmoothingCrossEntropy: smoothing must be in [0, 1)")
        self.smoothing, self.reduction = float(smoothing), reduction

    def forward(self, x: Tensor, target: TargetLike) -> Tensor:
        return _soft_ce(x, target, self.smoothing, self.reduction)
