"""Rotated RoIAlign for the Oriented R-CNN configs (csrc/rroi.hip): the reference's ``roi_align_rotated`` / ``RoIAlignRotated`` (mmdet/ops/roi_align_rotated, a CUDA
extension there) and the multi-level extractor around it as ONE autograd node -- one plan launch, one forward launch and one backward launch over all levels,
no ``nonzero``, no index copies, no host synchronisation, no floating-point atomics.

    from lemevit_amd.detection import RoIAlignRotated, roi_align_rotated          # the reference's names and signatures (single level)
    extractor = RotatedRoIExtractor(out_size=7, sample_num=2, featmap_strides=(4, 8, 16, 32), extend_factor=(1.4, 1.2))
    roi_feats = extractor(feats, rois)          # feats: the FPN levels [B, C, H_l, W_l]; rois float32 [R, 6] = (batch_index, cx, cy, w, h, theta in RADIANS)

Not supported: ``sample_num=0`` (the reference's adaptive grid: it raises), gradients for the RoIs, double backward, more than 5 levels.
``reference_rroi_align`` is the numpy float64 oracle (forward and adjoint); ``rroi_align_torch`` is the literal stock-PyTorch formulation, which the tests use
as their fp32 comparator and the probe as its other side.  include/lemevit_hip.h has the formulas.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from . import ops

Tensor = torch.Tensor
MAX_LEVELS = 5


def _check_sample_num(sample_num: int) -> int:
    s = int(sample_num)
    if s == 0:
        raise ValueError("roi_align_rotated: sample_num = 0 (the reference's adaptive sampling grid) is not supported; give 1 .. 4 (the Oriented R-CNN configs use 2)")
    if not 1 <= s <= 4:
        raise ValueError(f"roi_align_rotated: sample_num = {s} outside 1 .. 4")
    return s


class _RroiFn(torch.autograd.Function):
    """ONE node over all levels: forward = plan + forward launch, backward = one launch that writes every level's gradient once."""

    @staticmethod
    def forward(ctx, rois, levels, cfg, *feats):
        out_size, scales, sample_num, aligned, finest_scale, extend_factor = cfg
        feats = list(feats)
        plan = ops.rroi_plan(rois, [f.shape[-2:] for f in feats], scales, feats[0].shape[0], out_size, sample_num, aligned, levels, finest_scale, extend_factor)
        out = ops.rroi_align_fwd(feats, plan)
        ctx.plan = plan
        ctx.meta = [(tuple(f.shape), tuple(f.stride()), f.dtype, f.device) for f in feats]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if not any(ctx.needs_input_grad[3:]):
            return (None, None, None) + (None,) * len(ctx.meta)
        # dX in the feature's own layout; a layout in which two indices share an address (an expanded view) gets a contiguous gradient instead
        dx = [torch.empty_strided(shape, stride, dtype=dtype, device=device) if ops.strides_injective(shape, stride) else torch.empty(shape, dtype=dtype, device=device)
              for shape, stride, dtype, device in ctx.meta]
        ops.rroi_align_bwd(grad_out.contiguous(), ctx.plan, dx, dx=dx)
        return (None, None, None) + tuple(dx)


def _rroi_apply(feats: Sequence[Tensor], rois: Tensor, levels: Optional[Tensor], out_size, scales, sample_num, aligned, finest_scale, extend_factor) -> Tensor:
    if rois.dim() != 2 or rois.size(1) != 6:
        raise ValueError(f"roi_align_rotated: rois must be [R, 6] (batch_index, cx, cy, w, h, theta), got {tuple(rois.shape)}")
    if rois.requires_grad:
        raise RuntimeError("roi_align_rotated: there is no gradient for the RoIs (detach them)")
    oh, ow = _pair(out_size)
    cfg = ((int(oh), int(ow)), tuple(float(s) for s in scales), _check_sample_num(sample_num), bool(aligned), float(finest_scale), (float(extend_factor[0]), float(extend_factor[1])))
    return _RroiFn.apply(rois.detach().float().contiguous(), levels, cfg, *feats)


def roi_align_rotated(features: Tensor, rois: Tensor, out_size, spatial_scale: float, sample_num: int = 0, aligned: bool = True) -> Tensor:
    """The reference's ``roi_align_rotated(features, rois, out_size, spatial_scale, sample_num=0, aligned=True)`` (single level, under autograd).  ``rois`` [R, 6] rows
    ``(batch_index, cx, cy, w, h, theta)`` with theta in RADIANS.  ``sample_num`` keeps the reference's default of 0, which raises here (the adaptive grid is not
    supported): pass 1 .. 4."""
    return _rroi_apply([features], rois, None, out_size, (spatial_scale,), sample_num, aligned, 56.0, (1.0, 1.0))


class RoIAlignRotated(nn.Module):
    """Module form of ``roi_align_rotated`` under the reference's name: ``RoIAlignRotated(out_size, spatial_scale, sample_num=0, aligned=True)``; its ``repr`` prints
    the text the reference's module prints (the closing parenthesis is missing there too)."""

    def __init__(self, out_size, spatial_scale, sample_num=0, aligned=True):
        super().__init__()
        self.out_size, self.spatial_scale = _pair(out_size), float(spatial_scale)
        self.sample_num, self.aligned = int(sample_num), aligned

    def forward(self, features: Tensor, rois: Tensor) -> Tensor:
        return roi_align_rotated(features, rois, self.out_size, self.spatial_scale, self.sample_num, self.aligned)          # (_rroi_apply checks the [R, 6] shape)

    def __repr__(self) -> str:
        fields = [f"out_size={self.out_size}", f"spatial_scale={self.spatial_scale}", f"sample_num={self.sample_num}", f"aligned={self.aligned}"]
        return type(self).__name__ + "(" + "".join(f"\n    {f}," for f in fields)


class RotatedRoIExtractor(nn.Module):
    """The OBB single-level RoI extractor of the Oriented R-CNN configs (``roi_layer=dict(type='RoIAlignRotated', out_size=7, sample_num=2)``,
    ``featmap_strides=[4, 8, 16, 32]``, ``extend_factor=(1.4, 1.2)``) as ONE autograd node over all levels.  The level of a RoI is upstream mmdet's ``map_roi_levels``
    on the UN-extended box, ``clamp(floor(log2(sqrt(w h) / finest_scale + 1e-6)), 0, L - 1)``; after that ``w *= extend_factor[0]``, ``h *= extend_factor[1]``.  (The
    extractor's source is not part of the reference tree: this order restates upstream; ``levels=`` -- int32 [R] -- overrides the rule, so the other order is
    expressible.)  ``forward(feats, rois, levels=None)`` -> [R, out_channels, oh, ow]; it allocates its plan and output, synchronises nothing, and is capturable after one
    eager call per shape."""

    def __init__(self, out_size=7, sample_num=2, featmap_strides=(4, 8, 16, 32), out_channels=256, finest_scale=56, extend_factor=(1.4, 1.2), aligned=True):
        super().__init__()
        if not 1 <= len(featmap_strides) <= MAX_LEVELS:
            raise ValueError(f"RotatedRoIExtractor: {len(featmap_strides)} levels outside 1 .. {MAX_LEVELS}")
        self.out_size = _pair(out_size)
        self.sample_num = _check_sample_num(sample_num)
        self.featmap_strides = tuple(featmap_strides)
        self.out_channels = int(out_channels)
        self.finest_scale = float(finest_scale)
        self.extend_factor = (float(extend_factor[0]), float(extend_factor[1]))
        self.aligned = bool(aligned)

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def forward(self, feats: Sequence[Tensor], rois: Tensor, levels: Optional[Tensor] = None) -> Tensor:
        feats = list(feats)[:len(self.featmap_strides)]
        if len(feats) != len(self.featmap_strides):
            raise ValueError(f"RotatedRoIExtractor: {len(feats)} feature maps for {len(self.featmap_strides)} strides")
        if feats[0].shape[1] != self.out_channels:
            raise ValueError(f"RotatedRoIExtractor: {feats[0].shape[1]} channels, out_channels = {self.out_channels}")
        return _rroi_apply(feats, rois, levels, self.out_size, [1.0 / s for s in self.featmap_strides], self.sample_num, self.aligned, self.finest_scale, self.extend_factor)

    def extra_repr(self):
        return (f"out_size={self.out_size}, sample_num={self.sample_num}, featmap_strides={self.featmap_strides}, out_channels={self.out_channels}, "
                f"finest_scale={self.finest_scale}, extend_factor={self.extend_factor}, aligned={self.aligned}")


# -------------------------------------------------------------------------------------------
# The numpy float64 oracle
# -------------------------------------------------------------------------------------------
def map_roi_levels(rois, num_levels: int, finest_scale: float = 56.0):
    """Upstream mmdet's rule on [R, 6] rois (numpy, float64): ``clamp(floor(log2(sqrt(w h) / finest_scale + 1e-6)), 0, L - 1)``."""
    rois = np.asarray(rois, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.floor(np.log2(np.sqrt(rois[:, 3] * rois[:, 4]) / finest_scale + 1e-6))
    return np.clip(np.nan_to_num(lv, nan=0.0, neginf=0.0, posinf=float(num_levels - 1)), 0, num_levels - 1).astype(np.int64)


def reference_rroi_samples(roi, H: int, W: int, spatial_scale: float, out_size, sample_num: int, aligned: bool = True):
    """One RoI ``(batch_index, cx, cy, w, h, theta)`` (w, h already extended) on an H x W map, in float64: ``(y, x, empty, y_low, y_high, x_low, x_high, w[4])``,
    each of shape [oh, ow, s, s]; ``y`` / ``x`` are the map coordinates BEFORE the clamp (what the -1 / H / W rule looks at)."""
    oh, ow = out_size
    s = int(sample_num)
    _, cx, cy, w, h, theta = [float(v) for v in roi]
    off = 0.5 if aligned else 0.0
    cw, ch = cx * spatial_scale - off, cy * spatial_scale - off
    rw, rh = w * spatial_scale, h * spatial_scale
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bin_h, bin_w = rh / oh, rw / ow
    yy = (-rh / 2.0 + np.arange(oh)[:, None] * bin_h + (np.arange(s)[None, :] + 0.5) * bin_h / s)[:, None, :, None]          # [oh, 1, s, 1]
    xx = (-rw / 2.0 + np.arange(ow)[:, None] * bin_w + (np.arange(s)[None, :] + 0.5) * bin_w / s)[None, :, None, :]          # [1, ow, 1, s]
    ct, st = math.cos(theta), math.sin(theta)
    y = yy * ct - xx * st + ch
    x = yy * st + xx * ct + cw
    empty = (y < -1.0) | (y > H) | (x < -1.0) | (x > W)
    yc, xc = np.maximum(y, 0.0), np.maximum(x, 0.0)
    yl, xl = yc.astype(np.int64), xc.astype(np.int64)
    ty, tx = yl >= H - 1, xl >= W - 1
    yl, xl = np.where(ty, H - 1, yl), np.where(tx, W - 1, xl)
    yh, xh = np.where(ty, H - 1, yl + 1), np.where(tx, W - 1, xl + 1)
    yc, xc = np.where(ty, yl.astype(np.float64), yc), np.where(tx, xl.astype(np.float64), xc)
    ly, lx = yc - yl, xc - xl
    hy, hx = 1.0 - ly, 1.0 - lx
    wts = np.stack([hy * hx, hy * lx, ly * hx, ly * lx]) * (~empty)
    yl, yh, xl, xh = [np.where(empty, 0, v) for v in (yl, yh, xl, xh)]
    return y, x, empty, yl, yh, xl, xh, wts


def reference_rroi_align(feats, rois, out_size, spatial_scales, sample_num: int, aligned: bool = True, levels=None, finest_scale: float = 56.0,
                         extend_factor=(1.0, 1.0), grad_output=None):
    """The float64 oracle of ``RotatedRoIExtractor`` / ``roi_align_rotated``: ``feats``: a list of [B, C, H_l, W_l] arrays (or tensors), ``rois`` [R, 6].  Returns
    ``out`` [R, C, oh, ow]; with ``grad_output`` [R, C, oh, ow] it returns ``(out, [dX_l])``, the exact adjoint."""
    def arr(t):
        return (t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64))
    feats = [arr(f) for f in feats]
    rois = arr(rois).reshape(-1, 6)
    oh, ow = _pair(out_size)
    s = _check_sample_num(sample_num)
    L, (B, C_) = len(feats), feats[0].shape[:2]
    R = rois.shape[0]
    lv = map_roi_levels(rois, L, finest_scale) if levels is None else (levels.cpu().numpy() if isinstance(levels, torch.Tensor) else np.asarray(levels)).astype(np.int64)
    out = np.zeros((R, C_, oh, ow))
    g = None if grad_output is None else arr(grad_output)
    dxs = None if g is None else [np.zeros_like(f) for f in feats]
    for r in range(R):
        b, l = rois[r, 0], int(lv[r])
        if not (-1.0 < b < B) or not 0 <= l < L:          # (the batch index truncates towards zero, as a C++ int conversion does)
            continue
        b = int(b)
        H, W = feats[l].shape[2:]
        roi = rois[r].copy()
        roi[3] *= extend_factor[0]; roi[4] *= extend_factor[1]
        _, _, _, yl, yh, xl, xh, wts = reference_rroi_samples(roi, H, W, spatial_scales[l], (oh, ow), s, aligned)
        flat = np.stack([yl * W + xl, yl * W + xh, yh * W + xl, yh * W + xh]).reshape(4, oh * ow, s * s)
        uniq, inv = np.unique(flat, return_inverse=True)
        M = np.zeros((oh * ow, uniq.size))          # the RoI's pooling matrix over the pixels it touches
        np.add.at(M, (np.broadcast_to(np.arange(oh * ow)[None, :, None], flat.shape).reshape(-1), inv.reshape(-1)), wts.reshape(-1))
        M /= float(s * s)
        out[r] = (feats[l][b].reshape(C_, H * W)[:, uniq] @ M.T).reshape(C_, oh, ow)
        if g is not None:
            dxs[l][b].reshape(C_, H * W)[:, uniq] += g[r].reshape(C_, oh * ow) @ M
    return out if g is None else (out, dxs)


# -------------------------------------------------------------------------------------------
# The stock-PyTorch formulation
# -------------------------------------------------------------------------------------------
def _rroi_torch_level(feat: Tensor, rois: Tensor, out_size, scale: float, s: int, aligned: bool) -> Tensor:
    B, C_, H, W = feat.shape
    oh, ow = out_size
    dt, dev, vt = rois.dtype, feat.device, feat.dtype          # the geometry in the RoIs' dtype (float32), the values in the features'
    bi = rois[:, 0].long()
    ok = (bi >= 0) & (bi < B)
    off = 0.5 if aligned else 0.0
    cw, ch = rois[:, 1] * scale - off, rois[:, 2] * scale - off
    rw, rh = rois[:, 3] * scale, rois[:, 4] * scale
    if not aligned:
        rw, rh = rw.clamp(min=1.0), rh.clamp(min=1.0)
    bin_h, bin_w = rh / oh, rw / ow
    iy = (torch.arange(s, device=dev, dtype=dt) + 0.5)
    yy = -rh[:, None, None] / 2 + torch.arange(oh, device=dev, dtype=dt)[None, :, None] * bin_h[:, None, None] + iy[None, None, :] * bin_h[:, None, None] / s          # [R, oh, s]
    xx = -rw[:, None, None] / 2 + torch.arange(ow, device=dev, dtype=dt)[None, :, None] * bin_w[:, None, None] + iy[None, None, :] * bin_w[:, None, None] / s          # [R, ow, s]
    ct, st = torch.cos(rois[:, 5])[:, None, None, None, None], torch.sin(rois[:, 5])[:, None, None, None, None]
    yy, xx = yy[:, :, None, :, None], xx[:, None, :, None, :]
    y = yy * ct - xx * st + ch[:, None, None, None, None]
    x = yy * st + xx * ct + cw[:, None, None, None, None]
    keep = ~((y < -1) | (y > H) | (x < -1) | (x > W)) & ok[:, None, None, None, None]
    y, x = y.clamp(min=0), x.clamp(min=0)
    yl, xl = y.long(), x.long()
    ty, tx = yl >= H - 1, xl >= W - 1
    yl, xl = torch.where(ty, H - 1, yl), torch.where(tx, W - 1, xl)
    yh, xh = torch.where(ty, H - 1, yl + 1), torch.where(tx, W - 1, xl + 1)
    y, x = torch.where(ty, yl.to(dt), y), torch.where(tx, xl.to(dt), x)
    ly, lx = y - yl.to(dt), x - xl.to(dt)
    hy, hx = 1 - ly, 1 - lx
    k = keep.to(dt)
    w1, w2, w3, w4 = [(wt * k).to(vt).unsqueeze(-1) for wt in (hy * hx, hy * lx, ly * hx, ly * lx)]
    bb = bi.clamp(0, B - 1)[:, None, None, None, None].expand_as(yl)
    fl = feat.permute(0, 2, 3, 1)          # [B, H, W, C]: one gather gives [R, oh, ow, s, s, C]
    val = w1 * fl[bb, yl, xl] + w2 * fl[bb, yl, xh] + w3 * fl[bb, yh, xl] + w4 * fl[bb, yh, xh]
    return val.mean(dim=(3, 4)).permute(0, 3, 1, 2).contiguous()


def rroi_align_torch(feats: Sequence[Tensor], rois: Tensor, out_size, spatial_scales: Sequence[float], sample_num: int, aligned: bool = True,
                     levels: Optional[Tensor] = None, finest_scale: float = 56.0, extend_factor=(1.0, 1.0)) -> Tensor:
    """What a user would write today: the level rule and the coordinates with torch ops (``torch.cos`` / ``torch.sin``) in float32, the four corners by advanced
    indexing, weights and a mean in the features' dtype; with more than one level, the stock extractor's loop (``nonzero``, one call per level, index copy).  Autograd supplies the
    backward pass through ``index_put``.  Works on any device."""
    feats = list(feats)
    oh, ow = _pair(out_size)
    s = _check_sample_num(sample_num)
    L = len(feats)
    rois = rois.float()
    ext = rois.clone()
    ext[:, 3] = rois[:, 3] * extend_factor[0]
    ext[:, 4] = rois[:, 4] * extend_factor[1]
    if L == 1 and levels is None:
        return _rroi_torch_level(feats[0], ext, (oh, ow), spatial_scales[0], s, aligned)
    if levels is None:
        levels = torch.floor(torch.log2(torch.sqrt(rois[:, 3] * rois[:, 4]) / finest_scale + 1e-6)).clamp(min=0, max=L - 1).long()
    out = feats[0].new_zeros((rois.shape[0], feats[0].shape[1], oh, ow))
    for l in range(L):
        inds = (levels == l).nonzero(as_tuple=False).squeeze(1)
        if inds.numel() > 0:
            out[inds] = _rroi_torch_level(feats[l], ext[inds], (oh, ow), spatial_scales[l], s, aligned)
        else:
            out = out + sum(x.view(-1)[0] for x in feats[l:l + 1]) * 0.0          # (upstream keeps every level in the graph)
    return out
