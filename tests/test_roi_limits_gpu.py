"""Both RoIAlign operators (csrc/roi.hip, csrc/rroi.hip) at the limits their header promises: 256 bins (257 table entries), a sampling grid of 128, maps of 8192 /
65535 pixels per axis, 1024 samples per RoI, 64 / 65 / 130 RoIs on one backward tile, one-pixel second tiles, strided views, and the data rules on the device.  The
method is that of tests/test_roi_gpu.py and tests/test_rroi_gpu.py: float64 oracle, the bound max(4 E_torch, 1e-6 max(1, |ref|)) (+ 2^-8 |ref| in bf16) with E_torch
the fp32 error of the stock-PyTorch formulation on the same inputs on the same GPU, NaN-prefilled buffers, bit-identical repeats.  The inputs come from
tests/golden/gen_roi_limits.py; tests/test_roi_limits_cpu.py asserts their conditions on the oracle."""
import functools

import numpy as np
import pytest
import torch

from gen_roi_limits import (DYADIC_ROWS, NEGATIVE_ROWS, NONFINITE_FIRST, ROI_LIMITS, RROI_LIMITS, RULES_BAD, RULES_HALF, RULES_TWIN, roi_limit_case, roi_limit_valid_rows,
                            rroi_limit_case, rroi_limit_samples)
from lemevit_amd import ops
from lemevit_amd.detection import reference_roi_align, reference_rroi_align, roi_align_torch, rroi_align_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _check(got, ref, e_torch, bf16, what):
    """(tests/test_roi_gpu.py's, unchanged; returns the largest error / bound)"""
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    bound = np.maximum(4.0 * e_torch, 1e-6 * np.maximum(1.0, np.abs(ref)))
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)          # the final rounding to bf16 (8 significant bits: half an ulp is up to 2^-8 |ref|)
    worst = float(err.max()) if err.size else 0.0
    ratio = float((err / bound).max()) if err.size else 0.0
    print(f"    {what}: E_torch {e_torch:.3e}, kernel max error {worst:.3e}, largest error / bound {ratio:.3f}")
    assert not np.isnan(got).any(), f"{what}: NaN left in a pre-filled buffer (an element was not written)"
    assert (err <= bound).all(), f"{what}: max error {worst:.3e} against E_torch {e_torch:.3e}"
    return ratio


def _torch_errors(t, f32, dy, out_ref, dx_ref):
    t.backward(dy.float().to(DEV))
    e_fwd = float(np.abs(t.detach().double().cpu().numpy() - out_ref).max()) if out_ref.size else 0.0
    e_bwd = max(float(np.abs((f.grad if f.grad is not None else torch.zeros_like(f)).double().cpu().numpy() - d).max()) for f, d in zip(f32, dx_ref))
    return e_fwd, e_bwd


# ---- horizontal ------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _roi(name, bf16):
    """(case, feats, rois, levels, dy, out_ref, dx_ref, E_fwd, E_bwd): float64 CPU inputs (rounded to bf16 first when ``bf16``), the oracle's results, the largest errors
    of ``roi_align_torch`` in fp32 on the GPU.  Computed once, shared, never modified."""
    case, feats, rois, levels, dy = roi_limit_case(name)
    if bf16:
        feats, dy = [f.bfloat16().double() for f in feats], dy.bfloat16().double()
    out_ref, dx_ref = reference_roi_align(feats, rois, case["out_size"], case["scales"], case["s"], levels, 56.0, grad_output=dy)
    f32 = [f.float().to(DEV).requires_grad_(True) for f in feats]
    t = roi_align_torch(f32, rois.to(DEV), case["out_size"], case["scales"], case["s"], levels.to(DEV).long(), 56.0)
    return (case, feats, rois, levels, dy, out_ref, dx_ref) + _torch_errors(t, f32, dy, out_ref, dx_ref)


def _inputs(ref, layout, dtype):
    case, feats, rois, levels, dy = ref[:5]
    fmt = torch.channels_last if layout == "cl" else torch.contiguous_format
    x = [f.to(dtype).to(DEV).contiguous(memory_format=fmt) for f in feats]
    return case, x, rois.to(DEV), (None if levels is None else levels.to(DEV)), dy.to(dtype).to(DEV)


def _run_roi(case, x, rois, levels, dy):
    """ops-level plan + forward + backward into NaN-prefilled buffers"""
    plan = ops.roi_plan(rois, case["sizes"], case["scales"], case["B"], case["out_size"], case["s"], levels, 56.0)
    out = torch.full((rois.shape[0], case["C"]) + tuple(case["out_size"]), float("nan"), device=DEV, dtype=x[0].dtype)
    dx = [torch.full_like(f, float("nan")) for f in x]          # (full_like keeps the layout)
    assert all(d.stride() == f.stride() for d, f in zip(dx, x))
    ops.roi_align_fwd(x, plan, out=out)
    ops.roi_align_bwd(dy, plan, x, dx=dx)
    return out, dx


ROI_PARAMS = [(n, "nchw", torch.float32) for n in ROI_LIMITS] + [(n, "cl", torch.bfloat16) for n in ROI_LIMITS if ROI_LIMITS[n]["star"]]


@pytest.mark.parametrize("name,layout,dtype", ROI_PARAMS, ids=[f"{n}-{l}-{str(d).split('.')[-1]}" for n, l, d in ROI_PARAMS])
def test_roi_against_oracle(name, layout, dtype):
    """forward and dX within max(4 E_torch, 1e-6 max(1, |ref|)) (+ 2^-8 |ref| in bf16) of the float64 oracle; nothing left unwritten; two calls agree bit for bit; the
    rows of invalid RoIs (over the grid limit on one axis; NaN, inf, 1e30, reversed, bad batch index, NaN batch index, bad level) are exactly zero and dropping those
    RoIs changes no bit of dX; batch index -0.5 is image 0"""
    bf16 = dtype == torch.bfloat16
    ref = _roi(name, bf16)
    out_ref, dx_ref, e_fwd, e_bwd = ref[5:]
    case, x, rois, levels, dy = _inputs(ref, layout, dtype)
    out, dx = _run_roi(case, x, rois, levels, dy)
    print(f"\n  roi {name} {layout} {dtype}:")
    _check(out, out_ref, e_fwd, bf16, "forward")
    for l, (d, r) in enumerate(zip(dx, dx_ref)):
        _check(d, r, e_bwd, bf16, f"dX level {l}")
    out2, dx2 = _run_roi(case, x, rois, levels, dy)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(dx, dx2))
    rows = roi_limit_valid_rows(case, rois.cpu(), levels.cpu())
    keep = torch.zeros(case["R"], dtype=torch.bool, device=DEV)
    keep[torch.from_numpy(rows).to(DEV)] = True
    expect = {"rules": len(RULES_BAD), "g_over": 1}.get(name, 0)
    assert int((~keep).sum()) == expect
    if expect:
        assert not out[~keep].any() and bool(out[keep].flatten(1).any(1).all())
        _, dx3 = _run_roi(case, x, rois[keep].contiguous(), levels[keep].contiguous(), dy[keep].contiguous())
        assert all(torch.equal(a, c) for a, c in zip(dx, dx3))
    if name == "rules":
        assert torch.equal(out[RULES_HALF], out[RULES_TWIN]) and bool(keep[RULES_HALF]) and not keep[list(RULES_BAD)].any()


@pytest.mark.parametrize("name", ["b1x256_a", "e9x8192_b"])
def test_roi_strided_views(name):
    """the forward reads ``big[:, 3:3 + C, :, :W]`` of a larger tensor (a storage offset, sh != W, sb != C H W) and the backward writes dX into such a view of a tensor
    pre-filled with a finite sentinel: ops.roi_align_fwd / ops.roi_align_bwd take the views as they are, the results equal the contiguous run bit for bit, and every
    element of ``big`` outside the view still holds the sentinel"""
    ref = _roi(name, False)
    case, x, rois, levels, dy = _inputs(ref, "nchw", torch.float32)
    out, dx = _run_roi(case, x, rois, levels, dy)
    B, C, (H, W) = case["B"], case["C"], case["sizes"][0]
    big = torch.full((B, C + 6, H + 2, W + 5), 7.25, device=DEV)
    view = big[:, 3:3 + C, :H, :W]
    view.copy_(x[0])
    assert view.storage_offset() > 0 and view.stride(2) == W + 5 and view.stride(0) != C * H * W and view.data_ptr() != big.data_ptr()
    plan = ops.roi_plan(rois, case["sizes"], case["scales"], B, case["out_size"], case["s"], levels, 56.0)
    got = ops.roi_align_fwd([view], plan, out=torch.full_like(out, float("nan")))
    assert torch.equal(got, out)
    gbig = torch.full_like(big, -3.5)
    gview = gbig[:, 3:3 + C, :H, :W]
    res = ops.roi_align_bwd(dy, plan, [view], dx=[gview])
    assert res[0].data_ptr() == gview.data_ptr() and torch.equal(gview, dx[0])
    outside = torch.ones_like(gbig, dtype=torch.bool)
    outside[:, 3:3 + C, :H, :W] = False
    assert bool((gbig[outside] == -3.5).all()) and bool((big[outside] == 7.25).all())


# ---- rotated ---------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rroi(name, bf16, rows=None):
    """as ``_roi``; ``rows``: only the first ``rows`` RoIs of the case"""
    case, feats, rois, levels, dy = rroi_limit_case(name)
    if rows is not None:
        case, rois, dy, levels = dict(case, R=rows), rois[:rows].contiguous(), dy[:rows].contiguous(), (None if levels is None else levels[:rows].contiguous())
    if bf16:
        feats, dy = [f.bfloat16().double() for f in feats], dy.bfloat16().double()
    out_ref, dx_ref = reference_rroi_align(feats, rois, case["out_size"], case["scales"], case["s"], case["aligned"], levels, 56.0, case["ext"], grad_output=dy)
    f32 = [f.float().to(DEV).requires_grad_(True) for f in feats]
    t = rroi_align_torch(f32, rois.to(DEV), case["out_size"], case["scales"], case["s"], case["aligned"], None if levels is None else levels.to(DEV).long(), 56.0, case["ext"])
    return (case, feats, rois, levels, dy, out_ref, dx_ref) + _torch_errors(t, f32, dy, out_ref, dx_ref)


def _run_rroi(case, x, rois, levels, dy):
    """ops-level plan + forward + backward into NaN-prefilled buffers"""
    plan = ops.rroi_plan(rois, case["sizes"], case["scales"], case["B"], case["out_size"], case["s"], case["aligned"], levels, 56.0, case["ext"])
    out = torch.full((rois.shape[0], case["C"]) + tuple(case["out_size"]), float("nan"), device=DEV, dtype=x[0].dtype)
    dx = [torch.full_like(f, float("nan")) for f in x]          # (full_like keeps the layout)
    assert all(d.stride() == f.stride() for d, f in zip(dx, x))
    ops.rroi_align_fwd(x, plan, out=out)
    ops.rroi_align_bwd(dy, plan, x, dx=dx)
    return out, dx


RROI_PARAMS = ([(n, "nchw", torch.float32) for n in RROI_LIMITS if n != "negative"] + [(n, "cl", torch.bfloat16) for n in RROI_LIMITS if RROI_LIMITS[n]["star"]])


@pytest.mark.parametrize("name,layout,dtype", RROI_PARAMS, ids=[f"{n}-{l}-{str(d).split('.')[-1]}" for n, l, d in RROI_PARAMS])
def test_rroi_against_oracle(name, layout, dtype):
    """forward and dX within max(4 E_torch, 1e-6 max(1, |ref|)) (+ 2^-8 |ref| in bf16) of the float64 oracle; nothing left unwritten; two calls agree bit for bit; RoIs
    with NaN, +inf or -inf in cx, cy, w, h or theta give zero rows, leave no NaN anywhere, and dropping them changes no bit of dX"""
    bf16 = dtype == torch.bfloat16
    ref = _rroi(name, bf16)
    out_ref, dx_ref, e_fwd, e_bwd = ref[5:]
    case, x, rois, levels, dy = _inputs(ref, layout, dtype)
    out, dx = _run_rroi(case, x, rois, levels, dy)
    print(f"\n  rroi {name} {layout} {dtype}:")
    _check(out, out_ref, e_fwd, bf16, "forward")
    for l, (d, r) in enumerate(zip(dx, dx_ref)):
        _check(d, r, e_bwd, bf16, f"dX level {l}")
    out2, dx2 = _run_rroi(case, x, rois, levels, dy)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(dx, dx2))
    valid = [s[0] for s in rroi_limit_samples(case, rois.cpu(), None if levels is None else levels.cpu())]
    if name == "nonfinite":
        assert valid == list(range(NONFINITE_FIRST)) and case["R"] == NONFINITE_FIRST + 15
        assert not out[NONFINITE_FIRST:].any() and bool(out[:NONFINITE_FIRST].flatten(1).any(1).all())
        assert not torch.isnan(out).any() and not any(torch.isnan(d).any() for d in dx)
        n = NONFINITE_FIRST
        _, dx3 = _run_rroi(case, x, rois[:n].contiguous(), None, dy[:n].contiguous())
        assert all(torch.equal(a, c) for a, c in zip(dx, dx3))
    else:
        assert len(valid) == case["R"]


@pytest.mark.parametrize("name", [n for n in RROI_LIMITS if RROI_LIMITS[n]["kind"] == "far"])
def test_rroi_dyadic_rows_alone(name):
    """the dyadic RoIs of the far-end cases alone (theta = 0, every sample coordinate and weight exact in fp32, indices up to 65534): E_torch holds no coordinate
    rounding, so the bound is at its floor or close to it and a wrong index cannot hide behind it.  Printed: whether the 1e-6 floor alone would have sufficed."""
    ref = _rroi(name, False, DYADIC_ROWS)
    out_ref, dx_ref, e_fwd, e_bwd = ref[5:]
    case, x, rois, levels, dy = _inputs(ref, "nchw", torch.float32)
    out, dx = _run_rroi(case, x, rois, levels, dy)
    print(f"\n  rroi {name} dyadic rows:")
    _check(out, out_ref, e_fwd, False, "forward")
    _check(dx[0], dx_ref[0], e_bwd, False, "dX")
    for what, got, want in (("forward", out, out_ref), ("dX", dx[0], dx_ref[0])):
        q = float((np.abs(got.double().cpu().numpy() - want) / (1e-6 * np.maximum(1.0, np.abs(want)))).max())
        print(f"    {what}: largest error / (1e-6 max(1, |ref|)) {q:.3f}: the floor alone {'suffices' if q <= 1.0 else 'does NOT suffice'}")
    assert bool(out.flatten(1).any(1).all())


def test_rroi_negative_sizes():
    """finite negative w / h are not validated: nothing is left unwritten (NaN-prefilled buffers) and the repeat is bit-identical"""
    case, feats, rois, levels, dy = rroi_limit_case("negative")
    assert rois[NEGATIVE_ROWS[0], 3] < 0 and rois[NEGATIVE_ROWS[1], 4] < 0
    x = [f.float().to(DEV) for f in feats]
    out, dx = _run_rroi(case, x, rois.to(DEV), None, dy.float().to(DEV))
    out2, dx2 = _run_rroi(case, x, rois.to(DEV), None, dy.float().to(DEV))
    assert not torch.isnan(out).any() and not any(torch.isnan(d).any() for d in dx)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(dx, dx2))
