"""Horizontal RoIAlign with the adaptive grid on the GPU (csrc/roi.hip) against the float64 oracle, with the bound taken from the error of the stock-PyTorch
formulation in fp32 on the same inputs, and the exact properties: written once (NaN-prefilled buffers), bit-identical repeats, multi-level = per-level, invalid
RoIs, autograd, capture.  The inputs of every case come from tests/golden/gen_roi_golden.py; tests/test_roi_cpu.py checks their conditions on the oracle."""
import functools

import numpy as np
import pytest
import torch

from gen_roi_golden import NEGATIVE, OVER_LIMIT, roi_case, roi_valid_rows
from lemevit_amd import ops
from lemevit_amd.detection import RoIAlign, RoIExtractor, map_roi_levels_xyxy, reference_roi_align, roi_align, roi_align_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(name, bf16):
    """(case, feats, rois, levels, dy, out_ref, dx_ref, E_fwd, E_bwd): inputs as float64 CPU tensors (rounded to bf16 first when ``bf16``), the oracle's results, and
    the largest errors of ``roi_align_torch`` evaluated in fp32 on the GPU on those inputs.  Computed once, shared, never modified."""
    case, feats, rois, levels, dy = roi_case(name)
    if bf16:
        feats, dy = [f.bfloat16().double() for f in feats], dy.bfloat16().double()
    out_ref, dx_ref = reference_roi_align(feats, rois, case["out_size"], case["scales"], case["s"], levels, 56.0, grad_output=dy)
    f32 = [f.float().to(DEV).requires_grad_(True) for f in feats]
    t = roi_align_torch(f32, rois.to(DEV), case["out_size"], case["scales"], case["s"], None if levels is None else levels.to(DEV).long(), 56.0)
    t.backward(dy.float().to(DEV))
    e_fwd = float(np.abs(t.detach().double().cpu().numpy() - out_ref).max()) if out_ref.size else 0.0
    e_bwd = max(float(np.abs((f.grad if f.grad is not None else torch.zeros_like(f)).double().cpu().numpy() - d).max()) for f, d in zip(f32, dx_ref))
    return case, feats, rois, levels, dy, out_ref, dx_ref, e_fwd, e_bwd


def _inputs(name, layout, dtype):
    case, feats, rois, levels, dy = _case(name, dtype == torch.bfloat16)[:5]
    fmt = torch.channels_last if layout == "cl" else torch.contiguous_format
    x = [f.to(dtype).to(DEV).contiguous(memory_format=fmt) for f in feats]
    return case, x, rois.to(DEV), (None if levels is None else levels.to(DEV)), dy.to(dtype).to(DEV)


def _run(case, x, rois, levels, dy):
    """ops-level plan + forward + backward into NaN-prefilled buffers"""
    plan = ops.roi_plan(rois, case["sizes"], case["scales"], case["B"], case["out_size"], case["s"], levels, 56.0)
    out = torch.full((case["R"], case["C"]) + tuple(case["out_size"]), float("nan"), device=DEV, dtype=x[0].dtype)
    dx = [torch.full_like(f, float("nan")) for f in x]          # (full_like keeps the layout)
    assert all(d.stride() == f.stride() for d, f in zip(dx, x))
    ops.roi_align_fwd(x, plan, out=out)
    ops.roi_align_bwd(dy, plan, x, dx=dx)
    return out, dx


def _check(got, ref, e_torch, bf16, what):
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    bound = np.maximum(4.0 * e_torch, 1e-6 * np.maximum(1.0, np.abs(ref)))
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)          # the final rounding to bf16 (8 significant bits: half an ulp is up to 2^-8 |ref|)
    worst = float(err.max()) if err.size else 0.0
    print(f"    {what}: E_torch {e_torch:.3e}, kernel max error {worst:.3e}, largest error / bound {float((err / bound).max()) if err.size else 0.0:.3f}")
    assert not np.isnan(got).any(), f"{what}: NaN left in a pre-filled buffer (an element was not written)"
    assert (err <= bound).all(), f"{what}: max error {worst:.3e} against E_torch {e_torch:.3e}"


CASES_NCHW_F32 = ["a1_c5", "a1_c70_m14", "f1_s2", "f1_s3_35", "a4_c256", "a4_r300", "a2_explicit", "a1_big", "a1_r1", "a1_r0"]
PARAMS = ([(n, "nchw", torch.float32) for n in CASES_NCHW_F32] +
          [("a4_c256", "cl", torch.float32), ("a4_c256", "nchw", torch.bfloat16), ("a4_c256", "cl", torch.bfloat16), ("a1_c70_m14", "cl", torch.float32),
           ("a1_c70_m14", "nchw", torch.bfloat16), ("f1_s3_35", "cl", torch.bfloat16), ("a4_r300", "cl", torch.bfloat16), ("a2_explicit", "cl", torch.float32),
           ("a1_big", "cl", torch.bfloat16), ("a1_r0", "cl", torch.bfloat16)])


@pytest.mark.parametrize("name,layout,dtype", PARAMS, ids=[f"{n}-{l}-{str(d).split('.')[-1]}" for n, l, d in PARAMS])
def test_against_oracle(name, layout, dtype):
    """forward and dX within max(4 E_torch, 1e-6 max(1, |ref|)) (+ 2^-8 |ref| in bf16) of the float64 oracle; nothing left unwritten; two calls agree bit for bit;
    rows of invalid RoIs (a bad batch index, a grid over the limit, a negative width) are exactly zero, and dropping those RoIs changes no bit of dX"""
    bf16 = dtype == torch.bfloat16
    out_ref, dx_ref, e_fwd, e_bwd = _case(name, bf16)[5:]
    case, x, rois, levels, dy = _inputs(name, layout, dtype)
    out, dx = _run(case, x, rois, levels, dy)
    print(f"\n  {name} {layout} {dtype}:")
    _check(out, out_ref, e_fwd, bf16, "forward")
    for l, (d, r) in enumerate(zip(dx, dx_ref)):
        _check(d, r, e_bwd, bf16, f"dX level {l}")
    out2, dx2 = _run(case, x, rois, levels, dy)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(dx, dx2))
    rows = roi_valid_rows(case, rois.cpu(), None if levels is None else levels.cpu())
    bad = torch.ones(case["R"], dtype=torch.bool, device=DEV)
    bad[torch.from_numpy(rows).to(DEV)] = False
    if case["bad"] or case["special"]:
        assert int(bad.sum()) >= 2 and not out[bad].any()
        if case["special"]:
            assert bool(bad[OVER_LIMIT]) and bool(bad[NEGATIVE])
        keep = ~bad
        sub = dict(case, R=int(keep.sum()))
        _, dx3 = _run(sub, x, rois[keep].contiguous(), None if levels is None else levels[keep].contiguous(), dy[keep].contiguous())
        assert all(torch.equal(a, c) for a, c in zip(dx, dx3))
    else:
        assert not bad.any()
    if name == "a4_c256":
        assert not dx[2].any()          # the level without RoIs: all zeros, all written


@pytest.mark.parametrize("name,layout,dtype", [("a4_c256", "nchw", torch.float32), ("a4_r300", "cl", torch.float32), ("a2_explicit", "nchw", torch.bfloat16)],
                         ids=["a4_c256-nchw-float32", "a4_r300-cl-float32", "a2_explicit-nchw-bfloat16"])
def test_multilevel_equals_per_level(name, layout, dtype):
    """forward: the rows of a level's RoIs; backward: dX_l from that level's RoIs in the same order -- bit for bit"""
    case, x, rois, levels, dy = _inputs(name, layout, dtype)
    out, dx = _run(case, x, rois, levels, dy)
    lv = torch.from_numpy(map_roi_levels_xyxy(rois.cpu().numpy(), len(x))).to(DEV) if levels is None else levels.long()
    for l in range(len(x)):
        sel = lv == l
        one = dict(case, R=int(sel.sum()), sizes=[case["sizes"][l]], scales=[case["scales"][l]])
        out_l, dx_l = _run(one, [x[l]], rois[sel].contiguous(), None, dy[sel].contiguous())
        assert torch.equal(out[sel], out_l), f"forward rows of level {l}"
        assert torch.equal(dx[l], dx_l[0]), f"dX of level {l}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_autograd_modules_equal_ops(dtype):
    """RoIExtractor (one node over all levels) and the reference-named single-level entry points under torch.autograd -- with bf16 features under torch.autocast --
    give the ops-level results bit for bit"""
    case, x, rois, levels, dy = _inputs("a4_c256", "nchw", dtype)
    out, dx = _run(case, x, rois, levels, dy)
    ext = RoIExtractor(out_size=case["out_size"], sample_num=case["s"], featmap_strides=case["strides"], out_channels=case["C"])
    xs = [f.clone().requires_grad_(True) for f in x]
    with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
        got = ext(xs, rois)
    assert got.dtype == dtype and got.grad_fn is not None
    got.backward(dy)
    assert torch.equal(got, out) and all(torch.equal(f.grad, d) for f, d in zip(xs, dx))
    # single level, the mask head's 14 x 14: the module, the function, and the ops-level call
    case, x, rois, levels, dy = _inputs("a1_c70_m14", "cl", dtype)
    out, dx = _run(case, x, rois, levels, dy)
    m = RoIAlign(case["out_size"], case["scales"][0])          # the reference's defaults: sample_num = 0, aligned = True
    f = x[0].clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
        got = m(f, rois)
        again = roi_align(x[0], rois, case["out_size"], case["scales"][0])
    got.backward(dy)
    assert torch.equal(got, out) and torch.equal(again, out) and torch.equal(f.grad, dx[0]) and f.grad.stride() == f.stride()
    # an expanded feature map gets a contiguous gradient equal to that of a contiguous copy; the ops-level call refuses such a gradient buffer
    if dtype == torch.float32:
        case, x, rois, levels, dy = _inputs("f1_s3_35", "nchw", dtype)
        m = RoIAlign(case["out_size"], case["scales"][0], case["s"])
        ex = x[0][:1].clone().expand(case["B"], -1, -1, -1).requires_grad_(True)
        assert case["B"] == 3 and ex.stride(0) == 0
        dense = ex.detach().contiguous().requires_grad_(True)
        g_ex, = torch.autograd.grad(m(ex, rois), ex, dy)
        g_dense, = torch.autograd.grad(m(dense, rois), dense, dy)
        assert g_ex.is_contiguous() and torch.equal(g_ex, g_dense)
        plan = ops.roi_plan(rois, case["sizes"], case["scales"], case["B"], case["out_size"], case["s"])
        with pytest.raises(ValueError, match="aliases itself"):
            ops.roi_align_bwd(dy, plan, [dense], dx=[torch.zeros_like(x[0][:1]).expand(case["B"], -1, -1, -1)])


def test_captured_replay_equals_eager():
    """forward + backward of RoIExtractor captured after one eager call: the replay equals the eager call bit for bit.  The leaves are made, run eagerly and captured
    on ONE side stream, so that their gradient accumulators belong to the capturing stream."""
    case, x, rois, levels, dy = _inputs("a4_c256", "cl", torch.bfloat16)
    ext = RoIExtractor(out_size=case["out_size"], sample_num=case["s"], featmap_strides=case["strides"], out_channels=case["C"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs = [f.clone().requires_grad_(True) for f in x]
        eager = ext(xs, rois)          # the eager call
        eager.backward(dy)
        eager, eager_dx = eager.detach().clone(), [f.grad.clone() for f in xs]
        for f in xs:
            f.grad = None
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = ext(xs, rois)
        got.backward(dy)
    with torch.cuda.stream(side):
        got.detach().fill_(float("nan"))
        for f in xs:
            f.grad.fill_(float("nan"))
        graph.replay()
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.isnan(got).any() and torch.equal(got, eager) and all(torch.equal(f.grad, d) for f, d in zip(xs, eager_dx))
