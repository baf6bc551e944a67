"""Horizontal RoIAlign (adaptive grid) without a GPU: the float64 oracle against the reference's CPU extension (tests/golden/roi_align.npz), the adjoint identity, the
level rule and the data rules on hand-made boxes, the library's refusals, and the INPUT CONDITIONS of every case -- those of tests/test_roi_gpu.py included: no
sample coordinate near -1 / H / W, no bin size near an integer (where the fp32 grid could differ from the oracle's) and no box near a level threshold."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gen_roi_golden import NEGATIVE, OVER_LIMIT, ROI_CASES, ROI_GOLDEN, roi_case, roi_input_conditions, roi_valid_rows
from lemevit_amd.detection import (ROI_MAX_GRID, RoIAlign, RoIExtractor, map_roi_levels_xyxy, reference_roi_align, reference_roi_geometry, reference_roi_samples,
                                   roi_align, roi_align_torch)


def _oracle(name, grad=True):
    case, feats, rois, levels, dy = roi_case(name)
    res = reference_roi_align(feats, rois, case["out_size"], case["scales"], case["s"], levels, 56.0, grad_output=dy if grad else None)
    return case, feats, rois, levels, dy, res


def _grids(name):
    """[(g_h, g_w) or None] per RoI of a single-level case"""
    case, _, rois, _, _ = roi_case(name)
    return [reference_roi_geometry(r, case["scales"][0], case["out_size"], case["s"])[4:] for r in rois.double().numpy()]


@pytest.mark.parametrize("name", ROI_GOLDEN)
def test_oracle_matches_reference_extension(golden, name):
    """forward_v2 and backward_v2 of the reference's CPU extension in float64, to 1e-12 relative, on the valid RoIs; the rows of the others are zero; its float32 run is
    within float32 rounding of the oracle"""
    _, arrays = golden("roi_align")
    case, feats, rois, levels, dy, (out, dxs) = _oracle(name)
    rows = arrays[f"{name}.rows"]
    assert np.array_equal(rows, roi_valid_rows(case, rois, levels))
    rest = np.setdiff1d(np.arange(case["R"]), rows)
    assert not out[rest].any() and len(rest) == (2 if case["special"] else 0)
    g, gd = arrays[f"{name}.f64.out"], arrays[f"{name}.f64.dx"]
    assert np.abs(out[rows] - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(dxs[0] - gd).max() <= 1e-12 * np.abs(gd).max()
    assert np.abs(arrays[f"{name}.f32.out"] - out[rows]).max() <= 1e-4 * np.abs(out).max()
    assert np.abs(arrays[f"{name}.f32.dx"] - dxs[0]).max() <= 1e-4 * np.abs(dxs[0]).max()


@pytest.mark.parametrize("name", sorted(ROI_CASES))
def test_oracle_adjoint_identity(name):
    """<dY, fwd(X)> = <bwd(dY), X> to 1e-12"""
    case, feats, rois, levels, dy, (out, dxs) = _oracle(name)
    lhs = float((torch.from_numpy(out) * dy).sum())
    rhs = sum(float((torch.from_numpy(d) * x).sum()) for d, x in zip(dxs, feats))
    scale = sum(float((torch.from_numpy(d).abs() * x.abs()).sum()) for d, x in zip(dxs, feats))
    assert abs(lhs - rhs) <= 1e-12 * max(scale, 1.0)


@pytest.mark.parametrize("name", sorted(ROI_CASES))
def test_input_conditions(name):
    """every float64 sample coordinate is >= 1e-3 from -1, H and W; in adaptive cases every roi_h / oh and roi_w / ow is >= 1e-3 from an integer (exact zeros
    excepted); every level-rule argument is >= 1e-3 (relative) from a power of two: no case left out"""
    case, feats, rois, levels, dy = roi_case(name)
    d_coord, d_grid, d_level = roi_input_conditions(case, rois, levels)
    print(f"{name}: coordinates {d_coord:.3e}, grid {d_grid:.3e}, levels {d_level:.3e}")
    assert d_coord >= 1e-3 and d_grid >= 1e-3 and d_level >= 1e-3


def test_cases_reach_what_they_claim():
    """the adaptive cases hold a RoI with grid 1, one with a grid >= 5, one with g_h != g_w, the RoI over the grid limit and the one of negative width; a zero-width
    RoI (grid 0: a zero row); bad batch indices, a level without RoIs, an all-outside RoI and R in {0, 1, 40, 300}"""
    assert {ROI_CASES[n]["R"] for n in ROI_CASES} >= {0, 1, 40, 300} and {ROI_CASES[n]["C"] for n in ROI_CASES} >= {5, 70, 256}
    assert {ROI_CASES[n]["out_size"] for n in ROI_CASES} >= {(7, 7), (14, 14), (3, 5)} and {ROI_CASES[n]["s"] for n in ROI_CASES} == {0, 2, 3}
    for name in ("a1_c5", "a1_c70_m14", "a1_big"):
        grids = _grids(name)
        assert any(g == (1, 1) for g in grids), name
        assert any(g[0] == 0 or g[1] == 0 for g in grids if g[0] is not None), name
    grids = _grids("a1_big")
    assert any(g[0] is not None and min(g) >= 6 and g[0] != g[1] for g in grids)
    assert any(g[0] is not None and min(g) >= 2 and g[0] != g[1] for g in _grids("a1_c5"))
    case, _, rois, _, _ = roi_case("a1_big")
    r = rois.double().numpy()
    assert grids[OVER_LIMIT] == (None, None) and grids[NEGATIVE] == (None, None) and sum(g[0] is None for g in grids) == 2
    assert (r[OVER_LIMIT, 4] - r[OVER_LIMIT, 2]) * case["scales"][0] / case["out_size"][0] > ROI_MAX_GRID and r[NEGATIVE, 3] < r[NEGATIVE, 1]
    assert any((r[i, 3] - r[i, 1]) > case["image"][1] and (r[i, 4] - r[i, 2]) > case["image"][0] for i in range(len(r)) if grids[i][0] is not None)          # the whole map
    case, feats, rois, levels, dy, out = _oracle("a4_c256", grad=False)
    lv = map_roi_levels_xyxy(rois.numpy(), 4)
    r = rois.numpy()
    valid = (r[:, 0] >= 0) & (r[:, 0] < case["B"])
    assert set(lv[valid].tolist()) == {0, 1, 3}          # level 2 receives nothing
    assert (r[:, 0] == -1).any() and (r[:, 0] == case["B"]).any()
    assert all(not out[i].any() for i in range(len(r)) if not valid[i])
    assert any(valid[i] and r[i, 3] > r[i, 1] and not out[i].any() for i in range(len(r)))          # wholly outside
    assert any(valid[i] and r[i, 3] == r[i, 1] and not out[i].any() for i in range(len(r)))          # zero width


def test_level_rule_and_data_rules():
    """upstream's map_roi_levels on hand-made boxes; the sample grid of the specification by hand; every invalid kind gives a zero row and no gradient"""
    def box(w, h):
        return [0, 100.0, 50.0, 100.0 + w, 50.0 + h]
    rois = np.array([box(10, 10), box(111, 111), box(113, 113), box(223, 223), box(225, 225), box(447, 447), box(449, 449), box(5000, 5000), box(28, 448), box(0, 9)])
    assert map_roi_levels_xyxy(rois, 4).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 1, 0]
    assert map_roi_levels_xyxy(rois, 2).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0]
    assert map_roi_levels_xyxy(np.array([[0, 5.0, 5.0, 1.0, 9.0], [0, float("nan"), 0, 1, 1]]), 4).tolist() == [0, 0]          # a negative area, a NaN: level 0
    # a 12 x 20 box at (8, 4) .. (20, 24) on a 16 x 16 map of scale 0.5, 2 x 1 bins: roi_h = 10, roi_w = 6, grid ceil(10 / 2) x ceil(6 / 1) = 5 x 6
    start_h, start_w, roi_h, roi_w, gh, gw = reference_roi_geometry([0, 8.0, 4.0, 20.0, 24.0], 0.5, (2, 1), 0)
    assert (start_h, start_w, roi_h, roi_w, gh, gw) == (1.5, 3.5, 10.0, 6.0, 5, 6)
    y, x, _, _ = reference_roi_samples([0, 8.0, 4.0, 20.0, 24.0], 16, 16, 0.5, (2, 1), 0)
    assert np.allclose(y, [[2.0, 3.0, 4.0, 5.0, 6.0], [7.0, 8.0, 9.0, 10.0, 11.0]]) and np.allclose(x, [[4.0, 5.0, 6.0, 7.0, 8.0, 9.0]])
    assert reference_roi_geometry([0, 8.0, 4.0, 20.0, 24.0], 0.5, (2, 1), 3)[4:] == (3, 3)          # a fixed grid
    # integer sample coordinates: the bin is the plain mean of the pixels
    f = torch.arange(16 * 16, dtype=torch.float64).reshape(1, 1, 16, 16)
    out = reference_roi_align([f], torch.tensor([[0, 8.0, 4.0, 20.0, 24.0]]), (2, 1), [0.5])
    assert np.allclose(out.reshape(-1), [f[0, 0, 2:7, 4:10].mean(), f[0, 0, 7:12, 4:10].mean()])
    # the data rules
    good = [0, 8.0, 4.0, 20.0, 24.0]
    bad = [[-1, 8.0, 4.0, 20.0, 24.0], [1, 8.0, 4.0, 20.0, 24.0], [0, float("nan"), 4.0, 20.0, 24.0], [0, 8.0, 4.0, float("inf"), 24.0], [0, 20.0, 4.0, 8.0, 24.0],
           [0, 8.0, 24.0, 20.0, 4.0], [0, 8.0, 4.0, 20.0, 4.0 + 2.0 * 2 * (ROI_MAX_GRID + 0.5)], [0, 8.0, 4.0, 8.0, 24.0], [-0.5, 8.0, 4.0, 20.0, 24.0]]
    rois = torch.tensor([good] + bad)
    dy = torch.ones(len(rois), 1, 2, 1, dtype=torch.float64)
    out, dxs = reference_roi_align([f], rois, (2, 1), [0.5], grad_output=dy)
    one, d1 = reference_roi_align([f], rois[:1], (2, 1), [0.5], grad_output=dy[:1])
    assert not out[1:9].any() and np.array_equal(out[9], out[0]) and np.array_equal(out[0], one[0])          # (-0.5 truncates to image 0)
    assert np.array_equal(dxs[0], 2 * d1[0])
    out, _ = reference_roi_align([f], rois, (2, 1), [0.5], levels=torch.tensor([0, 0, 0, 0, 0, 0, 0, 0, 0, 1], dtype=torch.int32), grad_output=dy)
    assert not out[9].any()          # an explicit level outside [0, L)
    # a grid of exactly the limit is valid, one above is not
    assert reference_roi_geometry([0, 0.0, 0.0, 4.0, 2.0 * 2 * ROI_MAX_GRID - 0.5], 0.5, (2, 1), 0)[4] == ROI_MAX_GRID


@pytest.mark.parametrize("name", ["a4_r300", "a1_big", "f1_s3_35"])
def test_torch_formulation_matches_oracle_on_cpu(name):
    """the stock-PyTorch formulation (the GPU tests' fp32 comparator; the adaptive grid padded to the batch's largest grid) on float64 features on the CPU agrees with
    the oracle to the rounding of its float32 coordinates, forward and backward, all levels, invalid RoIs included"""
    case, feats, rois, levels, dy, (out, dxs) = _oracle(name)
    f = [x.clone().requires_grad_(True) for x in feats]
    t = roi_align_torch(f, rois, case["out_size"], case["scales"], case["s"], levels if levels is None else levels.long(), 56.0)
    t.backward(dy)
    assert np.abs(t.detach().numpy() - out).max() <= 1e-4
    assert all(np.abs(a.grad.numpy() - b).max() <= 1e-4 for a, b in zip(f, dxs))


def test_module_surface_without_gpu():
    """the reference's names, signatures and __repr__; what is not provided raises NotImplementedError; no CPU fallback"""
    m = RoIAlign(7, 0.25)
    assert repr(m) == "RoIAlign(\n    out_size=(7, 7),\n    spatial_scale=0.25,\n    sample_num=0,\n    use_torchvision=False,\n    aligned=True)"
    assert m.sample_num == 0 and m.aligned is True and RoIAlign((3, 5), 1, 2).out_size == (3, 5) and RoIAlign(14, 0.125, sample_num=2).sample_num == 2
    x, rois = torch.zeros(1, 4, 8, 8), torch.zeros(2, 5)
    with pytest.raises(NotImplementedError, match="aligned=False"):
        roi_align(x, rois, 7, 0.25, 0, False)
    with pytest.raises(NotImplementedError, match="aligned=False"):
        RoIAlign(7, 0.25, aligned=False)
    with pytest.raises(NotImplementedError, match="use_torchvision"):
        RoIAlign(7, 0.25, use_torchvision=True, aligned=False)
    with pytest.raises(ValueError, match="sample_num"):
        roi_align(x, rois, 7, 0.25, ROI_MAX_GRID + 1)
    with pytest.raises(ValueError, match="sample_num"):
        RoIExtractor(sample_num=-1)
    with pytest.raises(ValueError, match="levels"):
        RoIExtractor(featmap_strides=(4, 8, 16, 32, 64, 128))
    with pytest.raises(ValueError, match=r"\[R, 5\]"):
        m(x, torch.zeros(2, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, rois)
    with pytest.raises(RuntimeError, match="no gradient for the RoIs"):
        m(x, rois.requires_grad_(True))
    e = RoIExtractor()
    assert e.featmap_strides == (4, 8, 16, 32) and e.out_size == (7, 7) and e.sample_num == 0 and e.out_channels == 256 and e.finest_scale == 56.0 and e.num_inputs == 4
    assert RoIExtractor(out_size=14).out_size == (14, 14)
    with pytest.raises(ValueError, match="channels"):
        e([torch.zeros(1, 8, 4, 4)] * 4, rois.detach())
    with pytest.raises(ValueError, match="feature maps"):
        e([torch.zeros(1, 256, 4, 4)] * 3, rois.detach())


def test_roi_refusals_without_gpu():
    """Argument validation happens before any launch (the style of tests/test_rroi_cpu.py), with a message that starts "roi"; the plan size is bounded by the maps"""
    from lemevit_amd import _lib, ops
    from lemevit_amd._lib import lib, RroiLevel
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def lv(n=1, H=8, W=8, data=p):
        a = (RroiLevel * max(n, 1))()
        for i in range(max(n, 1)):
            a[i].data, a[i].sb, a[i].sc, a[i].sh, a[i].sw, a[i].H, a[i].W, a[i].spatial_scale = data, 4 * H * W, H * W, W, 1, H, W, 0.25
        return a

    def plan(R=2, levels=None, L=1, B=1, oh=7, ow=7, s=0, rois=p, out=p, nbytes=1 << 15, finest=56.0):
        return lib.lmv_roi_plan(rois, None, R, levels if levels is not None else lv(L), L, B, oh, ow, s, finest, out, nbytes, None)

    def fwd(R=2, levels=None, L=1, B=1, C=4, oh=7, ow=7, dtype=0, pl=p, out=p):
        return lib.lmv_roi_fwd(pl, R, levels if levels is not None else lv(L), L, B, C, oh, ow, dtype, out, None)

    def bwd(R=2, levels=None, L=1, B=1, C=4, oh=7, ow=7, dtype=0, pl=p, dy=p):
        return lib.lmv_roi_bwd(pl, R, dy, levels if levels is not None else lv(L), L, B, C, oh, ow, dtype, None)

    def msg():
        return lib.lmv_last_error()

    for call in (plan, fwd, bwd):
        assert call(L=0) == -1 and b"levels outside 1 .. 5" in msg() and msg().startswith(b"roi")
        assert call(L=6, levels=lv(6)) == -1 and b"levels outside 1 .. 5" in msg()
        assert call(oh=0) == -1 and b"out_size" in msg()
        assert call(ow=0) == -1 and b"out_size" in msg()
        assert call(oh=17, ow=16) == -1 and b"256 bins" in msg()
        assert call(R=-1) == -1 and call(B=0) == -1
        assert call(levels=lv(1, H=0)) == -1 and call(levels=lv(1, W=8193)) == -1 and b"8192" in msg() and msg().startswith(b"roi")
    assert lib.lmv_roi_plan(p, None, 2, None, 1, 1, 7, 7, 0, 56.0, p, 1 << 15, None) == -1 and b"null level table" in msg()
    assert plan(s=-1) == -1 and b"sample_num = -1" in msg() and plan(s=129) == -1 and b"sample_num = 129" in msg()
    assert plan(rois=None) == -1 and b"null rois / plan" in msg()
    assert plan(out=None) == -1 and b"null rois / plan" in msg()
    assert plan(nbytes=100) == -3 and b"lmv_roi_plan_bytes" in msg()
    assert plan(finest=0.0) == -1
    assert plan(rois=p + 2) == -1 and b"misaligned" in msg() and plan(out=p + 8) == -1 and b"misaligned" in msg()
    for call in (fwd, bwd):
        assert call(C=0) == -1 and b"C = 0" in msg()
        assert call(dtype=2) == -1 and b"dtype" in msg()
        assert call(levels=lv(1, data=None)) == -1 and b"null map" in msg()
        assert call(pl=None) == -1 and b"null plan" in msg()
        assert call(R=1 << 20, C=64) == -1 and b"2^31" in msg()          # R C oh ow
        assert call(levels=lv(1, H=4096, W=4096), B=2, C=64) == -1 and b"2^31" in msg()          # B C H W
    assert fwd(out=None) == -1 and bwd(dy=None) == -1
    # sizes: 48 + 16 (oh + ow) + 4 (H + 2 oh + W + 2 ow), rounded up to 16 -- whatever the grid; 0 for what the plan call refuses
    per = 48 + 16 * 14 + 4 * (8 + 14 + 8 + 14)
    assert per % 16 == 0 and lib.lmv_roi_plan_bytes(1, lv(), 1, 7, 7) == per and lib.lmv_roi_plan_bytes(1000, lv(), 1, 7, 7) == 1000 * per
    big = lv(2, H=200, W=336)
    assert lib.lmv_roi_plan_bytes(1, big, 2, 7, 7) == (48 + 16 * 14 + 4 * (214 + 350) + 15) // 16 * 16 == ops.roi_plan_bytes(1, [(200, 336), (200, 336)], (7, 7))
    assert lib.lmv_roi_plan_bytes(0, lv(), 1, 7, 7) == 0 and lib.lmv_roi_plan_bytes(3, lv(), 1, 17, 16) == 0 and lib.lmv_roi_plan_bytes(3, lv(), 0, 7, 7) == 0
    assert lib.lmv_roi_plan_bytes(3, lv(1, H=8193), 1, 7, 7) == 0 and lib.lmv_roi_plan_bytes(3, None, 1, 7, 7) == 0
    assert _lib.ROI_MAX_GRID == ROI_MAX_GRID >= 64
    with pytest.raises(ValueError, match="roi_plan_bytes"):
        ops.roi_plan_bytes(3, [(8, 8)], (17, 16))
    # R = 0 is legal for the plan and the forward, and launches nothing (no GPU is touched here)
    assert plan(R=0, rois=None, out=None, nbytes=0) == 0 and fwd(R=0, pl=None, out=None) == 0
