"""Rotated RoIAlign without a GPU: the float64 oracle against the reference's CPU extension (tests/golden/rroi_align.npz), the adjoint identity, the level rule and
the extension order on hand-made boxes, the library's refusals, and the INPUT CONDITIONS of every case -- those of tests/test_rroi_gpu.py included: no sample
coordinate near -1 / H / W and no box near a level threshold, where a rounding error would flip a sample or a level instead of moving a value."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gen_rroi_golden import CASES, GOLDEN, input_conditions, rroi_case
from lemevit_amd.detection import (RoIAlignRotated, RotatedRoIExtractor, map_roi_levels, reference_rroi_align, reference_rroi_samples, roi_align_rotated,
                                   rroi_align_torch)


def _oracle(name, grad=True):
    case, feats, rois, levels, dy = rroi_case(name)
    res = reference_rroi_align(feats, rois, case["out_size"], case["scales"], case["s"], case["aligned"], levels, 56.0, case["ext"], grad_output=dy if grad else None)
    return case, feats, rois, levels, dy, res


@pytest.mark.parametrize("name", GOLDEN)
def test_oracle_matches_reference_extension(golden, name):
    """forward and backward of the reference's CPU extension in float64, to 1e-12 relative; its float32 run is within float32 rounding of the oracle"""
    _, arrays = golden("rroi_align")
    case, feats, rois, levels, dy, (out, dxs) = _oracle(name)
    g, gd = arrays[f"{name}.f64.out"], arrays[f"{name}.f64.dx"]
    assert np.abs(out - g).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(dxs[0] - gd).max() <= 1e-12 * np.abs(gd).max()
    assert np.abs(arrays[f"{name}.f32.out"] - out).max() <= 1e-4 * np.abs(out).max()
    assert np.abs(arrays[f"{name}.f32.dx"] - dxs[0]).max() <= 1e-4 * np.abs(dxs[0]).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_adjoint_identity(name):
    """<dY, fwd(X)> = <bwd(dY), X> to 1e-12"""
    case, feats, rois, levels, dy, (out, dxs) = _oracle(name)
    lhs = float((torch.from_numpy(out) * dy).sum())
    rhs = sum(float((torch.from_numpy(d) * x).sum()) for d, x in zip(dxs, feats))
    scale = sum(float((torch.from_numpy(d).abs() * x.abs()).sum()) for d, x in zip(dxs, feats))
    assert abs(lhs - rhs) <= 1e-12 * max(scale, 1.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_input_conditions(name):
    """every float64 sample coordinate is >= 1e-3 from -1, H and W, and every sqrt(w h) / finest_scale >= 1e-3 (relative) from a power of two: no case left out"""
    case, feats, rois, levels, dy = rroi_case(name)
    d_coord, d_level = input_conditions(case, rois, levels)
    print(f"{name}: coordinates {d_coord:.3e}, levels {d_level:.3e}")
    assert d_coord >= 1e-3 and d_level >= 1e-3


def test_cases_reach_what_they_claim():
    """between them the cases hold an all-outside RoI (a zero row), a RoI smaller than a pixel, one covering the map, theta in {0, +-pi/2}, bad batch indices, a level
    without RoIs and R in {0, 1, 40, 300}"""
    assert {CASES[n]["R"] for n in CASES} >= {0, 1, 40, 300} and {CASES[n]["C"] for n in CASES} >= {5, 70, 256} and {CASES[n]["B"] for n in CASES} >= {1, 3}
    case, feats, rois, levels, dy, out = _oracle("l4_c256", grad=False)
    lv = map_roi_levels(rois.numpy(), 4)
    assert set(lv.tolist()) == {0, 1, 3}          # level 2 receives nothing
    r = rois.numpy()
    assert (r[:, 0] == -1).any() and (r[:, 0] == case["B"]).any()
    zero_rows = [i for i in range(len(r)) if not out[i].any()]
    assert any(0 <= r[i, 0] < case["B"] for i in zero_rows)          # wholly outside
    assert all(not out[i].any() for i in range(len(r)) if not 0 <= r[i, 0] < case["B"])
    th = set(np.round(r[:, 5].astype(np.float64), 5).tolist())
    assert {0.0, round(math.pi / 2, 5), -round(math.pi / 2, 5)} <= th
    assert ((r[:, 3] * case["scales"][0] < 1) & (r[:, 4] * case["scales"][0] < 1)).any()
    c1, _, r1, _, _ = rroi_case("l1_c5")
    assert ((r1[:, 3] > c1["image"][1]) & (r1[:, 4] > c1["image"][0])).any()


def test_level_rule_and_extension_order():
    """upstream's map_roi_levels on hand-made boxes, and: the level comes from the UN-extended box, the samples from the extended one"""
    def box(w, h):
        return [0, 100.0, 100.0, w, h, 0.0]
    rois = np.array([box(10, 10), box(111, 111), box(113, 113), box(223, 223), box(225, 225), box(447, 447), box(449, 449), box(5000, 5000), box(28, 448), box(0, 0)])
    assert map_roi_levels(rois, 4).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 1, 0]
    assert map_roi_levels(rois, 2).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0]
    assert map_roi_levels(rois, 4, finest_scale=28).tolist() == [0, 1, 2, 2, 3, 3, 3, 3, 2, 0]
    # a 100 x 100 box is on level 0 (100 < 112); extended by 1.4 x 1.2 its sqrt(w h) = 129.6 would be on level 1
    feats = [torch.arange(2 * 64 * 64, dtype=torch.float64).reshape(1, 2, 64, 64).sin(), torch.arange(2 * 32 * 32, dtype=torch.float64).reshape(1, 2, 32, 32).cos()]
    roi = torch.tensor([[0, 120.0, 130.0, 100.0, 100.0, 0.3]])
    got = reference_rroi_align(feats, roi, (3, 3), [0.25, 0.125], 2, True, None, 56.0, (1.4, 1.2))
    want = reference_rroi_align(feats[:1], torch.tensor([[0, 120.0, 130.0, 140.0, 120.0, 0.3]]), (3, 3), [0.25], 2)
    other = reference_rroi_align(feats, roi, (3, 3), [0.25, 0.125], 2, True, torch.tensor([1], dtype=torch.int32), 56.0, (1.4, 1.2))
    assert np.array_equal(got, want) and not np.allclose(got, other)
    assert np.array_equal(other, reference_rroi_align(feats[1:], torch.tensor([[0, 120.0, 130.0, 140.0, 120.0, 0.3]]), (3, 3), [0.125], 2))
    # the sample grid of the specification on one box by hand: theta = 0, aligned, a 4 x 2 box at (6, 5) on an 8 x 8 map of scale 0.5, 1 x 2 bins of 1 x 1 samples
    y, x, empty, yl, yh, xl, xh, w = reference_rroi_samples([0, 12.0, 10.0, 8.0, 4.0, 0.0], 8, 8, 0.5, (1, 2), 1)
    assert y.reshape(-1).tolist() == [4.5, 4.5] and x.reshape(-1).tolist() == [4.5, 6.5] and not empty.any()
    assert yl.reshape(-1).tolist() == [4, 4] and xh.reshape(-1).tolist() == [5, 7] and np.allclose(w, 0.25)
    # theta = +pi/2 turns the box's own x axis into the map's -y axis (y = yy cos - xx sin)
    y2, x2 = reference_rroi_samples([0, 12.0, 10.0, 8.0, 4.0, math.pi / 2], 8, 8, 0.5, (1, 2), 1)[:2]
    assert np.allclose(y2.reshape(-1), [5.5, 3.5]) and np.allclose(x2.reshape(-1), [5.5, 5.5])


def test_torch_formulation_matches_oracle_on_cpu():
    """the stock-PyTorch formulation (the GPU tests' fp32 comparator) in float64 on the CPU agrees with the oracle to rounding, forward and backward, all levels"""
    case, feats, rois, levels, dy, (out, dxs) = _oracle("l4_r300")
    f = [x.clone().requires_grad_(True) for x in feats]
    t = rroi_align_torch(f, rois, case["out_size"], case["scales"], case["s"], case["aligned"], None, 56.0, case["ext"])
    # (the RoIs are float32 numbers and the formulation keeps them so: feed float64 features, compare loosely enough for float32 coordinates)
    t.backward(dy)
    assert np.abs(t.detach().numpy() - out).max() <= 1e-4
    assert all(np.abs(a.grad.numpy() - b).max() <= 1e-4 for a, b in zip(f, dxs))


def test_module_surface_without_gpu():
    """the reference's names, signatures and __repr__; sample_num = 0 raises; no CPU fallback"""
    m = RoIAlignRotated(7, 0.25, 2)
    assert repr(m) == "RoIAlignRotated(\n    out_size=(7, 7),\n    spatial_scale=0.25,\n    sample_num=2,\n    aligned=True,"
    assert RoIAlignRotated(7, 0.25).sample_num == 0 and RoIAlignRotated((3, 5), 1).out_size == (3, 5)
    x, rois = torch.zeros(1, 4, 8, 8), torch.zeros(2, 6)
    with pytest.raises(ValueError, match="sample_num = 0"):
        roi_align_rotated(x, rois, 7, 0.25)
    with pytest.raises(ValueError, match="sample_num = 0"):
        RotatedRoIExtractor(sample_num=0)
    with pytest.raises(ValueError, match="levels"):
        RotatedRoIExtractor(featmap_strides=(4, 8, 16, 32, 64, 128))
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, rois)
    with pytest.raises(RuntimeError, match="no gradient for the RoIs"):
        m(x, rois.requires_grad_(True))
    e = RotatedRoIExtractor()
    assert e.featmap_strides == (4, 8, 16, 32) and e.extend_factor == (1.4, 1.2) and e.out_size == (7, 7) and e.sample_num == 2 and e.out_channels == 256
    with pytest.raises(ValueError, match="channels"):
        e([torch.zeros(1, 8, 4, 4)] * 4, rois.detach())


def test_strides_injective():
    """the host's test for layouts in which two indices share an address (a gradient in such a layout would have several writers per element)"""
    from lemevit_amd.ops import strides_injective
    t = torch.zeros(2, 3, 4, 5)
    for v in (t, t.contiguous(memory_format=torch.channels_last), t[:, 1:], t[:, :, ::2, 1:4], t.permute(0, 1, 3, 2), t[:1]):
        assert strides_injective(v.shape, v.stride())
    assert strides_injective((1, 3, 4, 5), (0, 20, 5, 1))          # (a stride of 0 on an extent of 1 shares nothing)
    assert not strides_injective(*(lambda e: (e.shape, e.stride()))(t[:1].expand(2, 3, 4, 5)))
    assert not strides_injective((2, 2), (1, 1)) and not strides_injective((2, 3, 4, 5), (60, 20, 4, 1))


def test_rroi_refusals_without_gpu():
    """Argument validation happens before any launch (the style of test_abi.py::test_error_reporting_without_gpu)"""
    from lemevit_amd import _lib
    from lemevit_amd._lib import lib, RroiLevel
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)

    def lv(n=1, H=8, W=8, data=p):
        a = (RroiLevel * max(n, 1))()
        for i in range(max(n, 1)):
            a[i].data, a[i].sb, a[i].sc, a[i].sh, a[i].sw, a[i].H, a[i].W, a[i].spatial_scale = data, 4 * H * W, H * W, W, 1, H, W, 0.25
        return a

    def plan(R=2, levels=None, L=1, B=1, oh=7, ow=7, s=2, rois=p, out=p, nbytes=1 << 16, aligned=1, finest=56.0):
        return lib.lmv_rroi_plan(rois, None, R, levels if levels is not None else lv(L), L, B, oh, ow, s, aligned, finest, 1.0, 1.0, out, nbytes, None)

    def fwd(R=2, levels=None, L=1, B=1, C=4, oh=7, ow=7, s=2, dtype=0, pl=p, out=p):
        return lib.lmv_rroi_fwd(pl, R, levels if levels is not None else lv(L), L, B, C, oh, ow, s, dtype, out, None)

    def bwd(R=2, levels=None, L=1, B=1, C=4, oh=7, ow=7, s=2, dtype=0, pl=p, dy=p):
        return lib.lmv_rroi_bwd(pl, R, dy, levels if levels is not None else lv(L), L, B, C, oh, ow, s, dtype, None)

    def msg():
        return lib.lmv_last_error()

    for call in (plan, fwd, bwd):
        assert call(L=0) == -1 and b"levels outside 1 .. 5" in msg() and msg().startswith(b"rroi")
        assert call(L=6, levels=lv(6)) == -1 and b"levels outside 1 .. 5" in msg()
        assert call(s=0) == -1 and b"sample_num = 0" in msg() and b"not supported" in msg()
        assert call(s=5) == -1 and b"sample_num = 5" in msg()
        assert call(oh=0) == -1 and b"out_size" in msg()
        assert call(ow=0) == -1 and b"out_size" in msg()
        assert call(oh=17, ow=16) == -1 and b"256 bins" in msg()
        assert call(oh=16, ow=16, s=3) == -1 and b"1024 samples" in msg()
        assert call(R=-1) == -1 and call(B=0) == -1
        assert call(R=1 << 22, oh=16, ow=16, s=2) == -1 and b"2^31" in msg()
        assert call(levels=lv(1, H=0)) == -1 and call(levels=lv(1, W=65536)) == -1 and b"65535" in msg()
    assert lib.lmv_rroi_plan(p, None, 2, None, 1, 1, 7, 7, 2, 1, 56.0, 1.0, 1.0, p, 1 << 16, None) == -1 and b"null level table" in msg()
    assert plan(rois=None) == -1 and b"null rois / plan" in msg()
    assert plan(out=None) == -1 and b"null rois / plan" in msg()
    assert plan(nbytes=100) == -3 and b"lmv_rroi_plan_bytes" in msg()
    assert plan(aligned=2) == -1 and plan(finest=0.0) == -1
    assert plan(rois=p + 2) == -1 and b"misaligned" in msg()
    for call in (fwd, bwd):
        assert call(C=0) == -1 and b"C = 0" in msg()
        assert call(dtype=2) == -1 and b"dtype" in msg()
        assert call(dtype=7) == -1
        assert call(levels=lv(1, data=None)) == -1 and b"null map" in msg()
        assert call(pl=None) == -1 and b"null plan" in msg()
        assert call(R=1 << 20, C=64) == -1 and b"2^31" in msg()          # R C oh ow
        assert call(levels=lv(1, H=4096, W=4096), B=2, C=64) == -1 and b"2^31" in msg()          # B C H W
    assert fwd(out=None) == -1 and bwd(dy=None) == -1
    # sizes: 32 B per RoI + 24 B per sample; 0 for what the plan call refuses
    assert lib.lmv_rroi_plan_bytes(1, 7, 7, 2) == 32 + 196 * 24 == _lib.RROI_HEADER_BYTES + 196 * _lib.RROI_SAMPLE_BYTES
    assert lib.lmv_rroi_plan_bytes(1024, 7, 7, 2) == 1024 * 4736 and lib.lmv_rroi_plan_bytes(0, 7, 7, 2) == 0
    assert lib.lmv_rroi_plan_bytes(3, 7, 7, 0) == 0 and lib.lmv_rroi_plan_bytes(3, 7, 7, 5) == 0 and lib.lmv_rroi_plan_bytes(3, 17, 16, 1) == 0
    # R = 0 is legal for the plan and the forward, and launches nothing (no GPU is touched here)
    assert plan(R=0, rois=None, out=None, nbytes=0) == 0 and fwd(R=0, pl=None, out=None) == 0
