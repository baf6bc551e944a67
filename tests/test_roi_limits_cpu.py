"""The size-limit cases of both RoIAlign operators without a GPU: every INPUT CONDITION of tests/test_roi_limits_gpu.py, asserted on the float64 oracle alone --
margins of the sample coordinates (max(1e-3, 16 fp32 ulps)), bin sizes away from integers, table entry 256 in use, weight records filled to the width of the map,
grids of exactly 128, indices with bit 15 set, every RoI on tile (0, 0), dyadic coordinates exact in float32 -- and the data rules for non-finite RoIs on the oracle
and on the stock-PyTorch formulation."""
import math

import numpy as np
import pytest
import torch

from gen_roi_limits import (DYADIC_ROWS, NEGATIVE_ROWS, NONFINITE_FIRST, ROI_LIMITS, RROI_LIMITS, RULES_BAD, RULES_HALF, RULES_TWIN, margin, roi_limit_case,
                            roi_limit_conditions, roi_limit_samples, roi_limit_valid_rows, rroi_limit_case, rroi_limit_conditions, rroi_limit_samples, rroi_samples_f32)
from lemevit_amd.detection import (ROI_MAX_GRID, _roi_corner, reference_roi_align, reference_roi_geometry, reference_rroi_align, roi_align_torch, rroi_align_torch)


def _names(table, kind):
    return [n for n in table if table[n]["kind"] == kind]


def test_margin_rule():
    """max(1e-3, 16 fp32 ulps): 1e-3 up to 512, 1 / 8 of a pixel at 65535"""
    assert margin(40.0) == 1e-3 and margin(512.0) == 1e-3 and margin(8192.0) == 16 * 2.0 ** -10 and margin(65535.0) == 0.125 and margin(65537.0) == 0.25


@pytest.mark.parametrize("name", sorted(ROI_LIMITS))
def test_roi_input_conditions(name):
    """no sample coordinate within the margin of -1, H or W; no adaptive bin size within 1e-3 of an integer; R <= 16 and C <= 5 except where the case is about them"""
    case, feats, rois, levels, dy = roi_limit_case(name)
    coord, grid = roi_limit_conditions(case, rois, levels)
    print(f"{name}: coordinates {coord:.2f} margins, grid {grid:.3e}")
    assert coord >= 1.0 and grid >= 1e-3 and rois.is_contiguous() and rois.dtype == torch.float32 and levels.dtype == torch.int32
    assert case["R"] <= 16 or case["kind"] in ("tile", "rules")
    assert case["C"] <= 5 or name.endswith("_c70")


@pytest.mark.parametrize("name", sorted(RROI_LIMITS))
def test_rroi_input_conditions(name):
    """no sample coordinate within the margin of -1, H or W; under the level rule no box within 1e-3 (relative) of the threshold"""
    case, feats, rois, levels, dy = rroi_limit_case(name)
    coord, level = rroi_limit_conditions(case, rois, levels)
    print(f"{name}: coordinates {coord:.2f} margins, level {level:.3e}")
    assert coord >= 1.0 and level >= 1e-3 and rois.is_contiguous() and rois.dtype == torch.float32
    assert case["R"] <= 16 or case["kind"] in ("tile", "nonfinite")
    assert case["C"] <= 5 or name.endswith("_c70")


def _runs(c, ext):
    """per bin of an axis: (first pixel, run length) of the non-empty samples [bins, g], as the plan kernel's first pass finds them"""
    empty, lo, hi, _, _ = _roi_corner(c, ext)
    res = []
    for p in range(c.shape[0]):
        live = ~empty[p]
        res.append((int(lo[p][live].min()), int(hi[p][live].max() - lo[p][live].min() + 1)) if live.any() else (0, 0))
    return res


@pytest.mark.parametrize("name", _names(ROI_LIMITS, "kinds"))
def test_bins_at_the_limit(name):
    """256 bins; with 1 x 256 and 256 x 1 the bin table has 257 entries and entry 256 (the last x bin / the only x bin) has a non-empty run in some RoI; the RoI kinds
    are all there"""
    case, feats, rois, levels, dy = roi_limit_case(name)
    oh, ow = case["out_size"]
    assert oh * ow == 256 and case["R"] == 12 and case["B"] == 2 and case["sizes"] == [(24, 40)]
    smp = roi_limit_samples(case, rois, levels)
    if oh + ow == 257:
        assert any(_runs(x, W)[256 - oh][1] > 0 and any(n > 0 for _, n in _runs(y, H)) for _, y, x, H, W in smp)
    r = rois.numpy()
    H, W = case["sizes"][0]
    assert (r[:, 1] < 0).any() and (r[:, 3] > W).any() and (r[:, 2] < 0).any() and (r[:, 4] > H).any()          # straddling each border
    assert ((r[:, 1] < 0) & (r[:, 3] > W) & (r[:, 2] < 0) & (r[:, 4] > H)).any() and (r[:, 3] == r[:, 1]).any()          # the whole map, zero width
    assert ((r[:, 3] - r[:, 1] < 1) & (r[:, 3] > r[:, 1]) & (r[:, 4] - r[:, 2] < 1)).any()          # tiny
    assert ((r[:, 1] > 0) & (r[:, 3] < W) & (r[:, 2] > 0) & (r[:, 4] < H) & (r[:, 3] - r[:, 1] > 2)).any()          # inside


def test_grid_at_the_limit():
    """g128_1x1: grids 128 x 128, 127 x 127, 128 x 1 and 1 x 128 from sizes inside (127 + 1e-3, 128 - 1e-3) etc.; g128_7x7: grid 128 on a 40 x 48 map, most samples
    empty; g_over: one RoI over the limit on the y axis alone (invalid) beside one just under it"""
    case, _, rois, levels, _ = roi_limit_case("g128_1x1")
    geo = [reference_roi_geometry(r, 1.0, case["out_size"], 0) for r in rois.double().numpy()]
    grids = [g[4:] for g in geo]
    assert grids[0] == (128, 128) and grids[1] == (127, 127) and grids[2] == (1, 128) and grids[3] == (128, 1) and grids[4] == grids[5] == (128, 128) == (ROI_MAX_GRID,) * 2
    assert all(127 + 1e-3 < v < 128 - 1e-3 for g in (geo[0], geo[4], geo[5]) for v in g[2:4]) and all(126 < v < 127 for v in geo[1][2:4])
    assert case["sizes"] == [(132, 132)] and case["out_size"] == (1, 1)
    case, _, rois, levels, _ = roi_limit_case("g128_7x7")
    _, y, x, H, W = roi_limit_samples(case, rois, levels)[0]
    assert y.shape == (7, 128) and x.shape == (7, 128) and rois[0, 3] - rois[0, 1] > 890 and rois[0, 4] - rois[0, 2] > 890
    ey, ex = _roi_corner(y, H)[0], _roi_corner(x, W)[0]
    assert ey.mean() > 0.9 and ex.mean() > 0.9 and (~ey).any() and (~ex).any()
    case, _, rois, levels, _ = roi_limit_case("g_over")
    geo = [reference_roi_geometry(r, 1.0, case["out_size"], 0) for r in rois.double().numpy()]
    assert geo[0][4] is None and 128 < geo[0][2] < 129 and geo[0][3] < 128 and geo[1][4:] == (128, 51) and roi_limit_valid_rows(case, rois, levels).tolist() == [1, 2]


@pytest.mark.parametrize("name", _names(ROI_LIMITS, "fill"))
def test_extent_fills_the_weight_record(name):
    """a RoI over the whole long axis with roi / 64 in (127, 128): grid 128, and the run lengths of that axis sum to at least its extent -- within two weights per bin of
    the record's capacity ext + 2 bins, which they never exceed; on a map of extent 1 every sample takes the clamped branch"""
    case, _, rois, levels, _ = roi_limit_case(name)
    H, W = case["sizes"][0]
    axis, E = (0, H) if H > W else (1, W)
    bins = case["out_size"][axis]
    assert E == 8192 and bins == 64 and case["out_size"][1 - axis] == 1
    total = []
    for r, y, x, _, _ in roi_limit_samples(case, rois, levels):
        c = (y, x)[axis]
        assert c.shape == (64, 128) and 127 < (c[1, 0] - c[0, 0]) < 128
        total.append(sum(n for _, n in _runs(c, E)))
        if min(H, W) == 1:
            o = (y, x)[1 - axis]
            _, lo, hi, _, _ = _roi_corner(o, 1)
            assert o.size >= 2 and not lo.any() and not hi.any()
    print(f"{name}: weights in use {total} of {E + 2 * bins}")
    assert total[0] >= E and all(t <= E + 2 * bins for t in total)


@pytest.mark.parametrize("name", _names(ROI_LIMITS, "far"))
def test_extent_far_end_and_seam(name):
    """RoIs of 3 .. 20 pixels: some touch the last pixel, some straddle the far border (empty samples beyond it), some cross pixel 4095 | 4096 (the seam of tile 256)"""
    case, _, rois, levels, _ = roi_limit_case(name)
    H, W = case["sizes"][0]
    axis, E = (0, H) if H > W else (1, W)
    last = seam = beyond = False
    for r, y, x, _, _ in roi_limit_samples(case, rois, levels):
        c = (y, x)[axis]
        size = float(rois[r, 3 + (1 - axis)] - rois[r, 1 + (1 - axis)])
        assert 3 <= size <= 20
        empty, lo, hi, _, _ = _roi_corner(c, E)
        live = ~empty
        last |= bool((hi[live] == E - 1).any())
        beyond |= bool((c > E).any())
        seam |= bool((lo[live] <= 4095).any() and (hi[live] >= 4096).any())
    assert last and seam and beyond and E == 8192


@pytest.mark.parametrize("name", _names(ROI_LIMITS, "tile"))
def test_every_roi_on_the_first_tile(name):
    """each of the R RoIs (64: one full ballot word; 65, 130: more) is valid, lies on the map and touches tile (0, 0) -- pixels y < 8, x < 16 -- of its image; on the
    9 x 17 map some also reach row 8 and column 16, the one-pixel second tiles; with B = 2 the RoIs of image 1 are the odd rows"""
    case, _, rois, levels, _ = roi_limit_case(name)
    H, W = case["sizes"][0]
    smp = roi_limit_samples(case, rois, levels)
    assert len(smp) == case["R"] and case["R"] in (64, 65, 130)
    r = rois.numpy()
    assert (r[:, 1] >= 0).all() and (r[:, 2] >= 0).all() and (r[:, 3] <= W).all() and (r[:, 4] <= H).all()
    reach = 0
    for _, y, x, _, _ in smp:
        ry, rx = _runs(y, H), _runs(x, W)
        assert min(f for f, n in ry if n) < 8 and min(f for f, n in rx if n) < 16
        reach += max(f + n for f, n in ry) == H and max(f + n for f, n in rx) == W
    assert reach >= case["R"] // 8
    if case["B"] == 2:
        assert np.array_equal(r[:, 0], np.arange(case["R"]) % 2)


def test_data_rule_case():
    """"rules": every invalid kind is there and is invalid on the oracle, everything else is valid; the row with batch index -0.5 equals its twin on image 0"""
    case, feats, rois, levels, dy = roi_limit_case("rules")
    r, lv = rois.numpy(), levels.numpy()
    b = RULES_BAD
    assert np.isnan(r[b[0], 1]) and np.isinf(r[b[1], 3]) and r[b[2], 3] < r[b[2], 1] and r[b[3], 4] < r[b[3], 2] and r[b[4], 0] == -1 and r[b[5], 0] == case["B"]
    assert np.isnan(r[b[6], 0]) and (np.abs(r[b[7], 1:]) == np.float32(1e30)).all() and lv[b[8]] == -1 and lv[b[9]] == len(case["sizes"]) == 2
    rows = roi_limit_valid_rows(case, rois, levels)
    assert rows.tolist() == [i for i in range(case["R"]) if i not in b] and r[RULES_HALF, 0] == -0.5 and set(lv[rows].tolist()) == {0, 1} and set(r[rows, 0].tolist()) == {0, 1, -0.5}
    out, dxs = reference_roi_align(feats, rois, case["out_size"], case["scales"], 0, levels, grad_output=dy)
    assert not np.isnan(out).any() and not out[list(b)].any() and out[rows].any(axis=(1, 2, 3)).all()
    g = dy.clone()
    g[RULES_TWIN] = g[RULES_HALF]
    assert np.array_equal(reference_roi_align(feats, rois, case["out_size"], case["scales"], 0, levels)[RULES_HALF], out[RULES_TWIN])
    keep = torch.from_numpy(rows)
    _, dx2 = reference_roi_align(feats, rois[keep], case["out_size"], case["scales"], 0, levels[keep], grad_output=dy[keep])
    assert all(np.array_equal(a, c) for a, c in zip(dxs, dx2))


@pytest.mark.parametrize("name", ["g128_1x1", "rules", "e1x8192_b", "b1x256_a"])
def test_roi_torch_formulation_at_the_limits(name):
    """the stock-PyTorch formulation (the GPU tests' fp32 comparator) on float64 features on the CPU agrees with the oracle to the rounding of its float32 coordinates at
    grid 128, at 8192 pixels, with 256 bins and on every invalid kind (no NaN, no index out of range)"""
    case, feats, rois, levels, dy = roi_limit_case(name)
    out, dxs = reference_roi_align(feats, rois, case["out_size"], case["scales"], case["s"], levels, grad_output=dy)
    f = [x.clone().requires_grad_(True) for x in feats]
    t = roi_align_torch(f, rois, case["out_size"], case["scales"], case["s"], levels.long())
    t.backward(dy)
    tol = 1e-4 * max(1.0, margin(max(max(s) for s in case["sizes"])) / 1e-3)          # (float32 coordinates: 16 ulps are 1e-3 up to 512 pixels)
    assert np.abs(t.detach().numpy() - out).max() <= tol
    assert all(np.abs((a.grad if a.grad is not None else torch.zeros_like(a)).numpy() - b).max() <= tol for a, b in zip(f, dxs))


# ---- rotated ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rroi_sample_limits():
    """(16, 16; 2) and (8, 8; 4) are 1024 samples, sample_num reaches 4, 1 x 256 and 256 x 1 are there; theta covers 0, +-pi/2, pi; both `aligned` values at (8, 8; 4)"""
    ns = {n: c["out_size"][0] * c["out_size"][1] * c["s"] ** 2 for n, c in RROI_LIMITS.items() if c["kind"] == "kinds"}
    assert ns["s16x16_2"] == ns["s8x8_4"] == ns["s8x8_4_na"] == ns["s1x256_2"] == ns["s16x16_2_c70"] == 1024 and ns["s256x1_1"] == ns["s16x16_1"] == 256 and ns["s7x7_4"] == 784
    assert RROI_LIMITS["s8x8_4"]["aligned"] and not RROI_LIMITS["s8x8_4_na"]["aligned"] and RROI_LIMITS["s16x16_2_c70"]["C"] == 70
    for n in ns:
        case, _, rois, _, _ = rroi_limit_case(n)
        th = rois[:, 5].numpy()
        assert case["sizes"] == [(32, 40)] and case["R"] == 12 and case["B"] == 2
        assert {np.float32(0.0), np.float32(math.pi / 2), np.float32(-math.pi / 2), np.float32(math.pi)} <= set(th.tolist()) and th.min() > -math.pi and th.max() <= np.float32(math.pi)
        assert len(set(th.tolist())) >= 7


@pytest.mark.parametrize("name", _names(RROI_LIMITS, "far"))
def test_rroi_extent_indices_and_dyadic_rows(name):
    """maps of 65535 (and 40000) pixels: in some non-empty sample BOTH indices of the long axis are >= 32768 (bits 15 and 31 of the packed word), in some the pair
    straddles 32767 | 32768, some reach the last pixel and some lie beyond the border; a RoI sits at the origin.  The dyadic rows (theta = 0) have sample
    coordinates that are exact in float32 -- the float32 restatement equals the float64 oracle -- the generic rows do not"""
    case, _, rois, levels, _ = rroi_limit_case(name)
    H, W = case["sizes"][0]
    axis, E = (0, H) if H > W else (1, W)
    smp = rroi_limit_samples(case, rois, levels)
    assert len(smp) == case["R"] == 16 and E in (65535, 40000) and case["out_size"] == (7, 7) and case["s"] == 2
    both = flip = last = beyond = origin = False
    exact = []
    for r, (y, x, empty, yl, yh, xl, xh, _), _, _ in smp:
        lo, hi, c = ((yl, yh, y), (xl, xh, x))[axis]
        live = ~empty
        both |= bool((lo[live] >= 32768).any())
        flip |= bool(((lo == 32767) & (hi == 32768) & live).any())
        last |= bool((hi[live] == E - 1).any())
        beyond |= bool((c > E).any())
        origin |= bool(((lo == 0) & live).any())
        y32, x32 = rroi_samples_f32(rois[r].numpy(), 1.0, case["out_size"], case["s"])
        exact.append(bool(np.array_equal(y32.astype(np.float64), y) and np.array_equal(x32.astype(np.float64), x)))
    assert both and flip and last and beyond and origin
    assert all(exact[:DYADIC_ROWS]) and not any(exact[DYADIC_ROWS:])
    th = rois[:, 5].numpy()
    assert not th[:DYADIC_ROWS].any() and (np.abs(th[DYADIC_ROWS:]) == np.float32(math.pi / 2)).sum() >= 3
    for r in np.nonzero(np.abs(th) == np.float32(math.pi / 2))[0]:          # the long side along the map
        w, h = float(rois[r, 3]), float(rois[r, 4])
        assert max(w, h) >= 12 and (h > w) == (axis == 1)


@pytest.mark.parametrize("name", _names(RROI_LIMITS, "tile"))
def test_every_rroi_on_the_first_tile(name):
    """each of the R rotated RoIs has a non-empty sample whose low corner lies on tile (0, 0) of its image; on the 9 x 17 map some reach row 8 and column 16"""
    case, _, rois, levels, _ = rroi_limit_case(name)
    H, W = case["sizes"][0]
    smp = rroi_limit_samples(case, rois, levels)
    assert len(smp) == case["R"] and case["R"] in (64, 65, 130)
    reach = 0
    for r, (y, x, empty, yl, yh, xl, xh, _), _, _ in smp:
        live = ~empty
        assert ((yl < 8) & (xl < 16) & live).any(), r
        reach += bool((yh[live] == H - 1).any() and (xh[live] == W - 1).any())
    assert reach >= case["R"] // 8
    if case["B"] == 2:
        assert np.array_equal(rois[:, 0].numpy(), np.arange(case["R"]) % 2)


def test_nonfinite_rotated_rois_are_invalid():
    """NaN, +inf and -inf in each of cx, cy, w, h, theta: the oracle and the stock formulation give zero rows, no NaN anywhere, and the dX of the run without those rows;
    the valid RoIs cover both levels and both images"""
    case, feats, rois, levels, dy = rroi_limit_case("nonfinite")
    r = rois.numpy()
    bad = list(range(NONFINITE_FIRST, NONFINITE_FIRST + 15))
    for k, row in enumerate(bad):
        v = r[row, 1 + k // 3]
        assert (np.isnan(v), v == np.inf, v == -np.inf)[k % 3] and np.isfinite(np.delete(r[row], 1 + k // 3)).all()
    assert levels is None and case["R"] == NONFINITE_FIRST + 15 and np.isfinite(r[:NONFINITE_FIRST]).all()
    smp = rroi_limit_samples(case, rois, levels)
    assert [s[0] for s in smp] == list(range(NONFINITE_FIRST)) and {s[2] for s in smp} == {13, 7} and set(r[:NONFINITE_FIRST, 0].tolist()) == {0, 1}
    out, dxs = reference_rroi_align(feats, rois, case["out_size"], case["scales"], case["s"], True, None, 56.0, grad_output=dy)
    assert not np.isnan(out).any() and not any(np.isnan(d).any() for d in dxs) and not out[bad].any() and out[:NONFINITE_FIRST].any(axis=(1, 2, 3)).all()
    _, dx2 = reference_rroi_align(feats, rois[:NONFINITE_FIRST], case["out_size"], case["scales"], case["s"], True, None, 56.0, grad_output=dy[:NONFINITE_FIRST])
    assert all(np.array_equal(a, c) for a, c in zip(dxs, dx2))
    f = [x.clone().requires_grad_(True) for x in feats]
    t = rroi_align_torch(f, rois, case["out_size"], case["scales"], case["s"], True, None, 56.0)
    t.backward(dy)
    assert not torch.isnan(t).any() and not t[bad].any() and np.abs(t.detach().numpy() - out).max() <= 1e-4
    assert all(not torch.isnan(a.grad).any() and np.abs(a.grad.numpy() - b).max() <= 1e-4 for a, b in zip(f, dxs))
    # a single level goes through the same rule
    one = rroi_align_torch(f[:1], rois, case["out_size"], case["scales"][:1], case["s"])
    assert not torch.isnan(one).any() and not one[bad].any()


def test_negative_sizes_are_not_validated():
    """finite negative w / h: the formulas apply as they are (the box mirrored), on the oracle and the stock formulation alike"""
    case, feats, rois, levels, dy = rroi_limit_case("negative")
    assert rois[NEGATIVE_ROWS[0], 3] < 0 and rois[NEGATIVE_ROWS[1], 4] < 0 and torch.isfinite(rois).all()
    out = reference_rroi_align(feats, rois, case["out_size"], case["scales"], case["s"], True, None, 56.0)
    t = rroi_align_torch(feats, rois, case["out_size"], case["scales"], case["s"], True, None, 56.0)
    assert out[list(NEGATIVE_ROWS)].any(axis=(1, 2, 3)).all() and np.abs(t.numpy() - out).max() <= 1e-4


def test_rroi_plan_refuses_strided_rois():
    """the library reads rows of 6 floats: ops.rroi_plan refuses a non-contiguous view before any launch, as ops.roi_plan does"""
    from lemevit_amd import ops
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.rroi_plan(torch.zeros(6, 4).t(), [(8, 8)], [1.0], 1, (7, 7), 2)
    with pytest.raises(ValueError, match="contiguous float32"):
        ops.roi_plan(torch.zeros(5, 4).t(), [(8, 8)], [1.0], 1, (7, 7))
