"""The box coders without a GPU (lemevit_amd/detection.py: MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder; csrc/coder.hip): the float64 oracles against the two hand
cases and against the stock-PyTorch formulations, round trips, the canonical form, the gathering encode's zero rows, the generated cases' conditions, the classes'
argument checks and empty inputs, the new symbols, and the refusals of the C entry points.

Round trips, measured on the float64 oracle over the cases of 1 .. 1000 rows (``-s`` prints them): OBB2OBB decode(encode(g)) is g to 1.1e-13 pixels (corner sets) on all
rows, midpoint to 2.0e-12 pixels on the rows whose gaps of condition (a) are at least 0.11; on the rows with a level edge (a gap of at most 0.09) it is
legitimately another box.  The bound asserted is ROUND_TRIP = 1e-9 pixels: float64 rounding (1.1e-16) of coordinates up to 2e3, amplified by at most the
conditioning of a direction taken from two points VERTEX / GAP margins apart (1e3 / 1e-2 = 1e5) and a few dozen operations -- 1.1e-16 x 2e3 x 1e5 x 40 < 1e-9.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gen_coder_golden as gen
from lemevit_amd.detection import (MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder, decode_map_torch, encode_assigned_torch, midpoint_decode_torch, midpoint_encode_torch,
                                   obb2obb_decode_torch, obb2obb_encode_torch, reference_encode_assigned, reference_midpoint_decode, reference_midpoint_encode,
                                   reference_obb2obb_decode, reference_obb2obb_encode, reference_obb_corners)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND_TRIP = 1e-9
TORCH_F64 = 1e-9


def corner_distance(a, b) -> np.ndarray:
    """[N]: per row, the maximum over the corners of one box of the distance to the nearest corner of the other, taken both ways (rows (cx, cy, w, h, theta))"""
    ca, cb = reference_obb_corners(a), reference_obb_corners(b)
    d = np.linalg.norm(ca[:, :, None] - cb[:, None], axis=-1)
    return np.maximum(d.min(2).max(1), d.min(1).max(1))


def as_rows(x) -> np.ndarray:
    """[N, 5 C] -> [N C, 5] float64"""
    x = x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)
    return x.reshape(-1, 5)


def test_hand_cases():
    """the two cases of include/lemevit_hip.h's rules worked by hand: anchor (40, 30, 60, 50), stds (1, 1, 1, 1, 0.5, 0.5)"""
    a = np.array([[40.0, 30.0, 60.0, 50.0]] * 2)
    g = np.array([[50.0, 40.0, 20.0, 10.0, 0.0], [50.0, 40.0, 20.0, 10.0, math.pi / 6]])
    e = reference_midpoint_encode(a, g, stds=gen.RPN_STDS)
    assert np.abs(e[0] - [0, 0, 0, -0.6931472, 1, 1]).max() < 5e-8
    assert np.abs(e[1] - [0, 0, 0.10977363, -0.06933646, 0.55198152, -0.07179677]).max() < 5e-8
    assert np.abs(reference_midpoint_decode(a, e, stds=gen.RPN_STDS) - g).max() < 1e-12
    t = midpoint_encode_torch(torch.from_numpy(a), torch.from_numpy(g), stds=gen.RPN_STDS)
    assert np.abs(t.numpy() - e).max() < 1e-12
    assert np.abs(midpoint_decode_torch(torch.from_numpy(a), t, stds=gen.RPN_STDS).numpy() - g).max() < 1e-12
    # OBB2OBB: a proposal against itself is a row of zeros; against its (h, w, theta + pi/2) twin too
    p = np.array([[10.0, 20.0, 8.0, 4.0, 0.3]])
    assert np.abs(reference_obb2obb_encode(p, p)).max() < 1e-15
    twin = np.array([[10.0, 20.0, 4.0, 8.0, 0.3 - math.pi / 2]])
    assert np.abs(reference_obb2obb_encode(p, twin)).max() < 1e-15
    # a shift of (3, 4) in the image is (3 c - 4 s', ...) in the proposal's frame: at theta = 0 it is (3 / w, 4 / h)
    q = np.array([[13.0, 24.0, 16.0, 2.0, 0.1]])
    e = reference_obb2obb_encode(np.array([[10.0, 20.0, 8.0, 4.0, 0.0]]), q)
    assert np.abs(e[0] - [3 / 8, 4 / 4, math.log(2), math.log(0.5), 0.1]).max() < 1e-15


@pytest.mark.parametrize("N", gen.ROWS)
def test_round_trips(N):
    """decode(encode(g)) == g as corner sets, within ROUND_TRIP pixels, on the float64 oracle and on the torch formulation in float64: OBB2OBB on all rows, midpoint on
    the rows whose gaps in (a) are at least 0.11"""
    c = gen.obb_encode_case(N)
    for enc, dec in ((reference_obb2obb_encode, reference_obb2obb_decode), (obb2obb_encode_torch, obb2obb_decode_torch)):
        p, g = (c["proposals"].double(), c["gts"].double())
        err = corner_distance(as_rows(dec(p, enc(p, g, stds=gen.RCNN_STDS), stds=gen.RCNN_STDS)), g.numpy()).max()
        print(f"    N {N} obb2obb {enc.__name__}: round trip {err:.2e} px")
        assert err <= ROUND_TRIP
    c = gen.midpoint_encode_case(N)
    clear = c["clear"]
    for enc, dec in ((reference_midpoint_encode, reference_midpoint_decode), (midpoint_encode_torch, midpoint_decode_torch)):
        a, g = (c["anchors"].double(), c["gts"].double())
        d = corner_distance(as_rows(dec(a, enc(a, g, stds=gen.RPN_STDS), stds=gen.RPN_STDS)), g.numpy())
        print(f"    N {N} midpoint {enc.__name__}: round trip {d[clear].max() if clear.any() else 0.0:.2e} px on {int(clear.sum())} clear rows")
        assert not clear.any() or d[clear].max() <= ROUND_TRIP


@pytest.mark.parametrize("N", gen.ROWS)
def test_torch_formulations_equal_the_oracles(N):
    """the stock-PyTorch formulations on float64 inputs on the CPU equal the oracles to 1e-9: encodes on the deltas, decodes on the corners of every row and on the
    five parameters of the rows whose canonical form is stable; every decoded row of both sides is canonical"""
    def canonical(o):
        o = as_rows(o)
        assert (o[:, 2] >= o[:, 3]).all() and (o[:, 4] >= -math.pi / 2).all() and (o[:, 4] < math.pi / 2).all()

    c = gen.midpoint_encode_case(N)
    assert np.abs(midpoint_encode_torch(c["anchors"].double(), c["gts"].double(), stds=gen.RPN_STDS).numpy()
                  - reference_midpoint_encode(c["anchors"], c["gts"], stds=gen.RPN_STDS)).max() <= TORCH_F64
    c = gen.obb_encode_case(N)
    assert np.abs(obb2obb_encode_torch(c["proposals"].double(), c["gts"].double(), stds=gen.RCNN_STDS).numpy()
                  - reference_obb2obb_encode(c["proposals"], c["gts"], stds=gen.RCNN_STDS)).max() <= TORCH_F64
    cases = [(gen.midpoint_decode_case(N), "anchors", midpoint_decode_torch, reference_midpoint_decode, gen.RPN_STDS),
             (gen.obb_decode_case(N), "proposals", obb2obb_decode_torch, reference_obb2obb_decode, gen.RCNN_STDS)]
    if N == 257:
        cases.append((gen.obb_decode_case(N, 15), "proposals", obb2obb_decode_torch, reference_obb2obb_decode, gen.RCNN_STDS))
    for c, key, stock, oracle, stds in cases:
        ref = oracle(c[key], c["deltas"], stds=stds)
        got = stock(c[key].double(), c["deltas"].double(), stds=stds)
        assert tuple(got.shape) == ref.shape
        canonical(ref)
        canonical(got)
        assert corner_distance(as_rows(got), as_rows(ref)).max() <= TORCH_F64
        rows = gen.param_rows(ref).reshape(-1)
        assert rows.mean() >= 0.9, f"{rows.mean():.3f} of the rows are compared on their parameters"
        assert np.abs(as_rows(got)[rows] - as_rows(ref)[rows]).max() <= TORCH_F64


def test_generated_cases_meet_the_conditions():
    """conditions (a), (b), (c) of gen_coder_golden's docstring on every generated case, and the special rows"""
    from lemevit_amd.detection import reference_regular_theta
    for N in gen.ROWS:
        c = gen.midpoint_encode_case(N)
        gp = gen.gaps(c["gts"].double().numpy())
        assert not ((gp > gen.GAP_LEVEL) & (gp < gen.GAP_CLEAR)).any()
        c = gen.obb_encode_case(N)
        d1 = reference_regular_theta(c["gts"][:, 4].double().numpy() - c["proposals"][:, 4].double().numpy())
        assert (np.abs(np.abs(d1) - math.pi / 4) >= gen.D1_MARGIN).all()
        c = gen.midpoint_decode_case(N)
        assert (gen.first_vertices_apart(c["anchors"].double().numpy(), c["deltas"].double().numpy(), gen.RPN_STDS) >= gen.VERTEX_MARGIN).all()
        if N >= gen.SPECIAL_FROM:
            for g in (gen.midpoint_encode_case(N)["gts"], gen.obb_encode_case(N)["gts"], gen.obb_decode_case(N)["proposals"]):
                assert float(g[N - 1, 4]) == 0.0 and float(g[N - 2, 4]) == float(np.float32(-math.pi / 2)) and float(g[N - 3, 2]) == float(g[N - 3, 3])
            d = gen.midpoint_decode_case(N)["deltas"]
            assert not d[N - 4].any() and float(d[N - 5, 2]) > gen.CLIP and float(d[N - 6, 3]) < -gen.CLIP
            assert float(d[N - 7, 4]) * 0.5 > 0.5 and float(d[N - 8, 5]) * 0.5 < -0.5
            d = gen.obb_decode_case(N)["deltas"]
            assert not d[N - 4].any() and float(d[N - 5, 2]) * 0.2 > gen.CLIP and float(d[N - 6, 3]) * 0.2 < -gen.CLIP
    for kind in gen.KINDS:
        c = gen.assigned_case(kind, 3, 257, 7)
        assert c["counts"].tolist() == [7, 5, 3] and torch.isnan(c["gts"][1, 5:]).all() and not torch.isnan(c["gts"][1, :5]).any()
        assert set(range(-1, 9)) <= set(c["gt_inds"][0].tolist())
    ch = gen.chain_case()
    assert (gen.gaps(ch["gts"].double().numpy()) >= gen.GAP_CLEAR).all()


@pytest.mark.parametrize("kind", gen.KINDS)
def test_reference_encode_assigned(kind):
    """gt_inds of -1, 0 and count + 1 and rows that are not sampled are zero rows with weight 0; live rows are the aligned oracle on the gathered pairs; ground-truth
    rows at and past the count (NaN in the case) reach nothing; the torch formulation (nonzero, gathers, scatters) in float64 equals it"""
    enc, stock, stds = ((reference_midpoint_encode, midpoint_encode_torch, gen.RPN_STDS) if kind == "midpoint" else
                        (reference_obb2obb_encode, obb2obb_encode_torch, gen.RCNN_STDS))
    means = (0.0,) * len(stds)
    for B, G in ((1, 0), (1, 1), (3, 7)):
        c = gen.assigned_case(kind, B, 257, G)
        for sampled in (None, c["sampled"]):
            t, w = reference_encode_assigned(kind, c["boxes"], c["gts"], c["gt_inds"], means, stds, c["counts"], sampled)
            assert t.shape == (B, 257, len(stds)) and w.shape == (B, 257) and not np.isnan(t).any()
            for b in range(B):
                ind, cnt = c["gt_inds"][b].numpy(), int(c["counts"][b])
                live = (ind >= 1) & (ind <= cnt) & (np.ones(257, dtype=bool) if sampled is None else sampled[b].numpy())
                assert (w[b] == live).all() and not t[b][~live].any()
                assert not live[(ind == -1) | (ind == 0) | (ind == cnt + 1)].any()
                if live.any():
                    want = enc(c["boxes"][b][live], c["gts"][b][ind[live] - 1], means, stds)
                    assert np.array_equal(t[b][live], want) and np.abs(want).max() > 0
            tt, tw = encode_assigned_torch(stock, c["boxes"].double(), c["gts"].double(), c["gt_inds"], means, stds, c["counts"], sampled)
            assert np.abs(tt.numpy() - t).max() <= TORCH_F64 and np.array_equal(tw.numpy(), w)
    # shared boxes [N, k]
    c = gen.assigned_case(kind, 3, 257, 7)
    t0, _ = reference_encode_assigned(kind, c["boxes"][0], c["gts"], c["gt_inds"], means, stds, c["counts"])
    t1, _ = reference_encode_assigned(kind, c["boxes"][0][None].repeat(3, 1, 1), c["gts"], c["gt_inds"], means, stds, c["counts"])
    assert np.array_equal(t0, t1)


def test_decode_map_torch_order():
    """the map form's row order: row r = (h W + w) A + a has delta d at channel a D + d"""
    A, H, W, D = 3, 5, 7, 6
    m = torch.arange(A * D * H * W, dtype=torch.float64).reshape(A * D, H, W)
    rows = m.permute(1, 2, 0).reshape(-1, D)
    for r in (0, 1, 17, A * H * W - 1):
        a, pos = r % A, r // A
        h, w = pos // W, pos % W
        assert rows[r].tolist() == [float(m[a * D + d, h, w]) for d in range(D)]
    c = gen.midpoint_decode_case(257)
    idx = torch.tensor([5, 0, 104])
    mp = c["deltas"][:105].double().reshape(5, 7, 18).permute(2, 0, 1)
    got = decode_map_torch(midpoint_decode_torch, c["anchors"][:105].double(), mp, idx, (0.0,) * 6, gen.RPN_STDS)
    assert torch.equal(got, midpoint_decode_torch(c["anchors"][:105].double()[idx], c["deltas"][:105].double()[idx], stds=gen.RPN_STDS))


def test_arguments_without_gpu():
    """the surface, the argument checks of the classes and of ops.box_encode / box_decode / box_decode_map that need no launch, and empty inputs"""
    import lemevit_amd
    from lemevit_amd import _lib, ops
    from lemevit_amd import detection
    for name in ("MidpointOffsetCoder", "OBB2OBBDeltaXYWHTCoder", "reference_midpoint_encode", "reference_midpoint_decode", "reference_obb2obb_encode",
                 "reference_obb2obb_decode", "reference_encode_assigned", "reference_obb_corners", "midpoint_encode_torch", "midpoint_decode_torch",
                 "obb2obb_encode_torch", "obb2obb_decode_torch"):
        assert hasattr(detection, name), name
    assert "target encoding" not in detection.__doc__ and "MidpointOffsetCoder(target_stds" in detection.__doc__
    rpn, rcnn = MidpointOffsetCoder(target_stds=[1, 1, 1, 1, 0.5, 0.5]), OBB2OBBDeltaXYWHTCoder(target_means=(0,) * 5, target_stds=[0.1, 0.1, 0.2, 0.2, 0.1])
    assert rpn.stds == gen.RPN_STDS and rcnn.stds == gen.RCNN_STDS and MidpointOffsetCoder().stds == gen.RPN_STDS and OBB2OBBDeltaXYWHTCoder().stds == (1.0,) * 5
    assert (rpn.k, rpn.D, rcnn.k, rcnn.D) == (4, 6, 5, 5) and "MidpointOffsetCoder" in repr(rpn)
    with pytest.raises(ValueError, match="6 means"):
        MidpointOffsetCoder(target_stds=(1, 1, 1, 1, 1))
    with pytest.raises(ValueError, match="NaN"):
        OBB2OBBDeltaXYWHTCoder(target_means=(0, 0, 0, 0, float("nan")))
    # empty inputs: no launch, no GPU
    assert tuple(rpn.encode(torch.zeros(0, 4), torch.zeros(0, 5)).shape) == (0, 6) and tuple(rcnn.encode(torch.zeros(0, 5), torch.zeros(0, 5)).shape) == (0, 5)
    assert tuple(rpn.decode(torch.zeros(0, 4), torch.zeros(0, 6)).shape) == (0, 5) and tuple(rcnn.decode(torch.zeros(0, 5), torch.zeros(0, 75), max_shape=(8, 8)).shape) == (0, 75)
    t, w = rcnn.encode_assigned(torch.zeros(2, 0, 5), torch.zeros(2, 3, 5), torch.zeros(2, 0, dtype=torch.int64))
    assert tuple(t.shape) == (2, 0, 5) and tuple(w.shape) == (2, 0)
    assert tuple(rpn.decode_map(torch.zeros(105, 4), torch.zeros(18, 5, 7), torch.zeros(0, dtype=torch.int64)).shape) == (0, 5)
    # the classes' checks
    with pytest.raises(ValueError, match="4 columns"):
        rpn.encode(torch.zeros(3, 5), torch.zeros(3, 5))
    with pytest.raises(ValueError, match="one of each per row"):
        rpn.encode(torch.zeros(3, 4), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="5 C"):
        rcnn.decode(torch.zeros(3, 5), torch.zeros(3, 6))
    with pytest.raises(ValueError, match="gt_inds"):
        rcnn.encode_assigned(torch.zeros(4, 5), torch.zeros(2, 3, 5), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="bbox_pred"):
        rpn.decode_map(torch.zeros(105, 4), torch.zeros(17, 5, 7), torch.zeros(2, dtype=torch.int64))
    # no CPU path for non-empty inputs
    with pytest.raises(RuntimeError, match="GPU"):
        rpn.encode(torch.zeros(3, 4), torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="GPU"):
        rcnn.decode(torch.zeros(3, 5), torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="GPU"):
        rpn.decode_map(torch.zeros(105, 4), torch.zeros(18, 5, 7), torch.zeros(2, dtype=torch.int64))
    # the operators' checks (before any pointer is taken)
    m6, s6 = (0.0,) * 6, gen.RPN_STDS
    with pytest.raises(ValueError, match="kind"):
        ops.box_encode("xywh", torch.zeros(3, 4), torch.zeros(1, 3, 5), m6, s6)
    with pytest.raises(ValueError, match="aligned form"):
        ops.box_encode("midpoint", torch.zeros(3, 4), torch.zeros(1, 2, 5), m6, s6)
    with pytest.raises(ValueError, match="boxes: float32"):
        ops.box_encode("midpoint", torch.zeros(3, 5), torch.zeros(1, 3, 5), m6, s6)
    with pytest.raises(ValueError, match="gts: float32"):
        ops.box_encode("midpoint", torch.zeros(3, 4), torch.zeros(1, 3, 4), m6, s6)
    with pytest.raises(ValueError, match="wh_ratio_clip"):
        ops.box_decode("midpoint", torch.zeros(3, 4), torch.zeros(3, 6), m6, s6, wh_ratio_clip=0.0)
    with pytest.raises(ValueError, match="at most 128"):
        ops.box_decode("obb2obb", torch.zeros(3, 5), torch.zeros(3, 5 * 129), (0.0,) * 5, gen.RCNN_STDS)
    with pytest.raises(ValueError, match=r"boxes: \[105, 4\]"):
        ops.box_decode_map("midpoint", torch.zeros(2, 4), torch.zeros(18, 5, 7), torch.zeros(2, dtype=torch.int64), m6, s6)
    with pytest.raises(ValueError, match=r"boxes: \[2, 4\]"):
        ops.box_decode_map("midpoint", torch.zeros(105, 4), torch.zeros(18, 5, 7), torch.zeros(2, dtype=torch.int64), m6, s6, gathered=True)
    with pytest.raises(TypeError, match="index"):
        ops.box_decode_map("midpoint", torch.zeros(105, 4), torch.zeros(18, 5, 7), torch.zeros(2, dtype=torch.int32), m6, s6)
    assert (_lib.CODER_MIDPOINT, _lib.CODER_OBB2OBB, _lib.CODER_MAX_SETS) == (0, 1, 128)
    assert lemevit_amd.detection is detection


def test_symbols():
    """the three entry points are declared in include/lemevit_hip.h, exported, listed in _lib.SIGNATURES; the header states the constants; the ABI version stays 14"""
    from lemevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lmv_box_encode", "lmv_box_decode", "lmv_box_decode_map"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    for name, value in (("LMV_CODER_MIDPOINT", _lib.CODER_MIDPOINT), ("LMV_CODER_OBB2OBB", _lib.CODER_OBB2OBB), ("LMV_CODER_MAX_SETS", _lib.CODER_MAX_SETS)):
        assert int(re.search(r"#define " + name + r" (\d+)", src).group(1)) == value
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    assert "coder.hip" in open(os.path.join(ROOT, "lemevit_amd", "csrc", "Makefile")).read()


def test_refusals_without_gpu():
    """Argument validation happens before any launch: LMV_ERR_SHAPE and a message that starts with the entry point's name"""
    from lemevit_amd._lib import lib
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    F = ctypes.c_float
    m6, s6, m5, s5 = (F * 6)(), (F * 6)(1, 1, 1, 1, 0.5, 0.5), (F * 5)(), (F * 5)(1, 1, 1, 1, 1)
    nan6 = (F * 6)(0, 0, float("nan"), 0, 0, 0)

    def enc(kind=0, boxes=p, bs=4, bb=0, N=8, gts=p, gs=5, B=1, Gmax=8, counts=None, inds=p, sampled=None, means=m6, stds=s6, targets=p, weights=p):
        return lib.lmv_box_encode(kind, boxes, bs, bb, N, gts, gs, B, Gmax, counts, inds, sampled, means, stds, targets, weights, None)

    def dec(kind=1, boxes=p, bs=5, deltas=p, ds=5, N=8, C=1, means=m5, stds=s5, clip=0.016, out=p):
        return lib.lmv_box_decode(kind, boxes, bs, deltas, ds, N, C, means, stds, clip, out, None)

    def dmap(kind=0, boxes=p, bs=4, gathered=0, mp=p, A=3, H=5, W=7, sc=35, sh=7, sw=1, index=p, K=8, means=m6, stds=s6, clip=0.016, out=p):
        return lib.lmv_box_decode_map(kind, boxes, bs, gathered, mp, A, H, W, sc, sh, sw, index, K, means, stds, clip, out, None)

    def msg():
        return lib.lmv_last_error()

    assert enc(kind=2) == -1 and msg().startswith(b"box_encode") and b"unknown kind" in msg()
    assert enc(B=0) == -1 and b"images" in msg() and enc(B=4097) == -1
    assert enc(N=-1) == -1 and b"negative" in msg() and enc(N=(1 << 20) + 1, Gmax=(1 << 20) + 1) == -1 and b"at most" in msg()
    assert enc(bs=3) == -1 and b"row strides" in msg() and enc(kind=1, bs=4) == -1 and enc(gs=4) == -1
    assert enc(bb=-1) == -1 and b"batch stride" in msg()
    assert enc(inds=None, Gmax=7) == -1 and b"aligned form" in msg()
    assert enc(means=None) == -1 and b"null means" in msg() and enc(stds=nan6) == -1 and b"NaN" in msg()
    assert enc(boxes=None) == -1 and b"null boxes" in msg() and enc(gts=None) == -1 and b"null ground truths" in msg()
    assert enc(targets=None) == -1 and enc(weights=None) == -1 and b"null targets" in msg()
    assert enc(boxes=p + 2) == -1 and b"misaligned" in msg() and enc(inds=p + 4) == -1 and b"misaligned" in msg()
    assert enc(N=0, Gmax=0, boxes=None, gts=None, targets=None, weights=None) == 0          # nothing to do: no launch

    assert dec(kind=-1) == -1 and msg().startswith(b"box_decode:") and dec(N=-1) == -1 and dec(N=(1 << 20) + 1) == -1
    assert dec(C=0) == -1 and b"delta sets" in msg() and dec(C=129, ds=5 * 129) == -1 and b"delta sets" in msg()
    assert dec(bs=4) == -1 and b"box row stride" in msg() and dec(C=15, ds=74) == -1 and b"delta row stride" in msg()
    assert dec(clip=0.0) == -1 and b"wh_ratio_clip" in msg() and dec(clip=float("nan")) == -1 and dec(clip=float("inf")) == -1 and dec(clip=-1.0) == -1
    assert dec(means=None) == -1 and dec(boxes=None) == -1 and b"null boxes" in msg() and dec(out=None) == -1 and dec(deltas=p + 1) == -1 and b"misaligned" in msg()
    assert dec(N=0, boxes=None, deltas=None, out=None) == 0

    assert dmap(kind=5) == -1 and msg().startswith(b"box_decode_map") and dmap(K=-1) == -1 and dmap(K=(1 << 20) + 1) == -1
    assert dmap(A=0) == -1 and b"anchors" in msg() and dmap(H=0) == -1 and dmap(W=0) == -1
    assert dmap(A=1 << 11, H=1 << 10, W=1 << 10) == -1 and b"2^31" in msg()
    assert dmap(gathered=2) == -1 and b"gathered" in msg() and dmap(bs=3) == -1
    assert dmap(index=None) == -1 and b"null" in msg() and dmap(mp=None) == -1 and dmap(index=p + 4) == -1 and b"misaligned" in msg()
    assert dmap(stds=nan6) == -1 and dmap(clip=0.0) == -1
    assert dmap(K=0, boxes=None, mp=None, index=None, out=None) == 0
