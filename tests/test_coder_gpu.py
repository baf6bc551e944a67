"""The box coders on the GPU (csrc/coder.hip; lemevit_amd/detection.py: MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder).

Against the float64 oracle, the tolerance is not fixed in advance: on the same inputs the error E_torch of the stock-PyTorch formulation in fp32 on the GPU is
measured against the oracle, and the kernel's error may be at most 2 E_torch plus one fp32 ulp of the case's largest coordinate (the largest magnitude among the
input boxes and the oracle's corners).  The two sides use different sincos / exp / log / atan2 implementations and neither is privileged.  Encodes are compared on
the deltas; decodes on the corners of every row (the maximum over the corners of one box of the distance to the nearest corner of the other, both ways) and on the
five parameters of the rows whose canonical form is stable (gen_coder_golden.param_rows: at least 90 % of every case, tests/test_coder_cpu.py).

Measured on an MI355X (``pytest -s`` prints every figure), the largest over the cases of gen_coder_golden.ROWS, kernel / stock PyTorch fp32; the two sides agree
to the third digit everywhere:
    encode, deltas                        midpoint 1.3e-05 / 1.3e-05, OBB2OBB 4.9e-06 / 4.9e-06; gathering form (B x N x G cases) 3.0e-6 / 3.0e-6 (midpoint), 3.1e-6 / 3.1e-6 (OBB2OBB)
    decode, corners (pixels)              midpoint 4.8e-3 / 4.8e-3, and 8.1e-2 / 8.1e-2 on the N = 255 case, whose dw-above-the-clip row is a box 60 000 pixels
                                          wide (1.3e-6 of its size); OBB2OBB 1.8e-3 / 1.8e-3; C = 15: 6.2e-4 / 6.2e-4
    decode, five parameters               midpoint 4.8e-3 / 4.8e-3 (8.1e-2 / 8.1e-2 at N = 255); OBB2OBB 1.1e-3 / 1.1e-3
    round trip, corners (pixels)          midpoint 8.6e-4 / 8.6e-4 on 996 rows; OBB2OBB 4.5e-5 / 4.5e-5 on 1000 rows
    chain                                 73 live anchors, smallest IoU of a decoded target with its ground truth 0.999994

Exact (bit-for-bit) properties need no tolerance: encode_assigned equals encode on the gathered rows and is exactly +0.0 with weight 0 elsewhere; a batch equals
its single images; decode_map equals decode on the permuted copy (contiguous, permuted, channel-sliced maps, both ``gathered`` settings, indices out of range give
zero rows); a class-specific decode equals the single decodes; row-strided operands equal contiguous ones; two calls agree.  encode_assigned and decode_map with
their outputs supplied allocate nothing and replay from a captured graph.  The end-to-end chain runs the configs' RPN settings on small inputs.
"""
import functools
import math

import numpy as np
import pytest
import torch

import gen_coder_golden as gen
from lemevit_amd import ops
from lemevit_amd.detection import (MaxIoUAssigner, MidpointOffsetCoder, OBB2OBBDeltaXYWHTCoder, decode_map_torch, encode_assigned_torch, midpoint_decode_torch,
                                   midpoint_encode_torch, obb2obb_decode_torch, obb2obb_encode_torch, obb_overlaps, reference_encode_assigned,
                                   reference_midpoint_decode, reference_midpoint_encode, reference_obb2obb_decode, reference_obb2obb_encode, reference_obb_corners)
from test_coder_cpu import as_rows, corner_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"

CODERS = {"midpoint": MidpointOffsetCoder(target_stds=gen.RPN_STDS), "obb2obb": OBB2OBBDeltaXYWHTCoder(target_stds=gen.RCNN_STDS)}
STOCK = {"midpoint": (midpoint_encode_torch, midpoint_decode_torch), "obb2obb": (obb2obb_encode_torch, obb2obb_decode_torch)}
ORACLE = {"midpoint": (reference_midpoint_encode, reference_midpoint_decode), "obb2obb": (reference_obb2obb_encode, reference_obb2obb_decode)}
STDS = {"midpoint": gen.RPN_STDS, "obb2obb": gen.RCNN_STDS}


def ulp(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def bound(e_torch: float, largest: float) -> float:
    return 2.0 * e_torch + ulp(largest)


def strided(t):
    """the same rows as the first columns of a [..., k + 1] tensor: read in place with a row stride of k + 1"""
    d = torch.full(t.shape[:-1] + (t.shape[-1] + 1,), 0.5, device=t.device)
    d[..., :-1] = t
    return d[..., :-1]


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b) -> bool:
    """bit for bit (NaN == NaN, +0.0 != -0.0)"""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def encode_inputs(kind, N):
    c = gen.midpoint_encode_case(N) if kind == "midpoint" else gen.obb_encode_case(N)
    return c["anchors" if kind == "midpoint" else "proposals"], c["gts"], c


def decode_inputs(kind, N, C=1):
    c = gen.midpoint_decode_case(N) if kind == "midpoint" else gen.obb_decode_case(N, C)
    return c["anchors" if kind == "midpoint" else "proposals"], c["deltas"]


def largest_coordinate(boxes, obbs) -> float:
    """the case's largest coordinate: over the input boxes' position columns and the corners of rows (cx, cy, w, h, theta)"""
    b = boxes.double().numpy()
    m = float(np.abs(b[:, :4] if b.shape[1] == 4 else b[:, :2]).max())
    return max(m, float(np.abs(reference_obb_corners(as_rows(obbs))).max()))


# ---- against the float64 oracle ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", gen.ROWS)
@pytest.mark.parametrize("kind", gen.KINDS)
def test_encode_against_oracle(kind, N):
    """the deltas of every row within 2 E_torch + 1 ulp of the oracle's; every element written (NaN prefill), weights all 1; row-strided operands and a second call
    give the same bits"""
    boxes, gts, _ = encode_inputs(kind, N)
    coder, stds = CODERS[kind], STDS[kind]
    ref = ORACLE[kind][0](boxes, gts, stds=stds)
    gb, gg = boxes.to(DEV), gts.to(DEV)
    e_torch = float(np.abs(STOCK[kind][0](gb, gg, stds=stds).double().cpu().numpy() - ref).max())
    t = torch.full((1, N, coder.D), float("nan"), device=DEV)
    w = torch.full((1, N), float("nan"), device=DEV)
    out = ops.box_encode(kind, gb, gg[None], coder.means, coder.stds, targets=t, weights=w)
    assert out[0] is t and out[1] is w and not torch.isnan(t).any() and bool((w == 1).all())
    err = float(np.abs(t[0].double().cpu().numpy() - ref).max())
    lim = bound(e_torch, largest_coordinate(boxes, gts))
    print(f"    encode {kind} N {N}: E_torch {e_torch:.3e}, kernel {err:.3e}, bound {lim:.3e}")
    assert err <= lim
    got = coder.encode(gb, gg)
    assert same(got, t[0]) and same(coder.encode(gb, gg), got), "upstream's signature; a second call"
    assert same(coder.encode(strided(gb), strided(gg)), got), "row strides k + 1 and 6"


@pytest.mark.parametrize("N", gen.ROWS)
@pytest.mark.parametrize("kind", gen.KINDS)
def test_decode_against_oracle(kind, N):
    """the corners of every row, and the five parameters of the rows whose canonical form is stable, within 2 E_torch + 1 ulp of the oracle's; every decoded row is
    canonical; every element written; row-strided operands and a second call give the same bits"""
    boxes, deltas = decode_inputs(kind, N)
    coder, stds = CODERS[kind], STDS[kind]
    ref = ORACLE[kind][1](boxes, deltas, stds=stds)
    gb, gd = boxes.to(DEV), deltas.to(DEV)
    stock = STOCK[kind][1](gb, gd, stds=stds).double().cpu().numpy()
    out = torch.full((N, 5), float("nan"), device=DEV)
    assert ops.box_decode(kind, gb, gd, coder.means, coder.stds, out=out) is out and not torch.isnan(out).any()
    got = out.double().cpu().numpy()
    half_pi = float(np.float32(math.pi / 2))          # (fp32: the interval's ends are the float32 values of -+pi/2; the upper one can be reached only by rounding)
    assert (got[:, 2] >= got[:, 3]).all() and (got[:, 4] >= -half_pi).all() and (got[:, 4] <= half_pi).all()
    big = largest_coordinate(boxes, ref)
    e_torch, err = float(corner_distance(stock, ref).max()), float(corner_distance(got, ref).max())
    print(f"    decode {kind} N {N}: corners: E_torch {e_torch:.3e}, kernel {err:.3e}, bound {bound(e_torch, big):.3e}")
    assert err <= bound(e_torch, big)
    rows = gen.param_rows(ref).reshape(-1)
    assert rows.mean() >= 0.9
    p_torch, p_err = float(np.abs(stock - ref)[rows].max()), float(np.abs(got - ref)[rows].max())
    print(f"    decode {kind} N {N}: parameters of {int(rows.sum())} rows: E_torch {p_torch:.3e}, kernel {p_err:.3e}, bound {bound(p_torch, big):.3e}")
    assert p_err <= bound(p_torch, big)
    assert same(coder.decode(gb, gd), out) and same(coder.decode(gb, gd, max_shape=(1024, 1024)), out), "upstream's signature; max_shape is not applied"
    assert same(coder.decode(strided(gb), strided(gd)), out), "row strides k + 1 and D + 1"


@pytest.mark.parametrize("kind", gen.KINDS)
def test_round_trip(kind):
    """decode(encode(g)) == g as corner sets on the kernels: within 2 E_torch + 1 ulp, E_torch the round trip of the stock formulation in fp32 (midpoint: on the rows
    whose gaps of condition (a) are at least 0.11)"""
    boxes, gts, c = encode_inputs(kind, 1000)
    rows = c["clear"] if kind == "midpoint" else np.ones(1000, dtype=bool)
    coder, stds = CODERS[kind], STDS[kind]
    gb, gg = boxes.to(DEV), gts.to(DEV)
    got = coder.decode(gb, coder.encode(gb, gg)).double().cpu().numpy()
    stock = STOCK[kind][1](gb, STOCK[kind][0](gb, gg, stds=stds), stds=stds).double().cpu().numpy()
    g = gts.double().numpy()
    e_torch, err = float(corner_distance(stock, g)[rows].max()), float(corner_distance(got, g)[rows].max())
    lim = bound(e_torch, largest_coordinate(boxes, g))
    print(f"    round trip {kind}: E_torch {e_torch:.3e} px, kernel {err:.3e} px, bound {lim:.3e} on {int(rows.sum())} rows")
    assert err <= lim


def test_hand_cases():
    """the two hand cases of include/lemevit_hip.h, on the kernel: the float64 values within a few fp32 roundings of the coordinates; decoding gives the ground truth back"""
    a = torch.tensor([[40.0, 30.0, 60.0, 50.0]] * 2, device=DEV)
    g = torch.tensor([[50.0, 40.0, 20.0, 10.0, 0.0], [50.0, 40.0, 20.0, 10.0, math.pi / 6]], device=DEV)
    e = CODERS["midpoint"].encode(a, g)
    want = torch.tensor([[0, 0, 0, -0.6931472, 1, 1], [0, 0, 0.10977363, -0.06933646, 0.55198152, -0.07179677]])
    tol = 8 * ulp(60.0)          # a few roundings at the magnitude of the coordinates (60); a delta divides them by a side of at least 10 and by a std of 0.5
    assert float((e.cpu() - want).abs().max()) <= tol / 10 / 0.5
    back = CODERS["midpoint"].decode(a, e).double().cpu().numpy()
    assert corner_distance(back, g.double().cpu().numpy()).max() <= tol


# ---- exact properties --------------------------------------------------------------------------------------------------------------------------------------------
ASSIGNED = [(B, 257, G) for B in gen.BATCHES for G in gen.GMAX] + [(3, n, 7) for n in gen.ROWS if n != 257] + [(1, 1, 1), (1, 64, 1)]


@pytest.mark.parametrize("B,N,G", ASSIGNED, ids=[f"{b}x{n}x{g}" for b, n, g in ASSIGNED])
@pytest.mark.parametrize("kind", gen.KINDS)
def test_encode_assigned(kind, B, N, G):
    """encode_assigned equals encode on the rows gathered by gt_inds, bit for bit; rows with gt_inds of -1, 0, count + 1 and rows that are not sampled are exactly
    +0.0 with weight 0; ground-truth rows past the count hold NaN and reach nothing; a batch equals its single images; shared boxes equal repeated ones; row strides;
    a second call; and the whole result is within 2 E_torch + 1 ulp of the oracle's"""
    c = gen.assigned_case(kind, B, N, G)
    coder, stds = CODERS[kind], STDS[kind]
    boxes, gts, counts, inds, sampled = (c[k].to(DEV) for k in ("boxes", "gts", "counts", "gt_inds", "sampled"))
    for smp in (None, sampled):
        t = torch.full((B, N, coder.D), float("nan"), device=DEV)
        w = torch.full((B, N), float("nan"), device=DEV)
        out = coder.encode_assigned(boxes, gts, inds, counts, smp, targets=t, weights=w)
        assert out[0] is t and out[1] is w and not torch.isnan(t).any() and not torch.isnan(w).any()
        live = (inds >= 1) & (inds <= counts[:, None].to(torch.int64))
        if smp is not None:
            live &= smp
        assert torch.equal(w, live.float()), "weights"
        assert not bits(t[~live]).any(), "a row that is not live is exactly +0.0"
        for b in range(B):
            if bool(live[b].any()):
                rows = live[b].nonzero().squeeze(1)
                assert same(t[b][rows], coder.encode(boxes[b][rows], gts[b][inds[b][rows] - 1])), "encode on the gathered rows"
            one = coder.encode_assigned(boxes[b], gts[b:b + 1], inds[b:b + 1], counts[b:b + 1], None if smp is None else smp[b:b + 1])
            assert same(one[0][0], t[b]) and same(one[1][0], w[b]), "a batch equals its single images"
        again = coder.encode_assigned(strided(boxes), strided(gts), inds, counts, smp)
        assert same(again[0], t) and same(again[1], w), "row strides k + 1 and 6; a second call"
        ref_t, ref_w = reference_encode_assigned(kind, c["boxes"], c["gts"], c["gt_inds"], coder.means, stds, c["counts"], None if smp is None else c["sampled"])
        st, sw = encode_assigned_torch(STOCK[kind][0], boxes, gts, inds, coder.means, stds, counts, smp)
        e_torch, err = float(np.abs(st.double().cpu().numpy() - ref_t).max()), float(np.abs(t.double().cpu().numpy() - ref_t).max())
        assert np.array_equal(w.cpu().numpy(), ref_w) and np.array_equal(sw.cpu().numpy(), ref_w)
        big = float(c["boxes"][..., :2].abs().max())
        print(f"    encode_assigned {kind} {B} x {N} x {G} sampled={smp is not None}: E_torch {e_torch:.3e}, kernel {err:.3e}, bound {bound(e_torch, big):.3e}")
        assert err <= bound(e_torch, big)
    shared = coder.encode_assigned(boxes[0], gts, inds, counts)
    rep = coder.encode_assigned(boxes[0][None].repeat(B, 1, 1), gts, inds, counts)
    assert same(shared[0], rep[0]) and same(shared[1], rep[1]), "shared boxes [N, k]"
    no_counts = coder.encode_assigned(boxes[:1], torch.nan_to_num(gts[:1]), inds[:1])          # image 0 has all its rows: count = Gmax
    full = coder.encode_assigned(boxes[:1], gts[:1], inds[:1], counts[:1])
    assert same(no_counts[0], full[0]) and same(no_counts[1], full[1]), "gt_counts=None is Gmax"


MAPS = [(3, 5, 7), (3, 16, 16)]


@pytest.mark.parametrize("K", gen.ROWS)
@pytest.mark.parametrize("A,H,W", MAPS, ids=[f"{a}x{h}x{w}" for a, h, w in MAPS])
@pytest.mark.parametrize("kind", gen.KINDS)
def test_decode_map(kind, A, H, W, K):
    """decode_map reads the regression map in place: equal, bit for bit, to decode on the rows of permute(1, 2, 0).reshape(-1, D) -- for a contiguous map, a permuted
    view, a channel slice of a larger tensor and one image of a batch; boxes gathered by the index or already gathered; indices out of range give zero rows"""
    coder, stds = CODERS[kind], STDS[kind]
    R, D = A * H * W, coder.D
    boxes, deltas = (t[:R].to(DEV) for t in decode_inputs(kind, 1000))
    view = deltas.reshape(H, W, A * D).permute(2, 0, 1)          # [A D, H, W] with strides (1, W A D, A D)
    dense = view.contiguous()
    big = torch.full((A * D + 5, H, W), float("nan"), device=DEV)
    big[3:3 + A * D] = dense
    batch = torch.full((2, A * D, H, W), float("nan"), device=DEV)
    batch[1] = dense
    assert same(dense.permute(1, 2, 0).reshape(-1, D), deltas)
    index = (torch.from_numpy(gen.det_uniform(K, 0x1DE + K + R)).to(DEV) * 0.5 + 0.5).mul(R).long().clamp(0, R - 1)
    if K >= 63:
        index[5], index[K - 1], index[K // 2], index[7], index[8] = -1, R, 1 << 40, 0, R - 1
    valid = (index >= 0) & (index < R)
    safe = index.clamp(0, R - 1)
    want = coder.decode(boxes[safe], deltas[safe]) * valid[:, None]
    want[~valid] = 0.0
    for name, mp in (("contiguous", dense), ("permuted view", view), ("channel slice", big[3:3 + A * D]), ("image of a batch", batch[1])):
        out = torch.full((K, 5), float("nan"), device=DEV)
        assert coder.decode_map(boxes, mp, index, out=out) is out
        assert same(out, want), name
        assert same(coder.decode_map(boxes[safe], mp, index, gathered=True), want), name + ", gathered"
        assert same(coder.decode_map(strided(boxes), mp, index), want), name + ", row stride k + 1"
    assert not bits(out[~valid]).any()
    stock = decode_map_torch(STOCK[kind][1], boxes, dense, safe, coder.means, stds)
    assert tuple(stock.shape) == (K, 5)


def test_class_specific_decode():
    """C = 15 delta sets per row (the R-CNN head's class-wise regression): [N, 75] -> [N, 75], equal bit for bit to 15 single decodes on the column slices, and within
    the oracle's tolerance"""
    N, C = 257, 15
    coder, stds = CODERS["obb2obb"], gen.RCNN_STDS
    boxes, deltas = decode_inputs("obb2obb", N, C)
    gb, gd = boxes.to(DEV), deltas.to(DEV)
    out = torch.full((N, 5 * C), float("nan"), device=DEV)
    assert ops.box_decode("obb2obb", gb, gd, coder.means, coder.stds, out=out) is out and not torch.isnan(out).any()
    for c in range(C):
        assert same(out[:, 5 * c:5 * c + 5], coder.decode(gb, gd[:, 5 * c:5 * c + 5])), f"set {c} (a column slice: row stride 75)"
    assert same(coder.decode(gb, gd), out)
    ref = reference_obb2obb_decode(boxes, deltas, stds=stds)
    stock = obb2obb_decode_torch(gb, gd, stds=stds)
    big = largest_coordinate(boxes, ref)
    e_torch, err = float(corner_distance(as_rows(stock), as_rows(ref)).max()), float(corner_distance(as_rows(out), as_rows(ref)).max())
    print(f"    class-specific decode: corners: E_torch {e_torch:.3e}, kernel {err:.3e}, bound {bound(e_torch, big):.3e}")
    assert err <= bound(e_torch, big)
    with pytest.raises(ValueError, match="at most 128"):
        coder.decode(gb, torch.zeros(N, 5 * 129, device=DEV))


# ---- no hidden work ----------------------------------------------------------------------------------------------------------------------------------------------
def _allocations() -> int:
    return int(torch.cuda.memory_stats()["allocation.all.allocated"])


@functools.lru_cache(maxsize=None)
def _level(kind, A=3, H=16, W=16, K=257):
    coder = CODERS[kind]
    R = A * H * W
    boxes, deltas = (t[:R].to(DEV) for t in decode_inputs(kind, 1000))
    mp = deltas.reshape(H, W, A * coder.D).permute(2, 0, 1)
    index = (torch.from_numpy(gen.det_uniform(K, 77)).to(DEV) * 0.5 + 0.5).mul(R).long().clamp(0, R - 1)
    return boxes, deltas, mp, index


@pytest.mark.parametrize("kind", gen.KINDS)
def test_no_allocation(kind):
    """encode_assigned and decode_map with their outputs supplied allocate nothing: the caching allocator's allocation count does not move over the calls"""
    coder = CODERS[kind]
    c = gen.assigned_case(kind, 3, 257, 7)
    boxes, gts, counts, inds, sampled = (c[k].to(DEV) for k in ("boxes", "gts", "counts", "gt_inds", "sampled"))
    t, w = torch.empty(3, 257, coder.D, device=DEV), torch.empty(3, 257, device=DEV)
    lb, ld, mp, index = _level(kind)
    out = torch.empty(index.shape[0], 5, device=DEV)
    want_t, want_w = coder.encode_assigned(boxes, gts, inds, counts, sampled)
    want_o = coder.decode_map(lb, mp, index)
    torch.cuda.synchronize()
    before = _allocations()
    coder.encode_assigned(boxes, gts, inds, counts, sampled, targets=t, weights=w)
    coder.decode_map(lb, mp, index, out=out)
    after = _allocations()
    torch.cuda.synchronize()
    assert after == before, f"{after - before} allocations"
    assert same(t, want_t) and same(w, want_w) and same(out, want_o)


@pytest.mark.parametrize("kind", gen.KINDS)
def test_capture(kind):
    """one eager call, then torch.cuda.graph capture with caller-supplied buffers: replays after new boxes, ground truths, indices and map contents are copied in
    equal the eager results"""
    coder = CODERS[kind]
    a, b = gen.assigned_case(kind, 3, 257, 7), gen.assigned_case(kind, 3, 257, 7, 1)
    boxes, gts, counts, inds, sampled = (a[k].to(DEV).clone() for k in ("boxes", "gts", "counts", "gt_inds", "sampled"))
    lb, ld, mp, index = (t.clone() for t in _level(kind))
    mp = ld.reshape(16, 16, 3 * coder.D).permute(2, 0, 1)          # (a view of the cloned rows)
    t, w = torch.empty(3, 257, coder.D, device=DEV), torch.empty(3, 257, device=DEV)
    out = torch.empty(index.shape[0], 5, device=DEV)
    eager_a = [x.clone() for x in coder.encode_assigned(boxes, gts, inds, counts, sampled)] + [coder.decode_map(lb, mp, index).clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        coder.encode_assigned(boxes, gts, inds, counts, sampled, targets=t, weights=w)
        coder.decode_map(lb, mp, index, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = coder.encode_assigned(boxes, gts, inds, counts, sampled, targets=t, weights=w)
        o = coder.decode_map(lb, mp, index, out=out)
    assert r[0] is t and r[1] is w and o is out
    t.fill_(float("nan")); w.fill_(float("nan")); out.fill_(float("nan"))
    graph.replay()
    assert same(t, eager_a[0]) and same(w, eager_a[1]) and same(out, eager_a[2])
    # new contents
    for dst, key in ((boxes, "boxes"), (gts, "gts"), (counts, "counts"), (inds, "gt_inds"), (sampled, "sampled")):
        dst.copy_(b[key].to(DEV))
    ld.copy_(ld.flip(0))
    lb.copy_(lb.flip(0))
    index.copy_((index * 7 + 3) % (3 * 16 * 16))
    graph.replay()
    eager_b = list(coder.encode_assigned(boxes, gts, inds, counts, sampled)) + [coder.decode_map(lb, mp, index)]
    assert same(t, eager_b[0]) and same(w, eager_b[1]) and same(out, eager_b[2])
    assert not same(t, eager_a[0]) and not same(out, eager_a[2])


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_rpn_chain():
    """257 anchors, 7 ground truths, the configs' RPN settings: MaxIoUAssigner (0.7 / 0.3 / 0.3, low-quality matches) on the anchors and the ground truths' hulls,
    encode_assigned from its gt_inds, and decoding the live rows' own targets gives boxes whose aligned rotated IoU with their ground truths is at least 1 - 1e-3"""
    c = gen.chain_case()
    anchors, gts = c["anchors"].to(DEV), c["gts"].to(DEV)
    hulls = torch.from_numpy(gen.hull(c["gts"].double().numpy()).astype(np.float32)).to(DEV)
    coder = CODERS["midpoint"]
    assigner = MaxIoUAssigner(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, gpu_assign_thr=200)
    gt_inds, _, _ = assigner.assign_batched(anchors, hulls[None])
    targets, weights = coder.encode_assigned(anchors, gts[None], gt_inds)
    live = weights[0] > 0
    assert torch.equal(live, gt_inds[0] > 0) and int(live.sum()) >= 7 and set(gt_inds[0][live].tolist()) == set(range(1, 8))
    assert not bits(targets[0][~live]).any()
    decoded = coder.decode(anchors, targets[0])
    rows = live.nonzero().squeeze(1)
    iou = obb_overlaps(decoded[rows], gts[gt_inds[0][rows] - 1], is_aligned=True)
    print(f"    chain: {int(live.sum())} live anchors, smallest IoU of a decoded target with its ground truth {float(iou.min()):.6f}")
    assert float(iou.min()) >= 1 - 1e-3
