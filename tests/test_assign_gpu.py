"""Max-IoU assignment and horizontal overlaps on the GPU (csrc/assign.hip).  Overlaps: against the float64 oracle with the bound taken from the error of the
stock-PyTorch formulation in fp32 on the same inputs (the rule of tests/test_obb_gpu.py), written once, repeatable, symmetric, aligned = diagonal.  Assignment: EQUAL
to upstream's procedure on the matrix of ops.bbox_overlaps / ops.obb_overlaps (both sides see the same fp32 values: no margin), equal to the float64 oracle on the
margin-checked cases of tests/golden/gen_assign_golden.py (tests/test_assign_cpu.py checks the margins), and the exact properties: written once, repeatable, batch =
single images, permuted ground truths, no matrix-sized allocation, capture."""
import functools
import itertools

import numpy as np
import pytest
import torch

import gen_assign_golden as gen
from gen_obb_golden import pair_case
from lemevit_amd import ops
from lemevit_amd.detection import (MaxIoUAssigner, bbox_overlaps, bbox_overlaps_torch, max_iou_assign_torch, obb_overlaps_torch, reference_bbox_overlaps,
                                   reference_max_iou_assign)
from test_assign_cpu import BATCH_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _strided(b):
    """the same rows as the first k columns of a [..., k + 1] tensor: read in place with a row stride of k + 1"""
    d = torch.full(b.shape[:-1] + (b.shape[-1] + 1,), 0.5, device=b.device)
    d[..., :-1] = b
    return d[..., :-1]


# ---- bbox_overlaps -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(N, M, aligned=False):
    """(b1, b2 on the GPU, {mode: (oracle, E_torch)}): the hulls of the rotated pair case; E_torch is the largest error of bbox_overlaps_torch in fp32 on the GPU"""
    r1, r2 = pair_case(N, M)
    b1 = torch.from_numpy(gen.hull(r1.double().numpy()).astype(np.float32)) if N else torch.zeros(0, 4)
    b2 = torch.from_numpy(gen.hull(r2.double().numpy()).astype(np.float32)) if M else torch.zeros(0, 4)
    return _with_refs(b1, b2, aligned)


def _with_refs(b1, b2, aligned):
    g1, g2 = b1.to(DEV), b2.to(DEV)
    refs = {}
    for mode in ("iou", "iof"):
        ref = reference_bbox_overlaps(b1, b2, mode, aligned)
        t = bbox_overlaps_torch(g1, g2, mode, aligned).double().cpu().numpy()
        refs[mode] = (ref, float(np.abs(t - ref).max()) if ref.size else 0.0)
    return g1, g2, refs


def _check(got, ref, e_torch, what):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), f"{what}: NaN left in a pre-filled buffer (an element was not written)"
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = max(4.0 * e_torch, 1e-6)
    print(f"    {what}: E_torch {e_torch:.3e}, kernel max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: max error {err:.3e} against E_torch {e_torch:.3e}"


OV_SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 129), (300, 7)]


@pytest.mark.parametrize("N,M", OV_SHAPES, ids=[f"{n}x{m}" for n, m in OV_SHAPES])
def test_bbox_overlaps_against_oracle(N, M):
    """iou and iof within max(4 E_torch, 1e-6) of the float64 oracle, with row strides 4 and 5; every element written (NaN prefill); two calls agree bit for bit; the
    transposed call gives the transposed iou matrix bit for bit"""
    b1, b2, refs = _pair(N, M)
    print(f"\n  {N} x {M}:")
    for mode in ("iou", "iof"):
        ref, e = refs[mode]
        out = torch.full((N, M), float("nan"), device=DEV)
        assert ops.bbox_overlaps(b1, b2, mode, out=out) is out
        _check(out, ref, e, f"{mode} stride 4")
        s1, s2 = _strided(b1), _strided(b2)
        assert N < 2 or s1.stride(0) == 5
        assert torch.equal(out, ops.bbox_overlaps(s1, s2, mode)), "row stride 5"
        assert torch.equal(out, ops.bbox_overlaps(b1, b2, mode)), "a second call"
        if mode == "iou":
            assert torch.equal(ops.bbox_overlaps(b2, b1, mode).t(), out), "the transposed call"
        assert torch.equal(bbox_overlaps(b1, b2, mode), out)          # upstream's name


@pytest.mark.parametrize("N", [1, 65, 300])
def test_bbox_overlaps_aligned(N):
    """the N aligned pairs: [N, 1], the same bound, written once, repeatable, and equal to the diagonal of the full matrix bit for bit"""
    b1, b2, refs = _pair(N, N, True)
    for mode in ("iou", "iof"):
        ref, e = refs[mode]
        out = torch.full((N, 1), float("nan"), device=DEV)
        ops.bbox_overlaps(b1, b2, mode, True, out=out)
        _check(out, ref, e, f"aligned {mode} N = {N}")
        assert torch.equal(out, ops.bbox_overlaps(_strided(b1), _strided(b2), mode, True))
        assert torch.equal(out[:, 0], ops.bbox_overlaps(b1, b2, mode).diagonal())
        assert torch.equal(bbox_overlaps(b1, b2, mode, is_aligned=True), out)


def test_bbox_overlaps_by_hand():
    """the hand-computed pairs of tests/test_assign_cpu.py: exact values where fp32 has them; non-finite boxes give all-zero rows and columns"""
    a = torch.tensor([[0.0, 0.0, 4.0, 2.0]], device=DEV)
    others = torch.tensor([[10.0, 10.0, 12.0, 12.0], [4.0, 0.0, 6.0, 2.0], [1.0, 0.5, 3.0, 1.5], [0.0, 0.0, 4.0, 2.0], [2.0, 1.0, 6.0, 3.0], [1.0, 1.0, 1.0, 1.0],
                           [float("nan"), 0.0, 4.0, 2.0], [0.0, 0.0, float("inf"), 2.0]], device=DEV)
    want = torch.tensor([0.0, 0.0, 0.25, 1.0, float(torch.tensor(2.0) / torch.tensor(14.0)), 0.0, 0.0, 0.0])          # (2 / 14: one fp32 division on both sides)
    assert torch.equal(ops.bbox_overlaps(a, others)[0].cpu(), want)
    assert torch.equal(ops.bbox_overlaps(a, others, "iof")[0].cpu(), torch.tensor([0.0, 0.0, 0.25, 1.0, 0.25, 0.0, 0.0, 0.0]))
    m = ops.bbox_overlaps(others, others)
    assert not m[6:].any() and not m[:, 6:].any() and float(m[3, 3]) == 1.0 and float(m[5, 5]) == 0.0          # zero area: 0 / 1e-6


# ---- assignment ----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind, N, G, seed=0):
    """(the generated case, boxes / gts / labels / ignore on the GPU, the fp32 matrix of the overlaps operator on the HOST, E_torch of the matrix)"""
    c = gen.assign_case(kind, N, G, seed)
    boxes, gts = c["boxes"].to(DEV), c["gts"].to(DEV)
    op, stock = (ops.obb_overlaps, obb_overlaps_torch) if kind == "rotated" else (ops.bbox_overlaps, bbox_overlaps_torch)
    if N and G:
        matrix = op(boxes, gts).cpu()
        e = float(np.abs(stock(boxes, gts).double().cpu().numpy() - c["ov"]).max())
    else:
        matrix, e = torch.zeros(N, G), 0.0
    return c, boxes, gts, c["labels"].to(DEV), c["ignore"].to(DEV), matrix, e


def _assign(boxes, gts, cfg, counts=None, labels=None, ignore=None):
    """ops.max_iou_assign into sentinel-prefilled buffers: every element must be overwritten, and a second call must agree bit for bit"""
    B, N = gts.shape[0], boxes.shape[-2]
    gi = torch.full((B, N), -7, dtype=torch.int64, device=DEV)
    mo = torch.full((B, N), float("nan"), device=DEV)
    lb = torch.full((B, N), -7, dtype=torch.int64, device=DEV) if labels is not None else None
    args = (boxes, gts, cfg["pos_iou_thr"], cfg["neg_iou_thr"], cfg["min_pos_iou"], counts, labels, ignore, cfg["match_low_quality"], cfg["gt_max_assign_all"])
    a, b, c = ops.max_iou_assign(*args, gt_inds=gi, max_overlaps=mo, labels=lb)
    assert a is gi and b is mo and c is lb
    assert not torch.isnan(mo).any() and (gi >= -1).all() and (lb is None or (lb != -7).all()), "an element was not written"
    a2, b2, c2 = ops.max_iou_assign(*args)
    assert torch.equal(a2, gi) and torch.equal(b2, mo) and (lb is None or torch.equal(c2, lb)), "a second call"
    return gi, mo, lb


SWITCHES = [dict(pos_iou_thr=0.7, neg_iou_thr=neg, min_pos_iou=mp, match_low_quality=mlq, gt_max_assign_all=all_)
            for mlq, all_, neg, mp in itertools.product((False, True), (False, True), (0.3, (0.1, 0.3)), (0.3, 0.0))]


@pytest.mark.parametrize("N,G", gen.SHAPES, ids=[f"{n}x{g}" for n, g in gen.SHAPES])
@pytest.mark.parametrize("kind", gen.KINDS)
def test_assign_equals_matrix_form(kind, N, G):
    """gt_inds, labels AND max_overlaps equal, bit for bit, upstream's procedure in stock tensor ops on the matrix of the overlaps operator -- for every combination
    of match_low_quality, gt_max_assign_all, float / tuple neg_iou_thr and min_pos_iou 0.3 / 0 (the untouched ground truth matches everything), with and without
    ignore, row strides k and k + 1.  Every case has ground truth 0's best box in the last workgroup and its duplicate in the first."""
    c, boxes, gts, labels, ignore, matrix, _ = _case(kind, N, G)
    for cfg in SWITCHES:
        for ign in (None, ignore):
            want = max_iou_assign_torch(matrix, gt_labels=labels.cpu(), ignore=None if ign is None else ign.cpu(), **cfg)
            gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=None if ign is None else ign[None])
            what = f"{kind} {N} x {G} {cfg} ignore={ign is not None}"
            assert torch.equal(gi[0].cpu(), want[0]), what
            assert torch.equal(mo[0].cpu(), want[1]), what
            assert torch.equal(lb[0].cpu(), want[2]), what
    cfg = SWITCHES[-2]
    gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=ignore[None])
    g2 = _assign(_strided(boxes), _strided(gts)[None], cfg, labels=labels[None], ignore=ignore[None])
    assert torch.equal(g2[0], gi) and torch.equal(g2[1], mo) and torch.equal(g2[2], lb), "row stride k + 1"
    if N >= 2 and G >= 1 and cfg["match_low_quality"]:          # gt 0's maximum: box 0 and box N - 1 (all), box 0 alone (lowest n)
        assert int(gi[0, 0]) == 1 and int(gi[0, N - 1]) == 1


@pytest.mark.parametrize("name", list(gen.CONFIGS))
@pytest.mark.parametrize("N,G", gen.SHAPES, ids=[f"{n}x{g}" for n, g in gen.SHAPES])
@pytest.mark.parametrize("kind", gen.KINDS)
def test_assign_against_oracle(kind, N, G, name):
    """on the margin-checked cases: gt_inds and labels equal to the float64 oracle's, max_overlaps within max(4 E_torch, 1e-6) of its row maxima; every box compared"""
    cfg = gen.CONFIGS[name]
    c, boxes, gts, labels, ignore, _, e = _case(kind, N, G)
    bound = max(4.0 * e, 1e-6)
    for ign in (None, ignore):
        want = reference_max_iou_assign(None, None, gt_labels=c["labels"], ignore=None if ign is None else c["ignore"], overlaps=c["ov"], **cfg)
        gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None], ignore=None if ign is None else ign[None])
        err = float(np.abs(mo[0].double().cpu().numpy() - want[1]).max())
        print(f"    {kind} {N} x {G} {name} ignore={ign is not None}: E_torch {e:.3e}, max_overlaps error {err:.3e}, bound {bound:.3e}")
        assert gi[0].tolist() == want[0].tolist()
        assert lb[0].tolist() == want[2].tolist()
        assert err <= bound


@pytest.mark.parametrize("N,G", BATCH_SHAPES, ids=[f"{n}x{g}" for n, g in BATCH_SHAPES])
@pytest.mark.parametrize("kind", gen.KINDS)
def test_batch_equals_single_images(kind, N, G):
    """B = 3 with per-image boxes: image 1 has gt_counts = 0, image 2 a count below Gmax with NaN in the padding rows (never read into a result).  The batched call
    equals the three single-image calls, which equal the oracle; shared boxes [N, k] equal the same boxes repeated; strides k + 1; assign (one image, upstream's
    signature) equals assign_batched"""
    bc = gen.batch_case(kind, N, G)
    boxes, gts, counts, labels, ignore = (bc[k].to(DEV) for k in ("boxes", "gts", "counts", "labels", "ignore"))
    assert torch.isnan(gts[1]).all() and torch.isnan(gts[2, int(counts[2]):]).all()
    for name, cfg in gen.CONFIGS.items():
        for ign in (None, ignore):
            gi, mo, lb = _assign(boxes, gts, cfg, counts, labels, ign)
            for b, c in enumerate(bc["cases"]):
                g = c["G"]
                s = _assign(boxes[b], gts[b:b + 1, :g], cfg, None, labels[b:b + 1, :g], None if ign is None else ign[b:b + 1])
                assert torch.equal(s[0][0], gi[b]) and torch.equal(s[1][0], mo[b]) and torch.equal(s[2][0], lb[b]), (name, b)
                want = reference_max_iou_assign(None, None, gt_labels=c["labels"], ignore=None if ign is None else c["ignore"], overlaps=c["ov"], **cfg)
                assert gi[b].tolist() == want[0].tolist() and lb[b].tolist() == want[2].tolist()
            if ign is not None:
                assert (gi[1][ign[1]] == -1).all() and (gi[1][~ign[1]] == 0).all() and (mo[1][~ign[1]] == 0).all()          # g = 0: ignored stays -1
            st = _assign(_strided(boxes), _strided(gts), cfg, counts, labels, ign)
            assert torch.equal(st[0], gi) and torch.equal(st[1], mo) and torch.equal(st[2], lb), "row stride k + 1"
    # shared boxes: [N, k] against the same boxes repeated per image
    cfg = gen.CONFIGS["rpn"]
    shared = _assign(boxes[0], gts, cfg, counts, labels, ignore)
    rep = _assign(boxes[0][None].repeat(3, 1, 1), gts, cfg, counts, labels, ignore)
    assert all(torch.equal(x, y) for x, y in zip(shared, rep))
    # the assigner: assign == assign_batched == the operator
    kw = dict(iou_calculator=dict(type="OBBOverlaps" if kind == "rotated" else "BboxOverlaps2D"))
    asg = MaxIoUAssigner(0.7, 0.3, 0.3, gpu_assign_thr=200, **kw)
    bi, bm, bl = asg.assign_batched(boxes, gts, counts, labels)
    want = _assign(boxes, gts, cfg, counts, labels, None)
    assert torch.equal(bi, want[0]) and torch.equal(bm, want[1]) and torch.equal(bl, want[2])
    for b, c in enumerate(bc["cases"]):
        r = asg.assign(boxes[b], gts[b, :c["G"]], None, labels[b, :c["G"]])
        assert r.num_gts == c["G"] and torch.equal(r.gt_inds, bi[b]) and torch.equal(r.max_overlaps, bm[b]) and torch.equal(r.labels, bl[b])
    assert asg.assign(boxes[0], gts[0]).labels is None


@pytest.mark.parametrize("kind", gen.KINDS)
def test_ignore_regions(kind):
    """ignore_iof_thr with gt_bboxes_ignore: the per-box maximum IoF against the regions (ignore_wrt_candidates: over the box's area; else over the region's) is the
    ignore mask of the fused call"""
    c, boxes, gts, labels, _, _, _ = _case(kind, 257, gen.CHUNK + 1)
    regions = gts[5:9].clone()
    op = ops.obb_overlaps if kind == "rotated" else ops.bbox_overlaps
    kw = dict(iou_calculator=dict(type="OBBOverlaps" if kind == "rotated" else "BboxOverlaps2D"))
    for wrt in (True, False):
        mask = (op(boxes, regions, "iof").max(1)[0] if wrt else op(regions, boxes, "iof").max(0)[0]) > 0.5
        assert 0 < int(mask.sum()) < 257
        r = MaxIoUAssigner(0.7, 0.3, 0.3, ignore_iof_thr=0.5, ignore_wrt_candidates=wrt, **kw).assign(boxes, gts, regions, labels)
        want = _assign(boxes, gts[None], gen.CONFIGS["rpn"], None, labels[None], mask[None])
        assert torch.equal(r.gt_inds, want[0][0]) and torch.equal(r.max_overlaps, want[1][0]) and torch.equal(r.labels, want[2][0])
        assert (r.gt_inds[mask] == -1).all() and (r.max_overlaps[mask] == -1).all()
        off = MaxIoUAssigner(0.7, 0.3, 0.3, ignore_iof_thr=-1, **kw).assign(boxes, gts, regions, labels)
        assert torch.equal(off.gt_inds, _assign(boxes, gts[None], gen.CONFIGS["rpn"], None, labels[None])[0][0])


@pytest.mark.parametrize("kind", gen.KINDS)
def test_permuted_ground_truths(kind):
    """permuting an image's ground truths leaves max_overlaps unchanged bit for bit and maps the positive gt_inds through the permutation, wherever the assignment
    does not rest on a tie (a box assigned to one of the duplicated ground-truth rows, or one that holds the maxima of several ground truths)"""
    N, G = 257, gen.CHUNK + 1
    c, boxes, gts, labels, _, matrix, _ = _case(kind, N, G)
    perm = torch.from_numpy(np.random.RandomState(5).permutation(G))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(G)
    dup = torch.tensor([(c["gts"] == c["gts"][j]).all(1).sum() > 1 for j in range(G)])
    gmax = matrix.max(0)[0]
    for cfg in (gen.CONFIGS["rcnn"], gen.CONFIGS["rpn"]):
        gi, mo, lb = _assign(boxes, gts[None], cfg, labels=labels[None])
        pi, pm, pl = _assign(boxes, gts[perm.to(DEV)][None], cfg, labels=labels[perm.to(DEV)][None])
        assert torch.equal(pm, mo)
        gi, pi = gi[0].cpu(), pi[0].cpu()
        holds = ((matrix == gmax[None]) & (gmax >= cfg["min_pos_iou"])[None]).sum(1) > 1 if cfg["match_low_quality"] else torch.zeros(N, dtype=torch.bool)
        pos = gi > 0
        clear = pos & ~holds
        clear[pos] &= ~dup[gi[pos] - 1]
        assert int(clear.sum()) >= 10 and torch.equal(pi[~pos], gi[~pos])
        assert torch.equal(pi[clear], inv[gi[clear] - 1] + 1) and torch.equal(pl[0].cpu()[clear], lb[0].cpu()[clear])


def test_no_matrix_allocation():
    """N = 65 536 horizontal boxes, G = 256: the increase of torch.cuda.max_memory_allocated over one call with a pre-warmed workspace stays below N G 4 / 8 = 8 MB
    (derived: the outputs are 1.3 MB, the matrix would be 64 MB); and the result equals the matrix form at 256 workgroups"""
    N, G = 65536, 256
    gen_ = torch.Generator().manual_seed(3)
    c = torch.rand(N + G, 2, generator=gen_) * 1024
    wh = 8 + torch.rand(N + G, 2, generator=gen_) ** 2 * 200
    b = torch.cat([c - wh / 2, c + wh / 2], 1)
    b[N:N + G] = b[torch.arange(G) * 200]          # every ground truth has an exact copy among the boxes
    boxes, gts = b[:N].to(DEV).contiguous(), b[N:].to(DEV).contiguous()[None]
    cfg = gen.CONFIGS["rpn"]
    ws = torch.empty(ops.max_iou_assign_workspace_bytes(1, G), dtype=torch.uint8, device=DEV)
    args = (boxes, gts, cfg["pos_iou_thr"], cfg["neg_iou_thr"], cfg["min_pos_iou"])
    ops.max_iou_assign(*args, workspace=ws)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    gi, mo, _ = ops.max_iou_assign(*args, workspace=ws)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"    peak allocation above the inputs: {grown / 1e6:.2f} MB (outputs {N * 12 / 1e6:.2f} MB, the matrix would be {N * G * 4 / 1e6:.0f} MB)")
    assert grown < N * G * 4 // 8
    want = max_iou_assign_torch(ops.bbox_overlaps(boxes, gts[0]), cfg["pos_iou_thr"], cfg["neg_iou_thr"], cfg["min_pos_iou"])
    assert torch.equal(gi[0], want[0]) and torch.equal(mo[0], want[1]) and int((gi[0] > 0).sum()) >= G


def test_capture():
    """one eager call, then torch.cuda.graph capture with caller-supplied buffers: replays after new boxes, ground truths and gt_counts are copied in equal the eager
    results"""
    kind, (N, G) = "rotated", BATCH_SHAPES[1]
    a, b = gen.batch_case(kind, N, G), gen.batch_case("rotated", N, G)
    boxes, gts, counts, labels = (a[k].to(DEV).clone() for k in ("boxes", "gts", "counts", "labels"))
    asg = MaxIoUAssigner(0.7, 0.3, 0.3, iou_calculator=dict(type="OBBOverlaps"))
    bufs = dict(gt_inds=torch.empty(3, N, dtype=torch.int64, device=DEV), max_overlaps=torch.empty(3, N, device=DEV), labels=torch.empty(3, N, dtype=torch.int64, device=DEV),
                workspace=torch.empty(ops.max_iou_assign_workspace_bytes(3, G), dtype=torch.uint8, device=DEV))
    eager_a = [t.clone() for t in asg.assign_batched(boxes, gts, counts, labels)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        asg.assign_batched(boxes, gts, counts, labels, **bufs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = asg.assign_batched(boxes, gts, counts, labels, **bufs)
    assert out[0] is bufs["gt_inds"] and out[1] is bufs["max_overlaps"] and out[2] is bufs["labels"]
    graph.replay()
    assert all(torch.equal(x, y) for x, y in zip(out, eager_a))
    # new contents: the images in another order (image 0 now has no ground truth), and other counts
    order = [1, 2, 0]
    boxes.copy_(b["boxes"][order].to(DEV))
    gts.copy_(b["gts"][order].to(DEV))
    labels.copy_(b["labels"][order].to(DEV))
    counts.copy_(b["counts"][order].to(DEV))
    graph.replay()
    eager_b = asg.assign_batched(boxes, gts, counts, labels)
    assert all(torch.equal(x, y) for x, y in zip(out, eager_b)) and not torch.equal(out[0], eager_a[0])
    for i, src in enumerate(order):
        c = b["cases"][src]
        want = reference_max_iou_assign(None, None, 0.7, 0.3, 0.3, gt_labels=c["labels"], overlaps=c["ov"])
        assert out[0][i].tolist() == want[0].tolist()
