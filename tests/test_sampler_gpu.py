"""The samplers on the GPU (csrc/sampler.hip; lemevit_amd/detection.py: RandomSampler, OBBRandomSampler), every comparison EXACT (torch.equal) against the numpy
oracles ``reference_random_sample`` / ``reference_sample_gather``: sizes around the chunk of 1024 elements, around the 16 384 elements one sweep of the per-image
workgroup covers, and past 16-bit indices; batches with a different class mix per image; candidate counts of 0, below, at, one above and far above the quota for both
classes; ground truths as proposals with counts 0 .. Gmax; every neg_pos_ub of the configs' family; crafted priorities with a tie on every threshold
(tests/test_sampler_cpu.py asserts the inputs' conditions); three keys; outputs and workspace pre-filled with 0xFF bytes; the gather; no allocation; capture; the
chain assigner -> sampler -> gather -> coder -> RoI extractor; and upstream's ``sample()``."""
import functools

import numpy as np
import pytest
import torch

import gen_coder_golden as cgen
import gen_sampler_cases as gen
from lemevit_amd import ops
from lemevit_amd.detection import (BatchSample, MaxIoUAssigner, OBB2OBBDeltaXYWHTCoder, OBBRandomSampler, RandomSampler, RotatedRoIExtractor, reference_random_sample,
                                   reference_sample_gather)
from lemevit_amd.recipe import pack_erase_key

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def key_on(key):
    return pack_erase_key(key).to(DEV)


def prio_on(p):
    return dev(np.asarray(p, dtype=np.uint32).view(np.int32))


def check(got, want, what=""):
    """(inds, num_pos, num_neg, mask) of the library against the oracle's, bit for bit, and the outputs' own consistency"""
    inds, n_pos, n_neg, mask = got[:4]
    for g, w, name in zip((inds, n_pos, n_neg, mask), want, ("inds", "num_pos", "num_neg", "mask")):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), f"{what}: {name} differs from the oracle"
    consistent(inds.cpu(), n_pos.cpu(), n_neg.cpu(), mask.cpu())


def consistent(inds, n_pos, n_neg, mask):
    """mask and inds name the same elements, in ascending order per class, and the counts are theirs"""
    for b in range(inds.shape[0]):
        p, n = int(n_pos[b]), int(n_neg[b])
        assert torch.equal(inds[b, :p], (mask[b] == 1).nonzero().squeeze(1)) and torch.equal(inds[b, p:p + n], (mask[b] == 2).nonzero().squeeze(1))
        assert bool((inds[b, p + n:] == -1).all()) and int((mask[b] > 2).sum()) == 0


@functools.lru_cache(maxsize=None)
def size_oracle(N, B, add_gt):
    g = gen.size_case(N, B)
    counts = np.array([7, 0, 3][:B], dtype=np.int32)
    return g, counts, reference_random_sample(g, 64, 0.25, -1, add_gt, counts, 7, key=gen.KEYS[0])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", gen.SIZES)
def test_sizes(N, B):
    """rule (b) at every size, with and without the ground truths as proposals (Gmax = 7: the boxes start at an odd element)"""
    for add_gt in (False, True):
        g, counts, want = size_oracle(N, B, add_gt)
        got = ops.random_sample(dev(g), 64, 16, -1, add_gt, 7, dev(counts), key=key_on(gen.KEYS[0]))
        check(got, want, f"N = {N}, B = {B}, add_gt = {add_gt}")


def test_candidate_counts():
    """25 images: every pairing of c = 0, c < k, c == k, c == k + 1, c >> k of the two classes"""
    g = gen.count_case()
    want = reference_random_sample(g, 16, 0.25, key=gen.KEYS[1])
    got = ops.random_sample(dev(g), 16, 4, key=key_on(gen.KEYS[1]))
    check(got, want, "count cases")
    for b, (c_pos, c_neg) in enumerate(gen.count_cases()):
        assert int(got[1][b]) == min(c_pos, 4) and int(got[2][b]) == min(c_neg, 16 - min(c_pos, 4))


@pytest.mark.parametrize("Gmax", gen.GMAXES)
def test_add_gt(Gmax):
    """image b has b valid ground truths (0 .. Gmax) -- and one image a count above Gmax, one a negative count: clamped; the padding rows are never chosen"""
    counts = np.array(list(range(Gmax + 1)) + [Gmax + 5, -3], dtype=np.int32)
    B = len(counts)
    g = np.stack([gen.mix(65, 6, 40, 40 + b) for b in range(B)])
    want = reference_random_sample(g, 32, 0.5, -1, True, counts, Gmax, key=gen.KEYS[2])
    got = ops.random_sample(dev(g), 32, 16, -1, True, Gmax, dev(counts), key=key_on(gen.KEYS[2]))
    check(got, want, f"Gmax = {Gmax}")
    mask = got[3].cpu()
    for b in range(B):
        c = min(max(int(counts[b]), 0), Gmax)
        assert bool((mask[b, :c] == 1).all()) and not mask[b, c:Gmax].any()          # (6 + c <= 16: every valid ground truth is taken)
    # null counts: Gmax everywhere
    want = reference_random_sample(g, 32, 0.5, -1, True, None, Gmax, key=gen.KEYS[2])
    check(ops.random_sample(dev(g), 32, 16, -1, True, Gmax, None, key=key_on(gen.KEYS[2])), want, f"Gmax = {Gmax}, null counts")


@pytest.mark.parametrize("ub", gen.UBS)
def test_neg_pos_ub(ub):
    """image 0 has positives (5 of them: n_pos = 5), image 1 none (max(1, n_pos) = 1), image 2 fewer negatives than the bound"""
    g = np.stack([gen.mix(1025, 5, 900, 1), gen.mix(1025, 0, 900, 2), gen.mix(1025, 5, 2, 3)])
    want = reference_random_sample(g, 64, 0.5, ub, key=gen.KEYS[0])
    got = ops.random_sample(dev(g), 64, 32, ub, key=key_on(gen.KEYS[0]))
    check(got, want, f"neg_pos_ub = {ub}")
    expect = {-1: [59, 64, 2], 0: [0, 0, 0], 0.5: [2, 0, 2], 1: [5, 1, 2], 3: [15, 3, 2]}[ub]
    assert got[2].tolist() == expect and got[1].tolist() == [5, 0, 5]


@pytest.mark.parametrize("N", gen.CRAFTED_SIZES)
@pytest.mark.parametrize("name", gen.CRAFTED)
def test_crafted_priorities(name, N):
    """rule (a): a tie on the threshold of both classes -- the choice among equal priorities is by index"""
    g, prio = gen.crafted(name, N)
    want = reference_random_sample(g, 64, 0.25, priorities=prio)
    got = ops.random_sample(dev(g), 64, 16, priorities=prio_on(prio))
    check(got, want, f"{name}, N = {N}")
    if name == "all_equal":
        assert got[0][0, :16].tolist() == np.nonzero(g[0] > 0)[0][:16].tolist() and got[0][0, 16:].tolist() == np.nonzero(g[0] == 0)[0][:48].tolist()
    # the same with the ground truths in front: the element index, not the box index, breaks the ties
    pg = np.concatenate([np.full((1, 3), prio[0, 0], dtype=np.uint32), prio], 1)
    want = reference_random_sample(g, 64, 0.25, -1, True, np.array([2]), 3, priorities=pg)
    check(ops.random_sample(dev(g), 64, 16, -1, True, 3, dev(np.array([2], dtype=np.int32)), priorities=prio_on(pg)), want, f"{name}, N = {N}, add_gt")


def test_keys():
    """three keys: each equals the oracle, different keys give different samples, two calls with one key agree bit for bit; priorities win over a key"""
    g = gen.size_case(4097, 3)
    outs = []
    for key in gen.KEYS:
        want = reference_random_sample(g, 256, 0.5, key=key)
        a = ops.random_sample(dev(g), 256, 128, key=key_on(key))
        b = ops.random_sample(dev(g), 256, 128, key=key_on(key))
        check(a, want, f"key {key}")
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        outs.append(a)
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[1][3], outs[2][3]) and not torch.equal(outs[0][3], outs[2][3])
    prio = np.random.default_rng(5).integers(0, 2 ** 32, size=(3, 4097), dtype=np.uint64)
    check(ops.random_sample(dev(g), 256, 128, priorities=prio_on(prio), key=key_on(gen.KEYS[0])), reference_random_sample(g, 256, 0.5, priorities=prio), "both given")


def test_prefilled_buffers():
    """nothing is assumed about what the outputs and the workspace hold: 0xFF bytes everywhere give the same bits, and a workspace larger than needed is fine"""
    g, counts = gen.size_case(1025, 3), np.array([7, 0, 3], dtype=np.int32)
    M = 7 + 1025
    want = reference_random_sample(g, 64, 0.25, 1, True, counts, 7, key=gen.KEYS[1])
    ws = torch.full((ops.random_sample_workspace_bytes(3, M) + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    inds = torch.full((3, 64), -1, dtype=torch.int64, device=DEV).view(torch.uint8).fill_(0xFF).view(torch.int64)
    n_pos, n_neg = (torch.full((3,), -1, dtype=torch.int32, device=DEV) for _ in range(2))
    mask = torch.full((3, M), 0xFF, dtype=torch.uint8, device=DEV)
    for _ in range(2):          # (the second call finds the first call's workspace)
        got = ops.random_sample(dev(g), 64, 16, 1, True, 7, dev(counts), key=key_on(gen.KEYS[1]), inds=inds, num_pos=n_pos, num_neg=n_neg, mask=mask, workspace=ws)
        assert got[0] is inds and got[3] is mask
        check(got, want, "pre-filled")
    # without a mask the other outputs are the same
    got = ops.random_sample(dev(g), 64, 16, 1, True, 7, dev(counts), key=key_on(gen.KEYS[1]), want_mask=False)
    assert got[3] is None and torch.equal(got[0], inds) and torch.equal(got[1], n_pos) and torch.equal(got[2], n_neg)


def test_empty_and_refusals():
    s = RandomSampler(16, 0.5, add_gt_as_proposals=False)
    out = s.sample_batched(torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    assert bool((out.inds == -1).all()) and out.num_pos.tolist() == [0, 0] and out.num_neg.tolist() == [0, 0] and out.mask.shape == (2, 0)
    g = torch.zeros(2, 10, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="workspace"):
        ops.random_sample(g, 16, 8, key=key_on((1, 2)), workspace=torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="or a key"):
        ops.random_sample(g, 16, 8)
    with pytest.raises(TypeError, match="priorities"):
        ops.random_sample(g, 16, 8, priorities=torch.zeros(2, 9, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="num ="):
        ops.random_sample(g, 16385, 8, key=key_on((1, 2)))


# ---- the gather ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("k", [4, 5])
def test_gather(k, shared):
    """shared and per-image boxes, a box row stride above k, ground-truth rows under add_gt, padding rows; and hand-made indices that name no candidate"""
    B, N, Gmax = 3, 257, 7
    rng = np.random.default_rng(k + 10 * shared)
    wide = torch.from_numpy(rng.normal(size=(N, k + 3) if shared else (B, N, k + 3)).astype(np.float32)).to(DEV)
    boxes = wide[..., :k]          # a row stride of k + 3
    gts = torch.from_numpy(rng.normal(size=(B, Gmax, k)).astype(np.float32)).to(DEV)
    g = np.stack([gen.mix(N, 20, 30, 60 + b) for b in range(B)])          # (16 + 30 < 64: padding rows)
    counts, labels = np.array([7, 0, 3], dtype=np.int32), rng.integers(0, 15, size=(B, Gmax))
    for add_gt in (True, False):
        sampler = OBBRandomSampler(64, 0.25, add_gt_as_proposals=add_gt, seed=1)
        s = sampler.sample_batched(dev(g), dev(counts), Gmax)
        for lab in (labels, None):
            rois, s_gt, s_lab = sampler.gather(s, boxes, gts, dev(g), None if lab is None else dev(lab), dev(counts), bg_label=15)
            want = reference_sample_gather(s.inds, boxes, gts, g, lab, counts, add_gt, 15)
            assert torch.equal(rois.cpu(), torch.from_numpy(want[0])) and torch.equal(s_gt.cpu(), torch.from_numpy(want[1]))
            assert (s_lab is None and want[2] is None) if lab is None else torch.equal(s_lab.cpu(), torch.from_numpy(want[2]))
        pad = (s.inds < 0).cpu()
        assert bool(pad.any()) and bool((rois.cpu()[pad][:, 0] == -1).all()) and not rois.cpu()[pad][:, 1:].any() and bool((s_gt.cpu()[pad] == -1).all())
        assert bool((rois.cpu()[~pad][:, 0] == torch.arange(B)[:, None].expand(B, 64)[~pad]).all())
        if add_gt:          # image 0 takes its 7 ground truths (they are positives: 27 candidates, 16 taken -- at least the mask says which)
            took = (s.inds[0] < Gmax) & (s.inds[0] >= 0)
            assert torch.equal(rois[0][took][:, 1:], gts[0][s.inds[0][took]]) and torch.equal(s_gt[0][took], s.inds[0][took] + 1)
    hand = torch.tensor([[0, 6, 7, 7 + N - 1, 7 + N, -1, -5, 1 << 40]] * B, dtype=torch.int64, device=DEV)          # gts, boxes, one past the end, negatives, far out
    sampler = OBBRandomSampler(8, 0.25, add_gt_as_proposals=True)
    rois, s_gt, s_lab = sampler.gather(hand, boxes, gts, dev(g), dev(labels), dev(counts), bg_label=15)
    want = reference_sample_gather(hand, boxes, gts, g, labels, counts, True, 15)
    assert torch.equal(rois.cpu(), torch.from_numpy(want[0])) and torch.equal(s_gt.cpu(), torch.from_numpy(want[1])) and torch.equal(s_lab.cpu(), torch.from_numpy(want[2]))
    assert s_gt[1].tolist()[:2] == [-1, -1] and s_gt[0].tolist()[:2] == [1, 7] and s_gt[2].tolist()[:2] == [1, -1]          # counts 7, 0, 3


# ---- no hidden work ------------------------------------------------------------------------------------------------------------------------------------------------
def _allocations() -> int:
    return int(torch.cuda.memory_stats()["allocation.all.allocated"])


def _buffers(B, N, Gmax, num, k):
    M = Gmax + N
    return dict(inds=torch.empty(B, num, dtype=torch.int64, device=DEV), num_pos=torch.empty(B, dtype=torch.int32, device=DEV),
                num_neg=torch.empty(B, dtype=torch.int32, device=DEV), mask=torch.empty(B, M, dtype=torch.uint8, device=DEV),
                workspace=torch.empty(ops.random_sample_workspace_bytes(B, M), dtype=torch.uint8, device=DEV)), \
        dict(rois=torch.empty(B, num, 1 + k, device=DEV), s_gt_inds=torch.empty(B, num, dtype=torch.int64, device=DEV),
             s_labels=torch.empty(B, num, dtype=torch.int64, device=DEV))


def _rcnn_inputs(seed=0, B=3, N=257, Gmax=7):
    rng = np.random.default_rng(seed)
    boxes = torch.from_numpy(rng.normal(size=(B, N, 5)).astype(np.float32)).to(DEV)
    gts = torch.from_numpy(rng.normal(size=(B, Gmax, 5)).astype(np.float32)).to(DEV)
    g = np.stack([gen.mix(N, 30, 150, 10 * seed + b) for b in range(B)])
    return boxes, gts, g, np.array([7, 2, 0], dtype=np.int32), rng.integers(0, 15, size=(B, Gmax))


def test_no_allocation():
    """sample_batched and gather with their outputs and the workspace supplied allocate nothing: the caching allocator's allocation count does not move"""
    boxes, gts, g, counts, labels = _rcnn_inputs()
    gd, cd, ld = dev(g), dev(counts), dev(labels)
    sampler = OBBRandomSampler(64, 0.25, seed=0)
    sb, gb = _buffers(3, 257, 7, 64, 5)
    want = sampler.sample_batched(gd, cd, 7)
    want_g = sampler.gather(want, boxes, gts, gd, ld, cd, 15)
    torch.cuda.synchronize()
    before = _allocations()
    s = sampler.sample_batched(gd, cd, 7, **sb)
    r = sampler.gather(s, boxes, gts, gd, ld, cd, 15, **gb)
    after = _allocations()
    torch.cuda.synchronize()
    assert after == before, f"{after - before} allocations"
    assert all(torch.equal(a, b) for a, b in zip(s, want)) and all(torch.equal(a, b) for a, b in zip(r, want_g))


def test_capture():
    """one eager call, then torch.cuda.graph capture with caller-supplied buffers (side-stream warm-up first): replays after new gt_inds contents and after draw()
    equal the eager and oracle results; a replay with a new key differs from the previous one"""
    boxes, gts, g, counts, labels = _rcnn_inputs()
    g2 = _rcnn_inputs(1)[2]
    gd, cd, ld = dev(g).clone(), dev(counts), dev(labels)
    sampler = OBBRandomSampler(64, 0.25, seed=7)
    sb, gb = _buffers(3, 257, 7, 64, 5)

    def run():
        s = sampler.sample_batched(gd, cd, 7, **sb)
        return s, sampler.gather(s, boxes, gts, gd, ld, cd, 15, **gb)

    def oracle(gi):
        want = reference_random_sample(gi, 64, 0.25, -1, True, counts, 7, key=sampler.host_key)
        return want, reference_sample_gather(want[0], boxes, gts, gi, labels, counts, True, 15)

    def equal_oracle(s, r, want):
        check(s, want[0], "capture")
        return all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(r, want[1]))
    s, r = run()          # eager: allocates the key
    assert equal_oracle(s, r, oracle(g))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s, r = run()
    assert s.inds is sb["inds"] and r[0] is gb["rois"]
    for t in list(sb.values()) + list(gb.values()):
        t.view(torch.uint8).fill_(0xFF)
    graph.replay()
    assert equal_oracle(s, r, oracle(g))
    first = s.inds.clone()
    gd.copy_(dev(g2))          # new contents
    graph.replay()
    assert equal_oracle(s, r, oracle(g2)) and not torch.equal(s.inds, first)
    eager = OBBRandomSampler(64, 0.25, seed=7).sample_batched(gd, cd, 7)          # (the same seed: the same first key)
    assert all(torch.equal(a, b) for a, b in zip(s, eager))
    second = s.inds.clone()
    old = sampler.host_key
    assert sampler.draw() != old          # a new key, read by the replayed kernel
    graph.replay()
    assert equal_oracle(s, r, oracle(g2)) and not torch.equal(s.inds, second)


# ---- the chain, and upstream's form -----------------------------------------------------------------------------------------------------------------------------------
def test_rcnn_chain():
    """257 proposals, 7 ground truths (the shapes of test_rpn_chain), the configs' R-CNN settings: MaxIoUAssigner (0.5 / 0.5 / 0.5, OBBOverlaps) -> OBBRandomSampler
    (512, 0.25, ground truths as proposals) -> gather -> encode_assigned on the gathered rows -> RotatedRoIExtractor on a tiny pyramid"""
    c = cgen.chain_case()
    gts = c["gts"].to(DEV)
    props = torch.from_numpy(cgen.jitter_proposals(c["gts"].double().numpy()[np.arange(257) % 7], 0xC0DE).astype(np.float32))
    props[np.arange(257) % 5 == 4, :2] += 5000.0          # background
    props = props.to(DEV)
    assigner = MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False, ignore_iof_thr=-1, iou_calculator=dict(type="OBBOverlaps"))
    labels = torch.arange(7, device=DEV)[None] % 15
    gt_inds, _, _ = assigner.assign_batched(props, gts[None], gt_labels=labels)
    sampler = OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True, seed=0)
    s = sampler.sample_batched(gt_inds, None, 7)
    check(s, reference_random_sample(gt_inds, 512, 0.25, -1, True, None, 7, key=sampler.host_key), "chain")
    rois, s_gt, s_lab = sampler.gather(s, props, gts[None], gt_inds, labels, None, bg_label=15)
    n_pos, n_neg = int(s.num_pos[0]), int(s.num_neg[0])
    assert n_pos + n_neg <= 512 and n_pos >= 7 and n_pos == min(128, 7 + int((gt_inds > 0).sum())) and n_neg == min(int((gt_inds == 0).sum()), 512 - n_pos)
    took = (s.inds[0] >= 0) & (s.inds[0] < 7)          # the ground truths that were drawn: they are their own targets
    assert bool(took.any()) and torch.equal(s_gt[0][took], s.inds[0][took] + 1) and torch.equal(rois[0][took][:, 1:], gts[s.inds[0][took]])
    coder = OBB2OBBDeltaXYWHTCoder(target_stds=cgen.RCNN_STDS)
    targets, weights = coder.encode_assigned(rois[..., 1:], gts[None], s_gt)
    assert torch.equal(weights[0] > 0, s_gt[0] > 0) and int((weights[0] > 0).sum()) == n_pos          # the live weights are the sampled positives
    assert float(targets[0][took].abs().max()) <= 1e-5          # a box against itself: zero deltas
    assert torch.equal(s_lab[0][s_gt[0] > 0], labels[0][s_gt[0][s_gt[0] > 0] - 1]) and bool((s_lab[0][s_gt[0] == 0] == 15).all()) and bool((s_lab[0][s_gt[0] < 0] == -1).all())
    feats = [torch.randn(1, 8, 1024 // st, 1024 // st, device=DEV) for st in (4, 8, 16, 32)]
    extractor = RotatedRoIExtractor(out_size=7, sample_num=2, featmap_strides=(4, 8, 16, 32), out_channels=8, extend_factor=(1.4, 1.2))
    out = extractor(feats, rois.reshape(-1, 6))
    pad = s_gt[0] < 0
    assert out.shape == (512, 8, 7, 7) and bool(pad.any()) and not out[pad].any() and float(out[took].abs().sum()) > 0          # padding rows: zero features


def test_sample_upstream_form():
    """``sample(assign_result, bboxes, gt_bboxes, gt_labels)``: every field of the SamplingResult equals upstream's definition computed from the oracle's indices"""
    boxes, gts, g, _, labels = _rcnn_inputs(3, B=1)
    lab = dev(labels[0])

    class Assigned:
        gt_inds, labels = dev(g[0]), None
    for cls, add_gt, G in ((OBBRandomSampler, True, 7), (RandomSampler, False, 7), (OBBRandomSampler, True, 0)):
        sampler = cls(64, 0.25, add_gt_as_proposals=add_gt, seed=11)
        r = sampler.sample(Assigned, boxes[0], gts[0, :G], lab[:G])
        inds, n_pos, n_neg, _ = reference_random_sample(g, 64, 0.25, -1, add_gt, None, G, key=sampler.host_key)
        p, n = int(n_pos[0]), int(n_neg[0])
        pos, neg = torch.from_numpy(inds[0, :p]), torch.from_numpy(inds[0, p:p + n])
        off = G if add_gt else 0
        all_boxes = torch.cat([gts[0, :off], boxes[0]]).cpu()
        all_inds = torch.cat([torch.arange(1, off + 1), torch.from_numpy(g[0])])
        assert torch.equal(r.pos_inds.cpu(), pos) and torch.equal(r.neg_inds.cpu(), neg) and r.num_gts == G
        assert torch.equal(r.pos_bboxes.cpu(), all_boxes[pos]) and torch.equal(r.neg_bboxes.cpu(), all_boxes[neg])
        assert torch.equal(r.bboxes.cpu(), torch.cat([all_boxes[pos], all_boxes[neg]]))
        assert r.pos_is_gt.dtype == torch.uint8 and torch.equal(r.pos_is_gt.cpu(), (pos < off).to(torch.uint8))
        assert torch.equal(r.pos_assigned_gt_inds.cpu(), all_inds[pos] - 1)
        if G > 0:
            assert torch.equal(r.pos_gt_bboxes.cpu(), gts[0].cpu()[all_inds[pos] - 1]) and torch.equal(r.pos_gt_labels.cpu(), torch.from_numpy(labels[0])[all_inds[pos] - 1])
        else:
            assert r.pos_gt_bboxes.shape == (0, 5)
