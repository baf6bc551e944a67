"""The samplers without a GPU (lemevit_amd/detection.py: RandomSampler, OBBRandomSampler; csrc/sampler.hip): the Philox known answer through the oracle's path, the
oracle against brute force on 200 small cases, the uniformity of the Philox priorities, the conditions of the GPU tests' inputs (asserted on the oracle), the new
symbols, and the refusals of the C entry points (validation runs before any launch).

Uniformity, N = 12 candidates, k = 4, image b = 1, keys (t, 7) for t = 0 .. 19 999: an element is chosen with probability 1/3 and a pair with 1/11, so over 20 000
draws the frequencies have sigma = sqrt(p (1 - p) / 20 000) = 0.00333 and 0.00203; the bounds are 4 sigma = 0.0133 and 0.0081.  Measured on the oracle: the worst
deviations are 0.0084 and 0.0045."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gen_sampler_cases as gen
from lemevit_amd import _lib
from lemevit_amd.detection import (SAMPLE_TAG, OBBRandomSampler, RandomSampler, SamplingResult, random_sample_torch, reference_random_sample, reference_sample_gather,
                                   sample_priorities, sample_quotas)
from lemevit_amd.recipe import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, WORKSPACE = -1, -3          # LMV_ERR_SHAPE, LMV_ERR_WORKSPACE


def test_philox_known_answer():
    """counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8 (Random123's known answer), and the oracle's priorities are word r0 of the counter (e, b, 0, tag)"""
    assert [int(x) for x in philox4x32_10((0, 0, 0, 0), (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    p = sample_priorities(3, 5, (11, 22))
    assert p.shape == (3, 5) and int(p.max()) < 2 ** 32
    for b in range(3):
        for e in range(5):
            assert int(p[b, e]) == int(philox4x32_10((e, b, 0, SAMPLE_TAG), (11, 22))[0])
    assert SAMPLE_TAG == int.from_bytes(b"SAMP", "big")
    # the oracle uses them: with zero key and one candidate class the chosen are the smallest (priority, e) pairs
    g = np.zeros((1, 9), dtype=np.int64)
    inds, n_pos, n_neg, mask = reference_random_sample(g, 4, 0.0, key=(0, 0))
    want = sorted(sorted(range(9), key=lambda e: (int(sample_priorities(1, 9, (0, 0))[0, e]), e))[:4])
    assert inds[0].tolist() == want and n_pos[0] == 0 and n_neg[0] == 4 and mask[0].tolist() == [2 if e in want else 0 for e in range(9)]


def brute(g, num, pos_fraction, ub, add_gt, count, Gmax, prio):
    """one image, by the rules, with sorted() of Python tuples"""
    off = Gmax if add_gt else 0
    cand = {1: [e for e in range(off) if e < min(max(count, 0), Gmax)] + [off + n for n, v in enumerate(g) if v > 0], 2: [off + n for n, v in enumerate(g) if v == 0]}
    n_pos = min(len(cand[1]), int(num * pos_fraction))
    expected = num - n_pos
    if ub >= 0:
        expected = min(expected, int(math.floor(ub * max(1, n_pos))))
    n_neg = min(len(cand[2]), expected)
    pos = sorted(e for _, e in sorted((int(prio[e]), e) for e in cand[1])[:n_pos])
    neg = sorted(e for _, e in sorted((int(prio[e]), e) for e in cand[2])[:n_neg])
    return pos + neg + [-1] * (num - n_pos - n_neg), n_pos, n_neg, [1 if e in pos else 2 if e in neg else 0 for e in range(off + len(g))]


def test_oracle_against_brute_force():
    """200 random small cases over every combination of add_gt, neg_pos_ub, counts 0 .. Gmax, all-ignored images, images without positives / negatives, num > M;
    small priority ranges put ties everywhere"""
    rng = np.random.default_rng(2024)
    seen = set()
    for i in range(200):
        add_gt, ub = bool(i % 2), gen.UBS[(i // 2) % 5]
        kind = (i // 10) % 5          # 0 mixed, 1 all ignored, 2 no positives, 3 no negatives, 4 mixed with num > M
        B, N, Gmax = int(rng.integers(1, 4)), int(rng.integers(0, 30)), int(rng.integers(0, 6))
        num = int(rng.integers(1, 12)) if kind != 4 else N + Gmax + int(rng.integers(1, 5))
        pf = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        g = rng.integers(-1, 4, size=(B, N))
        if kind == 1:
            g[:] = -1
        elif kind == 2:
            g[g > 0] = 0
        elif kind == 3:
            g[g == 0] = -1
        counts = rng.integers(0, Gmax + 1, size=B) if i % 3 else None
        M = (Gmax if add_gt else 0) + N
        prio = rng.integers(0, 4 if i % 4 else 2 ** 32, size=(B, M), dtype=np.uint64)
        inds, n_pos, n_neg, mask = reference_random_sample(g, num, pf, ub, add_gt, counts, Gmax, prio)
        for b in range(B):
            want = brute(g[b].tolist(), num, pf, ub, add_gt, Gmax if counts is None else int(counts[b]), Gmax, prio[b])
            assert (inds[b].tolist(), int(n_pos[b]), int(n_neg[b]), mask[b].tolist()) == want, (i, b)
        seen.add((add_gt, ub, kind))
    assert len(seen) == 50


def test_quotas():
    assert sample_quotas(100, 1000, 256, 128, -1) == (100, 156)
    assert sample_quotas(0, 1000, 256, 128, 0.5) == (0, 0)          # floor(0.5 * max(1, 0)) = 0
    assert sample_quotas(0, 1000, 256, 128, 3) == (0, 3)
    assert sample_quotas(5, 1000, 256, 128, 0.5) == (5, 2)
    assert sample_quotas(5, 1, 256, 128, 3) == (5, 1)
    assert sample_quotas(500, 1000, 512, 128, float("inf")) == (128, 384)


def test_uniformity():
    """rule (b): every inclusion frequency within 4 sigma of 1/3, every pair frequency within 4 sigma of 1/11 (the module docstring has the figures)"""
    T, N, k = 20000, 12, 4
    t, e = np.arange(T, dtype=np.uint64)[:, None], np.arange(N, dtype=np.uint64)[None, :]
    words = (philox4x32_10((e, 1, 0, SAMPLE_TAG), (t, 7))[0] << np.uint64(32)) | e
    chosen = np.zeros((T, N))
    np.put_along_axis(chosen, np.argsort(words, axis=1)[:, :k], 1.0, axis=1)
    g = np.zeros((2, N), dtype=np.int64)
    for key in (0, 1, 4242, T - 1):          # this IS the oracle's draw for image 1
        assert reference_random_sample(g, k, 0.0, key=(key, 7))[3][1].tolist() == (2 * chosen[key]).astype(int).tolist()
    single = np.abs(chosen.mean(0) - 1 / 3).max()
    pairs = np.abs(((chosen.T @ chosen) / T)[~np.eye(N, dtype=bool)] - 1 / 11).max()
    print(f"    uniformity: worst inclusion deviation {single:.4f} (bound 0.0133), worst pair deviation {pairs:.4f} (bound 0.0081)")
    assert single <= 4 * math.sqrt((1 / 3) * (2 / 3) / T) and pairs <= 4 * math.sqrt((1 / 11) * (10 / 11) / T)


def test_symbols_and_signatures():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "lemevit_hip.h")).read()
    assert _lib.ABI_VERSION == 14 and _lib.lib.lmv_abi_version() == 14
    assert _lib.SAMPLE_MAX_NUM == int(re.search(r"#define LMV_SAMPLE_MAX_NUM (\d+)", src).group(1)) == 16384
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("lmv_random_sample_workspace_bytes", "lmv_random_sample", "lmv_sample_gather"):
        assert hasattr(raw, name), name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.lib.lmv_random_sample_workspace_bytes(2, 33) == 2 * (2048 + 5 * 48)
    assert _lib.lib.lmv_random_sample_workspace_bytes(1, 0) == 2048
    for B, M in ((0, 5), (4097, 5), (1, -1), (1, (1 << 20) + 1)):
        assert _lib.lib.lmv_random_sample_workspace_bytes(B, M) == 0


A = 1 << 20          # an aligned address that is never dereferenced: every call below is refused before any launch


def sample_call(**kw):
    a = dict(gt_inds=A, N=100, B=2, gt_counts=None, Gmax=0, add_gt=0, num=16, P=4, ub=-1.0, priorities=None, key=A, ws=A, ws_bytes=1 << 30, inds=A, num_pos=A,
             num_neg=A, mask=A)
    a.update(kw)
    rc = _lib.lib.lmv_random_sample(a["gt_inds"], a["N"], a["B"], a["gt_counts"], a["Gmax"], a["add_gt"], a["num"], a["P"], a["ub"], a["priorities"], a["key"], a["ws"],
                                    a["ws_bytes"], a["inds"], a["num_pos"], a["num_neg"], a["mask"], None)
    return rc, _lib.lib.lmv_last_error().decode()


def gather_call(**kw):
    a = dict(inds=A, num=16, boxes=A, box_stride=5, box_batch=0, N=100, k=5, gts=A, gt_stride=5, B=2, Gmax=7, gt_inds=A, gt_labels=A, gt_counts=None, add_gt=1, bg=15,
             rois=A, s_gt=A, s_lab=A)
    a.update(kw)
    rc = _lib.lib.lmv_sample_gather(a["inds"], a["num"], a["boxes"], a["box_stride"], a["box_batch"], a["N"], a["k"], a["gts"], a["gt_stride"], a["B"], a["Gmax"],
                                    a["gt_inds"], a["gt_labels"], a["gt_counts"], a["add_gt"], a["bg"], a["rois"], a["s_gt"], a["s_lab"], None)
    return rc, _lib.lib.lmv_last_error().decode()


@pytest.mark.parametrize("kw, needle", [
    (dict(key=None), "neither priorities nor a key"),
    (dict(ub=float("nan")), "NaN"),
    (dict(add_gt=2), "add_gt"), (dict(add_gt=-1), "add_gt"),
    (dict(gt_inds=None), "null gt_inds"), (dict(inds=None), "null inds"), (dict(num_pos=None), "null inds"), (dict(num_neg=None), "null inds"),
    (dict(gt_inds=A + 4), "misaligned"), (dict(inds=A + 4), "misaligned"), (dict(gt_counts=A + 2, add_gt=1, Gmax=3), "misaligned"), (dict(key=A + 1), "misaligned"),
    (dict(priorities=A + 2, key=None), "misaligned"), (dict(num_pos=A + 2), "misaligned"), (dict(num_neg=A + 1), "misaligned"), (dict(ws=A + 8), "misaligned"),
    (dict(N=(1 << 20) + 1), "at most"), (dict(N=1 << 20, add_gt=1, Gmax=1), "at most"), (dict(N=-1), "negative"), (dict(Gmax=-1), "negative"),
    (dict(num=0), "num ="), (dict(num=16385, P=4), "num ="), (dict(P=-1), "P ="), (dict(P=17), "P ="), (dict(B=0), "B ="), (dict(B=4097), "B ="),
])
def test_random_sample_refusals(kw, needle):
    rc, msg = sample_call(**kw)
    assert rc == SHAPE and msg.startswith("random_sample") and needle in msg, (rc, msg)


def test_random_sample_workspace_refusal():
    need = _lib.lib.lmv_random_sample_workspace_bytes(2, 100)
    for kw in (dict(ws_bytes=need - 1), dict(ws=None), dict(ws_bytes=0)):
        rc, msg = sample_call(**kw)
        assert rc == WORKSPACE and msg.startswith("random_sample") and str(need) in msg, (rc, msg)
    assert sample_call(N=0, gt_inds=None, ws_bytes=4096)[0] == 0          # M == 0: accepted, and nothing is launched


@pytest.mark.parametrize("kw, needle", [
    (dict(k=3), "k ="), (dict(k=6), "k ="), (dict(add_gt=2), "add_gt"), (dict(box_stride=4), "row strides"), (dict(gt_stride=4), "row strides"),
    (dict(box_batch=-1), "negative batch stride"), (dict(boxes=None), "null boxes"), (dict(gt_inds=None), "null boxes"), (dict(gts=None), "null ground truths"),
    (dict(inds=None), "null inds"), (dict(rois=None), "null inds"), (dict(s_gt=None), "null inds"), (dict(gt_labels=None), "s_labels without gt_labels"),
    (dict(boxes=A + 2), "misaligned"), (dict(gts=A + 1), "misaligned"), (dict(inds=A + 4), "misaligned"), (dict(gt_inds=A + 4), "misaligned"),
    (dict(gt_labels=A + 4), "misaligned"), (dict(s_gt=A + 4), "misaligned"), (dict(s_lab=A + 4), "misaligned"), (dict(rois=A + 2), "misaligned"),
    (dict(gt_counts=A + 2), "misaligned"), (dict(num=0), "num ="), (dict(num=16385), "num ="), (dict(B=0), "B ="), (dict(N=-1), "negative"),
    (dict(N=1 << 20), "at most"),
])
def test_sample_gather_refusals(kw, needle):
    rc, msg = gather_call(**kw)
    assert rc == SHAPE and msg.startswith("sample_gather") and needle in msg, (rc, msg)


def test_gpu_input_conditions():
    """what tests/test_sampler_gpu.py relies on, asserted on the oracle: every crafted-priority case has a TIE on each class's threshold (more candidates equal to
    it than are taken, at least one taken) and is oversubscribed; the count cases hit c = 0, c < k, c == k, c == k + 1, c >> k for both classes; the size cases
    have an oversubscribed image where the size allows"""
    num, pf = 64, 0.25
    P = int(num * pf)
    for N in gen.CRAFTED_SIZES:
        for name in gen.CRAFTED:
            g, prio = gen.crafted(name, N, num, pf)
            assert g.shape == (1, N) and prio.dtype == np.uint32
            for positive, k in ((True, P), (False, num - P)):
                c, t, equal, taken = gen.threshold(g[0], prio[0], positive, k)
                assert c > k and equal > taken >= 1, (name, N, positive, c, k, hex(t), equal, taken)
                if name == "edge_low":
                    assert t == 0x00FFFFFF
                if name == "edge_high":
                    assert t == 0x01000000
                if name == "kth_equal":
                    assert (equal, taken) == (2, 1)
            if name == "extremes":
                assert 0 in prio[0][g[0] == 0] and 0xFFFFFFFF in prio[0][g[0] == 0]
    kinds = set()
    g = gen.count_case()
    for b, (c_pos, c_neg) in enumerate(gen.count_cases()):
        assert int((g[b] > 0).sum()) == c_pos and int((g[b] == 0).sum()) == c_neg
        k_neg = 16 - min(c_pos, 4)

        def rel(c, k):
            return "0" if c == 0 else "<" if c < k else "=" if c == k else "+1" if c == k + 1 else ">>"
        kinds.add((rel(c_pos, 4), rel(c_neg, k_neg)))
    assert len(kinds) == 25
    for N in gen.SIZES:
        g = gen.size_case(N, 3)
        assert g.shape == (3, N) and (g[1] == 0).all() and int((g[2] == 0).sum()) == 1 and int((g[0] > 0).sum()) >= 1
        if N >= 1023:
            assert int((g[0] > 0).sum()) > 16 and int((g[0] == 0).sum()) > 48 and int((g[1] == 0).sum()) > 64


def test_reference_gather_and_classes():
    """the gather oracle on a hand case, and the classes' argument checks and empty inputs (no launch, no GPU)"""
    boxes = np.arange(15, dtype=np.float32).reshape(3, 5)
    gts = (100 + np.arange(20, dtype=np.float32)).reshape(1, 4, 5)
    g = np.array([[2, 0, -1]])
    inds = np.array([[0, 3, 4, 5, 6, 1, -1, 99]])          # gts 0 and 3, boxes 0, 1, 2 (ignored), gt 1, padding, out of range
    rois, s_gt, s_lab = reference_sample_gather(inds, boxes, gts, g, np.array([[7, 8, 9, 10]]), np.array([2]), True, 15)
    assert s_gt[0].tolist() == [1, -1, 2, 0, -1, 2, -1, -1] and s_lab[0].tolist() == [7, -1, 8, 15, -1, 8, -1, -1]
    assert rois[0, :, 0].tolist() == [0, -1, 0, 0, -1, 0, -1, -1]
    assert rois[0, 0, 1:].tolist() == gts[0, 0].tolist() and rois[0, 2, 1:].tolist() == boxes[0].tolist() and not rois[0, 1, 1:].any()
    assert issubclass(OBBRandomSampler, RandomSampler)
    s = OBBRandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True, seed=3)
    assert s.num_expected_pos == 128 and "OBBRandomSampler(num=512" in repr(s)
    first = s.host_key
    assert s.draw() != first and s.key is None and OBBRandomSampler(512, 0.25, seed=3).host_key == first
    for bad in (dict(num=0, pos_fraction=0.5), dict(num=16385, pos_fraction=0.5), dict(num=4, pos_fraction=1.5), dict(num=4, pos_fraction=0.5, neg_pos_ub=float("nan"))):
        with pytest.raises(ValueError):
            RandomSampler(**bad)
    with pytest.raises(RuntimeError, match="GPU"):
        s.sample_batched(torch.zeros(1, 4, dtype=torch.int64))

    class Assigned:
        gt_inds, labels = torch.zeros(0, dtype=torch.int64), None
    r = s.sample(Assigned, torch.zeros(0, 5), torch.zeros(0, 5))
    assert isinstance(r, SamplingResult) and r.pos_inds.numel() == 0 and r.bboxes.shape == (0, 5) and r.num_gts == 0 and r.pos_gt_labels is None
    # upstream's literal code on the CPU: counts and class membership
    g = torch.from_numpy(gen.mix(300, 40, 200, 5))
    pos, neg = random_sample_torch(g, 64, 0.25, -1, True, 7)
    assert pos.numel() == 16 and neg.numel() == 48 and bool((torch.cat([torch.ones(7, dtype=torch.int64), g])[pos] > 0).all()) and bool((g[neg - 7] == 0).all())
