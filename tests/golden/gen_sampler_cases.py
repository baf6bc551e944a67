"""Deterministic inputs of the sampler tests (tests/test_sampler_cpu.py asserts their conditions on the oracle, tests/test_sampler_gpu.py runs them) and of
tools/sampler_probe.py.  Everything is numpy; nothing here needs the library."""
import numpy as np

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 70001)          # a partial chunk, a full one, one element over; several chunks; past 16-bit indices
UBS = (-1, 0, 0.5, 1, 3)
KEYS = ((0x9E3779B9, 7), (1, 2), (0xFFFFFFFF, 0))
GMAXES = (0, 1, 7)
CRAFTED = ("all_equal", "two_values", "top_byte_only", "bottom_byte_only", "extremes", "edge_low", "edge_high", "kth_equal")
CRAFTED_SIZES = (1500, 40000)          # one sweep of the per-image workgroup (16 384 elements), and three


def mix(N: int, c_pos: int, c_neg: int, seed: int, G: int = 7) -> np.ndarray:
    """gt_inds int64 [N]: exactly c_pos positives (values 1 .. G), c_neg negatives (0), the rest ignored (-1), at shuffled positions"""
    assert c_pos + c_neg <= N
    g = np.full(N, -1, dtype=np.int64)
    where = np.random.default_rng(seed).permutation(N)
    g[where[:c_pos]] = 1 + np.arange(c_pos) % max(G, 1)
    g[where[c_pos:c_pos + c_neg]] = 0
    return g


def size_case(N: int, B: int, seed: int = 0) -> np.ndarray:
    """gt_inds [B, N] with a different class mix per image: 0 a few positives and half negatives, 1 no positives, 2 all ignored but one negative"""
    rows = []
    for b in range(B):
        if b % 3 == 0:
            c_pos = min(N, max(1, N // 8))
            rows.append(mix(N, c_pos, (N - c_pos + 1) // 2, 100 * seed + b))
        elif b % 3 == 1:
            rows.append(mix(N, 0, N, 100 * seed + b))
        else:
            rows.append(mix(N, 0, 1, 100 * seed + b))
    return np.stack(rows)


def count_cases(num: int = 16, P: int = 4):
    """(c_pos, c_neg) for every pairing of c = 0, c < k, c == k, c == k + 1, c >> k of both classes (k_neg = num - n_pos follows the positives taken)"""
    out = []
    for c_pos in (0, P - 2, P, P + 1, 200):
        k_neg = num - min(c_pos, P)
        for c_neg in (0, k_neg - 3, k_neg, k_neg + 1, 700):
            out.append((c_pos, c_neg))
    return out


def count_case(N: int = 1025, num: int = 16, P: int = 4) -> np.ndarray:
    """gt_inds [25, N]: one image per pairing of count_cases"""
    return np.stack([mix(N, cp, cn, 300 + i) for i, (cp, cn) in enumerate(count_cases(num, P))])


def crafted(name: str, N: int = 1500, num: int = 64, pos_fraction: float = 0.25):
    """(gt_inds int64 [1, N], priorities uint32 [1, N]): 40 positives and 80 % negatives, both oversubscribed at num = 64 / pos_fraction = 0.25 (k = 16 / 48), with
    priorities that put a TIE on each class's threshold"""
    rng = np.random.default_rng(sum(map(ord, name)) + N)
    g = mix(N, 40, N * 4 // 5, 900 + N)

    def pick(values, p=None):
        return rng.choice(np.array(values, dtype=np.uint64), size=N, p=p).astype(np.uint32)
    if name == "all_equal":
        prio = np.full(N, 0x12345678, dtype=np.uint32)
    elif name == "two_values":
        prio = pick([5, 0x80000000], [0.6, 0.4])
    elif name == "top_byte_only":
        prio = pick([(t << 24) | 0x00ABCDEF for t in (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)])
    elif name == "bottom_byte_only":
        prio = pick([0x7F3A2100 | t for t in (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)])
    elif name == "extremes":
        prio = pick([0, 1, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF])
    elif name == "edge_low":          # the threshold is the last value of bin 0
        prio = pick([0x00FFFFFF, 0x01000000], [0.7, 0.3])
    elif name == "edge_high":         # the threshold is the first value of bin 1
        prio = np.full(N, 0x01000000, dtype=np.uint32)          # (five candidates of each class sit below it)
        prio[np.nonzero(g > 0)[0][5:10]] = 0x00FFFFFF
        prio[np.nonzero(g == 0)[0][7:12]] = 0x00FFFFFF
    elif name == "kth_equal":         # distinct priorities, then the (k + 1)-th candidate of each class takes the k-th's
        prio = rng.permutation(np.arange(N, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
        P = int(num * pos_fraction)
        for c, k in ((g > 0, P), (g == 0, num - P)):
            idx = np.nonzero(c)[0]
            order = idx[np.argsort((prio[idx].astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64))]
            prio[order[k]] = prio[order[k - 1]]
    else:
        raise ValueError(name)
    return g[None], prio[None]


def threshold(g: np.ndarray, prio: np.ndarray, positive: bool, k: int):
    """(candidates, threshold priority, candidates equal to it, how many of those the k smallest words take) of one class of one image"""
    idx = np.nonzero(g > 0 if positive else g == 0)[0]
    p = np.sort(prio[idx].astype(np.uint64))
    t = p[k - 1]
    return len(idx), int(t), int((p == t).sum()), int(k - (p < t).sum())
