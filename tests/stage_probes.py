"""Operand builders and closed-form references for the component probes of the persistent stage kernels (csrc/sstage.hip, csrc/dstage.hip).
Plain Python on the CPU: nothing of the GPU library is imported here, so tests/test_stage_probe_cpu.py can validate every probe against the float64 oracle.

A kernel instance is (kind, C, G): kind "D" (dstage kind 0), "C" (dstage kind 1), "S" (sstage at 14 x 14) or "S2" (dstage kind 2 at 24 x 24); "D2" is the D kernel with the
DualCrossAttention_v2 parameters (ops.d2stage_pack).  Every builder returns a Probe: per-block parameter dicts under the names of ops.DSTAGE_NAMES / SSTAGE_NAMES / CSTAGE_NAMES /
D2STAGE_NAMES (matrices bf16, vectors fp32, pos_embed.weight as [C, 9]), x [B, G G, C] and c [B, 16, C] in bf16, the expected outputs in float64, and `info`, the coverage lists
the tests assert.  The references are a convolution, a gather, or one polynomial; oracle/lemevit_oracle.py is what they are checked against, not what they are made of.

(a) probe_pos: everything but the position embedding is zero, operands are small integers: x_out is three integer convolutions, c_out is c.
(b) probe_select: every softmax row is one-hot by construction (a margin of >= 150 in the exp2 domain), the projections are identities: the outputs are a gather.
(c) probe_mlp: the attention contributes nothing, every fc1 row has one non-zero weight and every fc2 row a single 1: an output channel shows one hidden unit."""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

M = 16
LOG2E = 1.4426950408889634
EPS = 1e-6
_SHARED = ("mlp.0.weight", "mlp.3.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "mlp.0.bias", "mlp.3.bias", "pos_embed.weight", "pos_embed.bias")
ATTN_SHAPES = {          # name -> rows as a multiple of C (matrices are [rows, C], their biases [rows])
    "D": {"attn.qkv1": 3, "attn.qkv2": 3, "attn.proj_x": 1, "attn.proj_c": 1},
    "D2": {"attn.qv1": 2, "attn.kv2": 2, "attn.proj_x": 1, "attn.proj_c": 1},
    "S": {"attn.qkv": 3, "attn.proj": 1},
    "C": {"attn.q": 1, "attn.kv": 2, "attn.proj": 1},
}
ORACLE_TYPE = {"D": "D", "D2": "D2", "S": "S", "S2": "S", "C": "C"}


def family(kind):
    """The parameter-name family of a kind ("S2" is the S block in the D-stage kernel's layout)."""
    return "S" if kind == "S2" else kind


def names(kind):
    """The parameter names of a block of this kind (what ops.*STAGE_NAMES list, in any order)."""
    out = list(_SHARED)
    for n in ATTN_SHAPES[family(kind)]:
        out += [n + ".weight", n + ".bias"]
    return tuple(out)


def workgroups(kind, G):
    """[(first token, last token)] of the image workgroups of an instance (DG<> in csrc/dstage.hip: NT = 7 token tiles where 7 divides the grid, else 6; TOK = 16 NT tokens =
    ROWS whole grid rows; KWG = G / ROWS workgroups -- for "C" blocks a workgroup takes two such row groups in turn, the unit of hand-off stays the row group.  csrc/sstage.hip:
    two workgroups, tokens 0 .. 111 and 112 .. 195)."""
    if kind == "S":
        assert G == 14
        return [(0, 111), (112, 195)]
    NT = 7 if G % 7 == 0 else 6
    TOK = 16 * NT
    assert TOK % G == 0 and G % (TOK // G) == 0, (G, TOK)
    KWG = G // (TOK // G)
    return [(w * TOK, w * TOK + TOK - 1) for w in range(KWG)]


def scales(kind, C, G):
    """(s_x, s_c): the softmax scales of the image-token and the meta-token queries (models/lemevit.py:235,255-256; F.scaled_dot_product_attention for S and C blocks)."""
    if kind in ("D", "D2"):
        return math.log(M) / math.log(G * G) / math.sqrt(C), 1.0 / math.sqrt(C)
    return 1.0 / math.sqrt(32.0), 1.0 / math.sqrt(32.0)


def _mix(t):
    """int64 tensor -> well-mixed 32-bit values (a multiplicative hash: deterministic, no generator state)."""
    t = (t * 2654435761) & 0xFFFFFFFF
    t = t ^ (t >> 15)
    t = (t * 2246822519) & 0xFFFFFFFF
    return t ^ (t >> 13)


def _hash(shape, salt):
    n = int(np.prod(shape))
    return (_mix(torch.arange(n, dtype=torch.int64) + 1000003 * salt + 12345) >> 7).reshape(shape)


def zero_block(kind, C):
    """A block that is the identity but for nothing: all matrices and biases 0, both norms (1, 0), no position embedding."""
    blk = {"mlp.0.weight": torch.zeros(4 * C, C, dtype=torch.bfloat16), "mlp.3.weight": torch.zeros(C, 4 * C, dtype=torch.bfloat16), "mlp.0.bias": torch.zeros(4 * C),
           "mlp.3.bias": torch.zeros(C), "norm1.weight": torch.ones(C), "norm1.bias": torch.zeros(C), "norm2.weight": torch.ones(C), "norm2.bias": torch.zeros(C),
           "pos_embed.weight": torch.zeros(C, 9), "pos_embed.bias": torch.zeros(C)}
    for n, r in ATTN_SHAPES[family(kind)].items():
        blk[n + ".weight"] = torch.zeros(r * C, C, dtype=torch.bfloat16)
        blk[n + ".bias"] = torch.zeros(r * C)
    assert set(blk) == set(names(kind))
    return blk


def oracle_sd(blk):
    """A block dict as the float64 state dict oracle.lemevit_oracle.leme_block reads under the prefix "blk."."""
    C = blk["norm1.weight"].shape[0]
    return {"blk." + k: (v.reshape(C, 1, 3, 3) if k == "pos_embed.weight" else v).double() for k, v in blk.items()}


def _probe(kind, C, G, blocks, x, c, x_ref, c_ref, **info):
    for blk in blocks:
        for k, v in blk.items():
            mat = k.endswith(".weight") and k.startswith(("attn.", "mlp."))
            assert v.dtype == (torch.bfloat16 if mat else torch.float32), k
    assert x.dtype == torch.bfloat16 and c.dtype == torch.bfloat16 and x_ref.dtype == torch.float64 and c_ref.dtype == torch.float64
    return SimpleNamespace(kind=kind, C=C, G=G, heads=C // 32, blocks=blocks, x=x, c=c, x_ref=x_ref, c_ref=c_ref, info=SimpleNamespace(**info))


# ------------------------------------------------------------------------------------------------
# (a) the position embedding, exact
def pos_taps(C, j):
    """Block j: per channel at most two non-zero taps from {-1, +1} ([C, 9]), and an integer bias in [-2, 2]."""
    w = torch.zeros(C, 9)
    ch = torch.arange(C)
    sg = (_hash((C, 2), 40 + j) & 1) * 2 - 1
    w[ch, (4 * ch + 1 + j + ch // 9) % 9] = sg[:, 1].float()
    w[ch, (ch + 2 * j) % 9] = sg[:, 0].float()
    b = ((3 * ch + j) % 5 - 2).float()
    return w, b


@functools.lru_cache(maxsize=None)
def probe_pos(kind, C, G, B, nblocks=3):
    """x: integers in [-3, 3], a hash of (image, token, channel); c: bf16 values with a fraction (it must come back bit for bit).  Three blocks, so that both halo parities are
    written, read and overwritten and the rows of block gb - 2 differ from those of gb - 1."""
    N = G * G
    x = (_hash((B, N, C), 1) % 7 - 3).double()
    c = ((_hash((B, M, C), 2) % 255 - 127).double() / 16.0)
    blocks, taps_used = [], []
    xi = x.transpose(1, 2).reshape(B, C, G, G)
    peak = [float(xi.abs().max())]
    for j in range(nblocks):
        w, b = pos_taps(C, j)
        blk = zero_block(kind, C)
        blk["pos_embed.weight"], blk["pos_embed.bias"] = w, b
        blocks.append(blk)
        assert int((w != 0).sum(1).max()) <= 2 and int((w != 0).sum(1).min()) >= 1 and bool(((w == 0) | (w.abs() == 1)).all())
        taps_used.append(sorted(set((w != 0).nonzero()[:, 1].tolist())))
        with torch.no_grad():
            xi = xi + F.conv2d(xi, w.double().reshape(C, 1, 3, 3), b.double(), stride=1, padding=1, groups=C)
        assert bool((xi == xi.round()).all())
        peak.append(float(xi.abs().max()))
    x_ref = xi.reshape(B, C, N).transpose(1, 2).contiguous()
    if kind == "C":          # "C" blocks return x as it came: the position embedding only feeds norm1
        x_ref = x.clone()
    # what the probe's power rests on: the rows either side of every cut, the two border columns and the images all differ
    rows = x.reshape(B, G, G, C)
    rows_distinct = all(len({rows[b, r].numpy().tobytes() for r in range(G)}) == G for b in range(B))
    cols_distinct = all(not torch.equal(rows[b, :, 0], rows[b, :, G - 1]) and bool(rows[b, :, 0].abs().sum() > 0) and bool(rows[b, :, G - 1].abs().sum() > 0) for b in range(B))
    images_distinct = len({x[b].numpy().tobytes() for b in range(B)}) == B
    return _probe(kind, C, G, blocks, x.to(torch.bfloat16), c.to(torch.bfloat16), x_ref, c.clone(), peak=peak, taps_used=taps_used, rows_distinct=rows_distinct,
                  cols_distinct=cols_distinct, images_distinct=images_distinct)


# ------------------------------------------------------------------------------------------------
# (b) attention by selection
N_CODES = 12870
_PAY0 = 16          # codes 0 .. 15 are the meta tokens' own; the image tokens' payloads start here


@functools.lru_cache(maxsize=None)
def codes():
    """All balanced +-1 vectors of length 16 ([12870, 16] int64), in a scrambled order.  Two different ones differ in >= 2 places, so their dot product is <= 12."""
    comb = np.array(list(itertools.combinations(range(16), 8)))
    a = -np.ones((N_CODES, 16), dtype=np.int64)
    a[np.arange(N_CODES)[:, None], comb] = 1
    order = (np.arange(N_CODES) * 7919 + 101) % N_CODES
    assert len(set(order.tolist())) == N_CODES
    return torch.from_numpy(a[order])


def _lscale(s):
    """The power of two L with 4 L s log2 e >= 160: the runner-up of a softmax row lies 4 L s log2 e below the selected score in the exp2 domain; 160 leaves room for the kernel's
    two roundings of L s log2 e (fp32, then the bf16 operand: a factor >= 1 - 2^-8) above the 150 at which exp2 is 0 in fp32."""
    return 2.0 ** math.ceil(math.log2(160.0 / (4.0 * s * LOG2E)))


def _sel_rows(C, gain, src_off):
    """[C, C]: row 32 h + d (d < 16) takes `gain` x channel 32 h + src_off + d; the other rows are 0."""
    w = torch.zeros(C, C)
    for h in range(C // 32):
        for d in range(16):
            w[32 * h + d, 32 * h + src_off + d] = gain
    return w


def _targets(kind, C, G, B):
    """sigma [B, NH, 16]: the image token each (image, head, meta token) selects.  Selection k = ((b NH + h) 16 + m) goes to workgroup k mod KWG; the first visit of a workgroup
    takes its first or last token (by the parity of the workgroup), the second visit the other one, later visits an interior token."""
    wgs = workgroups(kind, G)
    KWG, NH = len(wgs), C // 32
    sigma = torch.zeros(B, NH, M, dtype=torch.int64)
    for b in range(B):
        for h in range(NH):
            for m in range(M):
                k = (b * NH + h) * M + m
                w, j = k % KWG, k // KWG
                lo, hi = wgs[w]
                if j < 2:
                    sigma[b, h, m] = lo if (j + w) % 2 == 0 else hi
                else:
                    sigma[b, h, m] = lo + 1 + (37 * j + 11 * w) % (hi - lo - 1)
    return sigma


def _margin(addr, pay, want, s):
    """addr [.., Q, 16], pay [.., K, 16] (+-1), want [.., Q] -> the smallest gap, over all queries, between the selected key's score and the best other key's, in the exp2 domain
    for a score scale s (L included); asserts the selected key IS the maximum."""
    sc = torch.einsum("...qd,...kd->...qk", addr.double(), pay.double()) * (s * LOG2E)
    top = sc.gather(-1, want.unsqueeze(-1)).squeeze(-1)
    assert bool((top == sc.max(-1).values).all())
    rest = sc.scatter(-1, want.unsqueeze(-1), -math.inf).max(-1).values
    return float((top - rest).min())


def _soft_attention(addr, key, sig, bias, scale):
    """addr [B, NH, Q, 16], key [B, NH, K, 16] (+-1 codes), sig [B, NH, K, 32] (+-1: the value rows without their bias [NH, 1, 32]), scale: scores -> exp2 domain.
    -> (attention output [B, NH, Q, 32] in float64, its elementwise error bound for the kernels):
      2^-8 |out|                                   the bf16 pack of the attention output (the proj operand; the projection is the identity),
      1.1 x 2^-8 ln 2 sum_k p_k |s_k - s_max| |v_k - out|   the ONE rounding of the scaled query to bf16 (relative 2^-8 on every score, first order + 10 %),
      2^-9 sum_k p_k |v_k|                         P in fp16 (2^-11 per weight) against row sums of the unrounded weights, v_exp_f32 and v_rcp_f32 (1 ulp each),
      1e-5                                         fp32 sums.
    Keys, values (small integers) and LayerNorm outputs (+-1) are exact operands.  A value is (+-1 + bias) per channel, so the sums over keys are two matrix products."""
    out, bound = [], []
    for b in range(addr.shape[0]):          # (per image: the score matrix of an S block at 24 x 24 is 576 x 576 per head)
        S = torch.einsum("hqd,hkd->hqk", addr[b].double(), key[b].double()) * scale
        S = S - S.max(-1, keepdim=True).values
        P = torch.exp2(S)
        P = P / P.sum(-1, keepdim=True)
        up = (sig[b] > 0).double()
        wp, wm = P @ up, P @ (1.0 - up)                     # the weight on the keys whose value is +1 / -1 in this channel
        o = wp - wm + bias
        W = P * S.abs()
        sp, sm = W @ up, W @ (1.0 - up)
        e_scale = sp * (1.0 + bias - o).abs() + sm * (-1.0 + bias - o).abs()
        a_mag = wp * (1.0 + bias).abs() + wm * (-1.0 + bias).abs()
        out.append(o)
        bound.append(2.0 ** -8 * o.abs() + 1.1 * 2.0 ** -8 * math.log(2.0) * e_scale + 2.0 ** -9 * a_mag + 1e-5)
    return torch.stack(out), torch.stack(bound)


@functools.lru_cache(maxsize=None)
def probe_select(kind, C, G, B, side="both", soft=False):
    """Inside a head's 32 channels a token is (address | payload), two balanced +-1 codes of 16: rows of mean 0 and variance 1, so norm1 gives +-1 exactly.  q copies the address
    x L, k the payload into the same 16 dimensions, v is the identity + an integer bias, the projections are identities.  A query selects the one key whose payload IS its address
    (dot product 16; every other key <= 12).
      "D", "C": image token t selects meta token pi(t) (D only); (image, head, meta token) selects image token sigma (_targets).
      "S", "S2": image token t selects image token pi(t) = (N - 1 - t + 5 h + 11 b) mod N (the far side of the image: another workgroup); the meta tokens select among themselves.
      "D2": q1 = k1 and q2 = k2, so both directions see ONE score matrix and cannot both be one-hot: side = "x" builds the image tokens' selection (x_out exact), side = "c" the
      meta tokens' (c_out exact); the other output is a softmax over ties and is not compared (info.exact says which is).
    soft = True: the same operands with L / 128 (L / 32 for the meta queries of D / C blocks) -- the runner-up lies 1.25 .. 2.5 (5 .. 10) below the selected score in the exp2
    domain, every softmax row is a graded mixture that moves
    with the scale, and the log-sum-exp combine over the workgroups rescales partials whose maxima differ by a few units.  The reference is the softmax in float64 of the closed-form
    scores L s (address . payload); info.x_bound / c_bound are the elementwise bounds of _soft_attention."""
    fam, N, NH = family(kind), G * G, C // 32
    cd = codes()
    s_x, s_c = scales(kind, C, G)
    Lx, Lc = _lscale(s_x), _lscale(s_c)
    if soft:
        assert kind != "D2"
        # (the meta queries of D / C blocks see hundreds to thousands of keys, dozens of them one step below the top: four times the step keeps the top key's weight near 1/2)
        Lx, Lc = Lx / 128.0, Lc / (32.0 if fam in ("D", "C") else 128.0)
    if kind == "D2":          # (both gains multiply every score: keep the one of the side under test)
        Lx, Lc = (Lx, 1.0) if side == "x" else (1.0, Lc)
    bi, hi_, ti, mi = torch.arange(B).view(B, 1, 1), torch.arange(NH).view(1, NH, 1), torch.arange(N).view(1, 1, N), torch.arange(M).view(1, 1, M)
    pay_x = _PAY0 + (4099 * ti + 131 * hi_ + 977 * bi) % (N_CODES - _PAY0)          # [B, NH, N]: distinct codes over the tokens of an (image, head)
    pay_c = (5 * mi + hi_ + 3 * bi) % M + 0 * ti[..., :1]                            # [B, NH, 16]: a permutation of codes 0 .. 15
    assert all(len(set(pay_x[b, h].tolist())) == N for b in range(B) for h in range(NH)) and all(sorted(pay_c[b, h].tolist()) == list(range(M)) for b in range(B) for h in range(NH))
    info = dict(Lx=Lx, Lc=Lc, exact=("x", "c"))
    if fam in ("S",):
        pi = (N - 1 - ti + 5 * hi_ + 11 * bi) % N                                    # [B, NH, N]
        rho = (5 * mi + hi_ + 3 + bi) % M                                            # [B, NH, 16]
        adr_x, adr_c = pay_x.gather(2, pi), pay_c.gather(2, rho)
        wg = torch.zeros(N, dtype=torch.int64)
        for w, (lo, hi) in enumerate(workgroups(kind, G)):
            wg[lo:hi + 1] = w
        info["cross_fraction"] = float((wg[pi] != wg[ti.expand_as(pi)]).double().mean())
        info["margin_x"] = _margin(cd[adr_x], cd[pay_x], pi, Lx * s_x)
        info["margin_c"] = _margin(cd[adr_c], cd[pay_c], rho, Lc * s_c)
    else:
        pi = (7 * ti + 3 * (ti // G) + 5 * hi_ + bi) % M                             # [B, NH, N]: the meta token an image token selects
        sigma = _targets(kind, C, G, B)                                               # [B, NH, 16]
        assert all(len(set(sigma[b, h].tolist())) == M for b in range(B) for h in range(NH))
        adr_x, adr_c = pay_c.gather(2, pi), pay_x.gather(2, sigma)
        if kind == "D2":
            # one score matrix: q_t . k_m with q_t the image token's address code and k_m the meta token's (its "address" half; the payload halves are not projected)
            if side == "x":          # image token t selects meta token pi(t): the meta codes are distinct
                adr_c = pay_c
            else:                    # meta token m selects image token sigma(m): the image codes are distinct
                adr_x = pay_x
                adr_c = pay_x.gather(2, sigma)
            info["exact"] = (side,)
            if side == "x":
                info["margin_x"] = _margin(cd[adr_x], cd[adr_c], pi, Lx * Lc * s_x)
            else:
                info["margin_c"] = _margin(cd[adr_c], cd[adr_x], sigma, Lx * Lc * s_c)
        else:
            if kind == "D":
                info["margin_x"] = _margin(cd[adr_x], cd[pay_c], pi, Lx * s_x)
                info["metas_selected"] = sorted(set(pi.flatten().tolist()))
            info["margin_c"] = _margin(cd[adr_c], cd[pay_x], sigma, Lc * s_c)
        wgs = workgroups(kind, G)
        hit = sigma.flatten().tolist()
        info["wg_covered"] = sorted({w for w, (lo, hi) in enumerate(wgs) for t in hit if lo <= t <= hi})
        info["wg_first"] = sorted({w for w, (lo, hi) in enumerate(wgs) if lo in hit})
        info["wg_last"] = sorted({w for w, (lo, hi) in enumerate(wgs) if hi in hit})
        info["nwg"], info["nsel"] = len(wgs), len(hit)
    # tokens: [B, tokens, NH, 32] = (address | payload)
    x = torch.cat([cd[adr_x], cd[pay_x]], -1).permute(0, 2, 1, 3).reshape(B, N, C).double()
    c = torch.cat([cd[adr_c], cd[pay_c]], -1).permute(0, 2, 1, 3).reshape(B, M, C).double()
    for t in (x, c):          # norm1 (1, 0) of such a row is +- rsqrt(1 + eps): +-1 as a bf16 operand
        assert bool((t.abs() == 1).all()) and bool((t.reshape(*t.shape[:2], NH, 2, 16).sum(-1) == 0).all())
    ch = torch.arange(C)
    bv1, bv2 = ((3 * ch) % 7 - 3).float(), ((5 * ch) % 9 - 4).float()
    eye, z = torch.eye(C), torch.zeros(C)
    blk = zero_block(kind, C)
    if fam == "D":
        blk["attn.qkv1.weight"] = torch.cat([_sel_rows(C, Lx, 0), _sel_rows(C, 1.0, 16), eye], 0).to(torch.bfloat16)
        blk["attn.qkv2.weight"] = torch.cat([_sel_rows(C, Lc, 0), _sel_rows(C, 1.0, 16), eye], 0).to(torch.bfloat16)
        blk["attn.qkv1.bias"], blk["attn.qkv2.bias"] = torch.cat([z, z, bv1]), torch.cat([z, z, bv2])
        blk["attn.proj_x.weight"] = blk["attn.proj_c.weight"] = eye.to(torch.bfloat16)
    elif fam == "D2":
        blk["attn.qv1.weight"] = torch.cat([_sel_rows(C, Lx, 0), eye], 0).to(torch.bfloat16)
        blk["attn.kv2.weight"] = torch.cat([_sel_rows(C, Lc, 0), eye], 0).to(torch.bfloat16)
        blk["attn.qv1.bias"], blk["attn.kv2.bias"] = torch.cat([z, bv1]), torch.cat([z, bv2])
        blk["attn.proj_x.weight"] = blk["attn.proj_c.weight"] = eye.to(torch.bfloat16)
    elif fam == "S":
        assert Lx == Lc
        blk["attn.qkv.weight"] = torch.cat([_sel_rows(C, Lx, 0), _sel_rows(C, 1.0, 16), eye], 0).to(torch.bfloat16)
        blk["attn.qkv.bias"] = torch.cat([z, z, bv1])
        blk["attn.proj.weight"] = eye.to(torch.bfloat16)
        bv2 = bv1
    else:
        blk["attn.q.weight"] = _sel_rows(C, Lc, 0).to(torch.bfloat16)
        blk["attn.kv.weight"] = torch.cat([_sel_rows(C, 1.0, 16), eye], 0).to(torch.bfloat16)
        blk["attn.kv.bias"] = torch.cat([z, bv1])
        blk["attn.proj.weight"] = eye.to(torch.bfloat16)
    # per head the value rows (the token itself, +-1, + the v bias) of the keys: [B, NH, keys, 32]
    xs, cs = x.reshape(B, N, NH, 32).permute(0, 2, 1, 3), c.reshape(B, M, NH, 32).permute(0, 2, 1, 3)
    if fam == "S":
        key_x, val_x, want_x, key_c, val_c, want_c = pay_x, xs, pi, pay_c, cs, rho
    else:
        key_x, val_x, want_x, key_c, val_c, want_c = (adr_c if kind == "D2" else pay_c), cs, pi, (adr_x if kind == "D2" else pay_x), xs, sigma
    if soft:
        ax, bx = _soft_attention(cd[adr_x], cd[key_x], val_x, bv2.double().reshape(NH, 1, 32), Lx * s_x * LOG2E)
        ac, bc = _soft_attention(cd[adr_c], cd[key_c], val_c, bv1.double().reshape(NH, 1, 32), Lc * s_c * LOG2E)
        ax, bx, ac, bc = [t.permute(0, 2, 1, 3).reshape(B, -1, C) for t in (ax, bx, ac, bc)]
        x_ref, c_ref = x + ax, c + ac
        info["x_bound"], info["c_bound"] = 2.0 ** -8 * x_ref.abs() + bx, 2.0 ** -8 * c_ref.abs() + bc
    else:          # the gather
        take_x = val_x.gather(2, want_x.unsqueeze(-1).expand(-1, -1, -1, 32))
        take_c = val_c.gather(2, want_c.unsqueeze(-1).expand(-1, -1, -1, 32))
        x_ref = x + take_x.permute(0, 2, 1, 3).reshape(B, N, C) + bv2.double()
        c_ref = c + take_c.permute(0, 2, 1, 3).reshape(B, M, C) + bv1.double()
    if kind == "C":
        x_ref = x.clone()
    return _probe(kind, C, G, [blk], x.to(torch.bfloat16), c.to(torch.bfloat16), x_ref, c_ref, **info)


# ------------------------------------------------------------------------------------------------
# (c) the MLP, one hidden unit at a time
def gelu_poly(x):
    """gelu_poly2 (csrc/common.h): x (1/2 + s q(s^2)), s = clamp(x / 4, -1, 1), in fp32 (as _gelu_poly of tests/test_parity_budget_gpu.py)."""
    x = x.float()
    s = (x * 0.25).clamp(-1.0, 1.0)
    u = s * s
    q = torch.full_like(u, -1.6300047636032104)
    for k in (7.93373966217041, -16.877059936523438, 20.921268463134766, -17.09065055847168, 9.8812894821167, -4.233964920043945, 1.595382571220398):
        q = q * u + k
    return (x * (s * q + 0.5)).double()


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def mlp_unit(C, p):
    """[C]: the hidden unit output channel o shows in pack p.  Over p = 0 .. 3 every one of the 4 C units is shown once, and a channel walks all four quarters of the hidden layer."""
    o = torch.arange(C)
    return C * ((p + o) % 4) + (5 * o + 3) % C


@functools.lru_cache(maxsize=None)
def _balanced_tokens(B, T, C, salt):
    """[B, T, C] of +-1 with equal counts inside every 32-channel segment, different per token."""
    cd = codes()
    idx = _hash((B, T, C // 16), salt) % N_CODES
    return cd[idx].reshape(B, T, C).double()


@functools.lru_cache(maxsize=None)
def probe_mlp(kind, C, G, B, p):
    """mlp.0.weight row j: one non-zero entry s_j (from 1/4 to 6 in steps of 1/4: the clamp of the polynomial at |u| = 4 is crossed) at the channel that shows unit j, bias a
    multiple of 1/16 in [-3/16, 3/16]: with norm2(x) = +-1 the pre-activation u = +-s_j + b_j is exact in fp32 and has the token's sign.  mlp.3.weight row o: a single 1 at unit
    mlp_unit(C, p)[o].  The attention matrices are NOT zero, the projections are: the branch must add exactly 0.
    x_ref / c_ref: token + bf16(gelu_poly(u)); info.x_erf / c_erf: token + erf GELU(u); info.hx / hc: the hidden value each output element shows (for the bounds)."""
    N, H = G * G, 4 * C
    x, c = _balanced_tokens(B, N, C, 7), _balanced_tokens(B, M, C, 8)
    j = torch.arange(H)
    s = (1 + (37 * j) % 24).double() / 4.0
    sign = torch.ones(H, dtype=torch.float64)
    col = torch.zeros(H, dtype=torch.int64)
    for q in range(4):
        col[mlp_unit(C, q)] = torch.arange(C)          # unit j reads the channel it is shown on (in the one pack that shows it)
    b1 = ((13 * j) % 7 - 3).double() / 16.0
    blk = zero_block(kind, C)
    w1 = torch.zeros(H, C, dtype=torch.float64)
    w1[j, col] = s * sign
    unit = mlp_unit(C, p)
    w2 = torch.zeros(C, H)
    w2[torch.arange(C), unit] = 1.0
    blk["mlp.0.weight"], blk["mlp.0.bias"], blk["mlp.3.weight"] = w1.to(torch.bfloat16), b1.float(), w2.to(torch.bfloat16)
    assert torch.equal(blk["mlp.0.weight"].double(), w1) and float(s.min()) == 0.25 and float(s.max()) == 6.0
    # a non-zero attention in front of a zero projection: the branch must contribute exactly 0
    for n in ATTN_SHAPES[family(kind)]:
        if "proj" not in n:
            r = blk[n + ".weight"].shape[0]
            blk[n + ".weight"] = ((_hash((r, C), 11) % 5 - 2).float() / 8.0).to(torch.bfloat16)
            blk[n + ".bias"] = (_hash((r,), 12) % 5 - 2).float() / 4.0

    def branch(t):
        assert torch.equal(col[unit], torch.arange(C))
        u = t * (s * sign)[unit] + b1[unit]          # [B, T, C]: the pre-activation of the unit each output channel shows
        assert bool((u.float().double() == u).all())
        h = gelu_poly(u).to(torch.bfloat16).double()
        g = gelu_erf(u)
        # the erf bound must hold for ANY hidden value within the polynomial's 1.9e-4 of the erf GELU, through the bf16 roundings of the hidden value and of the output (the
        # output is monotone in the hidden value: the two ends of the interval decide).  It would not with a residual of the opposite sign (token + h cancels, the rounding of h
        # does not) -- hence unit j reads the channel it is shown on with a positive weight: sign(h) = sign(token)
        for e in (-1.9e-4, 1.9e-4):
            out = (t.float() + (g + e).float().to(torch.bfloat16).float()).to(torch.bfloat16).double()
            sound.append(bool(((out - (t + g)).abs() <= 2.0 ** -8 * (t + g).abs() + 1.9e-4).all()))
        return u, h, t + h, t + g

    sound = []
    ux, hx, x_ref, x_erf = branch(x)
    uc, hc, c_ref, c_erf = branch(c)
    if kind == "C":
        x_ref = x_erf = x.clone()
        hx = torch.zeros_like(x)
    return _probe(kind, C, G, [blk], x.to(torch.bfloat16), c.to(torch.bfloat16), x_ref, c_ref, x_erf=x_erf, c_erf=c_erf, hx=hx, hc=hc, units=unit.tolist(), erf_bound_sound=all(sound),
                  u_min=float(min(ux.min(), uc.min())), u_max=float(max(ux.max(), uc.max())), u_small=float((uc.abs() <= 1.0).double().mean()))


def mlp_bounds(ref_poly, ref_erf, h):
    """Elementwise |error| bounds of an output element token + h, h = bf16(GELU(u)), u exact.
    Against the polynomial reference: the bf16 store of the output (2^-8 |ref|), one bf16 step of h where the fp32 evaluation of the polynomial (any order of its fused operations)
    lands on the other side of a rounding boundary than the emulation (2^-7 |h|), the fp32 sum (1e-6).
    Against the erf GELU: 2^-8 |ref| + 1.9e-4, the polynomial's documented bound (csrc/common.h) -- the bound of tests/test_stem_exact_gpu.py."""
    return 2.0 ** -8 * ref_poly.abs() + 2.0 ** -7 * h.abs() + 1e-6, 2.0 ** -8 * ref_erf.abs() + 1.9e-4
