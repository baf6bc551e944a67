"""The head losses on the GPU (csrc/headloss.hip; lemevit_amd/detection.py: rpn_head_loss, bbox_head_loss).

Against the float64 oracle no tolerance is fixed in advance.  The error of a loss value is |x - ref| / S with S = w / avg sum |terms| from the oracle (every term
of these losses is non-negative, so S is the oracle's loss itself; a loss whose S is 0 must be exactly 0); the error of a gradient tensor is max |g - ref| / max |ref|.
For each family -- RPN cls, RPN bbox, R-CNN cls, R-CNN bbox; values and gradients separately -- the bound of EVERY case is twice the LARGEST error the stock
formulation reaches in fp32 on the GPU over all of the family's cases (fp32 inputs and bf16-rounded inputs), plus 2^-22: a lucky zero of the stock side on a
one-term case does not set the bar, and neither side is privileged.  bf16: the oracle and the stock side get the bf16-rounded inputs; values use the same bound,
gradient elements additionally 2^-8 |ref| for the one rounding of the output.  ``acc`` and all counts are equal exactly.  ``pytest -s`` prints error / bound per family.

Measured on an MI355X, the largest error of the kernels over a family's cases / the family's bound:
    fp32 maps    RPN: cls value 5.5e-8 / 3.7e-7, bbox value 3.1e-6 / 6.6e-6, cls gradient 1.2e-7 / 4.7e-7, bbox gradient 4.1e-5 / 8.3e-5
                 R-CNN: cls value 4.0e-8 / 4.0e-7, bbox value 1.2e-7 / 4.9e-7, cls gradient 1.9e-7 / 5.1e-7, bbox gradient 2.9e-6 / 6.0e-6
    bf16 maps    values under the same bounds: RPN 4.1e-8, 3.1e-6; R-CNN 1.0e-7, 8.1e-8; gradients (before the 2^-8 |ref| allowance of the rounded output):
                 RPN 3.2e-3, 3.0e-3; R-CNN 3.5e-3, 3.4e-3 of the largest gradient

Exact (bit-for-bit) properties: two calls agree; contiguous, channels-last and channel-sliced maps agree, and so do the 16-byte and the byte-wise mask paths;
row-strided predictions agree with contiguous ones; buffers pre-filled with NaN come back with exact +0.0 at every unsampled / non-live / padding position; a
level without samples has loss exactly 0; a gout of 2 doubles the gradient of exactly its own loss; torch.autograd through the node gives the kernel's gradient;
the nodes' forward with ``stats`` / ``workspace`` supplied allocates nothing, and reusing a supplied ``stats`` before the backward raises.
The chain assigner -> sampler (-> gather) -> loss -> backward launch replays from one captured graph after draw() and after new ground-truth counts, equal to
eager (the forward through the node, the backward launch through ops.*_loss_bwd with the test's buffers: see test_rpn_chain_under_capture).
"""
import functools

import numpy as np
import pytest
import torch

import gen_coder_golden as cgen
import gen_headloss_golden as gen
from lemevit_amd import ops
from lemevit_amd.detection import (MaxIoUAssigner, OBBRandomSampler, RandomSampler, bbox_head_loss, bbox_head_loss_torch, reference_bbox_head_loss,
                                   reference_rpn_head_loss, rpn_head_loss, rpn_head_loss_torch)

pytestmark = pytest.mark.gpu
DEV = "cuda"
M6, M5 = (0.0,) * 6, (0.0,) * 5
SLACK = 2.0 ** -22
NAN = float("nan")


def bits(t):
    """the bit patterns of a float32 / bfloat16 tensor, in its shape"""
    t = t.detach().contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)) if t.dim() else bits(t.reshape(1)).reshape(())


def same(a, b) -> bool:
    """bit for bit (NaN == NaN, +0.0 != -0.0); integer tensors: equal"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b)


def f64(t):
    return t.detach().double().cpu().numpy()


def value_err(x: float, ref: float) -> float:
    return 0.0 if x == ref else (abs(x - ref) / ref if ref > 0 else float("inf"))


def grad_err(g, ref) -> float:
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if not np.asarray(g).any() else float("inf")
    return float(np.abs(g - ref).max() / scale)


# ---- the two sides and the oracle ----------------------------------------------------------------------------------------------------------------------------------
def rpn_aux(c, mask=None):
    return (c["anchors"].to(DEV), c["gts"].to(DEV), c["gt_inds"].to(DEV), (c["mask"] if mask is None else mask).to(DEV), c["counts"].to(DEV))


def rpn_maps(c, dtype=torch.float32):
    return [t.to(DEV).to(dtype) for t in c["cls_scores"] + c["bbox_preds"]]


def rpn_native(c, maps=None, gout=None, mask=None, aux=None):
    """(stats, the 2 L gradient maps written into NaN-filled buffers) of the two kernels' entry points"""
    maps = rpn_maps(c) if maps is None else maps
    aux = rpn_aux(c, mask) if aux is None else aux
    L = len(maps) // 2
    stats = ops.rpn_loss_fwd(maps[:L], maps[L:], *aux, M6, gen.RPN_STDS, gen.RPN_BETA, 1.0, 1.0, stats=torch.full((2 * L + 3,), NAN, device=DEV))
    grads = [torch.full_like(m, NAN) for m in maps]
    ops.rpn_loss_bwd(maps[:L], maps[L:], *aux, M6, gen.RPN_STDS, gen.RPN_BETA, 1.0, 1.0, stats, gout, grads[:L], grads[L:])
    return stats, grads


@functools.lru_cache(maxsize=None)
def rpn_oracle(name, bf16):
    c = gen.rpn_case(name, bf16)
    return reference_rpn_head_loss(c["cls_scores"], c["bbox_preds"], c["anchors"], c["gts"], c["gt_inds"], c["mask"], c["counts"], M6, gen.RPN_STDS, gen.RPN_BETA)


def rpn_stock(c):
    """the stock formulation in fp32 on the GPU: (loss_cls [L], loss_bbox [L], gradients of the sum of all losses)"""
    maps = [m.requires_grad_() for m in rpn_maps(c)]
    L = len(maps) // 2
    out = rpn_head_loss_torch(maps[:L], maps[L:], *rpn_aux(c), M6, gen.RPN_STDS, gen.RPN_BETA)
    (out["loss_rpn_cls"].sum() + out["loss_rpn_bbox"].sum()).backward()
    return f64(out["loss_rpn_cls"]), f64(out["loss_rpn_bbox"]), [f64(m.grad) for m in maps]


def rpn_errors(o, loss_cls, loss_bbox, grads):
    """the four family measures of one case: (cls value, bbox value, cls gradient, bbox gradient), each the largest over the levels"""
    L = len(o["loss_cls"])
    return (max(value_err(float(loss_cls[l]), o["loss_cls"][l]) for l in range(L)), max(value_err(float(loss_bbox[l]), o["loss_bbox"][l]) for l in range(L)),
            max(grad_err(grads[l], o["dcls"][l]) for l in range(L)), max(grad_err(grads[L + l], o["dreg"][l]) for l in range(L)))


def rcnn_aux(c):
    return (c["rois"].to(DEV), c["gts"].to(DEV), c["s_gt_inds"].to(DEV), c["s_labels"].to(DEV), c["counts"].to(DEV))


def rcnn_native(c, preds=None, gout=None):
    z, p = (c["cls_score"].to(DEV), c["bbox_pred"].to(DEV)) if preds is None else preds
    aux = rcnn_aux(c)
    stats = ops.rcnn_loss_fwd(z, p, *aux, M5, gen.RCNN_STDS, gen.RCNN_BETA, 1.0, 1.0, stats=torch.full((7,), NAN, device=DEV))
    dz, dp = torch.full(z.shape, NAN, device=DEV, dtype=z.dtype), torch.full(p.shape, NAN, device=DEV, dtype=p.dtype)
    ops.rcnn_loss_bwd(z, p, *aux, M5, gen.RCNN_STDS, gen.RCNN_BETA, 1.0, 1.0, stats, gout, dz, dp)
    return stats, dz, dp


@functools.lru_cache(maxsize=None)
def rcnn_oracle(name, bf16):
    c = gen.rcnn_case(name, bf16)
    return reference_bbox_head_loss(c["cls_score"], c["bbox_pred"], c["rois"], c["gts"], c["s_gt_inds"], c["s_labels"], c["counts"], M5, gen.RCNN_STDS, c["K"],
                                    gen.RCNN_BETA)


def rcnn_stock(c):
    z, p = c["cls_score"].to(DEV).requires_grad_(), c["bbox_pred"].to(DEV).requires_grad_()
    out = bbox_head_loss_torch(z, p, *rcnn_aux(c), M5, gen.RCNN_STDS, c["K"], c["C"] == 1, gen.RCNN_BETA)
    (out["loss_cls"] + out["loss_bbox"]).backward()
    return float(out["loss_cls"]), float(out["loss_bbox"]), float(out["acc"]), f64(z.grad), f64(p.grad)


def rcnn_errors(o, loss_cls, loss_bbox, dz, dp):
    return (value_err(loss_cls, o["loss_cls"]), value_err(loss_bbox, o["loss_bbox"]), grad_err(dz, o["dcls"]), grad_err(dp, o["dbbox"]))


FAMILIES = ("cls value", "bbox value", "cls gradient", "bbox gradient")


@functools.lru_cache(maxsize=None)
def bounds(head):
    """per family: 2 x the largest error of the stock formulation (fp32, on the GPU) over all of the head's cases, + 2^-22"""
    worst = [0.0] * 4
    names = gen.RPN_CASES if head == "rpn" else gen.RCNN_CASES
    for name in names:
        for bf16 in (False, True):
            if head == "rpn":
                e = rpn_errors(rpn_oracle(name, bf16), *rpn_stock(gen.rpn_case(name, bf16)))
            else:
                lc, lb, _, dz, dp = rcnn_stock(gen.rcnn_case(name, bf16))
                e = rcnn_errors(rcnn_oracle(name, bf16), lc, lb, dz, dp)
            worst = [max(w, x) for w, x in zip(worst, e)]
    assert all(np.isfinite(w) for w in worst), (head, worst)
    return tuple(2.0 * w + SLACK for w in worst)


def check_grad(g, ref, bound, bf16, what):
    """max |g - ref| <= bound max |ref| (+ 2^-8 |ref| element-wise for a bf16 output)"""
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    room = bound * scale + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)
    assert (np.abs(g - ref) <= room).all(), (what, float(np.abs(g - ref).max()), bound * scale)


# ---- against the float64 oracle ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(gen.RPN_CASES))
def test_rpn_against_oracle(name, bf16):
    """losses, counts, 1 / avg and all gradient maps against the oracle within the family bounds; NaN-filled buffers come back fully written, with exact +0.0 at
    every unsampled anchor and every row that is not live; a level without samples has loss exactly 0"""
    c, o, lim = gen.rpn_case(name, bf16), rpn_oracle(name, bf16), bounds("rpn")
    L = len(c["levels"])
    stats, grads = rpn_native(c, rpn_maps(c, torch.bfloat16 if bf16 else torch.float32))
    s = f64(stats)
    assert s[2 * L] == o["n_pos"] and s[2 * L + 1] == o["n_neg"] and s[2 * L + 2] == float(np.float32(1.0 / o["avg"]))
    e = rpn_errors(o, s[:L], s[L:2 * L], [f64(g) for g in grads])
    print(f"    rpn {name} {'bf16' if bf16 else 'fp32'}: " + ", ".join(f"{f} {x:.3e} / {b:.3e}" for f, x, b in zip(FAMILIES, e, lim)))
    assert e[0] <= lim[0] and e[1] <= lim[1]
    m = c["mask"].numpy()
    for l in range(L):
        check_grad(f64(grads[l]), o["dcls"][l], lim[2], bf16, f"dcls[{l}]")
        check_grad(f64(grads[L + l]), o["dreg"][l], lim[3], bf16, f"dreg[{l}]")
        H, W = c["levels"][l]
        ml = m[:, c["offsets"][l]:c["offsets"][l + 1]]
        unsampled = torch.from_numpy((ml == 0).reshape(c["B"], H, W, c["A"]).transpose(0, 3, 1, 2).copy())
        assert not bits(grads[l]).cpu()[unsampled].any(), "exact +0.0 at unsampled anchors"
        dead = torch.from_numpy(o["dreg"][l] == 0.0)
        assert not torch.isnan(grads[L + l]).any() and not bits(grads[L + l]).cpu()[dead].any(), "exact +0.0 on rows that are not live"
        if not (ml != 0).any():
            assert s[l] == 0.0 and s[L + l] == 0.0 and not bits(grads[l]).any() and not bits(grads[L + l]).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(gen.RCNN_CASES))
def test_rcnn_against_oracle(name, bf16):
    """losses and both gradients within the family bounds; acc and the counts exactly; padding rows and every set but the chosen one of a live row exactly +0.0"""
    c, o, lim = gen.rcnn_case(name, bf16), rcnn_oracle(name, bf16), bounds("rcnn")
    dt = torch.bfloat16 if bf16 else torch.float32
    stats, dz, dp = rcnn_native(c, (c["cls_score"].to(DEV).to(dt), c["bbox_pred"].to(DEV).to(dt)))
    s = f64(stats)
    assert s[3] == o["n_valid"] and s[4] == o["n_live"] and s[2] == float(np.float32(o["acc"]))
    assert s[5] == (float(np.float32(1.0 / max(o["n_valid"], 1)))) and s[6] == (float(np.float32(1.0 / o["n_valid"])) if o["n_valid"] else 0.0)
    e = rcnn_errors(o, s[0], s[1], f64(dz), f64(dp))
    print(f"    rcnn {name} {'bf16' if bf16 else 'fp32'}: " + ", ".join(f"{f} {x:.3e} / {b:.3e}" for f, x, b in zip(FAMILIES, e, lim)))
    assert e[0] <= lim[0] and e[1] <= lim[1]
    check_grad(f64(dz), o["dcls"], lim[2], bf16, "dcls")
    check_grad(f64(dp), o["dbbox"], lim[3], bf16, "dbbox")
    pad = torch.from_numpy(c["s_labels"].numpy() < 0)
    assert not bits(dz).cpu()[pad].any() and not torch.isnan(dz).any() and not torch.isnan(dp).any()
    assert not bits(dp).cpu()[torch.from_numpy(o["dbbox"] == 0.0)].any(), "exact +0.0 outside the chosen set of a live row"
    if name == "r1":          # the stock side's accuracy is the same number
        assert rcnn_stock(c)[2] == o["acc"]


def test_rcnn_empty():
    """R == 0 writes zero stats and nothing else"""
    c = gen.rcnn_case("r1")
    aux = (torch.zeros(0, 6, device=DEV), c["gts"].to(DEV), torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), None)
    stats = ops.rcnn_loss_fwd(torch.zeros(0, 16, device=DEV), torch.zeros(0, 5, device=DEV), *aux, M5, gen.RCNN_STDS, stats=torch.full((7,), NAN, device=DEV))
    assert not bits(stats).any()
    ops.rcnn_loss_bwd(torch.zeros(0, 16, device=DEV), torch.zeros(0, 5, device=DEV), *aux, M5, gen.RCNN_STDS, 1.0, 1.0, 1.0, stats, None,
                      torch.zeros(0, 16, device=DEV), torch.zeros(0, 5, device=DEV))


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------------------------------
def channels_last(t):
    return t.contiguous(memory_format=torch.channels_last)


def channel_sliced(t):
    big = torch.full((t.shape[0], t.shape[1] + 5, t.shape[2], t.shape[3]), 0.25, device=t.device, dtype=t.dtype)
    big[:, 2:2 + t.shape[1]] = t
    return big[:, 2:2 + t.shape[1]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(gen.RPN_CASES))
def test_rpn_layouts_and_repeats(name, dtype):
    """two calls; contiguous, channels-last and channel-sliced maps (gradients in those layouts too); a mask at an odd address (the byte-wise path): the same bits"""
    c = gen.rpn_case(name, dtype == torch.bfloat16)
    maps = rpn_maps(c, dtype)
    stats, grads = rpn_native(c, maps)
    again = rpn_native(c, maps)
    assert same(stats, again[0]) and all(same(a, b) for a, b in zip(grads, again[1])), "a second call"
    for layout in (channels_last, channel_sliced):
        s2, g2 = rpn_native(c, [layout(m) for m in maps])
        assert same(stats, s2) and all(same(a, b) for a, b in zip(grads, g2)), layout.__name__
    mixed = [channels_last(m) if i % 2 else m for i, m in enumerate(maps)]
    s3, g3 = rpn_native(c, mixed)
    assert same(stats, s3) and all(same(a, b) for a, b in zip(grads, g3)), "levels in different layouts"
    buf = torch.zeros(c["B"] * c["N"] + 16, dtype=torch.uint8, device=DEV)
    odd = buf[1:1 + c["B"] * c["N"]].view(c["B"], c["N"])
    odd.copy_(c["mask"].to(DEV))
    assert odd.data_ptr() % 16 != 0
    aux = rpn_aux(c)
    s4, g4 = rpn_native(c, maps, aux=aux[:3] + (odd,) + aux[4:])
    assert same(stats, s4) and all(same(a, b) for a, b in zip(grads, g4)), "the byte-wise mask path"


@pytest.mark.parametrize("name", ["r65", "c15", "r1000"])
def test_rcnn_strides_and_repeats(name):
    c = gen.rcnn_case(name)
    z, p = c["cls_score"].to(DEV), c["bbox_pred"].to(DEV)
    stats, dz, dp = rcnn_native(c)
    again = rcnn_native(c)
    assert same(stats, again[0]) and same(dz, again[1]) and same(dp, again[2]), "a second call"
    zs, ps = cgen_strided(z), cgen_strided(p)
    s2, dz2, dp2 = rcnn_native(c, (zs, ps))
    assert zs.stride(0) == z.shape[1] + 3 and same(stats, s2) and same(dz, dz2) and same(dp, dp2), "row-strided predictions"
    dzs, dps = cgen_strided(torch.full_like(z, NAN)), cgen_strided(torch.full_like(p, NAN))
    ops.rcnn_loss_bwd(zs, ps, *rcnn_aux(c), M5, gen.RCNN_STDS, gen.RCNN_BETA, 1.0, 1.0, stats, None, dzs, dps)
    assert same(dzs.contiguous(), dz) and same(dps.contiguous(), dp), "row-strided gradients"


def cgen_strided(t):
    d = torch.full((t.shape[0], t.shape[1] + 3), 0.5, device=t.device, dtype=t.dtype)
    d[:, :t.shape[1]] = t
    return d[:, :t.shape[1]]


def test_rpn_without_negatives():
    """loss_bbox equals that of a call on the mask with the negatives removed, times the ratio of the two avg (to rounding: the family bound)"""
    def avg_of(m):
        return float((np.maximum((m == 1).sum(1), 1) + np.maximum(((m != 0) & (m != 1)).sum(1), 1)).sum())
    for name in gen.RPN_CASES:
        c = gen.rpn_case(name)
        L = len(c["levels"])
        only_pos = torch.where(c["mask"] == 1, 1, 0).to(torch.uint8)
        a, b = f64(rpn_native(c)[0]), f64(rpn_native(c, mask=only_pos)[0])
        ratio = avg_of(only_pos.numpy()) / avg_of(c["mask"].numpy())
        assert b[2 * L + 1] == 0 and a[2 * L] == b[2 * L]
        for l in range(L):
            assert value_err(a[L + l], b[L + l] * ratio) <= bounds("rpn")[1], (name, l)


def test_gout_scales_its_own_loss():
    """a gout of 2 for one loss doubles exactly the gradient map of that loss and leaves every other bit alone"""
    c = gen.rpn_case("ii")
    L = len(c["levels"])
    _, base = rpn_native(c)
    ones = rpn_native(c, gout=torch.ones(2 * L, device=DEV))[1]
    assert all(same(a, b) for a, b in zip(base, ones)), "null gout is ones"
    for j in range(2 * L):
        g = torch.ones(2 * L, device=DEV)
        g[j] = 2.0
        got = rpn_native(c, gout=g)[1]
        assert all(same(got[i], base[i] * 2 if i == j else base[i]) for i in range(2 * L)), j
    r = gen.rcnn_case("c15")
    _, dz, dp = rcnn_native(r)
    _, dz2, dp2 = rcnn_native(r, gout=torch.tensor([2.0, 1.0], device=DEV))
    assert same(dz2, dz * 2) and same(dp2, dp)
    _, dz3, dp3 = rcnn_native(r, gout=torch.tensor([1.0, 2.0], device=DEV))
    assert same(dz3, dz) and same(dp3, dp * 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_autograd_gives_the_kernels_gradient(dtype):
    """rpn_head_loss / bbox_head_loss are one node each: their outputs are the kernels' stats, torch.autograd through them gives the backward kernels' gradients
    (per-loss upstream gradients reach the kernel through gout), nothing else is differentiable and acc carries no gradient"""
    c = gen.rpn_case("ii", dtype == torch.bfloat16)
    L = len(c["levels"])
    maps = [m.requires_grad_() for m in rpn_maps(c, dtype)]
    anchors, gts, gt_inds, mask, counts = rpn_aux(c)
    out = rpn_head_loss(maps[:L], maps[L:], anchors, gts, gt_inds, mask, counts)
    gout = torch.linspace(0.5, 1.5, 2 * L, device=DEV)
    stats, want = rpn_native(c, [m.detach() for m in maps], gout=gout)
    assert same(out["loss_rpn_cls"], stats[:L]) and same(out["loss_rpn_bbox"], stats[L:2 * L])
    fn = out["loss_rpn_cls"].grad_fn
    assert fn is not None and fn is out["loss_rpn_bbox"].grad_fn, "one node"
    ((out["loss_rpn_cls"] * gout[:L]).sum() + (out["loss_rpn_bbox"] * gout[L:]).sum()).backward()
    assert all(same(m.grad, w) for m, w in zip(maps, want))
    r = gen.rcnn_case("r257", dtype == torch.bfloat16)
    z, p = r["cls_score"].to(DEV).to(dtype).requires_grad_(), r["bbox_pred"].to(DEV).to(dtype).requires_grad_()
    rois, rg, ri, rl, rc = rcnn_aux(r)
    out = bbox_head_loss(z, p, rois, rg, ri, rl, rc, num_classes=r["K"])
    stats, dz, dp = rcnn_native(r, (z.detach(), p.detach()), gout=torch.tensor([0.5, 1.5], device=DEV))
    assert same(out["loss_cls"], stats[0]) and same(out["loss_bbox"], stats[1]) and same(out["acc"], stats[2]) and not out["acc"].requires_grad
    assert out["loss_cls"].grad_fn is out["loss_bbox"].grad_fn
    (0.5 * out["loss_cls"] + 1.5 * out["loss_bbox"]).backward()
    assert same(z.grad, dz) and same(p.grad, dp)


def _allocations() -> int:
    return int(torch.cuda.memory_stats()["allocation.all.allocated"])


def test_supplied_buffers():
    """``stats`` / ``workspace`` supplied: the forward of both nodes allocates nothing and returns views of ``stats`` with the bits of an allocating call; backward
    through autograd then gives the same gradients; and a supplied ``stats`` handed to a second call before the first one's backward makes that backward raise
    (it would read the second call's 1 / avg) instead of giving wrong gradients"""
    c = gen.rpn_case("ii")
    L = len(c["levels"])
    maps = [m.requires_grad_() for m in rpn_maps(c)]
    aux = rpn_aux(c)
    want = rpn_head_loss(maps[:L], maps[L:], *aux)
    (want["loss_rpn_cls"].sum() + want["loss_rpn_bbox"].sum()).backward()
    want_g = [m.grad.clone() for m in maps]
    stats, ws = torch.full((2 * L + 3,), NAN, device=DEV), torch.empty(ops.rpn_loss_workspace_bytes(c["B"], c["N"]), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = _allocations()
    out = rpn_head_loss(maps[:L], maps[L:], *aux, stats=stats, workspace=ws)
    assert _allocations() == before, "the forward allocated"
    assert out["loss_rpn_cls"].data_ptr() == stats.data_ptr() and same(out["loss_rpn_cls"], want["loss_rpn_cls"]) and same(out["loss_rpn_bbox"], want["loss_rpn_bbox"])
    for m in maps:
        m.grad = None
    (out["loss_rpn_cls"].sum() + out["loss_rpn_bbox"].sum()).backward()
    assert all(same(m.grad, g) for m, g in zip(maps, want_g))
    first = rpn_head_loss(maps[:L], maps[L:], *aux, stats=stats, workspace=ws)
    total = first["loss_rpn_cls"].sum() + first["loss_rpn_bbox"].sum()
    rpn_head_loss(maps[:L], maps[L:], *aux, stats=stats, workspace=ws)          # the same stats again, before the backward of `first`
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        total.backward()
    r = gen.rcnn_case("r257")
    z, p = r["cls_score"].to(DEV).requires_grad_(), r["bbox_pred"].to(DEV).requires_grad_()
    raux = rcnn_aux(r)
    want = bbox_head_loss(z, p, *raux, num_classes=r["K"])
    rstats, rws = torch.full((7,), NAN, device=DEV), torch.empty(ops.rcnn_loss_workspace_bytes(r["R"]), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = _allocations()
    out = bbox_head_loss(z, p, *raux, num_classes=r["K"], stats=rstats, workspace=rws)
    assert _allocations() == before, "the forward allocated"
    assert all(same(out[k], want[k]) for k in ("loss_cls", "loss_bbox", "acc")) and out["loss_cls"].data_ptr() == rstats.data_ptr()
    (want["loss_cls"] + want["loss_bbox"]).backward()
    gz, gp = z.grad.clone(), p.grad.clone()
    z.grad = p.grad = None
    (out["loss_cls"] + out["loss_bbox"]).backward()
    assert same(z.grad, gz) and same(p.grad, gp)


# ---- the chain under capture -------------------------------------------------------------------------------------------------------------------------------------------
def _capture(run):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = _allocations()
        out = run()
        after = _allocations()
    return graph, out, after - before


def test_rpn_chain_under_capture():
    """assign_batched -> sample_batched -> rpn_head_loss -> its backward launch in ONE captured graph (single stream, every buffer supplied: no allocation inside
    the capture); replays after draw() and after new ground-truth counts equal the eager results for the same key, bit for bit.  The forward goes through the
    node with ``stats`` / ``workspace`` supplied; the backward launch is the node's own (ops.rpn_loss_bwd with the test's buffers, which
    test_autograd_gives_the_kernels_gradient shows to be what torch.autograd runs).  Capturing ``.backward()`` through the node is not claimed and not run here:
    an earlier form of the node (caller-supplied gout / grads buffers filled by slice copies in its backward) ended a capture in a segmentation fault of the
    process, the cause was not found, and that surface was taken out."""
    A, levels, B, G = 3, ((8, 8), (4, 4), (2, 2), (1, 1)), 2, 7
    N = sum(h * w * A for h, w in levels)
    cc = cgen.chain_case(N, G)
    anchors = cc["anchors"].to(DEV)
    gts = cc["gts"].to(DEV)[None].repeat(B, 1, 1).contiguous()
    hulls = torch.from_numpy(cgen.hull(cc["gts"].double().numpy()).astype(np.float32)).to(DEV)[None].repeat(B, 1, 1).contiguous()
    counts = torch.tensor([7, 7], dtype=torch.int32, device=DEV)
    maps = [(0.5 * torch.from_numpy(cgen.det_uniform(B * ch * A * h * w, 77 + 3 * i + ch)).float().reshape(B, ch * A, h, w)).to(DEV).requires_grad_()
            for ch in (1, 6) for i, (h, w) in enumerate(levels)]
    L = len(levels)
    assigner = MaxIoUAssigner(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True)
    sampler = RandomSampler(num=32, pos_fraction=0.5, add_gt_as_proposals=False, seed=3)

    def buffers():
        return dict(
            assign=dict(gt_inds=torch.empty(B, N, dtype=torch.int64, device=DEV), max_overlaps=torch.empty(B, N, device=DEV),
                        workspace=torch.empty(max(ops.max_iou_assign_workspace_bytes(B, G), 16), dtype=torch.uint8, device=DEV)),
            sample=dict(inds=torch.empty(B, 32, dtype=torch.int64, device=DEV), num_pos=torch.empty(B, dtype=torch.int32, device=DEV),
                        num_neg=torch.empty(B, dtype=torch.int32, device=DEV), mask=torch.empty(B, N, dtype=torch.uint8, device=DEV),
                        workspace=torch.empty(ops.random_sample_workspace_bytes(B, N), dtype=torch.uint8, device=DEV)),
            loss=dict(stats=torch.empty(2 * L + 3, device=DEV), workspace=torch.empty(ops.rpn_loss_workspace_bytes(B, N), dtype=torch.uint8, device=DEV),
                      grads=[torch.empty_like(m) for m in maps]))
    gout = torch.cat([torch.linspace(0.5, 1.5, L, device=DEV), torch.linspace(1.5, 0.5, L, device=DEV)])
    coder_cfg = (M6, gen.RPN_STDS, 1.0 / 9.0, 1.0, 1.0)

    def step(buf):
        gt_inds, _, _ = assigner.assign_batched(anchors, hulls, counts, **buf["assign"])
        s = sampler.sample_batched(gt_inds, **buf["sample"])
        out = rpn_head_loss(maps[:L], maps[L:], anchors, gts, gt_inds, s.mask, counts, stats=buf["loss"]["stats"], workspace=buf["loss"]["workspace"])
        grads = buf["loss"]["grads"]          # the node's backward launch, into the test's buffers
        ops.rpn_loss_bwd(maps[:L], maps[L:], anchors, gts, gt_inds, s.mask, counts, *coder_cfg, buf["loss"]["stats"], gout, grads[:L], grads[L:])
        return out["loss_rpn_cls"], out["loss_rpn_bbox"], grads, s

    def snapshot(res):
        return [res[0].clone(), res[1].clone()] + [g.clone() for g in res[2]] + [res[3].mask.clone()]

    cap = buffers()
    first = snapshot(step(cap))          # eager: allocates the key
    assert int((first[-1] == 1).sum()) > 0 and int((first[-1] == 2).sum()) > 0 and float(first[1].detach().abs().sum()) > 0
    graph, res, allocated = _capture(lambda: step(cap))
    assert allocated == 0, f"{allocated} allocations inside the capture"
    for t in cap["loss"]["grads"]:          # (not the stats: the returned losses are views of that buffer)
        t.fill_(NAN)
    graph.replay()
    assert all(same(a, b) for a, b in zip(snapshot(res), first)), "replay equals eager"
    sampler.draw()
    graph.replay()
    second = snapshot(res)
    eager = snapshot(step(buffers()))          # the same key on the device
    assert all(same(a, b) for a, b in zip(second, eager)) and not torch.equal(second[-1], first[-1]), "after draw()"
    counts.copy_(torch.tensor([7, 3], dtype=torch.int32, device=DEV))
    graph.replay()
    third = snapshot(res)
    eager = snapshot(step(buffers()))
    assert all(same(a, b) for a, b in zip(third, eager)) and not same(third[1], second[1]), "after new ground-truth counts"


def test_rcnn_chain_under_capture():
    """assign_batched (rotated) -> OBBRandomSampler.sample_batched -> gather -> bbox_head_loss -> its backward launch in one captured graph"""
    B, N, G, num, K = 2, 257, 7, 64, 15
    cc = cgen.chain_case(N, G)
    gts = cc["gts"].to(DEV)[None].repeat(B, 1, 1).contiguous()
    props = torch.from_numpy(cgen.jitter_proposals(cc["gts"].double().numpy()[np.arange(N) % G], 0xAB1).astype(np.float32)).to(DEV)
    props[torch.arange(N, device=DEV) % 5 == 4, :2] += 5000.0          # far background
    labels = (torch.arange(B * G, device=DEV).reshape(B, G) * 5) % K
    counts = torch.tensor([7, 7], dtype=torch.int32, device=DEV)
    R = B * num
    z = (2.0 * torch.from_numpy(cgen.det_uniform(R * (K + 1), 91)).float().reshape(R, K + 1)).to(DEV).requires_grad_()
    p = (1.5 * torch.from_numpy(cgen.det_uniform(R * 5, 92)).float().reshape(R, 5)).to(DEV).requires_grad_()
    assigner = MaxIoUAssigner(0.5, 0.5, 0.5, match_low_quality=False, iou_calculator=dict(type="OBBOverlaps"))
    sampler = OBBRandomSampler(num=num, pos_fraction=0.25, add_gt_as_proposals=True, seed=4)

    def buffers():
        return dict(
            assign=dict(gt_inds=torch.empty(B, N, dtype=torch.int64, device=DEV), max_overlaps=torch.empty(B, N, device=DEV),
                        labels=torch.empty(B, N, dtype=torch.int64, device=DEV),
                        workspace=torch.empty(max(ops.max_iou_assign_workspace_bytes(B, G), 16), dtype=torch.uint8, device=DEV)),
            sample=dict(inds=torch.empty(B, num, dtype=torch.int64, device=DEV), num_pos=torch.empty(B, dtype=torch.int32, device=DEV),
                        num_neg=torch.empty(B, dtype=torch.int32, device=DEV), mask=torch.empty(B, G + N, dtype=torch.uint8, device=DEV),
                        workspace=torch.empty(ops.random_sample_workspace_bytes(B, G + N), dtype=torch.uint8, device=DEV)),
            gather=dict(rois=torch.empty(B, num, 6, device=DEV), s_gt_inds=torch.empty(B, num, dtype=torch.int64, device=DEV),
                        s_labels=torch.empty(B, num, dtype=torch.int64, device=DEV)),
            loss=dict(stats=torch.empty(7, device=DEV), workspace=torch.empty(max(ops.rcnn_loss_workspace_bytes(R), 16), dtype=torch.uint8, device=DEV),
                      grads=(torch.empty_like(z), torch.empty_like(p))))
    gout = torch.tensor([0.75, 1.25], device=DEV)

    def step(buf):
        gt_inds, _, _ = assigner.assign_batched(props, gts, counts, labels, **buf["assign"])
        s = sampler.sample_batched(gt_inds, counts, G, **buf["sample"])
        rois, s_gt, s_lab = sampler.gather(s, props, gts, gt_inds, labels, counts, K, **buf["gather"])
        out = bbox_head_loss(z, p, rois, gts, s_gt, s_lab, counts, num_classes=K, stats=buf["loss"]["stats"], workspace=buf["loss"]["workspace"])
        grads = buf["loss"]["grads"]          # the node's backward launch, into the test's buffers (see test_rpn_chain_under_capture)
        ops.rcnn_loss_bwd(z, p, rois.reshape(-1, 6), gts, s_gt.reshape(-1), s_lab.reshape(-1), counts, M5, gen.RCNN_STDS, 1.0, 1.0, 1.0, buf["loss"]["stats"], gout,
                          *grads)
        return out, grads, s

    def snapshot(res):
        return [res[0]["loss_cls"].clone(), res[0]["loss_bbox"].clone(), res[0]["acc"].clone(), res[1][0].clone(), res[1][1].clone(), res[2].inds.clone()]

    cap = buffers()
    first = snapshot(step(cap))
    assert float(first[1]) > 0 and float(first[0]) > 0
    graph, res, allocated = _capture(lambda: step(cap))
    assert allocated == 0, f"{allocated} allocations inside the capture"
    for t in cap["loss"]["grads"]:
        t.fill_(NAN)
    graph.replay()
    assert all(same(a, b) for a, b in zip(snapshot(res), first)), "replay equals eager"
    sampler.draw()
    graph.replay()
    second = snapshot(res)
    eager = snapshot(step(buffers()))
    assert all(same(a, b) for a, b in zip(second, eager)) and not torch.equal(second[-1], first[-1]), "after draw()"
    counts.copy_(torch.tensor([7, 3], dtype=torch.int32, device=DEV))
    graph.replay()
    third = snapshot(res)
    eager = snapshot(step(buffers()))
    assert all(same(a, b) for a, b in zip(third, eager)) and not torch.equal(third[-1], second[-1]), "after new counts"
