"""The dense-prediction backbone at the resolutions its downstream configurations run: 512 x 512 segmentation crops, 1024 x 1024
DOTA images, 1333 x 800 HRSC images padded to 1344 x 800, and 1000 x 600 (not a multiple of 32: stage maps 250 x 150, 125 x 75, 63 x 38, 32 x 19).  There
the kernels leave the ranges of the 224^2 tests: 65 536 / 67 200 image tokens in the stage-1 DCA, 4 096 / 4 200 keys on the streaming self-attention
kernel at C = 192, 256^2 position-embedding maps, 512^2 stem maps.  Every output and every parameter gradient is compared with the float64 oracle
(oracle.lemevit_dense_forward) on the same weights and image, B = 1."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from detfill import det_tensor
from oracle import lemevit_oracle as O
from test_model_gpu import DEV, _backbone, close

# the golden Tiny dense configuration (tests/golden/gen_golden.py, gen_dense)
TINY = dict(depth=[1, 2, 2, 8, 2], embed_dim=[64, 64, 128, 192, 320], head_dim=32, mlp_ratios=[4, 4, 4, 4, 4], attn_type=["C", "D", "D", "S", "S"], queries_len=16)
# the reduced one of the backward tests: one block per stage (two in stage 3), no DropPath
REDUCED = dict(TINY, depth=[1, 1, 1, 2, 1], drop_path_rate=0.0)


def _oracle_sd(m, grad):
    return {k: (v.detach().cpu().double().requires_grad_(grad and "running" not in k) if v.dtype.is_floating_point else v.detach().cpu())
            for k, v in m.state_dict().items()}


@pytest.mark.parametrize("H,W", [(512, 512), (1024, 1024), (800, 1344), (600, 1000)], ids=["512x512", "1024x1024", "1344x800", "1000x600"])
def test_dense_tiny_forward_large(H, W):
    """Eval-mode multi-scale outputs, fp32 (1e-5 of each output's max-abs) and bf16 autocast (2e-2), the tolerances of test_dense_backbone_forward.  Every
    element of every output map is compared: the edges (first / last row and column of each map, the ragged last tokens of 1000 x 600) included.
    Why 2e-2 holds in bf16 at these sizes: autocast rounds every GEMM operand and stored activation to bf16 (2^-9 relative), and those roundings accumulate
    along the residual stream with DEPTH (13 blocks up to stage 3 of Tiny), not with resolution -- more tokens only lengthen the attention / dwconv / token
    sums, which run in fp32.  So the error distribution is that of the 224^2 golden test at every size; the figure checked, max-abs error over max-abs
    output, is its extreme tail over the whole map (measured on MI355X: 1.6e-2 .. 1.95e-2, worst at 512^2 stage 3, while the rel-L2 of every output is
    printed and stays far below it)."""
    t0 = time.time()
    m = _backbone(TINY, 51).eval()
    img = det_tensor((1, 3, H, W), f"dense_large.{H}x{W}.img", 6)
    with torch.no_grad():
        refs = O.lemevit_dense_forward(_oracle_sd(m, False), TINY, img.double())
    t1 = time.time()
    shapes = [(1, 64, -(-H // 4), -(-W // 4)), (1, 128, -(-H // 8), -(-W // 8)), (1, 192, -(-H // 16), -(-W // 16)), (1, 320, -(-H // 32), -(-W // 32))]
    assert [tuple(r.shape) for r in refs] == shapes
    errs = {}
    for dtype, tol in [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)]:
        with torch.no_grad(), torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
            outs = m(img.to(DEV))
        assert [tuple(o.shape) for o in outs] == shapes
        errs[dtype] = [close(o, r, tol, f"{H}x{W} out{i} {dtype}") for i, (o, r) in enumerate(zip(outs, refs))]
        print(f"dense Tiny {W}x{H} {dtype}: rel-L2 per output", [f"{float((o.detach().double().cpu() - r).norm() / r.norm()):.1e}" for o, r in zip(outs, refs)])
    print(f"dense Tiny {W}x{H}: worst rel err fp32 {max(errs[torch.float32]):.2e} (bound 1e-5), bf16 {max(errs[torch.bfloat16]):.2e} (bound 2e-2); "
          f"per output fp32 {['%.1e' % e for e in errs[torch.float32]]}, bf16 {['%.1e' % e for e in errs[torch.bfloat16]]}; "
          f"oracle {t1 - t0:.1f} s, GPU + compare {time.time() - t1:.1f} s")


@pytest.mark.parametrize("H,W,dtype", [(512, 512, torch.float32), (512, 512, torch.bfloat16), (800, 1344, torch.bfloat16)],
                         ids=["512x512-fp32", "512x512-bf16", "1344x800-bf16"])
def test_dense_backward_large(H, W, dtype):
    """Train mode (norm layers frozen in eval mode, as the reference's train() keeps them), loss sum_i <out_i, g_i> with fixed cotangents: every parameter
    gradient against float64 autograd through the oracle.  fp32: 2e-4 of each tensor's max-abs (the per-tensor bound of test_train_step_fp32).  bf16 autocast:
    the statistics and bounds of test_base_224_bf16_gradients_vs_oracle (whole-gradient rel-L2 and cosine; per-tensor median and 90th percentile; worst cosine)."""
    t0 = time.time()
    m = _backbone(REDUCED, 3).train()
    assert not any(mod.training for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.LayerNorm)))
    img = det_tensor((1, 3, H, W), f"dense_large.grad.{H}x{W}.img", 6)
    ref_sd = _oracle_sd(m, True)
    with torch.autocast("cuda", torch.bfloat16, enabled=dtype == torch.bfloat16):
        outs = m(img.to(DEV))
    gs = [det_tensor(tuple(o.shape), f"dense_large.grad.g{i}", 6) for i, o in enumerate(outs)]
    sum((o.float() * g.to(DEV)).sum() for o, g in zip(outs, gs)).backward()
    t1 = time.time()
    refs = O.lemevit_dense_forward(ref_sd, REDUCED, img.double())
    sum((r * g.double()).sum() for r, g in zip(refs, gs)).backward()
    t2 = time.time()
    for i, (o, r) in enumerate(zip(outs, refs)):
        close(o, r.detach(), 1e-5 if dtype == torch.float32 else 2e-2, f"train-mode out{i}")
    gmax = max(float(v.grad.abs().max()) for v in ref_sd.values() if getattr(v, "grad", None) is not None)
    errs, n_zero = [], 0
    for k, p in m.named_parameters():
        r = ref_sd[k].grad
        if r is None:             # not on the backbone's path: extra_norms, norm, norm_c; the meta-token MLPs in front of the S stages (their zero gradient)
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        gq = p.grad.detach().double().cpu()
        assert torch.isfinite(gq).all(), k
        if float(r.abs().max()) <= 1e-5 * gmax:                         # mathematically zero gradient: rounding noise on both sides, held to a coarse bound
            n_zero += 1
            assert float(gq.abs().max()) <= (2e-4 if dtype == torch.float32 else 2e-2) * gmax, (k, float(gq.abs().max()), gmax)
            continue
        errs.append((float((gq - r).abs().max() / r.abs().max()), float((gq - r).norm() / r.norm()),
                     float(torch.nn.functional.cosine_similarity(gq.flatten(), r.flatten(), dim=0)), k))
    errs.sort(reverse=True)
    assert len(errs) >= 100, len(errs)
    print(f"dense backward {W}x{H} {dtype}: {len(errs)} tensors ({n_zero} zero), largest per-tensor errors (max-abs, rel-L2, cosine):",
          [(k, f"{e:.2e}", f"{l2:.2e}", f"{c:.5f}") for e, l2, c, k in errs[:6]], f"; GPU {t1 - t0:.1f} s, oracle {t2 - t1:.1f} s")
    if dtype == torch.float32:
        bad = [(k, e) for e, _, _, k in errs if e > 2e-4]
        assert not bad, bad
        return
    es = sorted(e for e, _, _, _ in errs)
    med, p90 = es[len(es) // 2], es[len(es) * 9 // 10]
    worst_cos = min((c, k) for _, _, c, k in errs)
    names = [k for k, p in m.named_parameters() if ref_sd[k].grad is not None]
    params = dict(m.named_parameters())
    gall = torch.cat([params[k].grad.detach().double().cpu().flatten() for k in names])
    rall = torch.cat([ref_sd[k].grad.flatten() for k in names])
    gl2 = float((gall - rall).norm() / rall.norm())
    gcos = float(torch.nn.functional.cosine_similarity(gall, rall, dim=0))
    print(f"  whole-gradient rel-L2 {gl2:.2e} (bound 3e-2), cosine {gcos:.6f} (>= 0.9995); per tensor median {med:.2e} (2e-2), 90th percentile {p90:.2e} (8e-2), "
          f"worst cosine {worst_cos[0]:.4f} ({worst_cos[1]}; >= 0.90)")
    assert gl2 <= 3e-2 and gcos >= 0.9995, (gl2, gcos)
    assert med <= 2e-2 and p90 <= 8e-2, (med, p90)
    assert worst_cos[0] >= 0.90, worst_cos
